"""The tanh GEMM epilogue (csrc/gemm.hip.h EpiTanh behind gemm_tanh) on its own, through the test hook cc_gemm_tanh, in all three operand
builds against float64 (tests/mlp_ref.py, tests/gemm_ref.py).

    C = h = tanh(u), u = A B^T + bias;   pre = t = 1 - h h from the fp32 h (the multiplier cc_gemm_dact act 3 applies in the backward)

Shapes: (1, 48, 24) one row, a sub-tile N, K below one MFMA step; (5, 96, 48) an odd number of rows; (130, 400, 200) crosses the 128-row and
the 256-column tile, ragged K; (16, 264, 64) what the 64-row skinny kernels accept, with an 8-column tail.  Every shape on the chooser's
kernel and on each forced tile kernel (both entry points of the functor: operator() on the 128-row / skinny kernels, bias8 / fin on the
256-row ones), with and without `pre`, `pre` stored plainly and non-temporally, and in the split-bf16 build with C as the consumer's
operand image as well.

Inputs: the operands of tests/test_gpu_gemm_epilogues.py's Problem; the bias spreads the pre-activations over [-12, 12] and puts a few
columns at +-40, where h must be exactly +-1 and t exactly 0.

Bounds, element-wise, no element exempt (none tuned):
    err_u = acc_bound(S, kp) + 2^-24 |u|                                           (accumulation, then the bias addition)
    |h - tanh u|         <= store_bound(tanh u, err_u + TANH_ULPS 2^-24, type)      (tanh is 1-Lipschitz)
    |t - (1 - tanh^2 u)| <= store_bound(1 - tanh^2 u, 4 / (3 sqrt 3) err_u + TANH_GRAD_ULPS 2^-24, type)
TANH_ULPS / TANH_GRAD_ULPS are measured allowances (4 x the raw figures test_measured_allowances prints with -s)."""
import pytest
import torch

from tests import gemm_ref as R
from tests import mlp_ref as MR
from tests.test_gpu_gemm_epilogues import Problem, Report, Scratch, _bytes, _lib, _p, _st, modes, padding_ok, twice

pytestmark = pytest.mark.gpu

SHAPES = [(1, 48, 24), (5, 96, 48), (130, 400, 200), (16, 264, 64)]
SAT = 40.0            # bias of the saturated columns
SAT_COLS = 4          # at each sign
EXACT_FROM = 20.0     # |u| from which float64 tanh is exactly +-1 as well (1 - 2 e^-40 rounds to 1)


def make_bias(N, seed):
    """per column: [-12, 12] evenly, in a random order; the first SAT_COLS columns at +40, the next SAT_COLS at -40"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    b = torch.linspace(-12.0, 12.0, N, device="cuda")[torch.randperm(N, device="cuda", generator=g)]
    b[:SAT_COLS] = SAT
    b[SAT_COLS:2 * SAT_COLS] = -SAT
    return b.contiguous()


@pytest.fixture(scope="module")
def problems():
    cache = {}

    def get(op, M, N, K):
        if (op, M, N, K) not in cache:
            cache[(op, M, N, K)] = Problem(op, M, N, K)
        return cache[(op, M, N, K)]
    return get


def run_tanh(rep, pb, skinny=0):
    l, M, N, K = _lib(), pb.M, pb.N, pb.K
    ldc = N + 8
    bias = make_bias(N, N + K)
    u = pb.acc + bias.double()
    err_u = R.acc_bound(pb.S, pb.kp, skinny, M) + R.U32 * u.abs()
    href, tref = MR.tanh(u), MR.tanh_grad(u)
    hb = R.store_bound(href, MR.TANH_LIP * err_u + MR.TANH_ULPS * R.U32, pb.dt)
    tb = R.store_bound(tref, MR.TANH_GRAD_LIP * err_u + MR.TANH_GRAD_ULPS * R.U32, pb.dt)
    sat = u.abs() >= EXACT_FROM
    rep.check("the saturated columns are not saturated", bool(sat[:, :2 * SAT_COLS].float().mean() > 0.5))
    outs_by = {}
    for with_pre, nt in ((0, 0), (1, 0), (1, 1)):
        name = f"tanh{'+pre' if with_pre else ''}{'+nt' if nt else ''}"
        sc = Scratch(pb.scratch_bytes)

        def fn():
            Cm, Pm = pb.out(ldc), pb.out(ldc) if with_pre else None
            rc = l.cc_gemm_tanh(pb.code, 0, 0, *pb.a_args(), _p(pb.B), pb.ldb, M, N, K, _p(Cm), 0, ldc, _p(bias), _p(Pm), nt, *sc.args(), _st())
            return rc, (Cm,) + ((Pm,) if with_pre else ())
        outs = twice(rep, name, fn)
        outs_by[(with_pre, nt)] = outs
        h = outs[0][:M, :N]
        rep.bound(f"{name} h", h, href, hb)
        rep.check(f"{name}: h is not exactly +-1 at |u| >= {EXACT_FROM}", bool((h.double()[sat] == torch.sign(u)[sat]).all()))
        rep.check(f"{name}: C padding written", padding_ok(outs[0], M, N))
        if with_pre:
            t = outs[1][:M, :N]
            rep.bound(f"{name} t", t, tref, tb)
            rep.check(f"{name}: t is not exactly 0 at |u| >= {EXACT_FROM}", bool((t.double()[sat] == 0).all()))
            rep.check(f"{name}: pre padding written", padding_ok(outs[1], M, N))
        rep.check(f"{name}: scratch guard written", sc.guard_ok())
    rep.check("h differs with and without pre", torch.equal(_bytes(outs_by[(0, 0)][0]), _bytes(outs_by[(1, 0)][0])))
    rep.check("non-temporal stores change values", all(torch.equal(_bytes(a), _bytes(b)) for a, b in zip(outs_by[(1, 0)], outs_by[(1, 1)])))
    if pb.x3:      # C as the [hi | hi | lo] image of the consumer GEMM's A operand; pre keeps the plain layout
        sc = Scratch(pb.scratch_bytes)
        img = torch.full((M + 1, 3 * N), float("nan"), dtype=torch.bfloat16, device="cuda")
        Pm = pb.out(ldc)
        rc = l.cc_gemm_tanh(2, 0, 0, *pb.a_args(), _p(pb.B), pb.ldb, M, N, K, _p(img), N, ldc, _p(bias), _p(Pm), 1, *sc.args(), _st())
        torch.cuda.synchronize()
        rep.check(f"image: rc {rc}", rc == 0)
        hi, lo, copy = R.unimage(img[:M], 0)
        rep.check("image: the two hi planes differ", torch.equal(_bytes(hi), _bytes(copy)))
        rep.check("image: row M written", bool(torch.isnan(img[M].float()).all()))
        rep.check("image: not the split of the plain h", torch.equal(_bytes(img[:M]), _bytes(R.image(outs_by[(1, 1)][0][:M, :N].contiguous(), 0))))
        rep.bound("image hi+lo", hi.double() + lo.double(), href, hb + R.U_BF16 ** 2 * href.abs() * (1 + R.U_BF16))
        rep.check("image: t differs from the plain call's", torch.equal(_bytes(Pm), _bytes(outs_by[(1, 1)][1])))
        rep.check("image: scratch guard written", sc.guard_ok())


def _cases():
    out = []
    for op in ("bf16", "fp16", "x3"):
        for M, N, K in SHAPES:
            for t in (-1, 0, 3, 4, 5, 6, 7):
                if op == "x3" and t in (6, 7):
                    continue      # the 160 x 256 kernels do not exist in the split-bf16 build (launch_gemm: can160)
                out.append(pytest.param(op, "tile", t, M, N, K, id=f"{op}-tile{t}-{M}x{N}x{K}"))
            if ((3 * K) if op == "x3" else K) % 64 == 0 and M <= 1024:
                for s in (1, 2, 3, 4):
                    out.append(pytest.param(op, "skinny", s, M, N, K, id=f"{op}-skinny{s}-{M}x{N}x{K}"))
    return out


@pytest.mark.parametrize("op,which,mode,M,N,K", _cases())
def test_tanh_epilogue(problems, op, which, mode, M, N, K):
    pb = problems(op, M, N, K)
    rep = Report(f"{op} tanh {which}{mode} {M}x{N}x{K}")
    with modes(tile=mode if which == "tile" else -1, skinny=mode if which == "skinny" else -1):
        run_tanh(rep, pb, skinny=mode if which == "skinny" else 0)
    rep.done()


def test_special_values():
    """u = bias exactly (zero A): u = 0 gives h = 0, t = 1 (a -0 cannot reach the functor: the accumulator is +0 and +0 + -0 = +0), NaN
    propagates to both outputs and nowhere else, +-inf, +-1e30 and +-88 give exactly +-1 / 0, h is odd in u, tiny arguments stay tiny"""
    l = _lib()
    M, N, K = 8, 16, 8
    A = torch.zeros(M, K, device="cuda")
    Bm = R.image(torch.randn(N, K, device="cuda"), 1)
    vals = [0.0, -0.0, float("nan"), float("inf"), -float("inf"), 1e30, -1e30, 88.0, -88.0, 9.5, -9.5, 1e-30, -1e-30, 1e-10, 0.5, -0.5]
    bias = torch.tensor(vals, device="cuda")
    Cm, Pm = torch.full((M, N), 7.0, device="cuda"), torch.full((M, N), 7.0, device="cuda")
    sc = Scratch(l.cc_x3_image_bytes(M, K))
    assert l.cc_gemm_tanh(2, 0, 0, _p(A), 0, K, _p(Bm), K, M, N, K, _p(Cm), 0, N, _p(bias), _p(Pm), 0, *sc.args(), _st()) == 0
    torch.cuda.synchronize()
    h, t = Cm[0].cpu(), Pm[0].cpu()
    ok = [i for i in range(N) if i != 2]
    assert torch.equal(Cm[:, ok], Cm[:1, ok].expand(M, N - 1)) and torch.equal(Pm[:, ok], Pm[:1, ok].expand(M, N - 1))
    assert h[0] == 0 and h[1] == 0 and t[0] == 1 and t[1] == 1
    assert torch.isnan(h[2]) and torch.isnan(t[2])
    assert int(torch.isnan(Cm).sum()) == M and int(torch.isnan(Pm).sum()) == M          # no NaN anywhere else
    for i in (3, 5, 7):
        assert h[i] == 1 and h[i + 1] == -1 and t[i] == 0 and t[i + 1] == 0, (vals[i], h[i], t[i])
    assert abs(h[9].item() - 1.0) <= 2.0 ** -23 and h[10] == -h[9]
    assert h[11].item() >= 0 and abs(h[11].item()) <= 1e-29 and h[12].item() <= 0          # tiny arguments: no blow-up, sign kept or +-0
    assert abs(h[13].item() - 1e-10) <= 2.0 ** -23
    assert abs(h[14].item() - 0.46211715726000974) <= MR.RAW_LIMIT * R.U32 and h[15] == -h[14]


def test_argument_errors_launch_nothing():
    l = _lib()
    A16, B16 = torch.randn(16, 64, device="cuda").bfloat16(), torch.randn(16, 64, device="cuda").bfloat16()
    C16 = torch.full((16, 16), float("nan"), dtype=torch.bfloat16, device="cuda")
    for code in (0, 1):
        assert l.cc_gemm_tanh(code, 0, 0, _p(A16), 64, 64, _p(B16), 64, 16, 16, 64, _p(C16), 0, 16, None, None, 0, None, 0, _st()) == -1      # A image
        assert l.cc_gemm_tanh(code, 0, 0, _p(A16), 0, 64, _p(B16), 64, 16, 16, 64, _p(C16), 16, 16, None, None, 0, None, 0, _st()) == -1      # C image
        assert l.cc_gemm_tanh(code, 0, 0, _p(A16), 0, 64, _p(B16), 64, 16, 16, 64, _p(C16), 0, 8, None, None, 0, None, 0, _st()) == -1       # ldc < N
        assert l.cc_gemm_tanh(code, 0, 0, None, 0, 64, _p(B16), 64, 16, 16, 64, _p(C16), 0, 16, None, None, 0, None, 0, _st()) == -1
    A32 = torch.randn(16, 64, device="cuda")
    C32 = torch.full((16, 16), float("nan"), device="cuda")
    assert l.cc_gemm_tanh(2, 0, 0, _p(A32), 0, 64, _p(B16), 64, 16, 16, 64, _p(C32), 0, 16, None, None, 0, None, 0, _st()) == -4             # no image scratch
    torch.cuda.synchronize()
    assert torch.isnan(C16.float()).all() and torch.isnan(C32).all()


def _device_tanh(u32, tile):
    """h, t of the device function on the fp32 arguments u32 [n] (n % 8 == 0): split-bf16 build, zero A, u = bias exactly"""
    l = _lib()
    n, M, K = u32.numel(), 8, 8
    A = torch.zeros(M, K, device="cuda")
    Bm = torch.zeros(n, 3 * K, dtype=torch.bfloat16, device="cuda")
    Cm, Pm = torch.empty(M, n, device="cuda"), torch.empty(M, n, device="cuda")
    sc = Scratch(l.cc_x3_image_bytes(M, K))
    with modes(tile=tile):
        assert l.cc_gemm_tanh(2, 0, 0, _p(A), 0, K, _p(Bm), K, M, n, K, _p(Cm), 0, n, _p(u32), _p(Pm), 0, *sc.args(), _st()) == 0
    return Cm[0].double(), Pm[0].double()


def test_measured_allowances(problems):
    """Re-measures the two figures tests/mlp_ref.py cannot derive and prints them (pytest -s): worst |device - float64| / 2^-24 of tanh_f and of
    t = 1 - h h on the same fp32 argument, in the split-bf16 build — a grid over [-20, 20] through the bias (u = bias exactly), and the
    inputs of test_tanh_epilogue, whose fp32 u the same kernel hands out through cc_gemm_act act 0.  Asserts that the raw figures are
    inside the allowances in force, and that neither exceeds 33 x 2^-24: beyond that tanh_f has a defect."""
    l = _lib()
    worst_h = worst_t = 0.0
    grid = torch.cat([torch.linspace(-20.0, 20.0, 262144 - 4096, device="cuda"), torch.linspace(-1.0, 1.0, 4096, device="cuda")]).contiguous()
    for tile in (0, 4):
        h, t = _device_tanh(grid, tile)
        eh = ((h - MR.tanh(grid)).abs() / R.U32).max().item()
        et = ((t - MR.tanh_grad(grid)).abs() / R.U32).max().item()
        print(f"MEASURED tanh grid [-20, 20] tile{tile}: tanh {eh:.3f} x 2^-24, 1 - tanh^2 {et:.3f} x 2^-24")
        worst_h, worst_t = max(worst_h, eh), max(worst_t, et)
    for M, N, K in SHAPES:
        pb = problems("x3", M, N, K)
        bias = make_bias(N, N + K)
        for tile in (-1, 0, 4):
            sc = Scratch(pb.scratch_bytes)
            U, H, T = pb.out(N + 8), pb.out(N + 8), pb.out(N + 8)
            common = (*pb.a_args(), _p(pb.B), pb.ldb, M, N, K)
            with modes(tile=tile):
                rcs = [l.cc_gemm_act(2, 0, 0, *common, _p(U), 0, N + 8, _p(bias), 0, None, *sc.args(), _st()),
                       l.cc_gemm_tanh(2, 0, 0, *common, _p(H), 0, N + 8, _p(bias), _p(T), 0, *sc.args(), _st())]
            assert rcs == [0, 0]
            u = U[:M, :N].double()
            eh = ((H[:M, :N].double() - MR.tanh(u)).abs() / R.U32).max().item()
            et = ((T[:M, :N].double() - MR.tanh_grad(u)).abs() / R.U32).max().item()
            print(f"MEASURED tanh {M}x{N}x{K} tile{tile} |u| <= {u.abs().max().item():.1f}: tanh {eh:.3f} x 2^-24, 1 - tanh^2 {et:.3f} x 2^-24")
            worst_h, worst_t = max(worst_h, eh), max(worst_t, et)
    print(f"MEASURED worst: tanh {worst_h:.3f} (allowance {MR.TANH_ULPS}), 1 - tanh^2 {worst_t:.3f} (allowance {MR.TANH_GRAD_ULPS})")
    assert worst_h <= MR.RAW_LIMIT and worst_t <= MR.RAW_LIMIT
    assert worst_h <= MR.TANH_ULPS and worst_t <= MR.TANH_GRAD_ULPS
