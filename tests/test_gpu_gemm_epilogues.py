"""The four GEMM wrappers every GEMM of a training step leaves through (gemm_bf16out, gemm_resid, gemm_dact, gemm_f32out; csrc/gemm_api.h) and
the split-bf16 operand path, one wrapper call at a time through the test hooks cc_gemm_act / cc_gemm_resid / cc_gemm_dact / cc_gemm_f32 /
cc_gemm_wgrad_split / cc_x3_split_rows, against float64 (tests/gemm_ref.py) in all three operand builds.

Reference: float64 products of the values the kernel really multiplies (the 16-bit-rounded operands; in the split-bf16 build the hi / lo
planes of tests/gemm_ref.py's own split), then the epilogue in float64.  Every epilogue has two entry points (operator() for the 128-row
and skinny kernels, pre4 / bias8 / fin for the 256-row kernels) plus compile-time specialisations: in the 16-bit-store and residual functors
both end in one shared body (activation, copies, stores), the fp32 and activation-gradient functors still write their arithmetic once per
entry point; the tile modes below force each entry point at every shape.

Bounds (derived in tests/gemm_ref.py, none tuned): accumulation (steps * MFMA_ROUNDINGS + additions) * 2^-24 * sum |terms| with the step
count of the kernel that ran; one 2^-24 rounding per epilogue addition; 16-bit stores u |ref| + (1 + u) * error, u = 2^-8 / 2^-11; the
activation's Lipschitz constant in front of the accumulation error.  Measured on the MI355X and allowed 4 x (gemm_ref.py, DESIGN.md
section 2): one MFMA step against the exact sum of its 32 products — worst 1.62 of 2^-24 * sum |terms|, more than one rounding inside a
step, allowance 6.5 roundings per step; device gelu_new 2.54 * 2^-24 * |x| (allowance 10.2), gelu_new' 33.07 * 2^-24 (allowance 132.3).

Split-bf16 (the kernels see K' = 3 K): element-wise against the three-term float64 sum with the same accumulation bound over 3 K terms,
against the exact float64 product with 3 u^2 sum |a||b| more, and — because an element-wise bound cannot see ONE dropped lo term at deep K —
the relative Frobenius error against the exact product, under the geometric mean of the float64-emulated correct result and the
float64-emulated defect (hi*lo or lo*hi term dropped) for the case's own operands.  The persistent 160 x 256 kernel (tile modes 6 / 7)
is never launched in this build (launch_gemm: can160 = !kX3), so its three- / two-stage rings cannot be reached; 128 | 3K would imply
192 | 3K anyway (and 64 | 3K likewise implies 192 | 3K).  K is picked by what 3 K selects — the classes that exist are 3 K % 192 == 0
(K = 64, 128, 256: the fused two-stage forms), 3 K % 32 == 0 only (K = 32, 96: the 256-row kernels' depth, not the 128-row kernels') and the
ragged rest (K = 40, 3 K = 120: the register-staged fallback).

The raw figures behind the measured allowances come from test_measured_allowances (run it with -s to see them)."""
import contextlib
import ctypes as C
import functools

import pytest
import torch

from tests import gemm_ref as R

pytestmark = pytest.mark.gpu

OPS = {"bf16": (0, torch.bfloat16), "fp16": (1, torch.float16), "x3": (2, torch.float32)}
GUARD = 4096          # bytes behind the image scratch that must stay untouched
PAD_VALUE = 3.0e4     # what the padding of the operands' leading dimensions holds: a kernel reading it cannot stay inside a bound


def _lib():
    from clipcap_amd import _lib
    return _lib.lib()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bytes(t):
    return t.contiguous().view(torch.uint8)


@contextlib.contextmanager
def modes(tile=-1, skinny=-1):
    l = _lib()
    ot, os_ = l.cc_gemm_tile_mode(tile), l.cc_gemm_skinny_mode(skinny)
    try:
        yield
    finally:
        torch.cuda.synchronize()
        l.cc_gemm_tile_mode(ot)
        l.cc_gemm_skinny_mode(os_)


class Scratch:
    """NaN-filled image scratch of exactly the queried size with a guard region behind it."""

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.buf = torch.full((self.n + GUARD,), 255, dtype=torch.uint8, device="cuda")

    def args(self):
        return (_p(self.buf), self.n) if self.n else (None, 0)

    def guard_ok(self):
        return bool((self.buf[self.n:] == 255).all())


def image_bytes(rows, depth):
    n = _lib().cc_x3_image_bytes(rows, depth)
    assert n >= rows * depth * 6 and n % 256 == 0 and n - rows * depth * 6 < 256
    return n


class Problem:
    """Operands of one NT GEMM C[M][N] = A[M][K] B[N][K]^T on the device and everything float64 the checks need."""

    def __init__(self, op, M, N, K, zero_rows=False):
        self.op, self.M, self.N, self.K = op, M, N, K
        self.code, self.dt = OPS[op]
        self.x3 = op == "x3"
        g = torch.Generator(device="cuda").manual_seed(M * 7919 + N * 31 + K)
        a = torch.randn(M, K, device="cuda", generator=g) + 0.3
        b = torch.randn(N, K, device="cuda", generator=g) * 0.5 + 0.1
        if zero_rows:
            a[::5] = 0.0
        self.lda, self.ldb = K + 8, K + 8
        self.kp = 3 * K if self.x3 else K
        if self.x3:
            self.A = torch.full((M, self.lda), PAD_VALUE, device="cuda")
            self.A[:, :K] = a
            self.Aimg = R.image(a, 0)
            self.B = torch.full((N, 3 * self.ldb), PAD_VALUE, dtype=torch.bfloat16, device="cuda")
            self.B[:, :3 * K] = R.image(b, 1)
            ahi, alo = R.split(a)
            bhi, blo = R.split(b)
            self.acc, self.S = R.three_term(ahi, alo, bhi, blo)
            self.exact = a.double() @ b.double().t()
            self.Sx = a.double().abs() @ b.double().abs().t()
            hh = ahi.double() @ bhi.double().t()
            self.defects = [hh + ahi.double() @ blo.double().t(), hh + alo.double() @ bhi.double().t()]      # lo*hi dropped, hi*lo dropped
        else:
            self.A = torch.full((M, self.lda), PAD_VALUE, dtype=self.dt, device="cuda")
            self.A[:, :K] = a.to(self.dt)
            self.B = torch.full((N, self.ldb), PAD_VALUE, dtype=self.dt, device="cuda")
            self.B[:, :K] = b.to(self.dt)
            a64, b64 = self.A[:, :K].double(), self.B[:, :K].double()
            self.acc = a64 @ b64.t()
            self.S = a64.abs() @ b64.abs().t()
        self.scratch_bytes = image_bytes(M, K) if self.x3 else 0

    def a_args(self, as_image=False):
        if as_image:
            return _p(self.Aimg), self.K, self.lda
        return _p(self.A), 0, self.lda

    def out(self, ld, dtype=None, rows=None):
        return torch.full(((rows or self.M) + 1, ld), float("nan"), dtype=dtype or self.dt, device="cuda")


@functools.lru_cache(maxsize=1)
def problem(op, M, N, K):
    return Problem(op, M, N, K)


class Report:
    """collects failures of one test and prints the worst measured / bound ratio of every check (pytest -s / -rP shows them)"""

    def __init__(self, tag):
        self.tag, self.fail = tag, []

    def bound(self, name, got, ref, bound):
        got = got.double()
        if not torch.isfinite(got).all():
            self.fail.append(f"{name}: non-finite output")
            return
        err = (got - ref).abs()
        exact = bound <= 0
        if exact.any() and (err[exact] != 0).any():
            self.fail.append(f"{name}: {int((err[exact] != 0).sum())} elements differ where the result is exact")
        ratio = (err[~exact] / bound[~exact]).max().item() if (~exact).any() else 0.0
        print(f"RATIO {self.tag} {name} {ratio:.4f}")
        if ratio > 1.0:
            self.fail.append(f"{name}: error / bound = {ratio:.3f}")

    def frob(self, name, got, epi, pb, emulate=lambda v: v):
        """split-bf16: relative Frobenius distance from the epilogue of the EXACT product, against the emulated correct / defect distances"""
        ref = epi(pb.exact)
        n = ref.norm().item()
        correct = (emulate(epi(pb.acc)) - ref).norm().item() / n
        defects = [(emulate(epi(d)) - ref).norm().item() / n for d in pb.defects]
        thr = R.frobenius_threshold(correct, defects)
        val = (got.double() - ref).norm().item() / n
        print(f"FROB {self.tag} {name} got {val:.3e} correct {correct:.3e} defect {min(defects):.3e} threshold {thr:.3e}")
        if not val <= thr:
            self.fail.append(f"{name}: relative Frobenius error {val:.3e} > {thr:.3e} (correct {correct:.3e}, dropped-term defect {min(defects):.3e})")

    def check(self, name, cond):
        if not cond:
            self.fail.append(name)

    def done(self):
        assert not self.fail, f"{self.tag}: " + "; ".join(self.fail)


def twice(rep, name, fn, deterministic=True):
    """runs fn() -> (rc, outputs) twice on fresh buffers; the bytes must agree (bit determinism of the hook)"""
    rc, outs = fn()
    rc2, outs2 = fn()
    torch.cuda.synchronize()
    rep.check(f"{name}: rc {rc} / {rc2}", rc == 0 and rc2 == 0)
    if deterministic and rc == 0 and rc2 == 0:
        rep.check(f"{name}: two runs differ", all(torch.equal(_bytes(x), _bytes(y)) for x, y in zip(outs, outs2)))
    return outs


def padding_ok(t, M, N):
    """columns [N, ld) and the row behind the last one still hold the NaN fill"""
    return bool(torch.isnan(t[:M, N:].float()).all() and torch.isnan(t[M].float()).all())


# ---- one wrapper, every variant of its epilogue -------------------------------------------------------------------------------------
def run_act(rep, pb, skinny=0, tile=-1, variants=None):
    l, M, N, K = _lib(), pb.M, pb.N, pb.K
    ldc = N + 8
    L1, L2 = R.gelu_lipschitz()
    g = torch.Generator(device="cuda").manual_seed(N)
    bias_t = torch.randn(N, device="cuda", generator=g)
    accb = R.acc_bound(pb.S, pb.kp, skinny, M)
    for act, with_pre, with_bias in variants or [(a, p, b) for a, p in ((0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1), (3, 1)) for b in (1, 0)]:
        name = f"act{act}{'+pre' if with_pre else ''}{'+bias' if with_bias else ''}"
        bias = bias_t if with_bias else None
        sc = Scratch(pb.scratch_bytes)

        def fn():
            Cm, Pm = pb.out(ldc), pb.out(ldc) if with_pre else None
            rc = l.cc_gemm_act(pb.code, 0, 0, *pb.a_args(), _p(pb.B), pb.ldb, M, N, K, _p(Cm), 0, ldc, _p(bias), act, _p(Pm), *sc.args(), _st())
            return rc, (Cm,) + ((Pm,) if with_pre else ())
        outs = twice(rep, name, fn)
        u = pb.acc + (bias.double() if with_bias else 0.0)
        eu = accb + (R.U32 * (pb.acc.abs() + bias.double().abs()) if with_bias else 0.0)
        f = {0: lambda v: v, 1: R.relu, 2: R.gelu_new, 3: R.gelu_new}[act]
        ec = eu if act < 2 else L1 * eu + R.GELU_ULPS * R.U32 * u.abs()
        rep.bound(f"{name} C", outs[0][:M, :N], f(u), R.store_bound(f(u), ec, pb.dt))
        rep.check(f"{name}: C padding written", padding_ok(outs[0], M, N))
        if with_pre:
            pref, ep = (R.gelu_new_grad(u), L2 * eu + R.GELU_GRAD_ULPS * R.U32) if act == 3 else (u, eu)
            rep.bound(f"{name} pre", outs[1][:M, :N], pref, R.store_bound(pref, ep, pb.dt))
            rep.check(f"{name}: pre padding written", padding_ok(outs[1], M, N))
        rep.check(f"{name}: scratch guard written", sc.guard_ok())
        if pb.x3:
            b64 = bias.double() if with_bias else 0.0
            rep.bound(f"{name} C vs exact", outs[0][:M, :N], f(pb.exact + b64),
                      ec + (1.0 if act < 2 else L1) * R.split_product_bound(pb.Sx))
            rep.frob(f"{name} C", outs[0][:M, :N], lambda v: f(v + b64), pb)


def run_resid(rep, pb, skinny=0, tile=-1):
    l, M, N, K = _lib(), pb.M, pb.N, pb.K
    g = torch.Generator(device="cuda").manual_seed(N + 1)
    bias_t = torch.randn(N, device="cuda", generator=g)
    p, seed, layer = 0.25, 0x1234567887654321, 3
    accb = R.acc_bound(pb.S, pb.kp, skinny, M)
    steps, adds = R.chain_steps(pb.kp, skinny, M)
    for with_bias in (1, 0):
        for alias in (1, 0):
            for site in (None, 2, 3):
                name = f"resid{'+bias' if with_bias else ''}{'+alias' if alias else ''}{'' if site is None else f'+drop{site}'}"
                ld = N if site is not None else N + 8        # dropout: the mask index is row * ld + col — ld == N makes it cc_dropout_mask's
                res = torch.randn(M + 1, ld, device="cuda", generator=g)
                bias = bias_t if with_bias else None
                sc = Scratch(pb.scratch_bytes)

                def fn():
                    out = res.clone() if alias else torch.full_like(res, float("nan"))
                    rin = out if alias else res
                    rc = l.cc_gemm_resid(pb.code, 0, 0, *pb.a_args(), _p(pb.B), pb.ldb, M, N, K, _p(out), _p(rin), ld, _p(bias),
                                         p if site is not None else 0.0, seed, site or 0, layer, *sc.args(), _st())
                    return rc, (out,)
                out, = twice(rep, name, fn)
                keep, scale = None, 1.0
                if site is not None:
                    keep = torch.empty(M * N, dtype=torch.uint8, device="cuda")
                    assert l.cc_dropout_mask(seed, site, layer, p, M * N, _p(keep), _st()) == 0
                    keep = keep.view(M, N)
                    scale = 1.0 / (1.0 - p)
                    changed = out[:M, :N] != res[:M, :N]
                    y = (pb.acc + (bias.double() if with_bias else 0.0)).abs()
                    odd = (changed != keep.bool()) & ~((keep == 1) & (scale * y <= 2 * R.U32 * res[:M, :N].double().abs()))
                    rep.check(f"{name}: kept set differs from cc_dropout_mask in {int(odd.sum())} elements", not odd.any())
                    rep.check(f"{name}: mask keeps {keep.float().mean().item():.3f}",       # four binomial standard deviations
                              abs(keep.float().mean().item() - (1 - p)) <= 4 * (p * (1 - p) / (M * N)) ** 0.5)
                epi = lambda v: R.resid_drop(res[:M, :N], v, bias, keep, p)
                # accumulation bound, then one rounding per epilogue operation: acc + bias, the mask multiplication, res + y
                r64, yabs = res[:M, :N].double().abs(), pb.acc.abs() + (bias.double().abs() if with_bias else 0.0)
                bnd = scale * (accb + (R.U32 * yabs if with_bias else 0.0) + (R.U32 * yabs if keep is not None else 0.0)) + R.U32 * (r64 + scale * yabs)
                if keep is None and skinny == 0 and tile != 0:
                    # EpiResid::acc_init (256-row kernels, dropout off): the accumulators START from the residual, so it passes through every
                    # MFMA step of the chain instead of one addition; which 256-row form honours the flag is the kernel's choice, so every
                    # launch that may reach one is given the term
                    bnd = bnd + (steps * R.MFMA_ROUNDINGS + adds) * R.U32 * r64
                if keep is not None:
                    bnd = torch.where(keep.bool(), bnd, torch.zeros_like(bnd))      # a dropped element is the residual, bit for bit
                rep.bound(f"{name} out", out[:M, :N], epi(pb.acc), bnd)
                if site is None:
                    rep.check(f"{name}: padding written", torch.equal(_bytes(out[:M, N:]), _bytes(res[:M, N:]) if alias else _bytes(out[:M, N:])) and
                              (alias or bool(torch.isnan(out[:M, N:]).all())))
                rep.check(f"{name}: row M written", torch.equal(out[M], res[M]) if alias else bool(torch.isnan(out[M]).all()))
                rep.check(f"{name}: scratch guard written", sc.guard_ok())
                if pb.x3:
                    rep.bound(f"{name} out vs exact", out[:M, :N], epi(pb.exact), bnd + scale * R.split_product_bound(pb.Sx) *
                              (keep.double() if keep is not None else 1.0))
                    rep.frob(f"{name} out", out[:M, :N], epi, pb)


def make_aux(pb, act, ldc, g):
    M, N = pb.M, pb.N
    aux = torch.full((M + 1, ldc), float("nan"), dtype=pb.dt, device="cuda")
    if act == 1:        # post-activation h of a relu: zeros (both signs) and positives
        h = torch.randn(M, N, device="cuda", generator=g)
        h = torch.where(h > 0.3, h, torch.where(h > -0.3, torch.zeros_like(h), -torch.zeros_like(h)))
    elif act == 2:      # pre-activation u
        h = torch.randn(M, N, device="cuda", generator=g) * 2.5
    else:               # gelu_new'(u) as the forward stored it
        h = torch.randn(M, N, device="cuda", generator=g) * 0.5 + 0.5
    aux[:M, :N] = h.to(pb.dt)
    return aux


def dact_factor(aux64, act):
    return (aux64 > 0).double() if act == 1 else R.gelu_new_grad(aux64) if act == 2 else aux64


def run_dact(rep, pb, skinny=0, tile=-1):
    l, M, N, K = _lib(), pb.M, pb.N, pb.K
    ldc = N + 8
    g = torch.Generator(device="cuda").manual_seed(N + 2)
    accb = R.acc_bound(pb.S, pb.kp, 0, M)        # (this epilogue never takes the skinny kernels: launch_gemm, epi_strip_aux)
    for act in (1, 2, 3):
        name = f"dact{act}"
        aux = make_aux(pb, act, ldc, g)
        sc = Scratch(pb.scratch_bytes)

        def fn():
            Cm = pb.out(ldc)
            rc = l.cc_gemm_dact(pb.code, 0, 0, *pb.a_args(), _p(pb.B), pb.ldb, M, N, K, _p(Cm), 0, ldc, _p(aux), act, *sc.args(), _st())
            return rc, (Cm,)
        Cm, = twice(rep, name, fn)
        d = dact_factor(aux[:M, :N].double(), act)
        ref = pb.acc * d
        err = d.abs() * accb + (R.GELU_GRAD_ULPS * R.U32 * pb.acc.abs() if act == 2 else 0.0) + (R.U32 * ref.abs() if act != 1 else 0.0)
        rep.bound(f"{name} C", Cm[:M, :N], ref, R.store_bound(ref, err, pb.dt))
        if act == 1:
            rep.check(f"{name}: non-zero output where aux is +0 / -0", bool((Cm[:M, :N][aux[:M, :N] == 0] == 0).all()))
        rep.check(f"{name}: C padding written", padding_ok(Cm, M, N))
        rep.check(f"{name}: scratch guard written", sc.guard_ok())
        if pb.x3:
            rep.bound(f"{name} C vs exact", Cm[:M, :N], pb.exact * d, err + d.abs() * R.split_product_bound(pb.Sx))
            rep.frob(f"{name} C", Cm[:M, :N], lambda v: v * d, pb)


def run_f32(rep, pb, skinny=0, tile=-1):
    l, M, N, K = _lib(), pb.M, pb.N, pb.K
    ldc = N + 8
    g = torch.Generator(device="cuda").manual_seed(N + 3)
    bias_t = torch.randn(N, device="cuda", generator=g)
    C0 = torch.randn(M + 1, ldc, device="cuda", generator=g) * 3 + 1
    for mode, alpha, with_bias, ks in ((0, 1.0, 1, 1), (0, 0.5, 0, 1), (1, -0.75, 0, 1), (2, 1.0, 0, 1), (2, 1.25, 0, 3)):
        name = f"f32 mode{mode} alpha{alpha}{'+bias' if with_bias else ''} ksplit{ks}"
        bias = bias_t if with_bias else None
        sc = Scratch(pb.scratch_bytes)

        def fn():
            Cm = C0.clone() if mode else torch.full_like(C0, float("nan"))
            rc = l.cc_gemm_f32(pb.code, 0, 0, *pb.a_args(), _p(pb.B), pb.ldb, M, N, K, _p(Cm), ldc, _p(bias), mode, alpha, ks, *sc.args(), _st())
            return rc, (Cm,)
        Cm, = twice(rep, name, fn, deterministic=ks == 1)       # K slices meet in fp32 atomics: order-dependent by design
        base = C0[:M, :N].double() if mode else (bias.double() if with_bias else 0.0)
        epi = lambda v: alpha * v + base
        # accumulation bound (its additions include the K slices), one rounding for alpha * acc, one per addition onto bias / C (ks atomic ones)
        babs = base.abs() if torch.is_tensor(base) else 0.0
        bnd = abs(alpha) * R.acc_bound(pb.S, pb.kp, skinny, M, ksplit=ks) + 2 * R.U32 * abs(alpha) * pb.acc.abs() + ks * R.U32 * babs
        rep.bound(f"{name} C", Cm[:M, :N], epi(pb.acc), bnd)
        if mode:
            rep.check(f"{name}: padding written", torch.equal(Cm[:M, N:], C0[:M, N:]) and torch.equal(Cm[M], C0[M]))
        else:
            rep.check(f"{name}: padding written", padding_ok(Cm, M, N))
        rep.check(f"{name}: scratch guard written", sc.guard_ok())
        if pb.x3:
            rep.bound(f"{name} C vs exact", Cm[:M, :N], epi(pb.exact), bnd + abs(alpha) * R.split_product_bound(pb.Sx))
            rep.frob(f"{name} C", Cm[:M, :N], epi, pb)


RUN = {"act": run_act, "resid": run_resid, "dact": run_dact, "f32": run_f32}

# test_gemm_nt_256_row_tiles' list: M ragged against 128 / 160 / 256 / 320, N % 8 == 0 but mostly not % 64, K on the three-stage ring of the
# persistent kernel (K % 192 == 0, K >= 384: 768, 384, 2304), its two-stage ring (1024, 256, 128 is too short), the staggered fallback
# (32, 96, 160, 64), and 6400 x 2048 = more tiles than CUs
SHAPES16 = [(256, 256, 32), (8, 8, 32), (520, 200, 96), (1000, 392, 1024), (300, 776, 160), (640, 512, 64), (330, 248, 128), (520, 776, 768),
            (161, 264, 384), (300, 520, 256), (6400, 2048, 384), (3000, 768, 2304)]
# split-bf16: K by what 3K selects (module docstring)
SHAPES_X3 = [(161, 264, 64), (330, 248, 128), (300, 520, 40), (520, 776, 256), (1000, 392, 96), (256, 200, 32), (6400, 2048, 128)]
TILE_MODES = [-1, 0, 3, 4, 5, 6, 7]
SKINNY_MODES = [1, 2, 3, 4]


def _cases():
    out = []
    for op in ("bf16", "fp16", "x3"):
        for M, N, K in (SHAPES_X3 if op == "x3" else SHAPES16):
            kp = 3 * K if op == "x3" else K
            for kind in RUN:
                for t in TILE_MODES:
                    if (op == "x3" or kind == "dact") and t in (6, 7):
                        continue      # the 160 x 256 kernels do not exist in the split-bf16 build nor for gemm_dact (launch_gemm: can160): tile -1 would run again
                    out.append(pytest.param(op, kind, "tile", t, M, N, K, id=f"{op}-{kind}-tile{t}-{M}x{N}x{K}"))
                if kind != "dact" and kp % 64 == 0 and M <= 1024:       # what the skinny kernels accept; anything else falls to the tile kernels above
                    for s in SKINNY_MODES:
                        out.append(pytest.param(op, kind, "skinny", s, M, N, K, id=f"{op}-{kind}-skinny{s}-{M}x{N}x{K}"))
    return out


@pytest.mark.parametrize("op,kind,which,mode,M,N,K", _cases())
def test_epilogue_on_every_tile_kernel(op, kind, which, mode, M, N, K):
    """every variant of one wrapper's epilogue on one forced tile kernel at one shape; see the module docstring for reference and bounds"""
    pb = problem(op, M, N, K)
    rep = Report(f"{op} {kind} {which}{mode} {M}x{N}x{K}")
    with modes(tile=mode if which == "tile" else -1, skinny=mode if which == "skinny" else -1):
        RUN[kind](rep, pb, skinny=mode if which == "skinny" else 0, tile=mode if which == "tile" else -1)
    rep.done()


@pytest.mark.parametrize("tile", [0, 4, 5, 7])
@pytest.mark.parametrize("op", ["bf16", "fp16", "x3"])
def test_relu_at_exact_zeros(op, tile):
    """acc + bias exactly 0 (zero rows of A, no bias / zero bias): relu (without a pre-activation copy, the form the mapper's fc1 runs, and with
    one) and the stored pre-activation are exactly 0 in both copies of the arithmetic; gemm_dact's relu mask at aux = +0 / -0 is covered by every
    dact1 case above."""
    M, N, K = 161, 264, 128
    pb = Problem(op, M, N, K, zero_rows=True)
    rep = Report(f"{op} zeros tile{tile}")
    with modes(tile=tile):
        run_act(rep, pb, variants=[(1, 0, 0), (2, 0, 0), (1, 1, 0)])
        zb = torch.zeros(N, device="cuda")
        Cm, Cn, Pm = pb.out(N + 8), pb.out(N + 8), pb.out(N + 8)
        sc = Scratch(pb.scratch_bytes)
        rc = [_lib().cc_gemm_act(pb.code, 0, 0, *pb.a_args(), _p(pb.B), pb.ldb, M, N, K, _p(Cn), 0, N + 8, _p(zb), 1, None, *sc.args(), _st()),
              _lib().cc_gemm_act(pb.code, 0, 0, *pb.a_args(), _p(pb.B), pb.ldb, M, N, K, _p(Cm), 0, N + 8, _p(zb), 1, _p(Pm), *sc.args(), _st())]
        torch.cuda.synchronize()
    rep.check(f"rc {rc}", rc == [0, 0])
    rep.check("relu(0 + 0) != 0", bool((Cn[:M:5, :N] == 0).all() and (Cm[:M:5, :N] == 0).all() and (Pm[:M:5, :N] == 0).all()))
    rep.check("with and without pre differ", torch.equal(_bytes(Cn), _bytes(Cm)))
    rep.check("other rows all zero", bool((Cn[1:M:5, :N] != 0).any()))
    rep.done()


def test_measured_allowances():
    """Re-measures the three figures tests/gemm_ref.py cannot derive and prints them (pytest -s): after a compiler or ROCm update, take the
    allowances as 4 x what this prints.  Asserts only that the raw figures are still inside the allowances in force.
      * one MFMA step: K = 32 GEMMs (a single v_mfma_f32_16x16x32 step on a zero accumulator), fp32 output without bias, against the exact
        float64 sum of the 32 products, in units of 2^-24 * sum |terms|; bf16 and fp16, the 128-row and the 256-row kernels;
      * device gelu_new / gelu_new': the split-bf16 build hands the fp32 pre-activation u out through `pre` and the fp32 result through C, so the
        device function is compared with float64 on the very same argument (|u| up to about 30 with a bias of 3 sigma); gelu_new_grad through
        gemm_dact act 2, with the accumulator itself read back through act 3 and aux = 1."""
    l = _lib()
    worst_step = 0.0
    for op in ("bf16", "fp16"):
        for M, N in ((520, 200), (256, 256), (1000, 392)):
            pb = Problem(op, M, N, 32)
            for tile in (0, 3, 4, 5, 6):
                with modes(tile=tile):
                    Cm = pb.out(N + 8, torch.float32)
                    assert l.cc_gemm_f32(pb.code, 0, 0, *pb.a_args(), _p(pb.B), pb.ldb, M, N, 32, _p(Cm), N + 8, None, 0, 1.0, 1, None, 0, _st()) == 0
                step = ((Cm[:M, :N].double() - pb.acc).abs() / (R.U32 * pb.S)).max().item()
                print(f"MEASURED mfma step {op} {M}x{N}x32 tile{tile}: {step:.4f} x 2^-24 sum|terms|")
                worst_step = max(worst_step, step)
    worst_g = worst_dg = 0.0
    for M, N, K in ((520, 776, 64), (1000, 392, 96), (3000, 768, 32)):
        pb = Problem("x3", M, N, K)
        g = torch.Generator(device="cuda").manual_seed(1)
        bias = torch.randn(N, device="cuda", generator=g) * 3
        aux, one = make_aux(pb, 2, N + 8, g), torch.ones(M + 1, N + 8, device="cuda")
        for tile in (0, 4):
            sc = Scratch(pb.scratch_bytes)
            C2, P2, C3, P3, Ca, Cg = (pb.out(N + 8) for _ in range(6))
            common = (*pb.a_args(), _p(pb.B), pb.ldb, M, N, K)
            with modes(tile=tile):
                rcs = [l.cc_gemm_act(2, 0, 0, *common, _p(C2), 0, N + 8, _p(bias), 2, _p(P2), *sc.args(), _st()),
                       l.cc_gemm_act(2, 0, 0, *common, _p(C3), 0, N + 8, _p(bias), 3, _p(P3), *sc.args(), _st()),
                       l.cc_gemm_dact(2, 0, 0, *common, _p(Ca), 0, N + 8, _p(one), 3, *sc.args(), _st()),
                       l.cc_gemm_dact(2, 0, 0, *common, _p(Cg), 0, N + 8, _p(aux), 2, *sc.args(), _st())]
            assert rcs == [0] * 4
            u = P2[:M, :N].double()
            scale = R.U32 * u.abs().clamp_min(1e-30)
            gf = max(((C[:M, :N].double() - R.gelu_new(u)).abs() / scale).max().item() for C in (C2, C3))
            dboth = ((P3[:M, :N].double() - R.gelu_new_grad(u)).abs() / R.U32).max().item()
            acc = Ca[:M, :N].double()
            ref = acc * R.gelu_new_grad(aux[:M, :N].double())
            dgrad = (((Cg[:M, :N].double() - ref).abs() - R.U32 * ref.abs()).clamp_min(0) / (R.U32 * acc.abs().clamp_min(1e-30))).max().item()
            print(f"MEASURED gelu {M}x{N}x{K} tile{tile} |u| <= {u.abs().max().item():.1f}: gelu_new {gf:.3f} x 2^-24 |x|, gelu_new' {dboth:.3f} x 2^-24 "
                  f"(gelu_new_both), {dgrad:.3f} x 2^-24 (gelu_new_grad)")
            worst_g, worst_dg = max(worst_g, gf), max(worst_dg, dboth, dgrad)
    print(f"MEASURED worst: mfma step {worst_step:.3f} (allowance {R.MFMA_ROUNDINGS}), gelu_new {worst_g:.3f} (allowance {R.GELU_ULPS}), "
          f"gelu_new' {worst_dg:.3f} (allowance {R.GELU_GRAD_ULPS})")
    assert worst_step <= R.MFMA_ROUNDINGS and worst_g <= R.GELU_ULPS and worst_dg <= R.GELU_GRAD_ULPS


# ---- split-bf16 only ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("rows,K,ld", [(70, 40, 48), (1, 8, 8), (333, 768, 776), (3000, 6400, 6404)])
def test_x3_split_rows_bit_exact(rows, K, ld, form):
    """k_x3_split_rows against the helper's split, bit for bit: ld > K, and rows * K / 8 below (350, 1, 31968) and above (2.4 M) the 8192 x 256
    units of one grid sweep"""
    g = torch.Generator(device="cuda").manual_seed(rows + K)
    src = torch.full((rows, ld), PAD_VALUE, device="cuda")
    src[:, :K] = torch.randn(rows, K, device="cuda", generator=g) * 37 + 0.3
    src[0, 0], src[0, 1] = 0.0, -0.0
    dst = torch.full((rows + 1, 3 * K), float("nan"), dtype=torch.bfloat16, device="cuda")
    assert _lib().cc_x3_split_rows(2, _p(src), ld, rows, K, form, _p(dst), _st()) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bytes(dst[:rows]), _bytes(R.image(src[:, :K].contiguous(), form)))
    assert torch.isnan(dst[rows].float()).all()
    for code in (0, 1):
        assert _lib().cc_x3_split_rows(code, _p(src), ld, rows, K, form, _p(dst), _st()) == -1


@pytest.mark.parametrize("tile", [0, 3, 4])
@pytest.mark.parametrize("M,N,K", [(161, 264, 64), (300, 520, 40), (520, 776, 256)])
def test_x3_image_output_feeds_the_next_gemm(tile, M, N, K):
    """C written as the consumer's operand image (epi_store8, c_img == N): both hi copies identical, lo within half a bf16 ulp of hi, hi + lo within
    the bound of the reference (+ u^2 |ref| for the split), and that image as the A operand of a second GEMM gives the bytes the plain fp32 C gives"""
    pb, l = Problem("x3", M, N, K), _lib()
    rep = Report(f"x3 image tile{tile} {M}x{N}x{K}")
    g = torch.Generator(device="cuda").manual_seed(5)
    bias = torch.randn(N, device="cuda", generator=g)
    N2 = 72
    B2 = R.image(torch.randn(N2, N, device="cuda", generator=g) * 0.5 + 0.1, 1)
    L1, _ = R.gelu_lipschitz()
    acc_only = R.acc_bound(pb.S, pb.kp, 0, M)
    accb = acc_only + R.U32 * (pb.acc.abs() + bias.double().abs())
    aux = make_aux(pb, 3, N + 8, g)
    a64 = aux[:M, :N].double()
    bhi, blo, _ = R.unimage(B2, 1)
    # (name, the hook call, the epilogue in float64, the error before the store as a function of the reference)
    cases = [("act0", lambda Cm, ci, sc: l.cc_gemm_act(2, 0, 0, *pb.a_args(), _p(pb.B), pb.ldb, M, N, K, _p(Cm), ci, N + 8, _p(bias), 0, None, *sc.args(), _st()),
              lambda v: v + bias.double(), lambda ref: accb),
             ("act2", lambda Cm, ci, sc: l.cc_gemm_act(2, 0, 0, *pb.a_args(), _p(pb.B), pb.ldb, M, N, K, _p(Cm), ci, N + 8, _p(bias), 2, None, *sc.args(), _st()),
              lambda v: R.gelu_new(v + bias.double()), lambda ref: L1 * accb + R.GELU_ULPS * R.U32 * (pb.acc + bias.double()).abs()),
             ("dact3", lambda Cm, ci, sc: l.cc_gemm_dact(2, 0, 0, *pb.a_args(), _p(pb.B), pb.ldb, M, N, K, _p(Cm), ci, N + 8, _p(aux), 3, *sc.args(), _st()),
              lambda v: v * a64, lambda ref: a64.abs() * acc_only + R.U32 * ref.abs())]
    with modes(tile=tile):
        for name, call, epi, err_of in cases:
            ref = epi(pb.acc)
            err = err_of(ref)
            sc = Scratch(pb.scratch_bytes)
            plain = pb.out(N + 8)
            img = torch.full((M + 1, 3 * N), float("nan"), dtype=torch.bfloat16, device="cuda")
            img2 = img.clone()
            rcs = [call(plain, 0, sc), call(img, N, sc), call(img2, N, sc)]
            torch.cuda.synchronize()
            rep.check(f"{name}: rc {rcs}", rcs == [0, 0, 0])
            rep.check(f"{name}: two runs differ", torch.equal(_bytes(img), _bytes(img2)))
            hi, lo, copy = R.unimage(img[:M], 0)
            rep.check(f"{name}: the two hi planes differ", torch.equal(_bytes(hi), _bytes(copy)))
            rep.check(f"{name}: row M of the image written", bool(torch.isnan(img[M].float()).all()))
            _, e = torch.frexp(hi.double().cpu())        # hi = m 2^e, m in [0.5, 1), 8 significant bits: ulp 2^(e - 8)
            rep.check(f"{name}: lo above half an ulp of hi", bool((lo.double().cpu().abs() <= torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - 9).double())).all()))
            rep.bound(f"{name} hi+lo", hi.double() + lo.double(), ref, err + R.U_BF16 ** 2 * ref.abs() * (1 + R.U_BF16))
            rep.frob(f"{name} hi+lo", hi.double() + lo.double(), epi, pb, emulate=lambda v: sum(t.double() for t in R.split(v.float())))
            # second GEMM: [M][N] x [N2][N]^T, A once as the image, once as the same values hi + lo in plain fp32 (exact: 16 significant bits)
            w = torch.full((M, N + 8), PAD_VALUE, device="cuda")
            w[:, :N] = hi.float() + lo.float()
            same = torch.equal(_bytes(R.image(w[:, :N].contiguous(), 0)), _bytes(img[:M]))      # (a lo of exactly half an ulp may re-split differently)
            sc2 = Scratch(image_bytes(M, N))
            o_img, o_plain = pb.out(N2, torch.float32), pb.out(N2, torch.float32)
            rc1 = l.cc_gemm_f32(2, 0, 0, _p(img), N, 0, _p(B2), N, M, N2, N, _p(o_img), N2, None, 0, 1.0, 1, None, 0, _st())
            rc2 = l.cc_gemm_f32(2, 0, 0, _p(w), 0, N + 8, _p(B2), N, M, N2, N, _p(o_plain), N2, None, 0, 1.0, 1, *sc2.args(), _st())
            torch.cuda.synchronize()
            rep.check(f"{name}: second GEMM rc {rc1} {rc2}", rc1 == 0 and rc2 == 0)
            rep.check(f"{name}: image-fed and fp32-fed second GEMM differ", not same or torch.equal(_bytes(o_img), _bytes(o_plain)))
            vw, sw = R.three_term(*R.split(w[:, :N].contiguous()), bhi, blo)
            rep.bound(f"{name} second GEMM fp32-fed", o_plain[:M], vw, R.acc_bound(sw, 3 * N, 0, M))
            v2, s2 = R.three_term(hi, lo, bhi, blo)
            rep.bound(f"{name} second GEMM", o_img[:M], v2, R.acc_bound(s2, 3 * N, 0, M))
            rep.check(f"{name}: scratch guard written", sc.guard_ok() and sc2.guard_ok())
    rep.done()


@pytest.mark.parametrize("ximg", [0, 1])
@pytest.mark.parametrize("mode", [4, 0, -1])
@pytest.mark.parametrize("K,Mw,Nw", [(5120, 768, 1536), (1024, 264, 200), (96, 8, 8), (2080, 520, 776), (12800, 768, 768), (1237, 192, 264)])
def test_x3_wgrad(K, Mw, Nw, mode, ximg):
    """gemm_wgrad in the split-bf16 build at test_gemm_wgrad_kernels' shapes: dW += X^T Y over K' = 3K rows (hi, hi, lo) x (hi, lo, hi), X plain or
    already an image, into a non-zero dW with a padded leading dimension.  Chain: the MFMA steps of all slices, one addition per K slice in the
    slab reduce (a slice is at least 256 deep); then one rounding for the addition into dW."""
    l = _lib()
    rep = Report(f"x3 wgrad mode{mode} ximg{ximg} {K}x{Mw}x{Nw}")
    g = torch.Generator(device="cuda").manual_seed(K + Mw + Nw)
    X = torch.randn(K, Mw, device="cuda", generator=g) + 0.3
    Y = torch.randn(K, Nw, device="cuda", generator=g) * 0.5 + 0.1
    ldx, ldy, ldw = Mw + 4, Nw + 8, Nw + 4
    Xp = torch.full((K, ldx), PAD_VALUE, device="cuda")
    Xp[:, :Mw] = X
    Yp = torch.full((K, ldy), PAD_VALUE, device="cuda")
    Yp[:, :Nw] = Y
    Ximg = R.image(X, 0)
    dW0 = torch.randn(Mw + 1, ldw, device="cuda", generator=g)
    xhi, xlo = R.split(X)
    yhi, ylo = R.split(Y)
    v, s = R.three_term(xhi.t(), xlo.t(), yhi.t(), ylo.t())
    exact = X.double().t() @ Y.double()
    sx = X.double().abs().t() @ Y.double().abs()
    hh = xhi.double().t() @ yhi.double()
    defects = [hh + xhi.double().t() @ ylo.double(), hh + xlo.double().t() @ yhi.double()]
    wscratch = torch.empty(l.cc_wgrad_scratch_bytes(), dtype=torch.uint8, device="cuda")
    sc = Scratch((0 if ximg else image_bytes(K, Mw)) + image_bytes(K, Nw))

    def fn():
        dW = dW0.clone()
        rc = l.cc_gemm_wgrad_split(2, _p(Ximg if ximg else Xp), Mw if ximg else 0, ldx, _p(Yp), ldy, Mw, Nw, K, _p(dW), ldw, _p(wscratch), *sc.args(), _st())
        return rc, (dW,)
    with modes(tile=mode):
        dW, = twice(rep, "wgrad", fn)
    kp = 3 * K
    chain = (-(-kp // R.MFMA_DEPTH_TILE)) * R.MFMA_ROUNDINGS + -(-kp // 256)
    ref0 = dW0[:Mw, :Nw].double()
    bnd = chain * R.U32 * s + R.U32 * (v.abs() + ref0.abs())
    rep.bound("dW", dW[:Mw, :Nw], ref0 + v, bnd)
    rep.bound("dW vs exact", dW[:Mw, :Nw], ref0 + exact, bnd + R.split_product_bound(sx))
    n = exact.norm().item()
    thr = R.frobenius_threshold((v - exact).norm().item() / n, [(d - exact).norm().item() / n for d in defects])
    val = (dW[:Mw, :Nw].double() - ref0 - exact).norm().item() / n
    print(f"FROB {rep.tag} got {val:.3e} threshold {thr:.3e}")
    rep.check(f"relative Frobenius error {val:.3e} > {thr:.3e}", val <= thr)
    rep.check("padding written", torch.equal(dW[:Mw, Nw:], dW0[:Mw, Nw:]) and torch.equal(dW[Mw], dW0[Mw]))
    rep.check("scratch guard written", sc.guard_ok())
    rep.done()


def test_x3_two_gemms_through_one_scratch():
    """the fill mark restarts with every GEMM: a large split followed by a small one in the same scratch gives each the bytes of its own fresh
    scratch, and the scratch is sized for the larger alone"""
    l = _lib()
    big, small = Problem("x3", 520, 200, 256), Problem("x3", 161, 264, 64)
    sc = Scratch(big.scratch_bytes)

    def run(pb, s):
        Cm = pb.out(pb.N + 8)
        rc = l.cc_gemm_act(2, 0, 0, *pb.a_args(), _p(pb.B), pb.ldb, pb.M, pb.N, pb.K, _p(Cm), 0, pb.N + 8, None, 0, None, *s.args(), _st())
        torch.cuda.synchronize()
        assert rc == 0
        return Cm
    shared = [run(big, sc), run(small, sc), run(big, sc)]
    fresh = [run(big, Scratch(big.scratch_bytes)), run(small, Scratch(small.scratch_bytes))]
    assert torch.equal(_bytes(shared[0]), _bytes(fresh[0])) and torch.equal(_bytes(shared[1]), _bytes(fresh[1]))
    assert torch.equal(_bytes(shared[2]), _bytes(fresh[0]))
    assert sc.guard_ok()


def test_x3_error_returns_write_nothing():
    l = _lib()
    pb = Problem("x3", 161, 264, 64)
    M, N, K = pb.M, pb.N, pb.K
    ldc = N + 8
    full = Scratch(pb.scratch_bytes)
    small = Scratch(pb.scratch_bytes - 256)
    aux = make_aux(pb, 3, ldc, torch.Generator(device="cuda").manual_seed(1))
    res = torch.randn(M + 1, ldc, device="cuda")

    def calls(a, al, bl, c_img, sc, B=None, ldb=None):
        B, ldb = (pb.B, pb.ldb) if B is None else (B, ldb)
        Cm, out = pb.out(ldc), torch.full_like(res, float("nan"))
        rcs = [l.cc_gemm_act(2, al, bl, *a, _p(B), ldb, M, N, K, _p(Cm), c_img, ldc, None, 0, None, *sc, _st()),
               l.cc_gemm_dact(2, al, bl, *a, _p(B), ldb, M, N, K, _p(Cm), c_img, ldc, _p(aux), 3, *sc, _st())]
        if not c_img:
            rcs += [l.cc_gemm_resid(2, al, bl, *a, _p(B), ldb, M, N, K, _p(out), _p(res), ldc, None, 0.0, 0, 0, 0, *sc, _st()),
                    l.cc_gemm_f32(2, al, bl, *a, _p(B), ldb, M, N, K, _p(out), ldc, None, 0, 1.0, 1, *sc, _st())]
        torch.cuda.synchronize()
        assert torch.isnan(Cm).all() and torch.isnan(out).all(), "a refused call wrote its output"
        return rcs
    assert calls(pb.a_args(), 0, 0, 0, (None, 0)) == [-4] * 4                  # no scratch
    assert calls(pb.a_args(), 0, 0, 0, small.args()) == [-4] * 4               # one 256-byte unit short
    assert (small.buf == 255).all(), "a refused call wrote its scratch"
    # al / bl != 0 with leading dimensions and buffers that are legal for the K-strided layouts ([K][M], [K][N]): the wrapper's own refusal answers
    big = max(M, N, K) + 8
    At = torch.zeros(big, big, device="cuda")
    Bt = torch.zeros(big, 3 * big, dtype=torch.bfloat16, device="cuda")
    assert calls((_p(At), 0, big), 1, 0, 0, full.args(), Bt, big) == [-1] * 4
    assert calls((_p(At), 0, big), 0, 1, 0, full.args(), Bt, big) == [-1] * 4
    assert calls((_p(At), 0, big), 1, 1, 0, full.args(), Bt, big) == [-1] * 4
    assert calls((_p(pb.Aimg), K + 8, pb.lda), 0, 0, 0, full.args()) == [-1] * 4   # image of another width
    assert calls(pb.a_args(), 0, 0, N + 8, full.args()) == [-1, -1]             # C image of another width
    assert (full.buf == 255).all()
    # an A that already is an image needs no scratch
    Cm = pb.out(ldc)
    assert l.cc_gemm_act(2, 0, 0, *pb.a_args(as_image=True), _p(pb.B), pb.ldb, M, N, K, _p(Cm), 0, ldc, None, 0, None, None, 0, _st()) == 0
    Cp = pb.out(ldc)
    assert l.cc_gemm_act(2, 0, 0, *pb.a_args(), _p(pb.B), pb.ldb, M, N, K, _p(Cp), 0, ldc, None, 0, None, *full.args(), _st()) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bytes(Cm), _bytes(Cp)) and full.guard_ok()
    # wgrad: scratch too small for the second image
    X, Y = torch.randn(96, 8, device="cuda"), torch.randn(96, 8, device="cuda")
    dW = torch.full((8, 8), float("nan"), device="cuda")
    one = Scratch(image_bytes(96, 8))
    assert l.cc_gemm_wgrad_split(2, _p(X), 0, 8, _p(Y), 8, 8, 8, 96, _p(dW), 8, None, *one.args(), _st()) == -4
    assert l.cc_gemm_wgrad_split(2, _p(X), 16, 8, _p(Y), 8, 8, 8, 96, _p(dW), 8, None, *one.args(), _st()) == -1
    torch.cuda.synchronize()
    assert torch.isnan(dW).all() and one.guard_ok()
    # the 16-bit builds take no image and no split, and the old bare hooks keep refusing split-bf16
    A16, B16 = torch.randn(16, 64, device="cuda").bfloat16(), torch.randn(16, 64, device="cuda").bfloat16()
    C16 = torch.full((16, 16), float("nan"), dtype=torch.bfloat16, device="cuda")
    for code in (0, 1):
        assert l.cc_gemm_act(code, 0, 0, _p(A16), 64, 64, _p(B16), 64, 16, 16, 64, _p(C16), 0, 16, None, 0, None, None, 0, _st()) == -1
        assert l.cc_gemm_act(code, 0, 0, _p(A16), 0, 64, _p(B16), 64, 16, 16, 64, _p(C16), 16, 16, None, 0, None, None, 0, _st()) == -1
        assert l.cc_gemm_wgrad_split(code, _p(X), 0, 8, _p(Y), 8, 8, 8, 96, _p(dW), 8, None, None, 0, _st()) == -1
    C32 = torch.full((16, 16), float("nan"), device="cuda")
    assert l.cc_gemm_op16_f32(2, 0, 0, _p(A16), 64, _p(B16), 64, 16, 16, 64, _p(C32), 16, None, 1, _st()) == -1
    assert l.cc_gemm_wgrad(2, _p(A16), 16, _p(B16), 16, 16, 16, 64, _p(C32), 16, None, _st()) == -1
    torch.cuda.synchronize()
    assert torch.isnan(C16.float()).all() and torch.isnan(C32).all()


def _arena_images(eng, mats):
    """(name, offset, rows, cols, has transpose) of every GEMM weight -> checks both images of the 6 * count arena bit for bit"""
    a = eng.arena
    torch.manual_seed(11)
    a.w32.copy_(torch.randn(a.n, device="cuda") * 3 + 0.3)
    a.w16.fill_(float("nan"))
    a.refresh_bf16()
    torch.cuda.synchronize()
    for name, off, Rr, Cc, tr in mats:
        w = a.w32[off:off + Rr * Cc].view(Rr, Cc)
        got = a.w16[3 * off:3 * off + 3 * Rr * Cc].view(Rr, 3 * Cc)
        assert torch.equal(_bytes(got), _bytes(R.image(w.contiguous(), 1))), f"{name}: [hi | lo | hi] image at 3 * offset"
        if tr:
            got_t = a.w16[3 * (a.n + off):3 * (a.n + off) + 3 * Rr * Cc].view(Cc, 3 * Rr)
            assert torch.equal(_bytes(got_t), _bytes(R.image(w.t().contiguous(), 1))), f"{name}: image of the transpose at 3 * (count + offset)"


def test_x3_mapper_sync_weights_arena():
    """k_x3_split_multi behind cc_mapper_sync_weights: weight matrices that are multiples of 64 in neither dimension (D = 72, Hm = 144, E = 40,
    P * D = 216): ragged 64 x 64 tiles in the direct and in the through-LDS transposing form"""
    from clipcap_amd.engine import MapperEngine
    E, D, L, P, H, N = 40, 72, 5, 3, 3, 2
    eng = MapperEngine(E, D, L, P, H, N, device="cuda", precision=32)
    o = eng.offsets
    mats = [("linear.weight", o[0], P * D, E, False)]
    for i in range(N):
        b = 4 + 12 * i
        mats += [(f"layer{i}.wq|wkv", o[b + 2], 3 * D, D, True), (f"layer{i}.wp", o[b + 4], D, D, True),
                 (f"layer{i}.w1", o[b + 8], 2 * D, D, True), (f"layer{i}.w2", o[b + 10], D, 2 * D, True)]
    _arena_images(eng, mats)


def test_x3_gpt2_sync_weights_arena():
    """the same behind cc_gpt2_sync_weights (D = 72: c_attn 72 x 216, c_fc 72 x 288, wte with its zero padding rows up to Vp = 256)"""
    from clipcap_amd.engine import Gpt2Engine
    D, H, NL, V, NPOS = 72, 3, 2, 157, 40
    eng = Gpt2Engine(D, H, NL, V, NPOS, device="cuda", precision=32)
    o = eng.offsets
    mats = [("wte", o[0], eng.dims["Vp"], D, True)]
    for i in range(NL):
        b = 2 + 12 * i
        mats += [(f"h{i}.c_attn", o[b + 2], D, 3 * D, True), (f"h{i}.attn.c_proj", o[b + 4], D, D, True),
                 (f"h{i}.c_fc", o[b + 8], D, 4 * D, True), (f"h{i}.mlp.c_proj", o[b + 10], 4 * D, D, True)]
    _arena_images(eng, mats)
