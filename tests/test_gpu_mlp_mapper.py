"""The MLP mapping network's engine (clipcap_amd.engine.MlpMapperEngine on cc_mlp_*; clipcap_amd/csrc/mlp.hip) stage by stage against float64
(tests/mlp_ref.py), in all three operand builds.

After forward(save=True) and backward(dout) the saved fields x16, h, t, g16, dU are read back with cc_mlp_get and EVERY stage is checked
against float64 fed with the device's own upstream values, so each is held to its own bound and none is tuned:
    x16, g16   equal to the cast, bit for bit
    h, t       the tanh epilogue: acc_bound over E (3 E) products + 2^-24 |u| for the bias, then tests/mlp_ref.py's measured allowances
    out        acc_bound over Hd products + one rounding for the bias
    dW2, dW1   mlp_ref.wgrad_bound: MFMA steps over B products, the slab fold, the addition into the gradient arena
    dU         |t| acc_bound over L D products + one rounding for the multiplication, then the store
    db2, db1   fp32 sums over the batch: rows * 2^-24 * sum |terms|
Shapes: (E, D, L) = (24, 32, 3) and (16, 40, 10) (Hd = 48 / 200: sub-tile and ragged against every tile), B = 1, 5, 130 (one row, an odd
count, more than one 128-row tile)."""
import ctypes as C

import pytest
import torch

from tests import gemm_ref as R
from tests import mlp_ref as MR

pytestmark = pytest.mark.gpu

DIMS = [(24, 32, 3), (16, 40, 10)]
BATCHES = [1, 5, 130]
PRECISIONS = {"bf16": (None, 0), "fp16": (16, 1), "x3": (32, 2)}


def _engine(E, D, L, prec):
    from clipcap_amd.engine import MlpMapperEngine
    eng = MlpMapperEngine(E, D, L, device="cuda", precision=PRECISIONS[prec][0])
    g = torch.Generator().manual_seed(E * 100 + D + L)
    v = eng.views(eng.arena.w32)
    v["model.0.weight"].copy_(torch.randn(v["model.0.weight"].shape, generator=g) * (1.5 / E ** 0.5))
    v["model.0.bias"].copy_(torch.randn(v["model.0.bias"].shape, generator=g))
    v["model.2.weight"].copy_(torch.randn(v["model.2.weight"].shape, generator=g) * (1.0 / eng.dims["Hd"] ** 0.5))
    v["model.2.bias"].copy_(torch.randn(v["model.2.bias"].shape, generator=g) * 0.3)
    return eng


@pytest.fixture(scope="module")
def engines():
    cache = {}

    def get(E, D, L, prec):
        if (E, D, L, prec) not in cache:
            cache[(E, D, L, prec)] = _engine(E, D, L, prec)
        return cache[(E, D, L, prec)]
    return get


def _inputs(E, D, L, B):
    g = torch.Generator().manual_seed(B * 7 + E)
    emb = torch.randn(B, E, generator=g).cuda()
    dout = (torch.randn(B, L, D, generator=g) * 0.1).cuda()
    return emb, dout


def _ratio(name, got, ref, bound, fails):
    got = got.double()
    if not torch.isfinite(got).all():
        fails.append(f"{name}: non-finite")
        return
    r = ((got - ref).abs() / bound.clamp_min(1e-300)).max().item()
    print(f"RATIO {name} {r:.4f}")
    if r > 1.0:
        fails.append(f"{name}: error / bound = {r:.3f}")


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("E,D,L", DIMS)
@pytest.mark.parametrize("prec", list(PRECISIONS))
def test_every_stage_against_float64(engines, prec, E, D, L, B):
    eng = engines(E, D, L, prec)
    dt = MR.DTYPES[PRECISIONS[prec][1]]
    Hd, LD = eng.dims["Hd"], L * D
    emb, dout = _inputs(E, D, L, B)
    w = {k: v.detach().clone() for k, v in eng.views(eng.arena.w32).items()}
    W1, b1, W2, b2 = (w[n] for n in eng.NAMES)
    out = eng.forward(emb, save=True)
    eng.arena.grads().zero_()
    eng.backward(dout)
    torch.cuda.synchronize()
    x16, h, t, g16, dU = (eng.get(B, f) for f in range(5))
    gv = eng.views(eng.arena.g32)
    fails = []
    tag = f"{prec} E{E} D{D} L{L} B{B}"
    assert x16.dtype == dt and h.shape == (B, Hd) and g16.shape == (B, LD)
    # casts
    if not torch.equal(x16, MR.cast(emb, dt)):
        fails.append("x16 is not the cast of emb")
    if not torch.equal(g16, MR.cast(dout.reshape(B, LD), dt)):
        fails.append("g16 is not the cast of dout")
    # h, t from the device's x16
    acc, S, kp = MR.nt(x16, W1, dt)
    u = acc + b1.double()
    err_u = R.acc_bound(S, kp, 0, B) + R.U32 * u.abs()
    _ratio(f"{tag} h", h, MR.tanh(u), R.store_bound(MR.tanh(u), MR.TANH_LIP * err_u + MR.TANH_ULPS * R.U32, dt), fails)
    _ratio(f"{tag} t", t, MR.tanh_grad(u), R.store_bound(MR.tanh_grad(u), MR.TANH_GRAD_LIP * err_u + MR.TANH_GRAD_ULPS * R.U32, dt), fails)
    # out from the device's h
    acc, S, kp = MR.nt(h, W2, dt)
    ref = acc + b2.double()
    _ratio(f"{tag} out", out.reshape(B, LD), ref, R.acc_bound(S, kp, 0, B) + R.U32 * ref.abs(), fails)
    # db2: fp32 sum of dout over the batch
    d64 = dout.reshape(B, LD).double()
    _ratio(f"{tag} db2", gv["model.2.bias"], d64.sum(0), B * R.U32 * d64.abs().sum(0) + 1e-300, fails)
    # dW2 = g16^T h
    v, S, kp = MR.tn(g16, h, dt)
    _ratio(f"{tag} dW2", gv["model.2.weight"], v, MR.wgrad_bound(S, kp, v, torch.zeros_like(v)) + 1e-300, fails)
    # dU = (g16 W2) * t: the NT GEMM reads the transposed copy of W2
    acc, S, kp = MR.nt(g16, W2.t().contiguous(), dt)
    t64 = t.double()
    ref = acc * t64
    _ratio(f"{tag} dU", dU, ref, R.store_bound(ref, t64.abs() * R.acc_bound(S, kp, 0, B) + R.U32 * ref.abs(), dt) + 1e-300, fails)
    # dW1 = dU^T x16, db1 = column sums of dU (the stored values)
    v, S, kp = MR.tn(dU, x16, dt)
    _ratio(f"{tag} dW1", gv["model.0.weight"], v, MR.wgrad_bound(S, kp, v, torch.zeros_like(v)) + 1e-300, fails)
    u64 = dU.double()
    _ratio(f"{tag} db1", gv["model.0.bias"], u64.sum(0), B * R.U32 * u64.abs().sum(0) + 1e-300, fails)
    assert not fails, f"{tag}: " + "; ".join(fails)


@pytest.mark.parametrize("prec", list(PRECISIONS))
def test_bitwise_properties(engines, prec):
    """save=False forward == save=True forward; two identical forward + backward runs give identical gradient bits; a second backward doubles
    the gradient arena exactly (every pass ACCUMULATES); with a hook the two spans are [off(model.2.weight), n) then [0, off(model.2.weight)),
    and the gradients equal the hook-less ones bit for bit."""
    E, D, L, B = 16, 40, 10, 130
    eng = engines(E, D, L, prec)
    emb, dout = _inputs(E, D, L, B)
    a = eng.arena

    def run(hook=None, times=1):
        out = eng.forward(emb, save=True)
        a.grads().zero_()
        for _ in range(times):
            eng.backward(dout, on_layers_done=hook)
        torch.cuda.synchronize()
        return out.clone(), a.g32.clone()
    o0 = eng.forward(emb, save=False).clone()
    o1, g1 = run()
    o2, g2 = run()
    assert torch.equal(o0, o1) and torch.equal(o1, o2)
    assert torch.equal(g1, g2) and float(g1.abs().sum()) > 0
    _, gd = run(times=2)
    assert torch.equal(gd, 2 * g1)
    spans = []
    _, gh = run(hook=lambda lo, hi: spans.append((lo, hi)))
    cut = eng.offsets[2]
    assert spans == [(cut, a.n), (0, cut)] and 0 < cut < a.n
    assert torch.equal(gh, g1)


def test_input_shapes_and_refusals():
    from clipcap_amd import _lib
    from clipcap_amd.engine import MlpMapperEngine
    eng = MlpMapperEngine(24, 32, 3, device="cuda")
    with pytest.raises(ValueError):
        eng.forward(torch.randn(2, 3, 24, device="cuda"))          # windowed input
    with pytest.raises(ValueError):
        eng.forward(torch.randn(2, 32, device="cuda"))
    with pytest.raises(RuntimeError):
        eng.backward(torch.randn(7, 3, 32, device="cuda"))          # no saving forward at this batch
    l = _lib.lib()
    a = eng.arena
    ws = eng._workspace(2, 1)
    emb = torch.randn(2, 24, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    out = torch.full((2, 96), float("nan"), device="cuda")
    assert l.cc_mlp_fwd(C.byref(eng.cfg), 0, p(a.w32), p(a.w16), p(emb), p(ws), p(out), 1, None) == -1
    assert l.cc_mlp_fwd(C.byref(eng.cfg), 2, p(a.w32), p(a.w16), None, p(ws), p(out), 1, None) == -1
    assert l.cc_mlp_bwd_part(C.byref(eng.cfg), 2, p(a.w32), p(a.w16), p(ws), p(out), p(a.grads()), 2, None) == -1
    assert l.cc_mlp_get(C.byref(eng.cfg), 2, p(ws), 5, p(out), 8, None) == -1
    assert l.cc_mlp_get(C.byref(eng.cfg), 2, p(ws), 1, p(out), 8, None) == -2
    bad = _lib.MlpCfg(E=24, D=32, L=3, Hd=48, op_dtype=1)          # a config of another operand mode than the arena's is still a valid config
    assert l.cc_mlp_param_count(C.byref(bad)) == a.n
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    assert eng.arena.w16.numel() == 2 * a.n
    eng.set_precision(32)
    assert eng.arena.w16.numel() == 6 * a.n
    assert l.cc_mlp_transpose_weights(C.byref(eng.cfg), p(eng.arena.w16), None) == -1
