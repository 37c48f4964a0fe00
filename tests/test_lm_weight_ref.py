"""Pins tests/lm_weight_ref.py on the CPU: the float64 statement of the loss with per-token weights against autograd of a hand-written
weighted (and smoothed) cross-entropy, the inventory of the tokens and weights, and that the bounds reject float64 emulations of each
wrong variant at the shapes the GPU test runs."""
import pytest
import torch

from tests import lm_ref as LM
from tests import lm_smooth_ref as SM
from tests import lm_weight_ref as WR

OPS = ("fp16", "bf16", "x3")
_IDS = [f"V{s[0]}-D{s[1]}-B{s[2]}x{s[3]}" for s in WR.SHAPES]
_CACHE = {}


def _inputs(c, op):
    key = (c.V, c.D, c.B, c.cap, c.L, op)
    if key not in _CACHE:
        x, gamma, beta, wte, _ = LM.make_inputs(c, op)
        tok = WR.make_tokens(c)
        hf = LM.store(LM.ln_rows(x, gamma, beta, c.B, c.L + c.cap, c.L, c.cap)["hf"], op)
        _CACHE[key] = (hf, wte, tok)
    return _CACHE[key]


def _close(a, b, tol):
    scale = max(1.0, b.abs().max().item())
    assert (a - b).abs().max().item() <= tol * scale, (a - b).abs().max().item()


@pytest.mark.parametrize("shape", WR.SHAPES, ids=_IDS)
def test_inventory(shape):
    """every case: ignored rows, -1 pads, a repeated target, a kept row of weight 0, a negative weight, NaN on an ignored row and on a pad,
    max |w| >= 1; the power-of-two set holds nothing but 0 and +-2^k, k = -2 .. 3"""
    c = WR.case(*shape, 2)
    tok = WR.make_tokens(c)
    flat = tok.reshape(-1)
    keep = flat > 0
    assert (flat == 0).any() and (flat == -1).any() and len(flat[keep].unique()) < int(keep.sum())
    for kind in ("pow2", "general"):
        w = WR.make_weights(tok, kind).reshape(-1)
        assert (w[keep] == 0).any() and (w[keep] < 0).any() and (w[keep] > 0).any() and w[keep].abs().max() >= 1
        assert torch.isfinite(w[keep]).all() and not torch.isfinite(w[~keep]).any()
        assert torch.isnan(w[flat == 0]).any() and torch.isnan(w[flat == -1]).any()
    p = WR.make_weights(tok, "pow2").reshape(-1)[keep]
    k = torch.log2(p[p != 0].abs())
    assert (k == k.round()).all() and k.min() >= -2 and k.max() <= 3
    g = WR.make_weights(tok, "general").reshape(-1)[keep]
    if keep.sum() > 50:
        m = g[g != 0].abs()
        assert m.max() / m.min() >= 100          # spread over (nearly) three decades
    o = WR.make_weights(tok, "ones").reshape(-1)
    assert (o[keep] == 1).all() and torch.isnan(o[flat == 0]).any()


@pytest.mark.parametrize("op", ("fp16", "bf16"))
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("shape", WR.SHAPES[:2], ids=_IDS[:2])
def test_statement_equals_autograd_of_a_handwritten_weighted_loss(shape, eps, mode, op):
    """16-bit builds, where lm_ref's chain is exact float64 algebra on the stored values (the split-bf16 chain carries the three-term
    products' 3 u^2, which lm_ref's own test accounts for): loss, d hf and d wte of sum_kept w ((1 - e) nll + e mean(-log p)) / n"""
    c = WR.case(*shape, mode)
    hf, wte, tok = _inputs(c, op)
    w = WR.make_weights(tok, "general")
    denom = LM.denom_of(c, tok)
    W, R, S = WR.statement(hf, wte, tok, w, c, op, denom, eps)
    tid, keep = tok.reshape(-1).clamp_min(0), tok.reshape(-1) > 0
    e = SM.eps32(eps)
    h = hf.double().requires_grad_(True)
    wt = SM.wte_read(wte, op).requires_grad_(True)
    logp = torch.log_softmax(h @ wt.t(), 1)
    row = -(1.0 - e) * logp.gather(1, tid.view(-1, 1)).squeeze(1) - e * logp.mean(1)
    wk = torch.where(keep, w.reshape(-1).double(), torch.zeros(keep.numel(), dtype=torch.float64))
    total = (wk[keep] * row[keep]).sum()
    (total * SM.inv_of(c, denom)).backward()
    _close(W["stats3"][0], total.detach(), 1e-12)
    assert W["stats3"][1].item() == float(keep.sum())
    _close(W["stats3"][2], -logp.detach().gather(1, tid.view(-1, 1)).squeeze(1)[keep].sum(), 1e-12)
    _close(W["dhf"], h.grad, 1e-12)
    assert (W["dhf"][~keep] == 0).all() and torch.isfinite(W["dhf"]).all()
    if mode == 2:
        _close(W["dwte"][:c.V], wt.grad, 1e-12)
        assert (W["dwte"][c.V:] == 0).all()


@pytest.mark.parametrize("op", OPS)
def test_unit_weights_are_the_unweighted_statements(op):
    c = WR.case(*WR.SHAPES[1], 2)
    hf, wte, tok = _inputs(c, op)
    denom = LM.denom_of(c, tok)
    W, R, S = WR.statement(hf, wte, tok, WR.make_weights(tok, "ones"), c, op, denom, 0.1)
    assert torch.equal(W["dhf"], R["dhf"] + S["d_dhf"]) and torch.equal(W["stats3"][1:], S["stats3"][1:])
    _close(W["stats3"][0], S["stats3"][0], 1e-14)
    _close(W["dwte"], R["dwte"] + S["d_dwte"], 1e-12)


# a missing loss scale can show only at the shape that runs with one
_PAIRS = [(d, s) for d in WR.DEFECTS for s in WR.SHAPES if not (d == "no_loss_scale" and s[5] is None)]


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("defect,shape", _PAIRS, ids=[f"{d}-V{s[0]}-D{s[1]}-B{s[2]}x{s[3]}" for d, s in _PAIRS])
def test_bounds_reject_each_wrong_variant(defect, shape, op):
    """float64 emulations of the wrong variants leave the bounds around the statement at every shape of the GPU test; the statement itself
    stays inside.  An unweighted smoothing term can show only where eps > 0."""
    c = WR.case(*shape, 2)
    hf, wte, tok = _inputs(c, op)
    denom = LM.denom_of(c, tok)
    for kind in ("pow2", "general"):
        w = WR.make_weights(tok, kind)
        for eps in ((0.1,) if defect == "smoothing_unweighted" else (0.0, 0.1)):
            W, R, S = WR.statement(hf, wte, tok, w, c, op, denom, eps)
            Bd = WR.bounds(W, R, S, c, op)
            assert WR.leaves_bound(W, W, Bd) is None
            Wd, _, _ = WR.statement(hf, wte, tok, w, c, op, denom, eps, defect=defect)
            assert WR.leaves_bound(Wd, W, Bd) is not None, (defect, kind, eps)


def test_bounds_are_small():
    """the bounds describe rounding, not slack: the loss sums to 1e-4 of the sum of the |terms| (lm_ref's own
    bound of a row loss is the larger part), d hf to 4 u of the stored type times
    max |w| relative to the largest unweighted gradient element"""
    c, op = WR.case(*WR.SHAPES[1], 2), "bf16"
    hf, wte, tok = _inputs(c, op)
    denom = LM.denom_of(c, tok)
    W, R, S = WR.statement(hf, wte, tok, WR.make_weights(tok, "general"), c, op, denom, 0.1)
    Bd = WR.bounds(W, R, S, c, op)
    assert Bd["stats3"][0] <= 1e-4 * (W["wl"].abs().sum() + W["wt"].abs().sum())
    assert Bd["stats3"][1] == 0
    assert Bd["dhf"].max() <= 4 * LM.U_OP[op] * WR.wmax_of(W) * (R["dhf"] + S["d_dhf"]).abs().max()
