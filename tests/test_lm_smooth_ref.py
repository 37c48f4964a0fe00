"""Pins tests/lm_smooth_ref.py on the CPU: the float64 statement of label smoothing as corrections around lm_ref's plain chain against
autograd of a hand-written smoothed cross-entropy, against F.cross_entropy(label_smoothing=), and with eps = 0 against the oracle's loss on
a golden fixture; the inputs' inventory; and that the bounds reject float64 emulations of each wrong variant."""
import pytest
import torch
import torch.nn.functional as F

from oracle import clipcap_oracle as O
from tests import lm_ref as LM
from tests import lm_smooth_ref as SM
from tests.util import load_golden, sd_of

# (V, D, B, cap, L, mode, denom rule, loss scale): make_tokens gives B >= 3, cap >= 3 shapes a -1 pad tail, a fully padded sample, an id 0 and
# targets shared by every third row
CASES = [LM.Case("a", "flat", 37, 16, 4, 3, 1, 2, 0, "kept", None, 0), LM.Case("b", "flat", 130, 96, 5, 9, 4, 2, 0, "x3", 1024.0, 0),
         LM.Case("c", "flat", 97, 64, 3, 3, 1, 1, 0, "kept", None, 0), LM.Case("d", "flat", 97, 64, 5, 1, 1, 2, 0, "kept", 1024.0, 0)]
OPS = ("fp16", "bf16", "x3")


def _inputs(c, op, all_ignored=False):
    x, gamma, beta, wte, tok = LM.make_inputs(c, op)
    if all_ignored:
        tok = tok.clone()
        tok[:] = -1
        tok[0, 0] = 0
    hf = LM.store(LM.ln_rows(x, gamma, beta, c.B, c.L + c.cap, c.L, c.cap)["hf"], op)
    return hf, wte, tok


def _smoothed_ce(hf64, w64, tid, keep, e):
    """sum over kept rows of (1 - e) nll + e * (mean over the V classes of -log p)"""
    logp = torch.log_softmax(hf64 @ w64.t(), 1)
    row = -(1.0 - e) * logp.gather(1, tid.view(-1, 1)).squeeze(1) - e * logp.mean(1)
    return (row * keep.double()).sum()


def _close(a, b, tol):
    scale = max(1.0, b.abs().max().item()) if b.numel() else 1.0
    assert (a - b).abs().max().item() <= tol * scale if b.numel() else True, (a - b).abs().max().item()


def test_inventory():
    """the inputs carry what the statement must get right: ignored rows with target 0, -1 pads, three rows sharing a target"""
    tok, _ = LM.make_tokens(CASES[1])
    flat = tok.reshape(-1)
    assert (flat == 0).any() and (flat == -1).any() and (tok == -1).all(1).any()
    ids, counts = flat[flat > 0].unique(return_counts=True)
    assert counts.max().item() >= 3
    _, _, tok0 = _inputs(CASES[0], "fp16", all_ignored=True)
    assert (tok0 <= 0).all()


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
@pytest.mark.parametrize("eps", [0.1, 0.5])
def test_statement_equals_autograd_of_a_handwritten_smoothed_loss(c, op, eps):
    """16-bit builds: lm_ref's plain chain is exact float64 algebra on the stored values, so chain + corrections is held to the smoothed
    loss's autograd.  Split-bf16: lm_ref's logits are the three-term products (3 u^2 off the exact ones), so there the corrections are held
    to the DIFFERENCE of the autograd at eps and at 0, with the exact target logit handed in."""
    for all_ignored in (False, True):
        hf, wte, tok = _inputs(c, op, all_ignored)
        denom = LM.denom_of(c, tok)
        inv = SM.inv_of(c, denom)
        tid, keep = tok.reshape(-1).clamp_min(0), tok.reshape(-1) > 0
        grads = {}
        for e in (0.0, SM.eps32(eps)):
            h = hf.double().requires_grad_(True)
            w = SM.wte_read(wte, op).requires_grad_(True)
            total = _smoothed_ce(h, w, tid, keep, e)
            (total * inv).backward()
            grads[e] = (total.detach(), h.grad, w.grad)
        plain, smooth = grads[0.0], grads[SM.eps32(eps)]
        if op == "x3":
            tgt = (hf.double() * SM.wte_read(wte, op)[tid]).sum(1)
            S = SM.statement(hf, wte, tok, c, op, denom, eps, tgt=tgt, nll=plain[0])
            dhf0, dwte0 = plain[1], plain[2]
        else:
            R0 = LM.chain(hf, wte, tok, c, op, denom)
            S = SM.statement(hf, wte, tok, c, op, denom, eps)
            dhf0, dwte0 = R0["dhf"], (R0["dwte"][:c.V] if c.mode == 2 else None)
            _close(S["stats3"][2], R0["stats"][0], 1e-12)
        _close(S["stats3"][0], smooth[0], 1e-12)
        _close(S["stats3"][2], plain[0], 1e-12)
        assert S["stats3"][1].item() == float((tok > 0).sum())
        _close(dhf0 + S["d_dhf"], smooth[1], 1e-12)
        if c.mode == 2:
            _close(dwte0 + S["d_dwte"][:c.V], smooth[2], 1e-12)
            assert (S["d_dwte"][c.V:] == 0).all()
        if all_ignored:
            assert S["stats3"][0].item() == 0.0 and (S["d_dhf"] == 0).all() and torch.isfinite(S["stats3"]).all()


@pytest.mark.parametrize("c", [CASES[0], CASES[2]], ids=lambda c: c.name)
def test_statement_equals_torch_cross_entropy(c):
    """F.cross_entropy(..., ignore_index=0, label_smoothing=eps): the loss to 1e-12, the gradients to 1e-7 (torch rounds eps to fp32 in its
    backward only; the statement takes the fp32 value throughout, so the loss is compared at that value)"""
    op, eps = "fp16", 0.1
    hf, wte, tok = _inputs(c, op)
    denom = float((tok > 0).sum())
    R0 = LM.chain(hf, wte, tok, c, op, denom)
    S = SM.statement(hf, wte, tok, c, op, denom, eps)
    h = hf.double().requires_grad_(True)
    w = SM.wte_read(wte, op).requires_grad_(True)
    loss = F.cross_entropy(h @ w.t(), S["tid"], ignore_index=0, label_smoothing=S["eps"])
    loss.backward()
    _close(S["stats3"][0] / S["stats3"][1], loss.detach(), 1e-12)
    _close(R0["dhf"] + S["d_dhf"], h.grad, 1e-7)
    if c.mode == 2:
        _close(R0["dwte"][:c.V] + S["d_dwte"][:c.V], w.grad, 1e-7)


def test_eps_zero_is_the_oracles_loss_on_the_golden():
    """eps = 0 through the statement = oracle.clipcap_oracle.clipcap_loss on train_prefix_only.  The oracle runs in fp32 (D-term dot
    products, a V-term log-sum-exp): a few 1e-7 relative per row; 1e-5 on a loss of a few units."""
    g = load_golden("train_prefix_only")
    E, D, P, L, H, N, n_head, n_layer, V, npos = [int(v) for v in g["cfg"]]
    sd = sd_of(g)
    tokens, embeds = torch.from_numpy(g["in.tokens"]), torch.from_numpy(g["in.embeds"])
    cfg = dict(projection_length=P, prefix_length=L, heads=H, layers=N, n_head=n_head, n_layer=n_layer)
    with torch.no_grad():
        ref = O.clipcap_loss(sd, tokens, embeds, cfg=cfg)
        prefix = O.mapper_forward(sd, embeds, projection_length=P, num_heads=H, num_layers=N, pre="transformer_mapper.")
        wte = sd["language_model.transformer.wte.weight"]
        x = torch.cat((prefix, wte[tokens.clamp_min(0)]), dim=1)
        hid, _ = O.gpt2_hidden(sd, x, n_head, n_layer, pre="language_model.transformer.")
    B, cap = tokens.shape
    hf = hid[:, L - 1:-1].reshape(B * cap, D)
    c = LM.Case("golden", "flat", V, D, B, cap, L, 1, 0, "kept", None, 0)
    denom = float((tokens > 0).sum())
    S = SM.statement(hf, wte, tokens, c, "x3", denom, 0.0)
    assert abs((S["stats3"][0] / S["stats3"][1]).item() - ref.item()) <= 1e-5
    assert S["stats3"][0].item() == S["stats3"][2].item() and (S["d_dhf"] == 0).all()


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("defect", SM.DEFECTS)
def test_bounds_reject_each_wrong_variant(op, defect):
    """float64 emulations of the wrong variants leave the bounds around the statement; the statement itself stays inside"""
    c = CASES[1]                                  # V = 130: Vp = 256, 126 pad rows; loss scale 1024; mode 2
    hf, wte, tok = _inputs(c, op)
    denom = LM.denom_of(c, tok)
    gen = torch.Generator().manual_seed(3)
    pad = 0.5 + torch.rand(LM.vp_of(c.V) - c.V, c.D, generator=gen)
    R0 = LM.chain(hf, wte, tok, c, op, denom)
    dhf0 = LM.store(R0["dhf"], op)
    S = SM.statement(hf, wte, tok, c, op, denom, 0.1, wte_pad=pad)
    Bd = SM.bounds(S, c, op, dhf0)
    assert SM.leaves_bound(S, S, Bd) is None
    Sd = SM.statement(hf, wte, tok, c, op, denom, 0.1, wte_pad=pad, defect=defect)
    assert SM.leaves_bound(Sd, S, Bd) is not None, defect


def test_bounds_are_small():
    """the bounds describe fp32 / stored-type rounding, not slack: relative to the correction's own size they stay below 2 u of the stored
    type for d hf and 1e-4 for the fp32 quantities"""
    c, op = CASES[1], "bf16"
    hf, wte, tok = _inputs(c, op)
    denom = LM.denom_of(c, tok)
    R0 = LM.chain(hf, wte, tok, c, op, denom)
    S = SM.statement(hf, wte, tok, c, op, denom, 0.1)
    Bd = SM.bounds(S, c, op, LM.store(R0["dhf"], op))
    new = (LM.store(R0["dhf"], op).double() + S["d_dhf"]).abs().max()
    assert Bd["d_dhf"].max() <= 2 * LM.U_OP[op] * new
    assert Bd["d_dwte"].max() <= 1e-4 * S["d_dwte"].abs().max()
    assert Bd["stats3"][0] <= 1e-4 * S["stats3"][0].abs()
