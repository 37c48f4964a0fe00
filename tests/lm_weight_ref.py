"""float64 statement of the fused lm_head loss with a weight per target token (cc_lmhead_ce_fwd_w, cc_lmhead_ce_bwd_w) on top of the plain
chain of tests/lm_ref.py and the smoothing corrections of tests/lm_smooth_ref.py, the per-element bounds the GPU test holds the kernels
to (tests/test_gpu_token_weights.py), the weights both tests use, and float64 emulations of the defects the bounds must catch.
tests/test_lm_weight_ref.py pins this module on the CPU.

With keep = (target != 0), n = the kept rows, inv = loss_scale / max(denom, 1) and wk[m] = keep ? w[m] : 0 BY SELECTION (the weight of a
row that is not kept may be NaN):
    stats3       = [sum_m wk (loss_row(0) + eps (z_t - zbar)),  n,  sum_m loss_row(0)]
    d hf_w[m]    = wk[m] (d hf(0)[m] + c[m] (wte[t] - wbar))                  every row of the input gradient scales with its weight
    d wte_w      = (wk dl)^T hf + the smoothing halves with c[m] wk[m]        dl: lm_ref's d logits of the unweighted loss
A kept row of weight 0 counts in n; the divisor is never the weight sum.

Rounding model (u32 = 2^-24).  The kernels multiply the row factor by the weight ONCE, where "kept" becomes a factor (row_factor in
csrc/kernels.h): fl(inv w) in k_ce_dlogits / k_lm_rowfac, fl(-(eps inv) w) in k_smooth_coef, fl(w row_loss) and fl(w term) on the loss side.  From there on
every row of every intermediate is the unweighted one times w[m], so each stage's own error (the GEMMs', the stores', the scatters')
is at most max |w| times what lm_ref / lm_smooth_ref allow for the unweighted pass (max |w| >= 1 in every weight set here, so the
absolute floors of those bounds hold too), plus:
  stats3[0]  per kept row one u32 for the product with w on the row loss and on the term, the row's own bound times |w|, one u32 per
             addition of each fixed-order block sum (rows / 1024 + 22, as lm_ref charges k_ce_stats) times sum |w loss| resp.
             sum |w term|, the final addition.  The GPU test hands the device's own lse and target logit in, so the row's own bound is
             the one rounding of lse - z_t.
  stats3[1]  exact.      stats3[2]  the plain chain's bound (and its bits, which the GPU test also checks).
  d hf       2 u32 |d hf_w|: fl(inv w) on the softmax gradient, fl(fl(eps inv) w) on the smoothing coefficient: one rounding more than the
             unweighted factor on each half.
  d wte      2 u32 (|wk dl|^T |hf|), the same factor row by row.
Nothing here is tuned to what the kernels return."""
import torch

from tests import lm_ref as LM
from tests import lm_smooth_ref as SM

U32 = LM.U32
DEFECTS = ("weight_sum_divisor", "abs_weight", "zero_weight_not_counted", "ignored_weight_applies", "no_loss_scale",
           "smoothing_unweighted", "nll_weighted")
KINDS = ("ones", "pow2", "general")


# V D B cap L loss_scale: the shapes of the GPU test (the smallest at which these kernels can go wrong, tests/test_gpu_label_smoothing.py)
SHAPES = ((97, 64, 5, 1, 1, None), (130, 96, 15, 9, 4, None), (4099, 256, 130, 1, 1, 1024.0), (130, 256, 257, 9, 4, None))


def case(V, D, B, cap, L, ls, mode):
    return LM.Case(f"V{V}-D{D}-B{B}x{cap}-L{L}-m{mode}", "flat", V, D, B, cap, L, mode, -1, "kept", ls, 0)


def make_tokens(c):
    """lm_ref's tokens; shapes too small for its specials get an id 0 and a -1 pad here, and every case a repeated target"""
    tok, _ = LM.make_tokens(c)
    flat = tok.reshape(-1).clone()
    if not (flat == 0).any():
        flat[1] = 0
    if not (flat == -1).any():
        flat[-1] = -1
    kept = (flat > 0).nonzero().view(-1)
    if len(flat[kept].unique()) == len(kept):
        flat[kept[-1]] = flat[kept[0]]
    return flat.view(c.B, c.cap)


def make_weights(tok, kind, seed=5):
    """fp32 [B][cap] weights for tokens tok (which must hold >= 3 kept rows, a target 0 and a -1 pad).  Every kind: NaN on the first
    ignored row (target 0) and on the first pad, inf on every other row that is not kept.  "ones": 1.0 on every kept row.  "pow2": +-2^k,
    k = -2 .. 3.  "general": mixed sign, magnitudes 10^(-1.5 .. 1.5).  pow2 / general: the first kept row has weight 0, the second a
    negative weight, the third the largest magnitude (8 resp. 31.5, so max |w| >= 1)."""
    flat = tok.reshape(-1).cpu()
    M = flat.numel()
    g = torch.Generator().manual_seed(seed + M)
    kept = (flat > 0).nonzero().view(-1)
    assert len(kept) >= 3 and (flat == 0).any() and (flat == -1).any()
    if kind == "ones":
        w = torch.ones(M)
    else:
        sign = torch.where(torch.rand(M, generator=g) < 0.5, -1.0, 1.0)
        if kind == "pow2":
            mag = 2.0 ** torch.randint(-2, 4, (M,), generator=g).float()
            top = 8.0
        else:
            mag = 10.0 ** (3.0 * torch.rand(M, generator=g) - 1.5)
            top = 31.5
        w = (sign * mag).float()
        w[kept[0]] = 0.0
        w[kept[1]] = -w[kept[1]].abs()
        w[kept[2]] = top
    w[flat <= 0] = float("inf")
    w[(flat == 0).nonzero()[0]] = float("nan")
    w[(flat == -1).nonzero()[0]] = float("nan")
    return w.view(tok.shape)


def statement(hf_st, wte, tok, w, c, op, denom, eps, lse=None, tgt=None, defect=None):
    """The module docstring's lines in float64.  hf_st [B cap][D] in the stored type; wte fp32 master [V][D]; tok int64 [B][cap]; w fp32
    [B][cap]; denom the divisor handed to the backward call; eps a Python float.  lse, tgt [B cap]: the pass's own stored values (default:
    lm_ref.chain's).  defect: one of DEFECTS.  Returns (W, R, S): the weighted statement, lm_ref's chain, lm_smooth_ref's statement."""
    dev = hf_st.device
    R = LM.chain(hf_st, wte, tok, c, op, denom)
    keep = R["keep"]
    tg = R["tgt"] if tgt is None else tgt.double().to(dev)
    if lse is None:
        loss0 = R["loss"]
    else:
        loss0 = torch.where(keep, lse.double().to(dev) - tg, torch.zeros_like(tg))
    S = SM.statement(hf_st, wte, tok, c, op, denom, eps, tgt=tg, nll=loss0.sum())
    wd = w.reshape(-1).double().to(dev)
    wk = torch.where(keep, wd, torch.zeros_like(wd))
    if defect == "ignored_weight_applies":
        wk = wd * keep.double()
    if defect == "abs_weight":
        wk = wk.abs()
    ws = keep.double() if defect == "smoothing_unweighted" else wk           # the weight on the smoothing term and its coefficient
    n = keep.double().sum()
    n_used = n
    if defect == "weight_sum_divisor":
        n_used = wk.sum()
    if defect == "zero_weight_not_counted":
        n_used = (keep & (wd != 0)).double().sum()
    # the caller hands stats3[1] to the backward call: a defect that changes it changes the gradients' divisor with it
    gfac = 1.0 if n_used is n else max(float(denom), 1.0) / max(float(n_used), 1.0)
    if defect == "no_loss_scale" and c.ls is not None:
        gfac = gfac / c.ls
    wl, wt = wk * loss0, ws * S["term"]
    nll = (wk * loss0).sum() if defect == "nll_weighted" else loss0.sum()
    W = dict(wk=wk, keep=keep, loss0=loss0, wl=wl, wt=wt, stats3=torch.stack([wl.sum() + wt.sum(), n_used, nll]),
             dhf=gfac * (wk.unsqueeze(1) * R["dhf"] + ws.unsqueeze(1) * S["d_dhf"]))
    if c.mode == 2:
        V, Vp = S["V"], S["Vp"]
        hfd = R["hfd"]
        full = torch.zeros(Vp, c.D, dtype=torch.float64, device=dev)
        full[:V] = (wk.unsqueeze(1) * R["dl"]).t() @ hfd
        mag = torch.zeros_like(full)
        mag[:V] = (wk.unsqueeze(1) * R["dl"]).abs().t() @ hfd.abs()
        val = (ws * S["crow"]).unsqueeze(1) * hfd
        sm = torch.zeros_like(full).index_add_(0, S["tid"], val)
        sm[:V] -= val.sum(0) / V
        W.update(dwte=gfac * (full + sm), dwte_mag=mag)
    return W, R, S


def wmax_of(W):
    return float(W["wk"].abs().max())


def bounds(W, R, S, c, op, dhf0=None, pre=None, own_rows=False):
    """per-element bounds of what statement() returns (module docstring).  dhf0 [B cap][D]: d hf of the UNWEIGHTED pass in the stored type
    (what lm_smooth_ref.bounds takes; default: lm_ref.chain's, stored); pre [Vp][D]: the wte rows of g32 before the backward call (mode 2);
    own_rows: lse and the target logit were the pass's own, so a row's loss carries the one rounding of its subtraction only."""
    Bl = LM.bounds(R, c, op)
    eps_on = S["eps"] != 0.0
    dhf0 = LM.store(R["dhf"], op) if dhf0 is None else dhf0
    Bs = SM.bounds(S, c, op, dhf0, g0=pre) if eps_on else None
    Mc = W["wk"].numel()
    wa = W["wk"].abs()
    wmax = max(wmax_of(W), 1.0)
    b_row = U32 * W["loss0"].abs() if own_rows else Bl["loss"]
    chain = (Mc // 1024 + 22) * U32
    b0 = (wa * b_row).sum() + (U32 + chain) * W["wl"].abs().sum() + U32 * W["stats3"][0].abs()
    if eps_on:
        b0 = b0 + (wa * Bs["term"]).sum() + (U32 + chain) * W["wt"].abs().sum() + U32 * W["wl"].sum().abs()
    b2 = b_row.sum() + chain * W["loss0"].abs().sum()
    out = dict(stats3=torch.stack([b0, torch.zeros_like(b0), b2]))
    b_dhf = wmax * Bl["dhf"] + 2 * U32 * W["dhf"].abs()
    if eps_on:
        b_dhf = b_dhf + wmax * Bs["d_dhf"]
    out["dhf"] = b_dhf * W["keep"].double().unsqueeze(1)                    # a row that is not kept is exactly zero
    if "dwte" in W:
        p = torch.zeros_like(W["dwte"]) if pre is None else pre.double()
        b = wmax * LM.dwte_bound(R, Bl, p) + 2 * U32 * W["dwte_mag"]
        if eps_on:
            b = b + wmax * Bs["d_dwte"]
        out["dwte"] = b
    return out


def leaves_bound(Wd, W, Bd):
    """does a defect emulation Wd leave the bounds Bd around the statement W in any checked quantity?  (quantity name or None)"""
    for k in ("stats3", "dhf", "dwte"):
        if k not in W:
            continue
        d = (Wd[k] - W[k]).abs()
        if bool((~torch.isfinite(Wd[k])).any()) or bool((d > Bd[k]).any()):
            return k
    return None
