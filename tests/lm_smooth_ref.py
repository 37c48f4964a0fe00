"""float64 statement of label smoothing in the fused lm_head loss (cc_lmhead_ce_fwd_smooth, cc_lmhead_ce_bwd_smooth) as corrections around
the plain chain of tests/lm_ref.py, the per-element bounds the GPU test holds the kernels of clipcap_amd/csrc/smooth.hip to
(tests/test_gpu_label_smoothing.py), and float64 emulations of the defects those bounds must catch.  tests/test_lm_smooth_ref.py pins this
module on the CPU.

With V real classes, t the row's target, keep = (t != 0), inv = loss_scale / max(denom, 1) (lm_ref's rules) and eps the float32 the
entry points take:
    wbar            = mean over v < V of wte[v]                       (rows V .. Vp - 1 take no part)
    zbar[m]         = hf[m] . wbar                                     (the row's mean logit)
    loss_row(eps)   = loss_row(0) + keep eps (z_t - zbar)
    c[m]            = keep eps inv
    d hf(eps)[m]    = d hf(0)[m] + c[m] (wte[t] - wbar)
    d wte(eps)[t]  += c[m] hf[m]                                       (a row scatter)
    d wte(eps)[v]  -= (sum_m c[m] hf[m]) / V     for v < V             (one vector, broadcast)
on the STORED values: hf in the build's stored type, wte as the lm_head GEMM reads it (the 16-bit operand image; the fp32 master in the
split-bf16 build).  z_t is what CC_LM_TGT names; the GPU test hands the device's own value in, so the GEMM's error stays out.

Rounding model (u32 = 2^-24, u the stored type's unit roundoff; products of two first-order terms: lm_ref.SECOND_ORDER):
  wbar    the two-stage sum of smooth_wbar: a thread adds ceil(rps / 32) rows, 32 row lanes are added in order, then ceil(slices / 16) slices
          per lane group, the 16 groups, and the division: wbar_chain(V) roundings of at most u32 mean |wte[:, d]| (never more than V).
  zbar    D products and D additions in fp32 (the wave tree is part of the D): 2 D u32 sum |hf||wbar|, plus |hf| . (wbar's bound).
  term    eps (z_t - zbar): the errors of both times eps, the subtraction and the product one u32 each.
  stats3  [0] = the plain sum + the sum of the terms: the rows' bounds, one u32 per addition of the fixed-order sum (rows / 1024 + 22, as
          lm_ref charges k_ce_stats) times sum |term|, one u32 of the result.  [1] and [2] are the plain chain's bits.
  c       one division and one product: 2 u32 relative.
  d hf    fl_stored(dhf0 + c (wte[t] - wbar)): c's error, wbar's bound times |c|, the subtraction, the product and the addition one u32 each,
          then ONE stored-type rounding of |d hf(0) + delta| (gemm_ref.store_bound).  Rows with c = 0 are not touched: exact.
  d wte   scatter: value = fl(c hf) (u32), a target's rows added in order (n_t - 1 additions), one addition onto the row.  Broadcast: hsum's
          slice partials (2 ceil(rps / 32) roundings in a thread, 32 row lanes), fold_partials (4 tree levels per 256 slices, 16 lanes), the
          division by V, the subtraction.  Rows >= V: exact, nothing is written.
Nothing here is tuned to what the kernels return."""
import torch

from tests import gemm_ref as G
from tests import lm_ref as LM

U32 = G.U32
SECOND_ORDER = LM.SECOND_ORDER
DEFECTS = ("wbar_over_vp", "inv_vp", "ignored_rows", "no_loss_scale", "no_broadcast")


def eps32(eps):
    """the float32 the C entry points receive"""
    return float(torch.tensor(eps, dtype=torch.float32))


def wte_read(wte, op):
    """wte [V][D] as the kernels read its rows, in float64: the operand type's rounding; the fp32 master in the split-bf16 build"""
    return wte.double() if op == "x3" else wte.to(LM.DT[op]).double()


def wbar_layout(V):
    """(slices, rows per slice) of smooth_wbar (kernels.h smooth_wbar_slices, smooth.hip)"""
    S = max(1, min((V + 127) // 128, 256))
    rps = (-(-V // S) + 31) // 32 * 32
    return -(-V // rps), rps


def wbar_chain(V):
    slices, rps = wbar_layout(V)
    return min(V, -(-rps // 32) + 32 + -(-slices // 16) + 16 + 1)


def hsum_layout(M):
    """(slices, rows per slice) of smooth_dwte_bcast"""
    S = max(1, min((M + 63) // 64, 256))
    rps = (-(-M // S) + 31) // 32 * 32
    return -(-M // rps), rps


def hsum_chain(M):
    slices, rps = hsum_layout(M)
    return 2 * -(-rps // 32) + 32 + 4 * -(-slices // 256) + 16 + 1


def inv_of(c, denom, defect=None):
    ls = 1.0 if (c.ls is None or defect == "no_loss_scale") else c.ls
    return ls / max(denom, 1.0)


def statement(hf_st, wte, tok, c, op, denom, eps, tgt=None, nll=None, wte_pad=None, defect=None):
    """The five lines of the module docstring in float64.  hf_st [B cap][D] in the stored type; wte fp32 master [V][D]; tok int64 [B][cap];
    denom the divisor handed to the backward call; eps a Python float (rounded to float32 here).  tgt [B cap]: the target logit to use
    (default: lm_ref.chain's); nll: the plain loss sum (default: lm_ref.chain's).  wte_pad [Vp - V][D]: what the pad rows of the arena hold
    (only a defect reads them).  defect: one of DEFECTS."""
    dev = hf_st.device
    V, D = wte.shape
    Vp = LM.vp_of(V)
    e = eps32(eps)
    hfd, wr = hf_st.double(), wte_read(wte, op).to(dev)
    tokf = tok.reshape(-1).to(dev)
    tid = tokf.clamp_min(0)
    keep = tid != 0
    if tgt is None or nll is None:
        R0 = LM.chain(hf_st, wte, tok, c, op, denom)
        tgt = R0["tgt"] if tgt is None else tgt
        nll = R0["stats"][0] if nll is None else nll
    tgt = tgt.double().to(dev)
    pad = torch.zeros(Vp - V, D, dtype=torch.float64, device=dev) if wte_pad is None else wte_pad.double().to(dev)
    wbar = wr.mean(0)
    if defect == "wbar_over_vp":
        wbar = torch.cat([wr, pad]).mean(0)
    zbar = hfd @ wbar
    on = torch.ones_like(keep) if defect == "ignored_rows" else keep
    term = on.double() * e * (tgt - zbar)
    crow = on.double() * e * inv_of(c, denom, defect)
    d_dhf = crow.unsqueeze(1) * (wr[tid] - wbar)
    S = dict(eps=e, V=V, Vp=Vp, D=D, keep=keep, tid=tid, tgt=tgt, wr=wr, hfd=hfd, wbar=wbar, zbar=zbar, term=term, crow=crow, d_dhf=d_dhf,
             stats3=torch.stack([torch.as_tensor(nll, dtype=torch.float64, device=dev) + term.sum(), keep.double().sum(),
                                 torch.as_tensor(nll, dtype=torch.float64, device=dev)]))
    if c.mode == 2:
        val = crow.unsqueeze(1) * hfd
        scat = torch.zeros(Vp, D, dtype=torch.float64, device=dev).index_add_(0, tid, val)
        hsum = val.sum(0)
        d = scat.clone()
        if defect != "no_broadcast":
            d[:V] -= hsum / (Vp if defect == "inv_vp" else V)
        S.update(d_dwte=d, scat=scat, hsum=hsum,
                 scat_abs=torch.zeros(Vp, D, dtype=torch.float64, device=dev).index_add_(0, tid, val.abs()),
                 hsum_abs=val.abs().sum(0), n_t=torch.zeros(Vp, dtype=torch.float64, device=dev).index_add_(0, tid, (crow != 0).double()))
    return S


def bounds(S, c, op, dhf0, g0=None, b_tgt=None):
    """per-element bounds of what statement() returns (module docstring).  dhf0 [B cap][D]: d hf of the plain chain (the device's own, so the
    bound is on the CORRECTION); g0 [Vp][D]: the wte rows of g32 after the plain backward (mode 2); b_tgt: the bound of the target logit that
    was handed in (None: it is the device's own value, exact)."""
    V, D, e = S["V"], S["D"], S["eps"]
    Mc = S["hfd"].shape[0]
    keep = S["keep"].double()
    wa, ha = S["wr"].abs(), S["hfd"].abs()
    b_wbar = wbar_chain(V) * U32 * wa.mean(0)
    b_z = 2 * D * U32 * (ha @ S["wbar"].abs()) + ha @ b_wbar
    bt = torch.zeros_like(b_z) if b_tgt is None else b_tgt.double()
    b_term = (S["term"] != 0).double() * (e * SECOND_ORDER * (bt + b_z) + U32 * (2 * S["term"].abs()))
    b_s0 = b_term.sum() + (Mc // 1024 + 22) * U32 * S["term"].abs().sum() + U32 * S["stats3"][0].abs()
    out = dict(wbar=b_wbar, zbar=b_z, term=b_term, stats3=torch.stack([b_s0, torch.zeros_like(b_s0), torch.zeros_like(b_s0)]))
    ca = S["crow"].abs().unsqueeze(1)
    new = dhf0.double() + S["d_dhf"]
    e_dhf = SECOND_ORDER * ca * (b_wbar + 4 * U32 * (wa[S["tid"]] + S["wbar"].abs())) + U32 * new.abs()
    out["d_dhf"] = (ca != 0).double() * G.store_bound(new, e_dhf, LM.DT[op])
    if "d_dwte" in S:
        base = torch.zeros_like(S["d_dwte"]) if g0 is None else g0.double()
        nt = S["n_t"].unsqueeze(1)
        real = torch.zeros(S["Vp"], 1, dtype=torch.float64, device=base.device)
        real[:V] = 1.0
        hit = (nt > 0).double()
        e_sc = hit * ((nt + 3) * U32 * S["scat_abs"] + U32 * (base + S["scat"]).abs())
        e_bc = real * ((hsum_chain(Mc) + 3) * U32 * S["hsum_abs"] / V + U32 * (base + S["d_dwte"]).abs())
        out["d_dwte"] = SECOND_ORDER * (e_sc + e_bc) * (S["crow"] != 0).any().double()
    return out


def leaves_bound(Sd, S, Bd):
    """does a defect emulation Sd leave the bounds Bd around the statement S in any checked quantity?  (quantity name or None)"""
    for k in ("stats3", "d_dhf", "d_dwte"):
        if k not in S:
            continue
        d = (Sd[k] - S[k]).abs()
        if bool((~torch.isfinite(Sd[k])).any()) or bool((d > Bd[k]).any()):
            return k
    return None
