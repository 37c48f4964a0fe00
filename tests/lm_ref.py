"""float64 reference of the fused ln_f -> lm_head -> softmax cross-entropy -> input / weight gradient chain (cc_lmhead_ce_fwd, cc_lmhead_ce_bwd,
cc_lmhead_score), the per-element bounds the GPU test holds it to (tests/test_gpu_lm_head.py), float64 emulations of the defects the
bounds must catch, and the case list both tests walk.  Plain torch on whatever device the inputs live on; tests/test_lm_ref.py pins this
module itself on the CPU.

The reference takes the STORED values the kernels multiply: hf rounded to the build's stored type (fp32 in the split-bf16 build, where the
GEMM sees its hi / lo split), wte rounded to the operand type (hi / lo split; the fp32 master row where k_lm_tgt_ref / k_lm_rows /
k_deepk_finish_lm read it).  The ln_f backward reference takes the device's own dhf (read back through cc_lmhead_get), so a GEMM defect
can neither hide in ln_bwd nor be blamed on it.

Forms (api.hip lm_exp_form): bf16 training and split-bf16 mode 1 run the EXPONENTIAL form, fp16 training and split-bf16 mode 2 the LOGIT
form, scoring (mode 0) the store-free logit form in every build.

Rounding model (u32 = 2^-24, u = the stored type's unit roundoff, t3 = 3 * 2^-16 the three-term product error, gemm_ref):
  logit         dz = gemm_ref.acc_bound(sum |hf||wte|, D or 3 D): fp32 accumulation only, operand products are exact.
  target logit  logit form: the epilogue's fp32 accumulator, error dz.  Exponential form: cref, a VALU dot product of D terms in fp32:
                2 D roundings of at most u32 sum |hf||wte[t]| (one per product, one per addition), against the exact dot product of the
                same stored values (split-bf16: hf times the fp32 master row, so the GEMM's logit differs from it by t3 sum |hf||wte| more).
  exponents     every exp argument x carries its inputs' errors dx; exp turns that into the relative error expm1(dx), plus the device
                function's own error, a MEASURED allowance (below) times u32 (1 + |x|) — v_exp_f32 of x log2(e): the product's rounding
                grows with |x|.  Exponential form: y = logit - cref, dy = dz + dcref + u32 (2 |z| + 2 |cref| + |y|) (log2(e) as a rounded
                constant on both terms, the fma's one rounding).
  row sum       the softmax-weighted mean of the per-column relative errors, plus one u32 per addition on the longest chain: 16 + 2 in a
                lane and its shuffles, max(16, ceil(npart / 64)) + 6 in the fold, one multiplication by exp(pmax - m).
  lse           m + logf(s): LOGF_ULPS u32 max(1, |log s|) + u32 (|lse| + |m|).
  loss, logprob lse - target: both errors + u32 |loss|.  stats / sample_stats: the sum of their rows' bounds + one u32 per addition of the
                fixed-order sum (rows / 1024 + 6 + 16, cap / 64 + 7) times sum |terms|.
  logit-form gradient   dl = (exp(zs - lse) - onehot) w with zs the STORED logit: u |z| + (1 + u) dz (fp16: + 2^-25) in the exponent, the
                device lse's own error, the subtraction's rounding — the bound scales with |logit|, which is why the offset family stops at
                +64 in fp16.  Then the one-hot subtraction, the multiplication by w (w itself one division), the 16-bit store.
  exponential-form gradient   dhf = r sum_v Es wte - w wte[t], r = exp(cref - lse) w, Es = E rounded once to 16 bits (split-bf16: to its
                hi + lo image, 2^-16).  r E_v = w p_v, so every term is w p_v |wte| times (E's relative error + r's + u); r's exponent
                carries the errors of lse and cref.
  dhf sum       gemm_ref.acc_bound over Vp (3 Vp) products with one fp32 addition per K slab (deep-K), finishing pass: 3 u32; the
                fallback (deepk_slabs: tile mode 0, or Vp too shallow for two slabs) stores sum Es wte to the stored type BEFORE the fix: one more u.
  dwte          the same per-element gradient errors through dl^T hf; exponential form: r hf rounded to 16 bits (u), E times fp32's
                smallest normal (r hf flushes below it); K = rows, at most rows / 64 + 1 slice additions; two accumulations into g32.
  ln_f          mean / rstd from fp32 VALU sums of D terms (2 D roundings each); see ln_bounds / ln_bwd_bounds.
Products of two first-order terms are covered by SECOND_ORDER.  None of this is tuned to what the kernels return.

Measured allowances (4 x the worst value seen on the MI355X, printed raw by
`pytest tests/test_gpu_lm_head.py -m gpu -s -k test_measured_allowances`):
  exp at arguments in [-80, 0] (row statistics, ce_row_fold, k_ce_dlogits, k_lm_rowfac): attn_ref.EXP_ULPS, the same instruction over the
      same range.
  EXP2_POS_ULPS   EpiLMHeadExp's v_exp_f32 at POSITIVE arguments up to 80 log2(e).  E leaves the kernel only rounded to 16 bits, so the
      figure is taken from lse of rows whose sum is one column (cref = 0, every other column 200 below it):
      |lse_dev - log(1 + e^y)| / (u32 (1 + y)), y = 0.5 .. 80: worst seen 3.1475 -> 12.6.  It contains logf's error as well and is
      charged to exp2 alone: an upper figure.
  LOGF_ULPS       k_ce_rows / k_score_rows call logf, not __logf: lse = logf(k) of rows with k equal columns (every other column 200
      below), k = 1 .. 97: |lse_dev - log k| / (u32 max(1, log k)): worst seen 2.3297 -> 9.3 (the figure __logf gave attn_ref).
"""
import collections
import math

import torch

from tests import attn_ref as A
from tests import gemm_ref as G

U32 = G.U32
SECOND_ORDER = A.SECOND_ORDER
DT = A.DT
U_OP = A.U_OP
T3 = 3.0 * G.U_BF16 ** 2
FP32_MIN_NORMAL = 2.0 ** -126
CLAMP = 80.0
EXP_ULPS = A.EXP_ULPS
# raw worst figures of test_measured_allowances on the MI355X and 4 x them (see the module docstring)
EXP2_POS_RAW, EXP2_POS_ULPS = 3.1475, 12.6
LOGF_RAW, LOGF_ULPS = 2.3297, 9.3

# Every bound grows with the two allowances, so a defect that leaves the bounds at CEILING leaves them at every smaller value: tests/test_lm_ref.py
# shows the separation at the ceiling (64 x what the same instructions measured on other ranges), and once the figures above exist it uses
# them and requires them to lie below it (measured: 12.6 and 9.3 against a ceiling of 294 and 595).
ALLOW_CEILING = (64.0 * A.EXP_ULPS, 64.0 * A.LOG_ULPS)

OPS = ("bf16", "fp16", "x3")
FAMILIES = ("flat", "confident", "wrong", "offset", "beyond")
OFFSET = {"bf16": 300.0, "fp16": 64.0, "x3": 300.0}


def form_of(op, mode):
    if mode == 0:
        return "score"
    if op == "bf16" or (op == "x3" and mode == 1):
        return "exp"
    return "logit"


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name family V D B cap L mode tile denom ls iz")
# family V D B cap L tile denom loss_scale: the smallest shapes at which each path exists (paths(): case -> kernel)
_TRAIN = (("flat", 97, 64, 5, 1, 1, 0, "kept", None), ("confident", 130, 96, 15, 9, 4, 7, "x3", None),
          ("wrong", 97, 256, 29, 9, 4, 4, "kept", None), ("beyond", 4099, 64, 330, 1, 1, 5, "kept", None),
          ("offset", 4099, 96, 15, 9, 1, 3, "zero", None), ("confident", 65601, 64, 5, 1, 1, 0, "kept", None),
          ("flat", 65601, 64, 1, 1, 4, 6, "kept", None), ("wrong", 65601, 64, 2, 3, 1, 4, "kept", None),
          ("beyond", 130, 64, 37, 9, 1, 4, "x3", 1024.0), ("offset", 130, 256, 257, 1, 4, 0, "kept", None),
          ("confident", 4099, 256, 130, 1, 1, 4, "kept", 1024.0), ("wrong", 4099, 64, 15, 9, 4, 6, "kept", None),
          ("flat", 97, 96, 3, 9, 1, 5, "x3", None),
          # split-bf16 refuses deep-K below Vp = 6144 (two chunks of 32 x 96 per slab): the fast fold with deep-K in that build
          ("wrong", 6100, 64, 15, 9, 4, 3, "kept", None), ("confident", 6100, 256, 130, 1, 1, 4, "kept", None))
_SCORE = (("flat", 97, 64, 5, 1, 1, 0, 0), ("confident", 4099, 256, 15, 9, 4, 4, 1), ("wrong", 97, 256, 15, 9, 4, 4, 1), ("confident", 65601, 64, 2, 3, 1, 0, 1),
          ("beyond", 65601, 64, 8, 1, 1, 5, 0), ("offset", 130, 96, 15, 9, 1, 3, 0))


def tile_for(op, tile):
    """cc_gemm_tile_mode accepts 6 and 7 in the 16-bit builds only (tests/test_gpu_edges.py); the split-bf16 build takes 3 there."""
    return 3 if (op == "x3" and tile in (6, 7)) else tile


def cases(op):
    out = []
    for mode in (1, 2):
        for fam, V, D, B, cap, L, tile, denom, ls in _TRAIN:
            t = tile_for(op, tile)
            out.append(Case(f"{fam}-V{V}-D{D}-B{B}x{cap}-L{L}-m{mode}-t{t}", fam, V, D, B, cap, L, mode, t, denom, ls, 0))
    for fam, V, D, B, cap, L, tile, iz in _SCORE:
        t = tile_for(op, tile)
        out.append(Case(f"{fam}-V{V}-D{D}-B{B}x{cap}-L{L}-score{iz}-t{t}", fam, V, D, B, cap, L, 0, t, "kept", None, iz))
    return out


def vp_of(V):
    return (V + 127) // 128 * 128


def paths(c, op):
    """(form, epilogue entry point, fold path, input-gradient path) of a case, from launch_gemm / ce_row_fold / gemm_nt_deepk: the row-strip
    epilogues run `strip` on the 256-row kernels (tile modes 4, 5, K % 64 == 0) and operator() on the 128 x 128 ones (every other mode: the
    192- and 160-wide forms cannot carry 64-column partials; K % 64 != 0: the register-staged kernel)."""
    Vp = vp_of(c.V)
    entry = "strip" if (c.tile in (4, 5) and c.D % 64 == 0) else "operator()"
    fold = "generic" if Vp // 64 > 1024 else "fast"
    if c.mode == 0:
        return ("score", entry, fold, "-")
    return (form_of(op, c.mode), entry, fold, "deepk" if deepk_slabs(c, op) else "fallback")


def deepk_slabs(c, op):
    """(slabs, K tiles of 64 per slab) gemm_nt_deepk runs the input-gradient GEMM with, or None where it refuses and the caller falls back
    to gemm_bf16out (+ lm_dgrad_fix).  Mirrors the launcher: 256 x 256 tiles, ks = min(256 / tiles, slabs that fit the scratch (du16),
    K / 2048), refused below 2 slabs or above 128 tiles; the split-bf16 build (fused 256 x 192 form, K % 96 == 0) then picks the k2 <= 8,
    k2 <= (K / 96) / 32 of least rounds x chunks.  Left out on purpose: the lab build's CC_DEEPK / CC_X3_FUSED knobs (product library:
    defaults), and the alignment refusals (N, lda, ldb, ldo multiples of 8, K of 64: true of every cfg the library accepts)."""
    if c.mode == 0 or c.tile == 0:
        return None
    K, N, M = vp_of(c.V), c.D, c.B * c.cap
    tiles = -(-M // 256) * -(-N // 256)
    fit = (c.B * (c.L + c.cap) * 4 * N * (4 if op == "x3" else 2)) // (M * N * 4)      # the scratch is du16 as gpt2_carve sizes it: B T 4 D elements
    ks = min(256 // tiles, fit, K // 2048)
    if ks < 2 or tiles > 128:
        return None
    if op == "x3" and K % 96 == 0:
        tl, nc = -(-M // 256) * -(-N // 192), K // 96
        best, best_ks = -1, ks
        for k2 in range(1, 9):
            if k2 > fit or k2 > nc // 32:
                break
            cost = -(-tl * k2 // 256) * -(-nc // k2)
            if best < 0 or cost < best:
                best, best_ks = cost, k2
        ks = best_ks
        if ks < 2:
            return None
    kt = K // 64
    per = -(-kt // ks)
    return -(-kt // per), per


def required_paths(op):
    """every reachable combination: strip + generic fold + fallback does not exist (Vp = 65664 always has two or more slabs unless tile
    mode 0, which is the operator() entry).  paths() is a model of launch_gemm / gemm_nt_deepk written from their source; the library has no
    query for the kernel it chose, so coverage is coverage of this model (the conditions it leaves out are named in deepk_slabs)."""
    forms = {"bf16": ("exp",), "fp16": ("logit",), "x3": ("exp", "logit")}[op]
    req = {(f, e, fo, d) for f in forms for e in ("strip", "operator()") for fo in ("fast", "generic") for d in ("deepk", "fallback")}
    req -= {(f, "strip", "generic", "fallback") for f in forms}
    req |= {("score", e, fo, "-") for e in ("strip", "operator()") for fo in ("fast", "generic")}
    return req


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
SPIKE = 40.0


def row_map(B, T, L, cap, device="cpu"):
    b = torch.arange(B, device=device).view(B, 1)
    return (b * T + L - 1 + torch.arange(cap, device=device).view(1, cap)).reshape(-1)


def group_ids(V):
    """the four target ids of a case: V - 1, another id of the last (partial) 8-column group where it has one, a middle id, a small one"""
    second = V - 2 if (V - 2) // 8 == (V - 1) // 8 else 9
    return [V - 1, second, V // 2, 7]


def hot_ids(V):
    return [3, V // 3, V - 4, 11, 13, V // 5, 2 * V // 3, V - 6]     # 0..2: the wrong family's rivals; 3..7: the beyond family's columns


def make_tokens(c):
    """tokens int64 [B][cap] and the group of every caption row.  A row of group g has target group_ids[g]; rows share ids within and across
    samples.  Specials: a -1 pad tail, a fully padded sample, an id 0 in the middle of a caption.  The whole inventory (with V - 1, an id of the
    last partial 8-column group and ids repeated within and across samples) needs three samples of three columns; every family has such
    cases.  The shapes below that exist for other reasons — cap = 1 for the row-tile crossings, B cap <= 8 at V = 65601, the single row —
    and carry what fits: cap = 1 with B >= 5 a padded sample and an id 0, the rest neither (tests/test_lm_ref.py asserts exactly this)."""
    Mc = c.B * c.cap
    r = torch.arange(Mc)
    g = r % 3
    tid = torch.tensor(group_ids(c.V))
    tok = tid[g].view(c.B, c.cap).clone()
    if c.cap >= 3 and c.B >= 3:
        tok[0, c.cap - 2:] = -1
        tok[c.B - 1, :] = -1
        tok[1, 1] = 0
    elif c.cap == 1 and c.B >= 5:
        tok[1, 0] = -1
        tok[3, 0] = 0
    if c.family == "beyond":
        ign = (tok.view(-1) <= 0).nonzero().view(-1)
        hit = (r % 23 == 5)
        if len(ign):
            hit[ign[0]] = True
        g = torch.where(hit, torch.full_like(g, 3), g)
        tok = torch.where((tok.view(-1) > 0) & hit, tid[3], tok.view(-1)).view(c.B, c.cap)
    return tok, g


def make_inputs(c, op, seed=0):
    """(x fp32 [B T][D], gamma, beta fp32 [D], wte fp32 [V][D], tokens) on the CPU.  gamma[0] = 0, beta[0] = 8: hf[:, 0] = 8 exactly, so
    wte[v, 0] moves logit v of EVERY row by 8 wte[v, 0] (the offset family).  Dimensions 1..4 are selectors: gamma = 1, beta = 0, and a row
    of group g carries a spike in dimension 1 + g, so wte[v, 1 + g] moves logit v in the rows of group g only."""
    gen = torch.Generator().manual_seed(1000 * seed + c.V + 7 * c.D + 13 * c.B + c.cap)
    T = c.L + c.cap
    D, V = c.D, c.V
    x = torch.randn(c.B * T, D, generator=gen)
    gamma = 1.0 + 0.05 * torch.randn(D, generator=gen)
    beta = 0.02 * torch.randn(D, generator=gen)
    gamma[0], beta[0] = 0.0, 8.0
    gamma[1:5], beta[1:5] = 1.0, 0.0
    wte = torch.randn(V, D, generator=gen) * (0.3 / math.sqrt(D))
    wte[:, 0] = 0.0
    tok, g = make_tokens(c)
    rows = row_map(c.B, T, c.L, c.cap)
    spiked = c.family in ("confident", "wrong") or (c.family == "beyond")
    if spiked:
        sel = (g < 3) if c.family != "beyond" else (g == 3)
        x[rows[sel], 1 + g[sel]] = SPIKE
        if c.family == "beyond":
            sel = torch.zeros_like(sel)
        wte[:, 1:5] = 0.0
    hf = ln_rows(x, gamma, beta, c.B, T, c.L, c.cap)["hf"]
    tid, hot = group_ids(V), hot_ids(V)
    if c.family in ("confident", "wrong"):
        for k in range(3):
            m = g == k
            if m.any():
                h = hf[m, 1 + k].median().item()
                if c.family == "confident":
                    wte[tid[k], 1 + k] = 40.0 / h
                else:
                    wte[hot[k], 1 + k] = 55.0 / h
    if c.family == "beyond":
        m = g == 3
        h = hf[m, 4].median().item()
        for v in hot[3:]:
            wte[v, 4] = 90.0 / h
    if c.family == "offset":
        wte[:, 0] = OFFSET[op] / 8.0
    if op != "x3":      # keep the master representable where a property is stated on stored values
        wte = wte.to(DT[op]).float()
    return x, gamma, beta, wte, tok


# ---- ln_f ----------------------------------------------------------------------------------------------------------------------------
def ln_rows(x, gamma, beta, B, T, L, cap, shift=0):
    rows = (row_map(B, T, L, cap, x.device) + shift).clamp_max(B * T - 1)
    xr = x.double()[rows]
    mu = xr.mean(-1, keepdim=True)
    var = ((xr - mu) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    xhat = (xr - mu) * rstd
    return dict(rows=rows, x=xr, mean=mu.squeeze(-1), rstd=rstd.squeeze(-1), xhat=xhat, hf=xhat * gamma.double() + beta.double())


def store(v, op):
    """float64 -> the build's stored type (through fp32, as the kernels round)"""
    return v.float().to(DT[op])


def _xhat_err(R, D):
    """absolute error of the device's (x - mean) rstd: mean from 2 D roundings of u32 mean |x|; the variance's sum likewise (relative 2 D u32,
    halved by the root), rsqrtf within 4 u32, the subtraction and the product one each"""
    e_mu = 2 * D * U32 * R["x"].abs().mean(-1, keepdim=True)
    rstd = R["rstd"].unsqueeze(-1)
    return rstd * 2 * e_mu + R["xhat"].abs() * (3 * D + 8) * U32


def ln_bounds(R, gamma, beta, op):
    D = R["x"].shape[1]
    e = gamma.double().abs() * _xhat_err(R, D) + 3 * U32 * ((R["xhat"] * gamma.double()).abs() + beta.double().abs())
    return G.store_bound(R["hf"], SECOND_ORDER * e, DT[op])


def ln_bwd(R, gamma, dy):
    """dx rows, dgamma, dbeta of LayerNorm backward from the upstream gradient dy [rows][D]"""
    g = dy.double() * gamma.double()
    c1 = g.mean(-1, keepdim=True)
    c2 = (g * R["xhat"]).mean(-1, keepdim=True)
    dx = R["rstd"].unsqueeze(-1) * (g - c1 - R["xhat"] * c2)
    return dict(dx=dx, dgamma=(dy.double() * R["xhat"]).sum(0), dbeta=dy.double().sum(0), g=g, c1=c1, c2=c2)


def ln_bwd_bounds(R, W, gamma, dy, pre_gamma, pre_beta):
    """bounds of dx [rows][D], dgamma, dbeta [D] (accumulated onto pre_*).  Row sums over D and column sums over the rows are fp32 VALU sums:
    2 n roundings of u32 sum |terms|, + 32 for the cross-wave / cross-block folds."""
    D, M = R["x"].shape[1], R["x"].shape[0]
    ex = _xhat_err(R, D)
    g, xh = W["g"], R["xhat"]
    rstd = R["rstd"].unsqueeze(-1)
    s1 = (2 * D + 32) * U32 * g.abs().mean(-1, keepdim=True)
    s2 = (2 * D + 32) * U32 * (g * xh).abs().mean(-1, keepdim=True) + (g.abs() * ex).mean(-1, keepdim=True)
    inner = s1 + xh.abs() * s2 + W["c2"].abs() * ex + 4 * U32 * (g.abs() + W["c1"].abs() + (xh * W["c2"]).abs())
    b_dx = SECOND_ORDER * (rstd * inner + W["dx"].abs() * (3 * D + 8) * U32)
    a = dy.double().abs()
    b_dg = SECOND_ORDER * ((a * ex).sum(0) + (2 * M + 32) * U32 * (a * xh.abs()).sum(0)) + 2 * U32 * (pre_gamma.double().abs() + W["dgamma"].abs())
    b_db = (2 * M + 32) * U32 * a.sum(0) + 2 * U32 * (pre_beta.double().abs() + W["dbeta"].abs())
    return dict(dx=b_dx, dgamma=b_dg, dbeta=b_db)


# ---- the chain -----------------------------------------------------------------------------------------------------------------------
DEFECTS = ("drop_partial", "fold_last_batch", "pad_as_zero", "neg_inf_unguarded", "target_plus_1", "target_minus_1", "row_map_plus_1",
           "pad_kept", "zero_kept", "zero_dropped_from_score", "clamp_60", "r_without_w", "no_loss_scale", "denom_unclamped", "no_onehot",
           "onehot_on_ignored", "second_slab_dropped", "rhf_unscaled", "dwte_pad_rows")
# the forms a defect can occur in (the others have no such code: no clamp, no r, no slab ...)
DEFECT_FORMS = {"clamp_60": ("exp",), "r_without_w": ("exp",), "rhf_unscaled": ("exp",), "zero_dropped_from_score": ("score",),
                "zero_kept": ("exp", "logit"), "pad_kept": ("exp", "logit", "score")}
_TRAIN_ONLY = ("no_loss_scale", "denom_unclamped", "no_onehot", "onehot_on_ignored", "second_slab_dropped", "dwte_pad_rows")


def defect_applies(d, form):
    if d in DEFECT_FORMS:
        return form in DEFECT_FORMS[d]
    if d in _TRAIN_ONLY:
        return form != "score"
    return True


def denom_of(c, tok):
    kept = int((tok > 0).sum())
    return {"zero": 0.0, "kept": float(kept), "x3": 3.0 * kept}[c.denom]


def chain(hf_st, wte, tok, c, op, denom, defect=None):
    """float64 reference of everything downstream of the stored ln_f rows.  hf_st [B cap][D] in the stored type; wte fp32 master [V][D];
    tok int64 [B][cap]; denom the divisor handed to cc_lmhead_ce_bwd.  defect: one of DEFECTS (float64 emulation of that bug)."""
    dev = hf_st.device
    V, D = wte.shape
    Vp, Mc = vp_of(V), hf_st.shape[0]
    form = form_of(op, c.mode)
    tokf = tok.reshape(-1).to(dev)
    tid = tokf.clamp_min(0)
    if op == "x3":
        ah, al = G.split(hf_st.float())
        bh, bl = G.split(wte.float())
        z, sabs = G.three_term(ah, al, bh, bl)
        hfd, wm = hf_st.double(), wte.double()          # the rows read elementwise: fp32 hf, fp32 master
        wg = wm
    else:
        hfd, wg = hf_st.double(), wte.to(DT[op]).double()
        wm = wg
        z, sabs = hfd @ wg.t(), hfd.abs() @ wg.abs().t()
    # kept rows
    if c.mode == 0:
        keep = (tokf >= 0) & ~((tokf == 0) & bool(c.iz))
        if defect == "zero_dropped_from_score":
            keep = tokf > 0
        if defect == "pad_kept":
            keep = keep | (tokf < 0)
    else:
        keep = tid != 0
        if defect == "pad_kept":
            keep = keep | (tokf < 0)
        if defect == "zero_kept":
            keep = keep | (tokf == 0)
    # target logit
    tcol = tid
    if defect == "target_plus_1":
        tcol = (tid + 1).clamp_max(V - 1)
    if defect == "target_minus_1":
        tcol = (tid - 1).clamp_min(0)
    if form == "exp":
        tgt = (hfd * wm[tcol]).sum(-1)
        sabs_t = (hfd.abs() * wm[tcol].abs()).sum(-1)
    else:
        tgt = z.gather(1, tcol.view(-1, 1)).squeeze(1)
        sabs_t = sabs.gather(1, tcol.view(-1, 1)).squeeze(1)
    # row sums
    zz = z
    col = torch.arange(V, device=dev)
    live = torch.ones(V, dtype=torch.bool, device=dev)
    npart = Vp // 64
    if defect == "drop_partial":
        blk = 1 if V > 64 else 0
        live = (col // 64) != blk
    if defect == "fold_last_batch" and npart > 64:
        live = (col // 64) < 64 * ((npart - 1) // 64)
    lim = 60.0 if defect == "clamp_60" else CLAMP
    if form == "exp":
        y = zz - tgt.unsqueeze(1)
        yc = y.clamp_max(lim)
        beyond = y.max(1).values > CLAMP
        e = torch.where(live, torch.exp(yc - yc.max(1, keepdim=True).values), torch.zeros_like(yc))
        ssum = e.sum(1)
        if defect == "pad_as_zero":
            ssum = ssum + (min(Vp, (V + 7) // 8 * 8) - V) * torch.exp(-tgt - yc.max(1).values)
        lse_c = tgt + yc.max(1).values + torch.log(ssum)             # what the clamped sum gives (= lse where nothing clamps)
        p = e / ssum.unsqueeze(1)                                    # r E / w
        lse = torch.logsumexp(z, 1)
        if defect is not None:
            lse = lse_c
    else:
        y = None
        beyond = torch.zeros(Mc, dtype=torch.bool, device=dev)
        m = zz.max(1, keepdim=True).values
        e = torch.where(live, torch.exp(zz - m), torch.zeros_like(zz))
        ssum = e.sum(1)
        if defect == "pad_as_zero":
            ssum = ssum + (min(Vp, (V + 7) // 8 * 8) - V) * torch.exp(-m.squeeze(1))
        lse = m.squeeze(1) + torch.log(ssum)
        lse_c = lse
        p = e / ssum.unsqueeze(1)
    if defect == "neg_inf_unguarded" and (Vp - 64 >= V):
        lse = lse * float("nan")
        lse_c = lse
    used = lse_c if form == "exp" else lse
    loss = torch.where(keep, used - tgt, torch.zeros_like(tgt))
    R = dict(form=form, z=z, sabs=sabs, y=y, tgt=tgt, sabs_t=sabs_t, lse=lse, lse_c=lse_c, p=p, keep=keep, beyond=beyond, ssum=ssum, tid=tid,
             hfd=hfd, wm=wm, wg=wg, npart=npart)
    if c.mode == 0:
        lp = torch.where(keep, tgt - used, torch.zeros_like(tgt))
        R["tlp"] = lp
        R["sstats"] = torch.stack([lp.view(c.B, c.cap).sum(1), keep.view(c.B, c.cap).double().sum(1)], 1)
        return R
    R["loss"] = loss
    R["stats"] = torch.stack([loss.sum(), keep.double().sum()])
    # gradient
    ls = 1.0 if (c.ls is None or defect == "no_loss_scale") else c.ls
    dn = denom if defect == "denom_unclamped" else max(denom, 1.0)
    inv = ls / dn if dn != 0 else float("inf")
    w = keep.double() * inv
    oh = torch.zeros_like(p)
    oh.scatter_(1, tid.view(-1, 1), 1.0)
    pw = p * (keep.double().unsqueeze(1) if defect == "r_without_w" else w.unsqueeze(1))
    ohw = oh * w.unsqueeze(1)
    if defect == "no_onehot":
        ohw = ohw * 0
    if defect == "onehot_on_ignored":
        ohw = oh * inv
    dl = pw - ohw
    wd = wm if form == "exp" or op == "x3" else wg
    slabs = deepk_slabs(c, op)
    if defect == "second_slab_dropped" and slabs:
        lo, hi = slabs[1] * 64, min(2 * slabs[1] * 64, V)                # the columns of slab 1
        cut = torch.ones(V, dtype=torch.float64, device=dev)
        cut[lo:hi] = 0
        dhf = ((pw * cut) @ wg - ohw @ wd) if form == "exp" else (dl * cut) @ wg
    else:
        dhf = (pw @ wg - ohw @ wd) if form == "exp" else dl @ wg
    R.update(w=w, inv=inv, dl=dl, pw=pw, ohw=ohw, dhf=dhf)
    if c.mode == 2:
        if defect == "rhf_unscaled":
            r = torch.exp(tgt - lse_c) * w
            dwte = (pw / r.clamp_min(1e-300).unsqueeze(1)).t() @ hfd - ohw.t() @ hfd
        else:
            dwte = dl.t() @ hfd
        full = torch.zeros(Vp, D, dtype=torch.float64, device=dev)
        full[:V] = dwte
        if defect == "dwte_pad_rows":
            full[V:] = (w * torch.exp(-lse_c)).sum() * hfd.abs().mean(0)
        R["dwte"] = full
    return R


def bounds(R, c, op, allow=None):
    """per-element bounds of what chain() returns (module docstring), for the kernels paths(c, op) names.  allow: (exp2-positive, logf)
    allowances in place of the measured ones (tests/test_lm_ref.py: ALLOW_CEILING)."""
    exp2_pos, logf = allow if allow is not None else (EXP2_POS_ULPS, LOGF_ULPS)
    assert exp2_pos is not None and logf is not None, "measure the allowances first (module docstring)"
    form = R["form"]
    u, dt = U_OP[op], DT[op]
    z, sabs = R["z"], R["sabs"]
    Mc, V = z.shape
    D = R["hfd"].shape[1]
    kp = 3 * D if op == "x3" else D
    dz = G.acc_bound(sabs, kp)
    n_adds = 18 + max(16, -(-R["npart"] // 64)) + 6 + 1
    p = R["p"]
    keep = R["keep"].double()
    if form == "exp":
        b_tgt = 2 * D * U32 * R["sabs_t"]
        y = R["y"].clamp_max(CLAMP)
        dy = dz + (T3 * sabs if op == "x3" else 0.0) + b_tgt.unsqueeze(1) + U32 * (2 * z.abs() + 2 * R["tgt"].abs().unsqueeze(1) + y.abs())
        ulps = torch.where(y > 0, torch.full_like(y, exp2_pos), torch.full_like(y, EXP_ULPS))
        rho = SECOND_ORDER * torch.expm1(dy) + U32 * ulps * (1.0 + y.abs())
        m = R["tgt"]
        logs = R["lse_c"] - R["tgt"]
    else:
        b_tgt = dz.gather(1, R["tid"].view(-1, 1)).squeeze(1)
        m = z.max(1).values
        x = z - m.unsqueeze(1)
        rho = SECOND_ORDER * torch.expm1(dz) + 2 * U32 * (EXP_ULPS + 1.0) * (2.0 + x.abs())
        logs = R["lse"] - m
    b_lse = SECOND_ORDER * (p * rho).sum(1) + n_adds * U32 + logf * U32 * logs.abs().clamp_min(1.0) + U32 * (R["lse"].abs() + m.abs())
    if form == "exp":
        b_lse = b_lse + b_tgt
    out = dict(lse=b_lse, tgt=b_tgt)
    if form == "score":
        b_lp = keep * (b_lse + b_tgt + U32 * R["tlp"].abs())
        out["tlp"] = b_lp
        s = b_lp.view(c.B, c.cap).sum(1) + (c.cap // 64 + 7) * U32 * R["tlp"].abs().view(c.B, c.cap).sum(1)
        out["sstats"] = torch.stack([s, torch.zeros_like(s)], 1)
        return out
    b_loss = keep * (b_lse + b_tgt + U32 * R["loss"].abs())
    out["loss"] = b_loss
    out["stats"] = torch.stack([b_loss.sum() + (Mc // 1024 + 22) * U32 * R["loss"].abs().sum(), torch.zeros_like(b_loss.sum())])
    # gradient
    w = R["w"].unsqueeze(1)
    wa = R["wg"].abs()
    slabs = deepk_slabs(c, op)
    deep = slabs is not None
    if form == "exp":
        a = R["tgt"] - R["lse_c"]
        b_a = b_lse + b_tgt + U32 * a.abs()
        rho_r = SECOND_ORDER * torch.expm1(b_a) + U32 * EXP_ULPS * (1.0 + a.abs()) + 3 * U32
        u_e = G.U_BF16 ** 2 if op == "x3" else u
        rel = SECOND_ORDER * (rho + rho_r.unsqueeze(1) + u_e + (T3 if op == "x3" else 0.0))
        pw = R["pw"]
        term = pw @ wa
        acc = G.acc_bound(term, 3 * vp_of(V) if op == "x3" else vp_of(V), ksplit=slabs[0] if deep else 1)
        e = (pw * rel) @ wa + acc + 3 * U32 * (term + R["ohw"] @ R["wm"].abs() + R["dhf"].abs())
        if not deep:
            e = e + u * (pw @ R["wg"]).abs() * (1 + u)
        out["dhf"] = G.store_bound(R["dhf"], e, dt)
        if "dwte" in R:
            ha = R["hfd"].abs()
            t2 = pw.t() @ ha
            E_abs = torch.exp(y) * keep.unsqueeze(1)
            e2 = (pw * (rel + 2 * u + 2 * U32)).t() @ ha + G.acc_bound(t2, 3 * Mc if op == "x3" else Mc, ksplit=Mc // 64 + 1) + \
                FP32_MIN_NORMAL * (E_abs.t() @ torch.ones_like(ha)) + (2 * U32) * (R["ohw"].t() @ ha) + Mc * U32 * (R["ohw"].t() @ ha)
            out["dwte_err"] = e2
    else:
        lse = R["lse"].unsqueeze(1)
        sub = G.FP16_SUBNORMAL_HALF if op == "fp16" else 0.0
        dx = u * z.abs() + (1 + u) * dz + sub + b_lse.unsqueeze(1) + U32 * (z - lse).abs()
        rho2 = SECOND_ORDER * torch.expm1(dx) + U32 * EXP_ULPS * (1.0 + (z - lse).abs())
        pp = torch.exp(z - lse)
        oh = (R["ohw"] != 0).double() if R["inv"] != 0 else torch.zeros_like(pp)
        e_dl = w * (pp * rho2 + FP32_MIN_NORMAL * 64 + 2 * U32 * (pp - oh).abs()) + 2 * U32 * R["dl"].abs()
        b_dl = G.store_bound(R["dl"], e_dl, dt) if op != "x3" else e_dl + T3 * R["dl"].abs()
        term = R["dl"].abs() @ wa
        acc = G.acc_bound(term, 3 * vp_of(V) if op == "x3" else vp_of(V), ksplit=slabs[0] if deep else 1)
        out["dhf"] = G.store_bound(R["dhf"], b_dl @ wa + acc + (T3 * term if op == "x3" else 0.0), dt)
        if "dwte" in R:
            ha = R["hfd"].abs()
            t2 = R["dl"].abs().t() @ ha
            out["dwte_err"] = b_dl.t() @ ha + G.acc_bound(t2, 3 * Mc if op == "x3" else Mc, ksplit=Mc // 64 + 1) + (T3 * t2 if op == "x3" else 0.0)
    return out


def dwte_bound(R, Bd, pre):
    """bound of g32's wte rows after the call minus the pre-fill: the gradient's error + the accumulations' roundings (two of them)"""
    e = torch.zeros_like(R["dwte"])
    V = Bd["dwte_err"].shape[0]
    e[:V] = Bd["dwte_err"]
    return e + 2 * U32 * (pre.double().abs() + R["dwte"].abs()) * (R["dwte"] != 0).double()


def leaves_bound(Rd, R, Bd):
    """does a defect emulation Rd leave the bounds Bd around the reference R in any checked quantity?  (quantity name or None)"""
    for k in ("lse", "tgt", "loss", "stats", "tlp", "sstats", "dhf", "dwte"):
        if k not in R:
            continue
        b = Bd["dwte_err"].new_zeros(R[k].shape) if k == "dwte" else Bd[k]
        if k == "dwte":
            b[:Bd["dwte_err"].shape[0]] = Bd["dwte_err"]
        d = (Rd[k] - R[k]).abs()
        if bool((~torch.isfinite(Rd[k])).any()) or bool((d > b).any()):
            return k
    return None
