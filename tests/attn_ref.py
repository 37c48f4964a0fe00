"""float64 reference of the attention launchers attn_fwd / attn_bwd (clipcap_amd/csrc/attention.hip), the per-element error bounds the GPU
test holds their kernels to (tests/test_gpu_attention_ref.py), float64 emulations of the defects those bounds must catch, and the case
list both tests walk.  Plain torch, no GPU needed (every function runs on whatever device its tensors are on); tests/test_attn_ref.py
pins this module itself.  It stands to attention as tests/gemm_ref.py stands to the GEMMs and reuses its constants.

Definitions (attention.hip, the comment above k_attn_bwd).  q, k, v, dO are [B][H][S][hd]; scale = hd^-1/2; keep M in {0, 1}, ks = 1/(1-p):
    s = q k^T scale (key j > query i masked when causal)    m = rowmax s    l = rowsum exp(s - m)    lse = m + log l    A = exp(s - lse)
    A_d = M A ks    out = A_d v                                   (dropout enters P V only; the row sum l does not see it)
    dA_d = dO v^T   dA = M ks dA_d   delta = rowsum(A dA) (= rowsum(dO out))   dS = A (dA - delta) scale
    dq = dS k       dk = dS^T q      dv = A_d^T dO

Rounding model.  u32 = 2^-24; u = 2^-8 (bf16) / 2^-11 (fp16) / 0 (split-bf16, where a product of two split operands instead misses the
exact one by 3 * 2^-16 * |a||b|, gemm_ref.split_product_bound).  A sum of n products costs, on the longest chain to one output,
    MFMA kernels (v_mfma_f32_32x32x16: 16 products per step)   ceil(n / 16) * MFMA_ROUNDINGS roundings   (x 3 in the three-term kernels)
    fp32 VALU kernels (any order of additions)                 2 n roundings (one per product unless contracted, one per addition)
each at most u32 * sum |terms|.  Sums over keys / queries run over whole 32-row blocks in the MFMA kernels (the causal ones stop at the
diagonal block), so n counts the blocks a row really visits.  Every other rounding is counted where it happens; see bounds().  Products of
two of these relative errors (each below 2^-7) are covered by the factor SECOND_ORDER.  Only the device exp / log cannot be counted: they
are measured allowances (EXP_ULPS, LOG_ULPS below)."""
import math

import torch

from tests import gemm_ref as G

U32 = G.U32
SECOND_ORDER = 1.02                       # (1 + 2^-7)^2 < 1.016: products of two first-order terms
TINY = 2.0 ** -120                        # fp32 flushes probabilities below 2^-126; times operand magnitudes of at most 2^6
BLK = 32                                  # key / query block of the MFMA kernels
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "x3": torch.float32}
U_OP = {"bf16": G.U_BF16, "fp16": G.U_FP16, "x3": 0.0}

# ---- measured allowances (MI355X, against float64; 4 x the worst value seen) --------------------------------------
# Re-measure with `pytest tests/test_gpu_attention_ref.py -m gpu -s -k test_measured_allowances`: it prints the raw figures.
# Both are read through the fp32 LDS/VALU kernels of the split-bf16 build, at inputs where the value under test reaches an output with no
# other rounding on the way (q = 0, so every score is exactly 0):
#   __expf: dv[j][d] = exp(-lse[d]) with dO = identity rows (k_attn_bwd_small, S = 31, hd = 32), lse handed in, 7936 arguments over [-80, 0]
#           (below -87 the result leaves fp32's normal range; TINY covers that): |dev - exp(x)| / (u32 * exp(x) * (1 + |x|)) worst seen 1.1504
#           -> allowance 4.6.  (v_exp_f32 of x * log2(e): the product's rounding grows with |x|, hence the 1 + |x|.)
#   __logf: lse = log(S) for S = 1 .. 180 (k_attn_fwd, hd = 8: l = S exactly): |dev - log(l)| / (u32 * max(1, log l)) worst seen 2.3297
#           -> allowance 9.3.
EXP_ULPS = 4.6
LOG_ULPS = 9.3


# ---- legality of the LDS-tile backward (attention.hip: attn_bwd_lds, 160 KiB of LDS) ------------------------------------------------------
LDS_BYTES = 160 * 1024


def attn_fwd_lds(S, hd):
    return (3 * S * (hd + 4) + S * (S + 1)) * 4


def attn_bwd_lds(S, hd):
    if S < 32:
        return (4 * S * (hd + 4) + 2 * S * (S + 1)) * 4
    S4 = (S + 3) & ~3
    return (4 * S4 * (hd + 4) + 2 * S4 * (S4 + 4)) * 4


def bwd_lds_edge(hd, lo=33):
    """largest S >= lo whose LDS-tile backward fits"""
    S = lo
    while attn_bwd_lds(S + 1, hd) <= LDS_BYTES:
        S += 1
    assert attn_bwd_lds(S, hd) <= LDS_BYTES
    return S


def paths(op, S, hd, mfma_bwd=True):
    """(forward kernel, backward kernel) the dispatch of attn_fwd / attn_bwd picks, and their rounding family
    ('mfma' 16-bit MFMA, 'mfma3' three-term MFMA, 'valu' fp32 accumulation on the VALU)."""
    if op != "x3":
        if hd in (64, 96, 128):
            fwd = ("k_attn_fwd_mfma", "mfma")
            if not mfma_bwd:
                bwd = ("k_attn_bwd_small" if S < 32 else "k_attn_bwd", "valu")
            elif S <= 32:
                bwd = ("k_attn_bwd_fused<1>", "mfma")
            elif S <= 64 and hd < 128:
                bwd = ("k_attn_bwd_fused<2>", "mfma")
            else:
                bwd = ("k_attn_bwd_dq+dkv", "mfma")
            return fwd, bwd
        return ("k_attn_fwd", "valu"), ("k_attn_bwd_small" if S < 32 else "k_attn_bwd", "valu")
    fwd = ("k_attn_fwd_mfma3", "mfma3") if hd in (64, 96, 128) else \
        (("k_attn_fwd", "valu") if attn_fwd_lds(S, hd) <= LDS_BYTES else ("k_attn_fwd_rows", "valu"))
    if hd in (64, 96) and S <= 64:
        bwd = ("k_attn_bwd_m3<%d>" % (1 if S <= 32 else 2), "mfma3")
    elif attn_bwd_lds(S, hd) <= LDS_BYTES:
        bwd = ("k_attn_bwd_small" if S < 32 else "k_attn_bwd", "valu")
    else:
        bwd = ("k_attn_bwd_rows", "valu")
    return fwd, bwd


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
FAMILIES = ("flat", "peaked", "rising", "offset")


def make_inputs(family, B, S, H, hd, seed):
    """fp32 (qkv [B*S][3 H hd], dout [B*S][H hd]) on the CPU.  flat: randn.  peaked: q x 6 (score deviation 6: rows dominated by a few keys).
    rising: coordinate 0 of every q is 8 and of key j is (j // 32) sqrt(hd), so every 32-key block lifts each row's maximum by 8 and the
    global maximum lies in the last block.  offset: coordinate 0 is q = 40, k = 20 (exact in bf16 and fp16): every score moves by
    800 / sqrt(hd) and softmax must not notice."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, S, 3, H, hd, generator=g)
    dout = torch.randn(B * S, H * hd, generator=g)
    if family != "rising":                # the last key is the last query's own direction: its score (about sqrt(hd)) tops that row, so the running
        qkv[:, S - 1, 1] = qkv[:, S - 1, 0]      # maximum still rises in the last key block, however few keys of it a causal row sees
    if family == "peaked":
        qkv[:, :, 0] *= 6.0
    elif family == "rising":
        qkv[:, :, 0, :, 0] = 8.0
        qkv[:, :, 1, :, 0] = ((torch.arange(S) // BLK).float() * math.sqrt(hd)).view(1, S, 1)
    elif family == "offset":
        qkv[:, :, 0, :, 0] = 40.0
        qkv[:, :, 1, :, 0] = 20.0
    else:
        assert family == "flat"
    return qkv.reshape(B * S, 3 * H * hd).contiguous(), dout


def heads(qkv, B, S, H, hd):
    """stored qkv [B*S][3 H hd] (any dtype) -> float64 q, k, v [B][H][S][hd]: the values the kernel multiplies"""
    x = qkv.double().view(B, S, 3, H, hd).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


def rows(x, B, S, H, hd):
    """[B*S][H hd] -> float64 [B][H][S][hd]"""
    return x.double().view(B, S, H, hd).permute(0, 2, 1, 3)


def unrows(x):
    """[B][H][S][hd] -> [B*S][H hd]"""
    B, H, S, hd = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * S, H * hd)


def keep_scale(p):
    """1 / (1 - p) as make_drop computes it (fp32)"""
    one = torch.tensor(1.0, dtype=torch.float32)
    return float(one / (one - torch.tensor(p, dtype=torch.float32)))


# ---- reference and defect emulations --------------------------------------------------------------------------------------------------
DEFECTS = ("mask_transposed", "mask_no_bh", "dv_no_scale", "delta_no_mask", "causal_off_by_one", "ragged_keys", "no_rescale")


def reference(q, k, v, do, causal, keep=None, p=0.0, defect=None):
    """float64 attention forward and backward.  keep: [B][H][S][S] flags (cc_dropout_mask's stream) or None.  Returns a dict with out, lse,
    dq, dk, dv and the intermediates bounds() needs.  defect: one of DEFECTS — the same computation with that one mistake in it:
      mask_transposed    the dropout mask read at (j, i)
      mask_no_bh         the mask row index without its (b H + h) term: every head reads the first head's mask
      dv_no_scale        dv = (M A)^T dO, the keep scale forgotten
      delta_no_mask      delta = rowsum(A dA_d), the mask (and its scale) forgotten
      causal_off_by_one  key i + 1 visible to query i
      ragged_keys        the zero-filled keys S .. 32 ceil(S / 32) - 1 of the last block take part (score 0, value 0)
      no_rescale         online softmax over 32-key blocks without the rescale: out and l of block b stay relative to the running maximum
                         of its own time (forward outputs only)"""
    B, H, S, hd = q.shape
    dev = q.device
    scale = hd ** -0.5
    if defect == "ragged_keys":
        pad = -S % BLK
        z = torch.zeros(B, H, pad, hd, dtype=q.dtype, device=dev)
        kx, vx = torch.cat([k, z], 2), torch.cat([v, z], 2)
    else:
        kx, vx = k, v
    Sk = kx.shape[2]
    s = q @ kx.transpose(-1, -2) * scale
    i_, j_ = torch.arange(S, device=dev).view(S, 1), torch.arange(Sk, device=dev).view(1, Sk)
    live = (j_ <= i_ + (1 if defect == "causal_off_by_one" else 0)) if causal else torch.ones(S, Sk, dtype=torch.bool, device=dev)
    s = s.masked_fill(~live, float("-inf"))
    m = s.max(-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    lse = m + torch.log(l)
    A = e / l
    if keep is not None:
        kp = keep.double()
        if defect == "mask_transposed":
            kp = kp.transpose(-1, -2)
        elif defect == "mask_no_bh":
            kp = kp[:1, :1].expand(B, H, S, S)
        ks = keep_scale(p)
        if Sk > S:
            kp = torch.cat([kp, torch.ones(B, H, S, Sk - S, dtype=kp.dtype, device=dev)], -1)
        mk = kp * ks
    else:
        kp, ks, mk = None, 1.0, torch.ones_like(A)
    Ad = A * mk
    out = Ad @ vx
    lse_o = lse
    if defect == "no_rescale":
        nb = -(-Sk // BLK)
        o2, l2, mrun = torch.zeros_like(out), torch.zeros_like(l), torch.full_like(m, float("-inf"))
        for b in range(nb):
            sb = s[..., b * BLK:(b + 1) * BLK]
            mrun = torch.maximum(mrun, sb.max(-1, keepdim=True).values)
            eb = torch.where(torch.isinf(mrun), torch.zeros_like(sb), torch.exp(sb - mrun))
            o2 = o2 + (eb * mk[..., b * BLK:(b + 1) * BLK]) @ vx[..., b * BLK:(b + 1) * BLK, :]
            l2 = l2 + eb.sum(-1, keepdim=True)
        out, lse_o = o2 / l2, mrun + torch.log(l2)
    dAd = do @ vx.transpose(-1, -2)
    dA = mk * dAd
    delta = (A * (dAd if defect == "delta_no_mask" else dA)).sum(-1, keepdim=True)
    dS = A * (dA - delta) * scale
    dq = dS @ kx
    dk = (dS.transpose(-1, -2) @ q)[..., :S, :]
    dv = (((A * kp) if defect == "dv_no_scale" and kp is not None else Ad).transpose(-1, -2) @ do)[..., :S, :]
    return dict(out=out, lse=lse_o.squeeze(-1), dq=dq, dk=dk, dv=dv, s=s, m=m, l=l, A=A, Ad=Ad, mk=mk, dA=dA, delta=delta, dS=dS, live=live,
                q=q, k=k, v=v, do=do, causal=causal)


def applicable(defect, causal, p, S, B, H, fam_fwd, with_bwd, family="flat"):
    """whether a defect can show at a case at all (fam_fwd: rounding family of the forward kernel)"""
    if defect in ("mask_transposed", "mask_no_bh"):
        return p > 0 and S > 1 and (defect != "mask_no_bh" or B * H > 1)
    if defect in ("dv_no_scale", "delta_no_mask"):
        return p > 0 and with_bwd and (defect == "dv_no_scale" or S > 1)
    if defect == "causal_off_by_one":
        return bool(causal) and S > 1
    if defect == "ragged_keys":           # only kernels that walk whole 32-key blocks have such keys; a causal mask hides them
        # ... and so does a row maximum far above 0: a zero-score key then weighs exp(-m), nothing in fp32 (offset: m about 800 / sqrt(hd);
        # rising: m about 8 per block; peaked: m about 6 x 3, and 6 sqrt(hd) in the last row).  Every shape meets the defect in the flat family.
        return not causal and S % BLK != 0 and fam_fwd != "valu" and (family == "flat" or (family == "rising" and S < BLK))
    if defect == "no_rescale":            # needs a second key block
        return S > BLK and fam_fwd != "valu"
    raise ValueError(defect)


# ---- bounds ---------------------------------------------------------------------------------------------------------------------------
def _roundings(fam, n):
    """roundings on the longest chain of an n-product sum (n a number or a tensor), in units of u32 * sum |terms|"""
    n = torch.as_tensor(n, dtype=torch.float64)
    if fam == "valu":
        return 2.0 * n
    return torch.ceil(n / 16.0) * G.MFMA_ROUNDINGS * (3.0 if fam == "mfma3" else 1.0)


def _store(ref, err, op):
    return G.store_bound(ref, err, DT[op]) + TINY


def _counts(S, causal, fam, dev):
    """terms of a sum over keys for query i / over queries for key j, as the kernel family walks them: [S][1] float64 tensors"""
    r = torch.arange(S, device=dev, dtype=torch.float64).view(S, 1)
    if fam == "valu":
        return (r + 1 if causal else torch.full_like(r, S)), (S - r if causal else torch.full_like(r, S))
    nb = -(-S // BLK)
    blk = torch.floor(r / BLK)
    return BLK * (blk + 1 if causal else torch.full_like(r, nb)), BLK * (nb - blk if causal else torch.full_like(r, nb))


def fwd_bounds(R, op, fam):
    """per-element bounds of out [B][H][S][hd] and lse [B][H][S] for a forward kernel of rounding family `fam`.

    score        ds = scale (roundings(hd) u32 + t3) sum_d |q||k| + 3 u32 |s|            (accumulation, three-term product error, the scale's own
                                                                                          rounding and the multiplication by it)
    weight       every key's weight e_j = exp(s_j - m) reaches out AND l with the same relative error
                     rho_j = ds_j + u32 [(EXP_ULPS + 1)(n_j + x_j)]
                 n_j exponentials with arguments of total magnitude x_j on the way: one in the LDS/VALU kernel (x_j = m - s_j); in the
                 flash loop exp(s_j - M_b) at the key's block b plus one exp(M_b' - M_b'+1) per later block (M_b the running maximum), each
                 with its subtraction's rounding (the + 1); x_j = (M_b - s_j) + (m - M_b).  A common error of numerator and denominator
                 moves out = sum w_j mv_j / sum w_j by at most sum_j A_j rho_j (|mv_j| + |out|) / (1 - max rho): the softmax's sensitivity.
    P -> P V     (u + t3 + 3 u32) sum_j A_d |v|: P rounded to the operand type (three-term: split), the keep scale's multiplication, the
                 normalisation's; fp16: + 2^-25 per key below the normal range.
    P V sum      (roundings(keys visited) + blocks) u32 sum_j A_d |v|                     (+ blocks: o *= alpha once per block)
    l            (l_adds + 5) u32 |out|: the additions into l (flash: 16 + 1 + 2 per block; VALU: ceil(S / 64) + 7), 1 / l within 4 u32, times
    store        gemm_ref.store_bound
    lse = m + log l:  sum_j A_j rho_j / (1 - max rho) + l_adds u32 + LOG_ULPS u32 max(1, log l) + u32 (|lse| + |m|)."""
    q, k, v, s, m, l, A, Ad, mk, live = (R[x] for x in ("q", "k", "v", "s", "m", "l", "A", "Ad", "mk", "live"))
    B, H, S, hd = q.shape
    dev = q.device
    scale = hd ** -0.5
    u = U_OP[op]
    t3 = 3.0 * G.U_BF16 ** 2 if fam == "mfma3" else 0.0
    sf = torch.where(live, s, torch.zeros_like(s))
    ds = scale * (_roundings(fam, hd) * U32 + t3) * (q.abs() @ k.abs().transpose(-1, -2)) + 3.0 * U32 * sf.abs()
    nkeys, _ = _counts(S, R["causal"], fam, dev)
    if fam == "valu":
        nexp = torch.ones_like(sf)
        xabs = m - sf
        l_adds = math.ceil(S / 64) + 7.0
        nblk_row = torch.zeros(S, 1, dtype=torch.float64, device=dev)
    else:
        nb = -(-S // BLK)
        sp = torch.nn.functional.pad(s, (0, nb * BLK - S), value=float("-inf")).view(B, H, S, nb, BLK)
        mrun = torch.cummax(sp.max(-1).values, -1).values                              # [B][H][S][nb]: running maximum after block b
        mrun_j = mrun.repeat_interleave(BLK, -1)[..., :S]
        mrun_j = torch.where(live, mrun_j, m.expand_as(mrun_j))
        nblk_row = nkeys / BLK                                                          # blocks row i visits
        jb = torch.floor(torch.arange(S, device=dev, dtype=torch.float64) / BLK).view(1, S)
        nexp = (nblk_row - jb).clamp_min(1.0).expand_as(sf)
        xabs = (mrun_j - sf) + (m - mrun_j)
        l_adds = 19.0 * nblk_row.view(S)
    rho = torch.where(live, ds + U32 * (EXP_ULPS + 1.0) * (nexp + xabs), torch.zeros_like(sf))
    rmax = rho.max().item()
    assert rmax < 0.25, rmax
    Arho = A * rho
    out = R["out"]
    e1 = ((Arho * mk) @ v.abs() + Arho.sum(-1, keepdim=True) * out.abs()) / (1.0 - rmax)
    sav = Ad @ v.abs()
    e2 = (u + t3 + 3.0 * U32) * sav
    if op == "fp16":
        e2 = e2 + G.FP16_SUBNORMAL_HALF * ((mk * live) @ v.abs())
    e3 = (_roundings(fam, nkeys) + nblk_row) * U32 * sav
    la = torch.as_tensor(l_adds, dtype=torch.float64, device=dev).view(-1, 1) if torch.is_tensor(l_adds) else l_adds
    e4 = (la + 5.0) * U32 * out.abs()
    b_out = _store(out, SECOND_ORDER * (e1 + e2 + e3 + e4), op)
    la1 = la.view(-1) if torch.is_tensor(la) else la
    logl = torch.log(l.squeeze(-1))
    b_lse = SECOND_ORDER * (Arho.sum(-1) / (1.0 - rmax) + la1 * U32) + LOG_ULPS * U32 * logl.clamp_min(1.0) + \
        U32 * (R["lse"].abs() + m.squeeze(-1).abs()) + TINY
    return dict(out=b_out, lse=b_lse)


def bwd_bounds(R, op, fam, delta_from_o, lse_in, o_in):
    """per-element bounds of dq, dk, dv [B][H][S][hd] for a backward kernel of rounding family `fam` that was handed lse_in (fp32) and — where it
    takes delta from it (delta_from_o: the MFMA pair, the fused kernel, the row kernels) — the stored forward output o_in.

    score, dA_d  accumulation (+ three-term) over hd as in fwd_bounds: ds, ddp = (roundings(hd) u32 + t3) sum_d |dO||v|
    A            exp(s - lse_in): relative error rho = ds + u32 (|x| + |lse|) + |lse_in - lse| + EXP_ULPS u32 (1 + |x|), x = s - lse
    delta        from O: sum_d dO o_in, (2 hd + 2) u32 sum_d |dO||o_in| + |sum_d dO (o_in - out)| measured on the handed-in tensor itself;
                 from sum_j A dA: sum_j A (rho |dA| + mk ddp + u32 |dA|) + c u32 sum_j A |dA|, c = 2 ceil(S / 64) + 6 (LDS/VALU: strided lane
                 sums, 6 wave steps) or 19 (three-term kernel: 8 per thread, 3 shuffles)
    dS           scale [A (rho |dA - delta| + mk ddp + d_delta) + 4 u32 A (|dA| + |delta|)], then (u + t3) |dS| for the operand rounding / split
                 (not in the LDS/VALU kernels, which keep dS and P in fp32); fp16: + 2^-25 below the normal range
    dq, dk       |error of dS| times |k| / |q| summed, + roundings(rows visited) u32 sum |dS||k| (|q|)
    dv           A_d (rho + u32 + u + t3) times |dO| summed (+ 2^-25 in fp16), + roundings u32 sum A_d |dO|
    store        gemm_ref.store_bound"""
    q, k, v, do, s, A, Ad, mk, dA, delta, dS, live = (R[x] for x in ("q", "k", "v", "do", "s", "A", "Ad", "mk", "dA", "delta", "dS", "live"))
    B, H, S, hd = q.shape
    dev = q.device
    scale = hd ** -0.5
    u = U_OP[op] if fam != "valu" else 0.0
    t3 = 3.0 * G.U_BF16 ** 2 if fam == "mfma3" else 0.0
    sub = G.FP16_SUBNORMAL_HALF if (op == "fp16" and fam != "valu") else 0.0
    lse = R["lse"].unsqueeze(-1)
    sf = torch.where(live, s, torch.zeros_like(s))
    x = torch.where(live, sf - lse, torch.zeros_like(sf))
    racc = _roundings(fam, hd) * U32 + t3
    ds = scale * racc * (q.abs() @ k.abs().transpose(-1, -2)) + 3.0 * U32 * sf.abs()
    rho = ds + U32 * (x.abs() + lse.abs()) + (lse_in.double().unsqueeze(-1) - lse).abs() + EXP_ULPS * U32 * (1.0 + x.abs())
    rho = torch.where(live, rho, torch.zeros_like(rho))
    assert rho.max().item() < 0.25
    ddp = racc * (do.abs() @ v.abs().transpose(-1, -2))
    if delta_from_o:
        oi = o_in.double()
        d_delta = (2.0 * hd + 2.0) * U32 * (do.abs() * oi.abs()).sum(-1, keepdim=True) + ((do * oi).sum(-1, keepdim=True) - delta).abs()
    else:
        c = 19.0 if fam == "mfma3" else 2.0 * math.ceil(S / 64) + 6.0
        d_delta = (A * (rho * dA.abs() + mk * ddp + U32 * dA.abs())).sum(-1, keepdim=True) + c * U32 * (A * dA.abs()).sum(-1, keepdim=True)
    e_ds = scale * (A * (rho * (dA - delta).abs() + mk * ddp + d_delta) + 4.0 * U32 * A * (dA.abs() + delta.abs()))
    w = SECOND_ORDER * e_ds + (u + t3) * dS.abs() + sub * live
    nkeys, nq = _counts(S, R["causal"], fam, dev)
    b_dq = _store(R["dq"], w @ k.abs() + _roundings(fam, nkeys) * U32 * (dS.abs() @ k.abs()), op)
    b_dk = _store(R["dk"], w.transpose(-1, -2) @ q.abs() + _roundings(fam, nq) * U32 * (dS.abs().transpose(-1, -2) @ q.abs()), op)
    wv = Ad * (SECOND_ORDER * (rho + U32) + u + t3) + sub * mk * live
    b_dv = _store(R["dv"], wv.transpose(-1, -2) @ do.abs() + _roundings(fam, nq) * U32 * (Ad.transpose(-1, -2) @ do.abs()), op)
    return dict(dq=b_dq, dk=b_dk, dv=b_dv)


# ---- the cases both tests walk ------------------------------------------------------------------------------------------------------------
FWD_S = (1, 31, 32, 33, 64, 65, 97, 160, 200)
BWD_S = {64: (32, 33, 64, 65, 97, 160), 96: (32, 33, 64, 65), 128: (32, 33)}
BH = {"flat": (2, 2), "peaked": (3, 3), "rising": (3, 2), "offset": (2, 3)}      # B H ceil(S / 32) takes every residue mod 4 over the S list
DROPS = ((0.1, 0x1234567, 3, "flat"), (0.5, 0x1234567, 3, "peaked"), (0.1, 0xFEDCBA9876543, 11, "rising"), (0.5, 0xFEDCBA9876543, 11, "offset"))


class Case:
    def __init__(self, family, hd, S, causal, bwd, mfma_bwd=True, p=0.0, seed=0, layer=0, BH_=None):
        self.family, self.hd, self.S, self.causal, self.bwd, self.mfma_bwd, self.p, self.seed, self.layer = family, hd, S, causal, bwd, mfma_bwd, p, seed, layer
        self.B, self.H = BH_ or BH[family]

    @property
    def id(self):
        return f"{self.family}-hd{self.hd}-S{self.S}-B{self.B}H{self.H}-{'causal' if self.causal else 'full'}" + \
            (f"-p{self.p}-seed{self.seed:x}-layer{self.layer}" if self.p else "") + ("" if self.mfma_bwd else "-ldsbwd")

    def inputs(self):
        return make_inputs(self.family, self.B, self.S, self.H, self.hd, self.S * 1009 + self.hd * 7 + self.causal + FAMILIES.index(self.family) * 131)


def plain_cases():
    out = []
    for fam in FAMILIES:
        for hd in (64, 96, 128):
            for S in FWD_S:
                for causal in (0, 1):
                    out.append(Case(fam, hd, S, causal, bwd=S in BWD_S[hd]))
        for hd in (8, 40):                       # LDS/VALU kernels in every build; o and delta_ws NULL
            for S in (7, 31, 32, 50):
                for causal in (0, 1):
                    out.append(Case(fam, hd, S, causal, bwd=True, mfma_bwd=False))
    return out


def dropout_cases(op):
    out = []
    for p, seed, layer, fam in DROPS:
        for hd in (64, 96, 128):
            for S in FWD_S:
                # (the split-bf16 build's row kernels carry no dropout: head dim 64 beyond the LDS tile refuses, tested as a refusal)
                out.append(Case(fam, hd, S, 1, bwd=S in BWD_S[hd] and "rows" not in paths(op, S, hd)[1][0], p=p, seed=seed, layer=layer))
        if op == "x3":                           # the VALU kernels carry dropout in the split-bf16 build only
            for S in (17, 40):
                out.append(Case(fam, 32, S, 1, bwd=True, mfma_bwd=False, p=p, seed=seed, layer=layer))
    return out
