"""float64 reference of the sampling step cc_sample_step / cc_sample_step_lp (clipcap_amd/csrc/sample.hip: k_sample_rows), the admissible
cuts and per-element bounds the GPU test holds the kernel to (tests/test_gpu_sample_ref.py), an fp32 emulation of the kernel's rule with
the defects those checks must catch, and the case list both tests walk.  numpy only, no GPU needed; tests/test_sample_ref.py pins this
module itself.  It stands to the sampler as tests/decode_ref.py stands to the decode attention and reuses attn_ref's constants.

Definition (one row; sample.hip).  Everything that decides ORDER is exact fp32 arithmetic, reproduced here bit for bit:
    value     v_i = fl32(pen(x_i) * fl32(1 / T)),  pen(x) = x * rep (x < 0) or x / rep, applied ONCE to every token id that occurs in
              history[:hist_len] and lies in [0, V); no penalty with an empty history or rep == 1
    order     value descending, index ascending; -0.0 == +0.0
    top-k     0 < k < V: mode 0 keeps the first k of the order; mode 1 every element >= the k-th value.  A prefix of the order, length K
    top-p     top_p > 0: masses e_i = exp(v_i - max v) over that order; mode 0: the minimal prefix with mass >= top_p * sum of ALL V masses
              (never empty); mode 1: the minimal prefix with mass > top_p * mass of the top-k set; a prefix that never gets there: all K
    length    stop >= 0 and a non-empty history: a kept token in the history whose value == float(stop) becomes fl32(v * len_pen)
    result    p = softmax of the final values over the kept set; the token is the inverse CDF of p in INDEX order at
              min(max(u, 0), 0.99999994).  A row of only -inf: p = 0 everywhere, token 0.

Only the masses go through the device's __expf, as 2^-32 fixed point: w_i = trunc(fl32(__expf(fl32(v_i - m)) * S)), S = 4294967040.  Error
of one weight against S e_i, counted where it happens (u32 = 2^-24):
    fl32(v - m)            |x| u32 of the argument, the same relative error in the weight           x = v - m <= 0
    __expf                 attn_ref.EXP_ULPS u32 (1 + |x|): attn_ref's measured allowance, same device function, arguments inside its range
    times S                one rounding, u32
    truncation             below one unit, absolute
so |w_i - S e_i| <= S e_i rho_i + 1, rho_i = SECOND_ORDER u32 (EXP_ULPS (1 + |x|) + |x| + 1).  An element with x = 0 or x = -inf carries
no error at all (__expf(0) == 1, __expf(-inf) == 0, S is an fp32 number): rows whose candidates all sit at the maximum are EXACT, and the
GPU test asserts the two facts through their probabilities.  A cumulative device mass C_n differs from c_n = S * (float64 prefix sum) by at
most dC_n = the sum of its elements' errors; the device target trunc(double(top_p) * Z) differs from T = top_p * S * (float64 Z) by at most
top_p * dZ + 1 (the truncation; 0 when Z is exact and top_p * Z an integer).  The prefix's weights are part of Z, so the comparison's
two sides share them: C_n - target = (1 - top_p) (prefix weights) - top_p (the rest of Z), and its error is at most
    d_n = |1 - top_p| dC_n + top_p (dZ - dC_n) + 1          (never more than dC_n + top_p dZ + 1, the two sides taken apart)
(plus (c_n + T) 2^-40 for the rounding of the float64 sums and of the double product here: below 2^-7 unit, absent on exact rows)
A prefix length n is ADMISSIBLE when
    mode 0:  c_{n-1} < T + d_{n-1}   and   c_n >= T - d_n            mode 1:  the same with <= and >
(n = K needs the first half only: never reached = everything kept).  The order already puts equal values in index order, so a cut inside
a group of equal values is counted in members of the group.  check_row() holds a kernel result to: support == the first n of the order
for an admissible n (tokens whose weight may truncate to 0 excepted), every probability within the bound of RowRef.final() of the float64 softmax over
that set, the drawn token's float64 CDF interval (widened by the weights' errors) containing the clamped u.  Nothing is tuned to what
the kernel returns."""
from fractions import Fraction

import numpy as np

from tests import attn_ref as A

U32 = 2.0 ** -24
S = 4294967040.0                          # 2^32 - 256: the largest fp32 below 2^32
DIV_ROUNDINGS = 5.0                       # 1 / total within 4 u32 and one multiplication (attn_ref.fwd_bounds, "l")
NW, WAVE_STEP = 16, 64                    # index-order work: 16 wave ranges, each a multiple of 64 long
U_MAX = np.float32(0.99999994)
LDS_LIMIT = 150 * 1024
F32 = np.float32


def lds_bytes(V):
    """the kernel's dynamic LDS (the layout at the top of k_sample_rows): hist_w[2048] u64 | red[16 + 2] u64 | hist_n[2048] u32 | bcast[4] u32 |
    fred[16] f32 | fred2[16] f32 | bitmap[ceil(V / 32)] u32"""
    return 2048 * 8 + (16 + 2) * 8 + 2048 * 4 + 4 * 4 + 16 * 4 + 16 * 4 + (V + 31) // 32 * 4


def wave_range(V):
    """length of one wave's index range"""
    return ((V + NW - 1) // NW + WAVE_STEP - 1) // WAVE_STEP * WAVE_STEP


class Params:
    def __init__(self, temperature=1.0, top_k=0, top_p=0.0, mode=0, rep_pen=1.0, hist_len=0, stop_tok=-1, len_pen=1.0):
        self.temperature, self.top_k, self.top_p, self.mode = float(temperature), int(top_k), F32(top_p), int(mode)
        self.rep_pen, self.hist_len, self.stop_tok, self.len_pen = F32(rep_pen), int(hist_len), int(stop_tok), F32(len_pen)

    @property
    def inv_temp(self):
        return F32(1.0) / F32(self.temperature) if self.temperature > 0 else F32(1.0)


def _bitmap(V, hist, hist_len):
    bm = np.zeros(V, dtype=bool)
    if hist is not None and hist_len > 0:
        h = np.asarray(hist[:hist_len], dtype=np.int64)
        bm[h[(h >= 0) & (h < V)]] = True
    return bm


def _pen(v, rep):
    with np.errstate(invalid="ignore"):
        return np.where(v < 0, v * rep, v / rep).astype(F32)


def row_values(x, P, hist):
    """(v fp32 [V], bitmap): the element values exactly as the kernel defines them"""
    x = np.asarray(x, dtype=F32)
    bm = _bitmap(x.size, hist, P.hist_len)
    v = x
    if P.hist_len > 0 and hist is not None and P.rep_pen != F32(1.0):
        v = np.where(bm, _pen(x, P.rep_pen), x).astype(F32)
    return (v * P.inv_temp).astype(F32), bm


def _weights(v, m):
    """float64 masses e = exp(v - m) and the bound on |device weight - S e| (module docstring)"""
    with np.errstate(invalid="ignore", over="ignore"):
        x = v.astype(np.float64) - float(m)
        e = np.exp(x)
    ax = np.where(np.isfinite(x), -x, 0.0)
    err = S * e * A.SECOND_ORDER * U32 * (A.EXP_ULPS * (1.0 + ax) + ax + 1.0) + 1.0
    err = np.where((x == 0.0) | (x == -np.inf), 0.0, err)
    return e, err


class RowRef:
    """the float64 reference of one row"""

    def __init__(self, x, P, hist, u):
        self.P, self.V = P, int(np.asarray(x).size)
        V = self.V
        self.v, self.bm = row_values(x, P, hist)
        v = self.v
        self.order = np.argsort(-v, kind="stable")               # -(-0.0) == +0.0 compare equal: ties stay in index order
        self.rank = np.empty(V, dtype=np.int64)
        self.rank[self.order] = np.arange(V)
        self.m = v.max()
        self.dead = not np.isfinite(self.m) and self.m < 0        # only -inf
        k = P.top_k
        if 0 < k < V:
            kth = v[self.order[k - 1]]
            self.K = k if P.mode == 0 else int((v >= kth).sum())
        else:
            self.K = V
        K = self.K
        self.uu = float(min(max(F32(u), F32(0.0)), U_MAX))
        self.slp = P.stop_tok >= 0 and P.hist_len > 0 and hist is not None
        if self.dead:
            self.adm = np.zeros(K + 1, dtype=bool)
            self.adm[K] = True
            return
        e, err = _weights(v, self.m)
        es, errs = e[self.order[:K]], err[self.order[:K]]
        self.c = np.concatenate(([0.0], S * np.cumsum(es)))
        self.dC = np.concatenate(([0.0], np.cumsum(errs)))
        self.adm = np.zeros(K + 1, dtype=bool)
        if not P.top_p > 0:
            self.adm[K] = True
            self.T = None
            return
        tp = float(P.top_p)
        if P.mode == 0:
            Z, dZ = S * e.sum(), err.sum()
        else:
            Z, dZ = self.c[K], self.dC[K]
        T = tp * Z
        whole = dZ == 0.0 and (Fraction(tp) * int(round(Z))).denominator == 1 and Fraction(tp) * int(round(Z)) < 2 ** 53
        # C_n - target = (1 - top_p) * (the prefix's weights) - top_p * (the other weights of Z): every weight's error counted once, with the
        # coefficient it really has; the target's truncation; the rounding of the float64 sums here and of the device's double product
        c = self.c
        d = abs(1.0 - tp) * self.dC + tp * (dZ - self.dC) + (0.0 if whole else 1.0 + (c + T) * 2.0 ** -40)
        self.T, self.d = T, d
        n = np.arange(1, K + 1)
        if P.mode == 0:
            before, through = c[n - 1] < T + d[n - 1], c[n] >= T - d[n]
        else:
            before, through = c[n - 1] <= T + d[n - 1], c[n] > T - d[n]
        through[K - 1] = True
        self.adm[1:] = before & through
        assert self.adm.any()

    @property
    def exact(self):
        return int(self.adm.sum()) == 1

    def kept(self, n):
        return self.order[:n]

    def final(self, n):
        """dict(p float64 [V], bound [V], may_zero bool [V], E [V + 1] index-order cumulative masses, slack) for the kept prefix n"""
        V, v, P = self.V, self.v, self.P
        ks = np.zeros(V, dtype=bool)
        ks[self.order[:n]] = True
        f = v
        if self.slp:
            f = np.where(self.bm & (v == F32(P.stop_tok)), (v * P.len_pen).astype(F32), v).astype(F32)
        m2 = f[ks].max() if self.slp else self.m
        e, err = _weights(f, m2)
        e, err = np.where(ks, e, 0.0), np.where(ks, err, 0.0)
        tot, dtot = e.sum(), err.sum()
        p = e / tot
        rel = A.SECOND_ORDER * ((2.0 + DIV_ROUNDINGS) * U32 + dtot / (S * tot))          # (float)w, (float)total, the reciprocal and the product
        bound = np.where(ks, err / (S * tot) + p * rel + A.TINY, 0.0)
        may_zero = ks & (S * e - err < 1.0) & (err > 0)
        return dict(p=p, bound=bound, may_zero=may_zero | ~np.isfinite(f), E=np.concatenate(([0.0], np.cumsum(e))), slack=2.0 * dtot / S, ks=ks)


def check_row(ref, probs, token):
    """Hold one row's result to the reference.  probs: fp32 [V] or None.  Returns (worst err / bound, n used).  AssertionError otherwise."""
    V = ref.V
    token = int(token)
    if ref.dead:
        assert token == 0, f"a row of only -inf draws token 0, not {token}"
        assert probs is None or not np.any(probs), "a row of only -inf has probability 0 everywhere"
        return 0.0, ref.K
    assert 0 <= token < V, f"token {token} outside [0, {V})"
    if probs is not None:
        probs = np.asarray(probs)
        assert np.isfinite(probs).all(), "non-finite probability"
        sup = probs > 0
        assert sup.any(), "empty support"
        n_min = int(ref.rank[sup].max()) + 1
        assert n_min <= ref.K, f"support reaches rank {n_min} of the order, the top-k set ends at {ref.K}"
    else:
        n_min = int(ref.rank[token]) + 1
    ok = n_min + np.flatnonzero(ref.adm[n_min:])
    lens = np.flatnonzero(ref.adm)
    assert ok.size, f"support needs a prefix of {n_min}, admissible: {lens[0]} .. {lens[-1]}"
    n = int(ok[0])
    if probs is None:
        return 0.0, _check_token_alone(ref, token, ok)
    fin = ref.final(n)
    sup = probs > 0
    lost = fin["ks"] & ~sup & ~fin["may_zero"]
    assert not lost.any(), f"prefix {n} (admissible {lens[0]} .. {lens[-1]}): kept tokens {np.flatnonzero(lost)[:8]} have probability 0"
    err = np.abs(probs.astype(np.float64) - fin["p"])
    assert not np.any(probs[~fin["ks"]]), "probability outside the kept set"
    ratio = np.where(fin["ks"], err / np.where(fin["bound"] > 0, fin["bound"], 1.0), 0.0)
    worst = float(ratio.max())
    at = int(ratio.argmax())
    assert worst <= 1.0, f"p[{at}] = {probs[at]!r}, float64 {fin['p'][at]!r}: err / bound = {worst:.3f}"
    assert sup[token], f"token {token} has probability 0"
    assert fin["ks"][token], f"token {token} is not in the kept set (prefix {n})"
    why = _token_outside(ref, fin, fin, token)
    assert why is None, why
    return worst, n


def _token_outside(ref, fa, fb, token):
    """None when u * total can lie in the token's CDF interval for a kept prefix between those of fa and fb (the same: exactly that one),
    else the message.  Every quantity grows with the prefix, so the interval's ends are taken at the favourable side.  The device compares
    integers: trunc(u * total) in [lo, lo + w), each side within the sum of the weights' errors of its float64 value."""
    V = ref.V
    sl = max(fa["slack"], fb["slack"])
    sl = sl + 1.0 / S if sl > 0 else 0.0
    lo, hi = fa["E"][token], fb["E"][token + 1]
    qa, qb = ref.uu * fa["E"][V], ref.uu * fb["E"][V]
    if lo - sl <= qb and (qa < hi + sl if sl > 0 else qa < hi):
        return None
    return f"token {token}: u * total = {qa!r} .. {qb!r} outside its CDF interval [{lo!r}, {hi!r}) +- {sl:.3g}"


def _check_token_alone(ref, token, lens):
    """a call without probs_out: the token must be the draw for SOME admissible prefix length that holds it.  -> the first that fits"""
    if lens.size > 64 and not ref.slp:           # a row cut at top_p = 1: thousands of lengths that differ by weights of a unit or two
        fa, fb = ref.final(int(lens[0])), ref.final(int(lens[-1]))
        why = _token_outside(ref, fa, fb, token)
        assert why is None, why
        return int(lens[0])
    why = None
    for n in lens:
        fin = ref.final(int(n))
        why = _token_outside(ref, fin, fin, token)
        if why is None:
            return int(n)
    raise AssertionError(f"{why} (prefix {lens[0]} .. {lens[-1]})")


# ---- fp32 emulation of the kernel's rule, and the defects ---------------------------------------------------------------------------------
DEFECTS = ("mode0_strict", "mode1_not_strict", "mode0_mass_of_topk", "mode0_all_topk_ties", "mode1_exactly_k", "ties_reverse_index",
           "topp_ties_all_kept", "penalty_after_temperature", "duplicate_penalised_twice", "draw_in_sorted_order", "u_not_clamped",
           "wave_prefix_dropped", "ld_taken_as_V", "negative_zero_below_zero", "final_maximum_only_raised")
NONE = 0xFFFFFFFF


def _keys(v, canonical):
    u = v.view(np.uint32).astype(np.int64)
    if canonical:
        u = np.where((u & 0x7FFFFFFF) == 0, 0, u)
    return np.where(u & 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000)


def _fix(v, m):
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.exp((v - m).astype(F32)).astype(F32) * F32(S)
    return np.where(np.isfinite(w), w, 0).astype(np.int64)         # trunc; NaN -> 0 as v_cvt_u32_f32 does


def _locate(nth, pred, V, drop_prefix):
    """index of the nth (1-based) True of pred in index order, found wave range by wave range as the kernel does"""
    CW, base = wave_range(V), 0
    for w in range(NW):
        lo, hi = w * CW, min(V, (w + 1) * CW)
        if lo >= hi:
            break
        idx = np.flatnonzero(pred[lo:hi])
        if nth > 0 and base < nth <= base + idx.size:
            return lo + int(idx[nth - base - 1])
        if not drop_prefix:
            base += idx.size
    return NONE


def emulate_row(x, P, hist, u, defect=None):
    """(token, probs fp32 [V]) by the kernel's passes in fp32 with integer masses.  defect: one of DEFECTS (not ld_taken_as_V: emulate_case)."""
    x = np.asarray(x, dtype=F32)
    V, mode = x.size, P.mode
    idx = np.arange(V)
    bm = _bitmap(V, hist, P.hist_len)
    use_rep = P.hist_len > 0 and hist is not None and P.rep_pen != F32(1.0)
    times = bm.astype(np.int64)
    if defect == "duplicate_penalised_twice" and use_rep:
        h = np.asarray(hist[:P.hist_len], dtype=np.int64)
        times = np.bincount(h[(h >= 0) & (h < V)], minlength=V)
    v = x
    if defect == "penalty_after_temperature":
        v = (v * P.inv_temp).astype(F32)
    for t in range(int(times.max()) if use_rep else 0):
        v = np.where(times > t, _pen(v, P.rep_pen), v).astype(F32)
    if defect != "penalty_after_temperature":
        v = (v * P.inv_temp).astype(F32)
    key = _keys(v, defect != "negative_zero_below_zero")
    order = np.lexsort((-idx if defect == "ties_reverse_index" else idx, -key))
    m = v.max()
    w = _fix(v, m)
    k = P.top_k
    use_k = 0 < k < V
    K = V
    if use_k:
        Tk = key[order[k - 1]]
        every = (mode == 1) != (defect in ("mode0_all_topk_ties", "mode1_exactly_k") and defect.startswith("mode%d" % mode))
        K = int((key >= Tk).sum()) if every else k
    cand = order[:K]
    n = K
    if P.top_p > 0:
        Z = int(w.sum()) if (mode == 0 and defect != "mode0_mass_of_topk") else int(w[cand].sum())
        target = int(float(P.top_p) * float(Z))
        if mode == 0 and target == 0:
            target = 1
        strict = (mode == 1) != (defect in ("mode0_strict", "mode1_not_strict") and defect.startswith("mode%d" % mode))
        cum = np.cumsum(w[cand])
        hit = np.flatnonzero(cum > target if strict else cum >= target)
        if hit.size and not (target == 0 and not strict):
            n = int(hit[0]) + 1
            if defect == "topp_ties_all_kept":
                n = int((key[cand] >= key[cand[n - 1]]).sum())
    if defect == "ties_reverse_index":
        ks = np.zeros(V, dtype=bool)
        ks[order[:n]] = True
    else:       # membership as the kernel holds it: a threshold key and the index of the last tie kept, found wave range by wave range
        drop = defect == "wave_prefix_dropped"

        def prefix_set(members, length, inside):
            if length == 0:
                return np.zeros(V, dtype=bool)
            T_ = key[members[length - 1]]
            ties = inside & (key == T_)
            keep = length - int((inside & (key > T_)).sum())
            last = _locate(keep, ties, V, drop) if 0 < keep < int(ties.sum()) else NONE
            return inside & ((key > T_) | (ties & (idx <= last)))
        topk = prefix_set(order, K, np.ones(V, dtype=bool))
        ks = prefix_set(order, n, topk) if n < K else topk
    f = v
    slp = P.stop_tok >= 0 and P.hist_len > 0 and hist is not None
    if slp:
        f = np.where(bm & (v == F32(P.stop_tok)), (v * P.len_pen).astype(F32), v).astype(F32)
    m2 = f[ks].max() if (slp and ks.any()) else m
    if defect == "final_maximum_only_raised":
        m2 = max(m, m2)
    wf = np.where(ks, _fix(f, m2), 0)
    total = int(wf.sum())
    uu = F32(u) if defect == "u_not_clamped" else min(max(F32(u), F32(0.0)), U_MAX)
    pick = float(uu) * float(total)
    pick = int(pick) if 0 <= pick < 2.0 ** 63 else -1
    tok = 0
    if defect == "draw_in_sorted_order":
        cum = np.cumsum(wf[order])
        j = int(np.searchsorted(cum, pick, side="right"))
        tok = int(order[j]) if 0 <= pick < total else 0
    elif defect == "wave_prefix_dropped":
        CW = wave_range(V)
        for wv in range(NW):
            lo, hi = wv * CW, min(V, (wv + 1) * CW)
            if lo < hi and 0 <= pick < int(wf[lo:hi].sum()):
                tok = lo + int(np.searchsorted(np.cumsum(wf[lo:hi]), pick, side="right"))
                break
    elif 0 <= pick < total:
        tok = int(np.searchsorted(np.cumsum(wf), pick, side="right"))
    inv = F32(1.0) / F32(total) if total > 0 else F32(0.0)
    return tok, (wf.astype(F32) * inv).astype(F32)


# ---- cases --------------------------------------------------------------------------------------------------------------------------------
PAD = 13                                  # ld = V + PAD, the padding holds NaN
HIST_PAD = 3                              # hist_ld = hist_len + HIST_PAD, the padding holds ids a stray read would penalise


class Case:
    """one launch: rows x [R][V] fp32, history [R][hist_ld] int64 (or None), u [R] fp32, the call's parameters"""

    def __init__(self, name, kind, x, P, u, hist=None):
        self.name, self.kind, self.P = name, kind, P
        self.x = np.ascontiguousarray(x, dtype=F32)
        self.R, self.V = self.x.shape
        self.u = np.asarray(u, dtype=F32)
        self.hist = hist
        assert self.u.shape == (self.R,) and self.R <= 8
        assert hist is None or hist.shape == (self.R, P.hist_len + HIST_PAD)
        self._refs = None

    @property
    def ld(self):
        return self.V + PAD

    @property
    def hist_ld(self):
        return self.P.hist_len + HIST_PAD

    def padded(self):
        buf = np.full((self.R, self.ld), np.nan, dtype=F32)
        buf[:, :self.V] = self.x
        return buf

    def h(self, r):
        return None if self.hist is None else self.hist[r]

    def refs(self):
        """the rows' references, computed once and shared"""
        if self._refs is None:
            self._refs = [RowRef(self.x[r], self.P, self.h(r), self.u[r]) for r in range(self.R)]
        return self._refs


def emulate_case(c, defect=None):
    """(tokens [R], probs [R][V]) of the fp32 emulation on the buffers a launch is handed"""
    buf = c.padded()
    if defect == "ld_taken_as_V":
        flat = np.nan_to_num(buf.reshape(-1), nan=0.0)
        rows = [flat[r * c.V:(r + 1) * c.V] for r in range(c.R)]
        defect = None
    else:
        rows = [buf[r, :c.V] for r in range(c.R)]
    out = [emulate_row(rows[r], c.P, c.h(r), c.u[r], defect) for r in range(c.R)]
    return np.array([t for t, _ in out]), np.stack([p for _, p in out])


def check_case(c, tokens, probs):
    """-> (worst err / bound, rows decided exactly).  probs None: tokens only."""
    worst, exact = 0.0, 0
    for r, ref in enumerate(c.refs()):
        try:
            w, _ = check_row(ref, None if probs is None else probs[r], tokens[r])
        except AssertionError as e:
            raise AssertionError(f"{c.name} row {r}: {e}") from None
        worst, exact = max(worst, w), exact + ref.exact
    return worst, exact


def _place(n, V, where):
    """n ascending indices: front = inside wave range 0 (more than one 256-element step when n allows), spread = over the whole row (the
    cut lands in a middle wave), back = inside the last populated wave range (every earlier range holds nothing)"""
    CW = wave_range(V)
    last = (V - 1) // CW * CW
    lo, hi = {"front": (0, min(CW, V)), "spread": (0, V), "back": (last, V)}[where]
    assert hi - lo >= n, (n, V, where)
    pos = lo + (np.arange(n) * (hi - lo)) // n + ((hi - lo) // n - 1) // 2
    assert np.unique(pos).size == n and pos.max() < V
    return pos


def _tied_row(V, pos, value=1.5):
    x = np.full(V, -np.inf, dtype=F32)
    x[pos] = value
    return x


def _exact_rows(V):
    """(n, where) of up to 8 different rows of equal candidates at this V: every n of 4, 8, 64, 300 and every placement that fits"""
    CW = wave_range(V)
    last_len = V - (V - 1) // CW * CW
    if V <= WAVE_STEP:                                          # one wave range: the placements coincide
        return [(n, "spread") for n in (4, 8, 64) if n <= V]
    pref = [(300, "front"), (300, "back"), (64, "spread"), (64, "back"), (8, "front"), (8, "back"), (4, "spread"), (4, "back"), (300, "spread"),
            (64, "front"), (8, "spread"), (4, "front")]
    fits = [(n, wh) for n, wh in pref if n <= V and (wh != "front" or n <= min(CW, V)) and (wh != "back" or n <= last_len)]
    return fits[:8]


def exact_cases():
    """rows whose candidates all share one value: every weight is S, delta = 0, every cut and every draw decided"""
    out = []
    for V in (4, 64, 97, 1000, 4099, 50257):
        rows = _exact_rows(V)
        x = np.stack([_tied_row(V, _place(n, V, wh)) for n, wh in rows])
        u = (np.arange(len(rows)) + 0.5) / len(rows)
        for mode in (0, 1):
            for tp in (0.25, 0.5, 0.75):
                out.append(Case(f"exact-V{V}-p{tp}-m{mode}", "exact", x, Params(top_p=tp, mode=mode), u))
            out.append(Case(f"exact-V{V}-k3-p0.5-m{mode}", "exact", x, Params(top_k=3, top_p=0.5, mode=mode, temperature=0.5), u))
            out.append(Case(f"exact-V{V}-k3-m{mode}", "exact", x, Params(top_k=3, mode=mode), u))
        out.append(Case(f"exact-V{V}-tiny-p", "exact", x, Params(top_p=2.0 ** -44, mode=0), u))
    return out


def singleton_cases():
    """a higher singleton (weight S, exact) plus 8 ties one below it (weight S / e): top_k = 6 keeps 5 of the 8 ties and top_p = 0.5 cuts
    inside those: the top-k and the top-p tie counters are both partial at once.  Margins of 0.1 S against a delta of a few units."""
    out = []
    for V in (64, 4099, 50257):
        rows = []
        for wh in ("front", "spread", "back"):
            if wh == "front" and V == 64:
                continue
            pos = _place(9, V, wh)
            for top in (0, 4, 8):
                x = _tied_row(V, pos, 1.0)
                x[pos[top]] = 2.0
                rows.append(x)
        x = np.stack(rows[:8])
        u = (np.arange(len(x)) + 0.25) / len(x)
        for mode in (0, 1):
            out.append(Case(f"singleton-V{V}-m{mode}", "exact", x, Params(top_k=6, top_p=0.5, mode=mode), u))
    return out


def draw_cases():
    """draws on rows of n equal candidates, nothing cut: token j of the kept set for EVERY j of n = 4, 8, 64, 300 (u = (j + 0.5) / n, eight
    to a launch), both ends of intervals (n = 8), the clamp"""
    out = []
    for V, wh in ((4099, "back"), (50257, "spread"), (97, "spread")):
        for n in (4, 8):
            x = np.stack([_tied_row(V, _place(n + (j % 2), V, wh)[:n] + j) for j in range(n)])      # every row its own positions
            out.append(Case(f"draw-V{V}-{wh}-n{n}-mid", "draw", x, Params(), (np.arange(n) + 0.5) / n))
        x = np.stack([_tied_row(V, _place(8, V, wh) + j) for j in range(8)])
        ends = [F32(j) / F32(8) for j in (1, 3, 5, 7)]
        out.append(Case(f"draw-V{V}-{wh}-n8-ends", "draw", x, Params(), ends + [np.nextafter(e, F32(0)) for e in ends]))
        out.append(Case(f"draw-V{V}-{wh}-n8-clamp", "draw", x[:5], Params(mode=1), [0.0, -1.0, 1.0, 2.0, U_MAX]))
        for n in (64, 300):
            if n > V or (wh == "back" and n > V - (V - 1) // wave_range(V) * wave_range(V)):
                continue
            pos = _place(n, V, wh)
            x = np.stack([_tied_row(V, pos + (i if pos.max() + 7 < V else i % 2)) for i in range(8)])
            for j0 in range(0, n, 8):            # every j, eight to a launch
                js = np.arange(j0, min(j0 + 8, n))
                out.append(Case(f"draw-V{V}-{wh}-n{n}-j{j0}", "draw", x[:js.size], Params(mode=1), (js + 0.5) / n))
    return out


def zero_cases():
    """[3, 2, +0.0, -0.0, -1, ...] and its mirror: equal floats are equal whatever their sign bit"""
    out = []
    for V in (64, 4099):
        rows = []
        for a, b in ((0.0, -0.0), (-0.0, 0.0)):
            x = np.full(V, -2.0, dtype=F32) - np.arange(V, dtype=F32) / V
            x[:5] = [3.0, 2.0, a, b, -1.0]
            rows.append(x)
            y = x[::-1].copy()                                   # the same row back to front: the zeros in the last wave range
            rows.append(y)
        for mode in (0, 1):
            out.append(Case(f"zero-V{V}-m{mode}", "zero", np.stack(rows), Params(top_k=3, mode=mode), [0.1, 0.95, 0.6, 0.99]))
    return out


ROW_KINDS = ("gauss", "gauss_wide", "grid", "far", "equal", "banned", "one_left", "dead")
# temperature, top_k (-1: V - 1, -2: V, -3: V + 5), top_p, mode, history length (0: no history), V's
COMBOS = (
    (1.0, 0, 0.8, 0, 0, (97, 50257)), (0.7, 40, 0.5, 0, 6, (1000, 4099)), (1.3, 0, 0.95, 0, 1500, (50257, 64)), (1.0, 0, 1.0, 0, 0, (1000, 4)),
    (1.0, 0, 0.05, 0, 6, (4099, 97)), (1.0, 1, 0.8, 0, 0, (64, 50257)), (0.7, -1, 0.5, 0, 0, (97, 1000)), (1.3, -2, 0.8, 0, 6, (4, 4099)),
    (1.0, -3, 0.95, 0, 0, (64, 1000)), (1.0, 40, 0.0, 0, 1500, (4099, 97)), (1.0, 0, 0.0, 0, 6, (4, 50257)), (0.7, 40, 1.0, 0, 0, (1000, 64)),
    (1.0, 0, 0.8, 1, 6, (97, 50257)), (0.7, 40, 0.5, 1, 0, (1000, 4099)), (1.3, 0, 0.95, 1, 0, (50257, 64)), (1.0, 0, 1.0, 1, 6, (1000, 4)),
    (1.0, 0, 0.05, 1, 0, (4099, 97)), (1.0, 1, 0.8, 1, 6, (64, 50257)), (0.7, -1, 0.5, 1, 1500, (97, 1000)), (1.3, -2, 0.8, 1, 0, (4, 4099)),
    (1.0, -3, 0.95, 1, 6, (64, 1000)), (1.0, 40, 0.0, 1, 0, (4099, 97)), (1.0, 0, 0.0, 1, 1500, (4, 50257)), (1.3, 40, 0.8, 1, 6, (50257, 1000)),
)
SCALE = {4: 2.0, 64: 2.0, 97: 3.0, 1000: 4.0, 4099: 5.0, 50257: 6.0}
SEED0 = 20
SALT = {}            # (combo, V) -> a further seed offset, see random_cases()


def _random_rows(V, rng):
    sc = SCALE[V]
    rows = {}
    rows["gauss"] = rng.standard_normal(V) * sc
    rows["gauss_wide"] = rng.standard_normal(V) * 5.0
    rows["grid"] = np.round(rng.standard_normal(V) * 3.0 * 4.0) / 4.0
    rows["far"] = rng.standard_normal(V) * sc
    rows["far"][int(rng.integers(V))] = -1e4
    rows["equal"] = np.full(V, F32(rng.standard_normal() * 3.0))
    rows["banned"] = rng.standard_normal(V) * sc
    rows["banned"][rng.choice(V, size=min(5, V - 1), replace=False)] = -np.inf
    rows["one_left"] = np.full(V, -np.inf)
    rows["one_left"][int(rng.integers(V))] = rng.standard_normal() * sc
    rows["dead"] = np.full(V, -np.inf)
    return np.stack([rows[k] for k in ROW_KINDS]).astype(F32)


def _history(x, hl, rng):
    """[R][hl + HIST_PAD]: random ids with duplicates, -1 and V among them, the row's largest tokens (what a penalty moves most) in the first
    places — and, as poison, the NEXT largest in the padding beyond hist_len"""
    R, V = x.shape
    h = rng.integers(0, V, size=(R, hl + HIST_PAD))
    top = np.argsort(-x, axis=1, kind="stable")
    nt = min(2, V)
    h[:, :nt] = top[:, :nt]
    h[:, 2] = h[:, 0]                                            # a duplicate
    h[:, 3], h[:, 4] = -1, V
    h[:, hl:] = top[:, nt:nt + HIST_PAD] if V >= nt + HIST_PAD else top[:, nt:nt + 1]
    return h.astype(np.int64)


def random_cases():
    out = []
    for i, (T, k, tp, mode, hl, Vs) in enumerate(COMBOS):
        for V in Vs:
            rng = np.random.default_rng(SEED0 + 1000 * i + V + 100000 * SALT.get((i, V), 0))
            x = _random_rows(V, rng)
            kk = {-1: V - 1, -2: V, -3: V + 5}.get(k, k)
            hist = _history(x, hl, rng) if hl else None
            P = Params(temperature=T, top_k=kk, top_p=tp, mode=mode, rep_pen=1.2 if hl else 1.0, hist_len=hl)
            out.append(Case(f"random-V{V}-T{T}-k{kk}-p{tp}-m{mode}-h{hl}", "random", x, P, rng.random(len(x)), hist))
    return out


def length_cases():
    """the sentence-length penalty: history tokens whose value == float(stop) are scaled after the cut.  raise: 5 * 3 = 15 tops the row
    (final maximum above the row maximum in every row); shrink: the row's maximum itself is the stop value and halves — in the even rows
    every maximal token fires and the final maximum lies BELOW the row maximum; the odd rows carry stop-valued poison beyond hist_len
    (a stray read of the history would scale it), which stays at 5.0.  rep 2.0 with a logit of 10 gives the 5.0 through the penalty.
    deep: nothing is cut, one to three fired maxima at 5.0 -> 2.5 and every other token 19 to 21 below the old maximum: relative to the
    right maximum those weights are 100 to 300 units, relative to the old one 9 to 24 — a kernel that lets the second maximum only rise
    leaves their bounds by its coarser truncation."""
    out = []
    stop = 5
    for V in (97, 4099, 50257):
        for what, lp, rep in (("raise", 3.0, 1.0), ("shrink", 0.5, 1.0), ("raise", 3.0, 2.0)):
            for mode in (0, 1):
                rng = np.random.default_rng(7000 + V + mode + int(lp * 10) + int(rep))
                x = np.minimum(rng.standard_normal((6, V)) * 2.0, 4.5).astype(F32)
                x[1] = np.round(x[1] * 4.0) / 4.0
                hl = 6
                hist = rng.integers(0, V, size=(6, hl + HIST_PAD)).astype(np.int64)
                hist[:, 3] = hist[:, 0]
                hist[:, 4] = V
                for r in range(6):
                    live = np.unique(hist[r, :hl][hist[r, :hl] < V])
                    if what == "raise" or r % 2:
                        x[r, hist[r, hl:]] = 5.0                 # poison: equal to the stop value, but beyond hist_len and not penalised
                    x[r, live[: 1 + r % 3]] = 5.0 * rep          # these fire
                    x[r, live[-1]] = 5.0 * rep if r % 2 else x[r, live[-1]]
                P = Params(top_k=40 if mode else 0, top_p=0.9, mode=mode, rep_pen=rep, hist_len=hl, stop_tok=stop, len_pen=lp)
                out.append(Case(f"length-{what}-V{V}-rep{rep}-m{mode}", "length", x, P, rng.random(6), hist))
    for V in (97, 4099):
        for mode in (0, 1):
            rng = np.random.default_rng(7700 + V + mode)
            x = (-16.0 + 2.0 * rng.random((3, V))).astype(F32)
            hl = 4
            hist = np.stack([rng.choice(V, size=hl + HIST_PAD, replace=False) for _ in range(3)]).astype(np.int64)
            hist[:, 3] = hist[:, 0]
            for r in range(3):
                x[r, hist[r, : 1 + r]] = 5.0
            P = Params(mode=mode, hist_len=hl, stop_tok=stop, len_pen=0.5)
            out.append(Case(f"length-shrink-deep-V{V}-m{mode}", "length", x, P, rng.random(3), hist))
    return out


def _penalty_order_row():
    """a history token a (logit x_a > 0) and a free token b whose values are EQUAL with the penalty first and differ with it last"""
    rep, it = F32(1.2), F32(1.0) / F32(0.7)
    for i in range(1, 4000):
        xa = F32(2.0) + F32(i) * F32(2.0 ** -12)
        good, bad = F32(xa / rep) * it, F32(F32(xa * it) / rep)
        if good != bad:
            for j in range(-8, 9):
                xb = F32(good / it) + F32(j) * np.spacing(F32(good / it))
                if F32(xb * it) == good:
                    return xa, xb
    raise AssertionError("no such pair")


def penalty_order_case():
    xa, xb = _penalty_order_row()
    V = 64
    x = np.full((2, V), -3.0, dtype=F32) - np.arange(V, dtype=F32) / 8
    x[:, 7] = 6.0
    x[0, 20], x[0, 41] = xa, xb
    x[1, 41], x[1, 20] = xa, xb
    hist = np.array([[20, 20, V, -1] + [7] * HIST_PAD, [41, -1, 41, V] + [7] * HIST_PAD], dtype=np.int64)
    P = Params(temperature=0.7, top_k=2, mode=1, rep_pen=1.2, hist_len=4)
    return Case("penalty-then-temperature-tie", "order", x, P, [0.3, 0.7], hist)


def lds_edge():
    """(largest V the kernel's LDS admits, one exact row there)"""
    V = (LDS_LIMIT - lds_bytes(0)) // 4 * 32
    assert lds_bytes(V) <= LDS_LIMIT < lds_bytes(V + 1)
    x = _tied_row(V, _place(8, V, "spread"))[None]
    return Case(f"lds-edge-V{V}", "exact", x, Params(top_p=0.5, mode=1), [0.7])


_ALL = None


def all_cases():
    """every case, built once (the references inside are computed once and shared too)"""
    global _ALL
    if _ALL is None:
        _ALL = exact_cases() + singleton_cases() + draw_cases() + zero_cases() + random_cases() + length_cases() + [penalty_order_case()]
        assert len({c.name for c in _ALL}) == len(_ALL)
    return _ALL


def by_name(name):
    return next(c for c in all_cases() if c.name == name)
