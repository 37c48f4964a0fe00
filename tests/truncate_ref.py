"""float64 statement of the sampling truncation rules cc_logits_truncate (clipcap_amd/csrc/truncate.hip: k_logits_truncate; min-p, epsilon
cutoff, eta cutoff, locally typical sampling), the per-row report the GPU test holds the kernel to (tests/test_gpu_truncate.py), an fp32
emulation of the kernel's passes with the defects those checks must catch, and the case list both tests walk.  numpy only, no GPU needed;
tests/test_truncate_ref.py pins this module itself.  It stands to truncate.hip as tests/sample_ref.py stands to the sampler and reuses its
value definition (row_values), PAD, HIST_PAD and attn_ref's constants.

Definition (one row; include/clipcap_hip.h).  The values are the sampler's, exact fp32: v = sample_ref.row_values.  From there
float64 over the V real columns: m = max v, lse = m + log sum exp(v_i - m), p_i = exp(v_i - lse), H = -sum over p_i > 0 of p_i (v_i - lse).
    min-p      min_p > 0:           keep v_i >= m + ln(min_p)
    epsilon    epsilon_cutoff > 0:  keep v_i >= lse + ln(eps)
    eta        eta_cutoff > 0:      keep v_i >= lse + min(ln eta, ln(eta) / 2 - H)
    typical    typical_p < 1:       keep d_i <= d*, d_i = |lse - v_i - H| (+inf for -inf); the tokens ordered by d ascending, d* = the d of the
               first token at which the cumulative p reaches >= typical_p (never: the last finite d); every tie at d* is kept
The kept set is the intersection of the rules that are on, all taken against the same p and H; an empty intersection keeps every token
with v_i == m; a row of only -inf stays as it is.  The raw logit of a removed token becomes -inf, everything else keeps its bits.

What the device computes, and the error of each quantity, counted where it happens (u32 = 2^-24; x_i = v_i - m <= 0):
    fl32(v - m)          |x| u32 of the argument
    __expf               attn_ref.EXP_ULPS u32 (1 + |x|), the same allowance sample_ref uses; together |e'_i - e_i| <= e_i rho_i,
                         rho_i = SECOND_ORDER u32 (EXP_ULPS (1 + |x|) + |x|); x == 0 and x == -inf carry no error; below x = -87 the result
                         leaves fp32's normal range and may be flushed: rho_i = 1 there (the whole term, below 2^-125)
    S0 = sum e'_i, S1 = sum e'_i x'_i      fp64 accumulators in a fixed order (V terms of one sign: V 2^-53 relative, inside FP64 below):
                         dS0 = sum e_i rho_i,  dS1 = SECOND_ORDER sum e_i |x_i| (rho_i + u32)
    log S0               fp64: |d log S0| <= SECOND_ORDER dS0 / S0                                                      =: dL
    q = S1 / S0          |dq| <= SECOND_ORDER (dS1 + |q| dS0) / S0                                                      =: dQ
    lse = m + log S0 (error dL),  H = log S0 - q (error dL + dQ),  centre c = lse - H = m + q (error dQ)
    thresholds           min-p: m + ln(min_p), both exact inputs: FP64 (|m| + |ln min_p|), and 0 when min_p == 1 (m + 0 is exact);
                         epsilon: dL;  eta: dL where ln eta is the smaller branch by more than dL + dQ, else 2 dL + dQ;  each + FP64 (|lse| + |ln|).
                         The device rounds the fp64 threshold UP to the next fp32 and compares in fp32, which decides every fp32 v as the
                         fp64 compare would: no further error.  A token is UNDECIDED for a threshold rule when |v_i - threshold| <= its band.
    d'_i = fl32(|c' - v_i|)   |d'_i - d_i| <= b_i = dQ + u32 d_i + FP64 (|c| + |v_i|)
    masses               the sampler's 2^-32 fixed point, w'_i = trunc(fl32(e'_i S)): sample_ref._weights gives S e_i and err_i (one more
                         rounding and the truncation, below one unit); the target trunc(double(typical_p) Z') lies within
                         dT = typical_p sum err_i + 1 + 2^-40 T of T = typical_p S sum e_i, and is at least 1
The typical rule on the device keeps i iff the mass of the tokens STRICTLY closer (d'_j < d'_i) is below the target.  Tokens of equal v have
equal d' and equal w' (same arithmetic), so they are never strictly closer than one another.  Hence
    surely kept      sum over {j : d_j - b_j <= d_i + b_i, v_j != v_i} of (S e_j + err_j) < max(1, T - dT)
    surely dropped   sum over {j : d_j + b_j <  d_i - b_i} of (S e_j - err_j) >= max(1, T + dT)
and everything else is undecided: the admissible WINDOW of cut positions is the run of undecided groups of equal v in d order, one cut
behind each and one in front: window = undecided groups + 1, a group always whole.  check_row() holds a kernel row to: padding and kept
logits bit-identical, removed = -inf; every surely-kept token (by every rule that is on) kept, every surely-dropped one (by any) removed;
tokens of equal v decided alike; the kept tokens separable from the dropped ones by ONE threshold (in v for the threshold rules, in d
within the bands for typical); an intersection that is surely empty gives exactly the maxima.  Nothing is tuned to what the kernel
returns."""
import numpy as np

from tests import attn_ref as A
from tests import sample_ref as SR

F32 = np.float32
U32 = SR.U32
S = SR.S
PAD, HIST_PAD = SR.PAD, SR.HIST_PAD
FP64 = 2.0 ** -48                          # a handful of fp64 roundings (2^-53 each) and the V-term fp64 sums, with room
LDS_LIMIT = 150 * 1024
MAX_UNDECIDED, MAX_WINDOW = 8, 8
RULES = ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")


def lds_bytes(V):
    """the kernel's dynamic LDS: hist_w[2048] u64 | red[16 + 2] u64 | dred[32] f64 | fred[32] f32 | bcast[4] u32 | bitmap[ceil(V / 32)] u32"""
    return 2048 * 8 + (16 + 2) * 8 + 32 * 8 + 32 * 4 + 4 * 4 + (V + 31) // 32 * 4


class Params:
    def __init__(self, temperature=1.0, rep_pen=1.0, hist_len=0, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0):
        self.temperature, self.rep_pen, self.hist_len = float(temperature), F32(rep_pen), int(hist_len)
        self.min_p, self.typical_p, self.eps, self.eta = F32(min_p), F32(typical_p), F32(epsilon_cutoff), F32(eta_cutoff)
        self.sample = SR.Params(temperature=temperature, rep_pen=rep_pen, hist_len=hist_len)        # what row_values reads

    @property
    def on(self):
        return dict(min_p=self.min_p > 0, typical_p=self.typical_p < 1, epsilon_cutoff=self.eps > 0, eta_cutoff=self.eta > 0)

    def args(self):
        """the call's four options in the entry point's order"""
        return float(self.min_p), float(self.typical_p), float(self.eps), float(self.eta)

    def only(self, rule):
        off = dict(min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)
        off[rule] = float(dict(min_p=self.min_p, typical_p=self.typical_p, epsilon_cutoff=self.eps, eta_cutoff=self.eta)[rule])
        return Params(self.temperature, self.rep_pen, self.hist_len, **off)


def _ln(a):
    return float(np.log(np.float64(a)))


def _group_ids(v):
    """ids of the groups of equal values (-0.0 == +0.0)"""
    _, inv = np.unique(v.astype(np.float64) + 0.0, return_inverse=True)
    return inv.reshape(-1)


class RowRef:
    """the float64 reference of one row and its report: kept (the definition's kept set), sure_in / sure_out / undecided, window"""

    def __init__(self, x, P, hist):
        self.P = P
        self.v, self.bm = SR.row_values(x, P.sample, hist)
        v = self.v
        V = self.V = v.size
        self.fin = v > -np.inf
        self.m = v.max()
        self.dead = not self.fin.any()
        self.window, self.n_undecided = 1, 0
        if self.dead:
            self.kept = np.zeros(V, dtype=bool)
            self.sure_in, self.sure_out = self.kept.copy(), ~self.kept
            self.undecided = self.kept.copy()
            self.surely_empty = self.maybe_empty = False
            return
        fin, m = self.fin, float(self.m)
        v64 = v.astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            x_ = np.where(fin, v64 - m, -np.inf)
            e = np.exp(x_)
        ax = np.where(fin, -x_, 0.0)
        rho = A.SECOND_ORDER * U32 * (A.EXP_ULPS * (1.0 + ax) + ax)
        rho = np.where(ax > 87.0, 1.0, rho)
        rho = np.where((x_ == 0.0) | ~fin, 0.0, rho)
        S0 = e.sum()
        S1 = float(np.sum(np.where(e > 0, e * np.where(fin, x_, 0.0), 0.0)))
        dS0 = float((e * rho).sum())
        dS1 = A.SECOND_ORDER * float((e * ax * (rho + U32)).sum())
        L, q = float(np.log(S0)), S1 / S0
        dL = A.SECOND_ORDER * dS0 / S0
        dQ = A.SECOND_ORDER * (dS1 + abs(q) * dS0) / S0
        self.lse, self.H, self.c = m + L, L - q, m + q
        self.p = e / S0
        self.dL, self.dQ = dL, dQ
        lse, H = self.lse, self.H
        on = P.on
        # ---- the threshold rules: (threshold, band)
        self.thr = {}
        if on["min_p"]:
            ln = _ln(P.min_p)
            self.thr["min_p"] = (m + ln, 0.0 if ln == 0.0 else FP64 * (abs(m) + abs(ln)))
        if on["epsilon_cutoff"]:
            ln = _ln(P.eps)
            self.thr["epsilon_cutoff"] = (lse + ln, dL + FP64 * (abs(lse) + abs(ln)))
        if on["eta_cutoff"]:
            ln = _ln(P.eta)
            flat, ent = ln, 0.5 * ln - H
            band = dL if flat < ent - (dL + dQ) else 2.0 * dL + dQ
            self.thr["eta_cutoff"] = (lse + min(flat, ent), band + FP64 * (abs(lse) + abs(ln)))
        thr_keep = np.ones(V, dtype=bool)         # the definition's decision
        thr_in, thr_out = fin.copy(), ~fin
        self.thr_undecided = np.zeros(V, dtype=bool)
        for t, band in self.thr.values():
            und = fin & (np.abs(v64 - t) <= band) & (band > 0)
            ok = v64 >= t
            thr_keep &= ok
            thr_in &= ok & ~und
            thr_out |= ~ok & ~und
            self.thr_undecided |= und
        thr_keep &= fin
        self.thr_keep, self.thr_in, self.thr_out = thr_keep, thr_in, thr_out
        # ---- typical
        typ_keep, typ_in, typ_out = fin.copy(), fin.copy(), ~fin
        self.d = np.where(fin, np.abs(self.c - np.where(fin, v64, 0.0)), np.inf)
        self.b = np.where(fin, dQ + U32 * self.d + FP64 * (abs(self.c) + np.abs(np.where(fin, v64, 0.0))), 0.0)
        if on["typical_p"]:
            tp = float(P.typical_p)
            idx = np.flatnonzero(fin)
            d, b = self.d[idx], self.b[idx]
            order = np.argsort(d, kind="stable")
            cum = np.cumsum(self.p[idx][order])
            hit = np.flatnonzero(cum >= tp)
            dstar = d[order[hit[0]]] if hit.size else d[order[-1]]
            typ_keep = np.zeros(V, dtype=bool)
            typ_keep[idx[d <= dstar]] = True
            we, werr = SR._weights(v, self.m)
            w, err = S * we[idx], werr[idx]
            T = tp * float(w.sum())
            dT = tp * float(err.sum()) + 1.0 + T * 2.0 ** -40
            lo, hi = d - b, d + b
            g = _group_ids(v[idx])
            up, dn = w + err, np.maximum(w - err, 0.0)
            # possibly closer: lo_j <= hi_i, the token's own group of equal values taken out
            by_lo = np.argsort(lo, kind="stable")
            cum_up = np.concatenate(([0.0], np.cumsum(up[by_lo])))
            n_le = np.searchsorted(lo[by_lo], hi, side="right")
            own = np.bincount(g, weights=up)[g]
            before_up = cum_up[n_le] - own
            # surely closer: hi_j < lo_i
            by_hi = np.argsort(hi, kind="stable")
            cum_dn = np.concatenate(([0.0], np.cumsum(dn[by_hi])))
            before_dn = cum_dn[np.searchsorted(hi[by_hi], lo, side="left")]
            tin = before_up * (1.0 + FP64) < max(1.0, T - dT)
            tout = before_dn * (1.0 - FP64) >= max(1.0, T + dT)
            assert not (tin & tout).any()
            typ_in, typ_out = np.zeros(V, dtype=bool), ~fin
            typ_in[idx[tin]] = True
            typ_out[idx[tout]] = True
            und = ~tin & ~tout
            self.window = 1 + np.unique(g[und]).size
        self.typ_keep, self.typ_in, self.typ_out = typ_keep, typ_in, typ_out
        # ---- the intersection, and what an empty one keeps
        self.maxima = fin & (v == self.m)
        inter = thr_keep & typ_keep
        self.kept = inter if inter.any() else self.maxima.copy()
        self.sure_in = thr_in & typ_in
        self.sure_out = thr_out | typ_out
        self.undecided = ~self.sure_in & ~self.sure_out
        self.surely_empty = bool(self.sure_out.all())
        self.maybe_empty = not self.sure_in.any()
        self.n_undecided = int(self.undecided.sum())

    @property
    def decided(self):
        return self.n_undecided == 0


def check_row(ref, x_in, x_out):
    """Hold one row's result (the V real columns, fp32) to the reference.  AssertionError otherwise."""
    x_in, x_out = np.asarray(x_in, dtype=F32), np.asarray(x_out, dtype=F32)
    same = x_in.view(np.uint32) == x_out.view(np.uint32)
    if ref.dead:
        assert same.all(), "a row of only -inf was written"
        return
    removed = ~same
    assert np.all(x_out[removed] == -np.inf), f"changed logits that are not -inf at {np.flatnonzero(removed & (x_out != -np.inf))[:8]}"
    kept = ref.fin & (x_out > -np.inf)            # a logit that was -inf has nothing to lose; the rest is kept iff it kept its bits
    fin = ref.fin & (x_in > -np.inf)
    assert np.array_equal(fin, ref.fin)
    assert kept.any(), "every token removed"
    v = ref.v
    if ref.maybe_empty and np.array_equal(kept, ref.maxima):
        return                                    # the empty intersection's answer, where the intersection can be empty
    assert not ref.surely_empty, f"the intersection is empty: the maxima {np.flatnonzero(ref.maxima)[:8]} stay, kept {np.flatnonzero(kept)[:8]}"
    lost = ref.sure_in & ~kept
    assert not lost.any(), f"removed tokens that every rule keeps: {np.flatnonzero(lost)[:8]}"
    extra = ref.sure_out & kept
    assert not extra.any(), f"kept tokens that a rule removes: {np.flatnonzero(extra)[:8]}"
    g = _group_ids(v)
    per = np.bincount(g, weights=kept.astype(np.float64)) / np.bincount(g)
    assert np.all((per == 0) | (per == 1)), "tokens of equal value decided differently"
    on = ref.P.on
    dropped = fin & ~kept
    if not on["typical_p"]:
        if dropped.any():
            assert v[kept].min() > v[dropped].max(), "a threshold rule kept a smaller value than one it removed"
    else:
        among = fin & (ref.thr_in if ref.thr else fin)          # tokens no threshold rule can have removed: typical alone decided them
        k, dr = kept & among, dropped & among
        if k.any() and dr.any():
            assert (ref.d[k] - ref.b[k]).max() <= (ref.d[dr] + ref.b[dr]).min(), "typical kept a token farther from the entropy than one it removed"


# ---- fp32 emulation of the kernel's passes, and the defects -------------------------------------------------------------------------------
DEFECTS = ("typical_descending", "typical_ties_dropped", "typical_cut_strict", "entropy_in_bits", "entropy_untempered",
           "penalty_after_temperature", "eta_max", "eta_no_sqrt", "min_p_relative_to_one", "ld_taken_as_V", "padding_written",
           "history_beyond_hist_len", "empty_left_empty", "kept_rewritten")
# typical_cut_strict: the kept side of the cut taken strictly, d_i < d* in place of d_i <= d* (the token that reaches the mass is lost).  The
# OTHER strictness, cumulative mass > target in place of >=, differs only where two integer masses are equal, which no float64 statement can
# certify once a weight other than the maximum's has been truncated: no sound check can see it, so it is not in the list.


def emulate_row(x, P, hist, defect=None):
    """the row the kernel leaves (fp32 [V]), by its passes: fp32 values and __expf arguments, fp64 sums, integer masses"""
    x = np.asarray(x, dtype=F32)
    V = x.size
    hl = P.hist_len + (HIST_PAD if defect == "history_beyond_hist_len" and hist is not None and P.hist_len > 0 else 0)
    bm = SR._bitmap(V, hist, hl)
    use_rep = P.hist_len > 0 and hist is not None and P.rep_pen != F32(1.0)
    it = P.sample.inv_temp
    pen = np.where(bm, SR._pen(x, P.rep_pen), x).astype(F32) if use_rep else x
    if defect == "penalty_after_temperature" and use_rep:
        t = (x * it).astype(F32)
        v = np.where(bm, SR._pen(t, P.rep_pen), t).astype(F32)
    else:
        v = (pen * it).astype(F32)
    out = x.copy()
    fin = v > -np.inf
    if not fin.any():
        return out
    m = v.max()

    def stats(vals):
        mm = vals.max()
        with np.errstate(invalid="ignore"):
            xm = (vals - mm).astype(F32)
            e = np.exp(xm).astype(F32)
        pos = e > 0
        s0 = float(e[pos].astype(np.float64).sum())
        s1 = float((e[pos].astype(np.float64) * xm[pos].astype(np.float64)).sum())
        return float(mm), np.log(s0), s1 / s0

    mf, ls, q = stats(v)
    lse, H = mf + ls, ls - q
    if defect == "entropy_untempered":
        _, ls0, q0 = stats(pen)
        H = ls0 - q0
    if defect == "entropy_in_bits":
        H = H / np.log(2.0)
    centre = lse - H
    on = P.on
    thr = -np.inf
    if on["min_p"]:
        thr = max(thr, (lse if defect == "min_p_relative_to_one" else mf) + _ln(P.min_p))
    if on["epsilon_cutoff"]:
        thr = max(thr, lse + _ln(P.eps))
    if on["eta_cutoff"]:
        ln = _ln(P.eta)
        ent = (ln if defect == "eta_no_sqrt" else 0.5 * ln) - H
        thr = max(thr, lse + (max(ln, ent) if defect == "eta_max" else min(ln, ent)))
    keep = fin & (v.astype(np.float64) >= thr)
    if on["typical_p"]:
        idx = np.flatnonzero(fin)
        d = np.abs(centre - v[idx].astype(np.float64)).astype(F32)
        w = SR._fix(v, m)[idx]
        order = np.argsort(-d if defect == "typical_descending" else d, kind="stable")
        cum = np.cumsum(w[order])
        target = max(1, int(float(P.typical_p) * float(cum[-1])))
        hit = np.flatnonzero(cum >= target)
        n = int(hit[0]) if hit.size else idx.size - 1
        dstar = d[order[n]]
        if defect == "typical_ties_dropped":
            tk = np.zeros(idx.size, dtype=bool)
            tk[order[:n + 1]] = True
        elif defect == "typical_cut_strict":
            tk = d < dstar
        elif defect == "typical_descending":
            tk = d >= dstar
        else:
            tk = d <= dstar
        typ = np.zeros(V, dtype=bool)
        typ[idx[tk]] = True
        keep &= typ
    if not keep.any() and defect != "empty_left_empty":
        keep = fin & (v == m)
    out[~keep] = -np.inf
    if defect == "kept_rewritten":
        out[keep] = v[keep]
    return out


# ---- cases --------------------------------------------------------------------------------------------------------------------------------
class Case:
    """one launch: rows x [R][V] fp32, history [R][hist_len + HIST_PAD] int64 (or None), the call's parameters"""

    def __init__(self, name, kind, x, P, hist=None):
        self.name, self.kind, self.P = name, kind, P
        self.x = np.ascontiguousarray(x, dtype=F32)
        self.R, self.V = self.x.shape
        self.hist = hist
        assert self.R <= 8
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
            self._refs = [RowRef(self.x[r], self.P, self.h(r)) for r in range(self.R)]
        return self._refs


def emulate_case(c, defect=None):
    """the [R][ld] buffer the fp32 emulation leaves behind"""
    buf = c.padded()
    out = buf.copy()
    if defect == "ld_taken_as_V":
        flat = buf.reshape(-1).copy()
        for r in range(c.R):
            row = np.nan_to_num(flat[r * c.V:(r + 1) * c.V], nan=0.0, posinf=np.inf, neginf=-np.inf)      # the padding read as a number
            flat[r * c.V:(r + 1) * c.V] = emulate_row(row, c.P, c.h(r))
        return flat.reshape(buf.shape)
    for r in range(c.R):
        out[r, :c.V] = emulate_row(buf[r, :c.V], c.P, c.h(r), defect)
    if defect == "padding_written":
        out[:, c.V:] = -np.inf
    return out


def check_case(c, out):
    """out: the [R][ld] buffer after the call"""
    out = np.asarray(out, dtype=F32).reshape(c.R, c.ld)
    buf = c.padded()
    assert np.array_equal(out[:, c.V:].view(np.uint32), buf[:, c.V:].view(np.uint32)), f"{c.name}: the padding columns changed"
    for r, ref in enumerate(c.refs()):
        try:
            check_row(ref, c.x[r], out[r, :c.V])
        except AssertionError as e:
            raise AssertionError(f"{c.name} row {r}: {e}") from None


# temperature, min_p, typical_p, epsilon, eta, history length (0: none), V's.  Every rule alone, all four, the extremes
COMBOS = (
    (1.0, 0.1, 1.0, 0.0, 0.0, 0, (4, 97, 50257)), (0.7, 0.0, 0.9, 0.0, 0.0, 6, (64, 1000, 50257)), (1.3, 0.0, 1.0, 3e-4, 0.0, 0, (97, 4099)),
    (1.0, 0.0, 1.0, 0.0, 2e-3, 6, (4, 1000, 50257)), (0.7, 0.05, 0.95, 3e-4, 6e-4, 1500, (64, 4099, 50257)), (1.0, 0.0, 0.2, 0.0, 0.0, 0, (97, 1000, 4099)),
    (1.3, 1.0, 1.0, 0.0, 0.0, 0, (64,)), (1.0, 0.0, 0.5, 0.9, 0.0, 6, (1000,)), (0.7, 0.0, 1.0, 0.0, 0.3, 0, (4099,)),
)
SEED0 = 4100
SALT = {}            # (combo, V) -> a further seed offset: a seed whose reference leaves the conditions (MAX_UNDECIDED, MAX_WINDOW) is replaced


def random_cases():
    out = []
    for i, (T, mp, tp, eps, eta, hl, Vs) in enumerate(COMBOS):
        for V in Vs:
            rng = np.random.default_rng(SEED0 + 1000 * i + V + 100000 * SALT.get((i, V), 0))
            x = SR._random_rows(V, rng)
            hist = SR._history(x, hl, rng) if hl else None
            P = Params(temperature=T, rep_pen=1.2 if hl else 1.0, hist_len=hl, min_p=mp, typical_p=tp, epsilon_cutoff=eps, eta_cutoff=eta)
            out.append(Case(f"random-V{V}-T{T}-minp{mp}-typ{tp}-eps{eps}-eta{eta}-h{hl}", "random", x, P, hist))
    return out


def _grouped_row(V, groups, offset=0):
    """-inf everywhere but groups of equal values [(value, count), ...], their members dealt out over the row in turn"""
    n = sum(c for _, c in groups)
    pos = SR._place(n, V, "spread") + offset
    vals = np.concatenate([np.full(c, val) for val, c in groups])
    x = np.full(V, -np.inf, dtype=F32)
    x[pos] = vals[np.argsort(np.arange(n) * 7 % n, kind="stable")] if n > 1 else vals
    return x


ABC = ((3.0, 1), (1.0, 6), (-1.0, 5))       # p = 0.526 | 6 x 0.0711 | 5 x 0.0096, H = 1.69: d = 1.05 | 0.95 | 2.95 — the order is B, A, C
LADDER = ((3.0, 1), (1.05, 1), (1.04, 1), (1.03, 1), (1.02, 1), (1.01, 1), (1.0, 1), (-1.0, 5))      # group B as six different values


def designed_cases():
    """rows of a few groups of equal values: every margin (in v against a threshold, in d and in mass against the cut) is more than a hundred
    times its bound, so every decision is exact: no undecided token, one admissible cut"""
    out = []
    for V in (97, 4099):
        rows = np.stack([_grouped_row(V, ABC, o) for o in (0, 1, 2)])
        # the cut falls inside the six ties of B (0.3 of the mass is reached at its fifth member): all six stay, nothing else
        out.append(Case(f"designed-V{V}-tie-group-straddles-cut", "designed", rows, Params(typical_p=0.3)))
        # 0.5 is reached at A, the second group: B and A
        out.append(Case(f"designed-V{V}-two-groups", "designed", rows, Params(typical_p=0.5)))
        # typical keeps B, epsilon keeps A: nothing in common -> the maximum A
        out.append(Case(f"designed-V{V}-typical-and-epsilon-disjoint", "designed", rows, Params(typical_p=0.3, epsilon_cutoff=0.2)))
        # eta = 0.25: min(0.25, 0.5 e^-H = 0.092): B (0.071) goes, A stays; in bits, without the root or with max the answer differs
        out.append(Case(f"designed-V{V}-eta", "designed", rows, Params(eta_cutoff=0.25)))
        out.append(Case(f"designed-V{V}-eta-small", "designed", rows, Params(eta_cutoff=0.04)))
        out.append(Case(f"designed-V{V}-epsilon", "designed", rows, Params(epsilon_cutoff=0.05)))
        out.append(Case(f"designed-V{V}-min-p", "designed", rows, Params(min_p=0.1, temperature=0.5)))
        lad = np.stack([_grouped_row(V, LADDER, o) for o in (0, 3)])
        # a mass so small that the closest token alone reaches it: one token remains, and not the maximum
        out.append(Case(f"designed-V{V}-one-token", "designed", lad, Params(typical_p=1e-3)))
        out.append(Case(f"designed-V{V}-ladder", "designed", lad, Params(typical_p=0.25, temperature=1.0)))
    out.append(_penalty_case())
    out.append(_penalty_order_case())
    return out


def _penalty_case():
    """min_p = 0.3 keeps v >= 4 - 1.204 = 2.796.  Token 20 (logit 3.0) is in the history: the penalty of 2 makes it 1.5 and only that removes
    it; token 30 (3.2) sits in the history's PADDING beyond hist_len and stays; token 40 (-2.0 -> -4.0) is removed either way"""
    V = 64
    x = np.full((2, V), -5.0, dtype=F32)
    x[:, 7], x[:, 20], x[:, 30], x[:, 40] = 4.0, 3.0, 3.2, -2.0
    x[1] = np.roll(x[1], 11)
    hist = np.array([[20, 40, 20, -1, V] + [30] * HIST_PAD, [31, 51, -1, V, 31] + [41] * HIST_PAD], dtype=np.int64)
    return Case("designed-penalty-crosses-min-p", "designed", x, Params(rep_pen=2.0, hist_len=5, min_p=0.3), hist)


def _penalty_order_case():
    """sample_ref's pair: a history token and a free one whose values are EQUAL with the penalty before the temperature and differ with it
    after.  They are the row's maxima and min_p = 1 keeps exactly the maxima: both, or — in the wrong order — one"""
    xa, xb = SR._penalty_order_row()
    V = 64
    x = np.full((2, V), -3.0, dtype=F32) - np.arange(V, dtype=F32) / 8
    x[0, 20], x[0, 41] = xa, xb
    x[1, 41], x[1, 20] = xa, xb
    hist = np.array([[20, 20, V, -1] + [7] * HIST_PAD, [41, -1, 41, V] + [7] * HIST_PAD], dtype=np.int64)
    return Case("designed-penalty-then-temperature", "designed", x, Params(temperature=0.7, rep_pen=1.2, hist_len=4, min_p=1.0), hist)


def lds_edge():
    """(largest V the kernel's LDS admits, one designed row there, all four rules on)"""
    V = (LDS_LIMIT - lds_bytes(0)) // 4 * 32
    assert lds_bytes(V) <= LDS_LIMIT < lds_bytes(V + 1)
    x = _grouped_row(V, ABC)[None]
    hist = np.array([[5, 9, V - 1, V, -1] + [0] * HIST_PAD], dtype=np.int64)
    return Case(f"lds-edge-V{V}", "designed", x, Params(rep_pen=1.2, hist_len=5, min_p=0.05, typical_p=0.5, epsilon_cutoff=1e-3, eta_cutoff=1e-3), hist)


_ALL = None


def all_cases():
    """every case, built once (the references inside are computed once and shared too)"""
    global _ALL
    if _ALL is None:
        _ALL = designed_cases() + random_cases()
        assert len({c.name for c in _ALL}) == len(_ALL)
    return _ALL


def by_name(name):
    return next(c for c in all_cases() if c.name == name)
