"""float64 reference of the KV-cached attention step of one decode layer (clipcap_amd/csrc/decode.hip: k_decode_attn, k_group_union +
k_decode_attn_group, reached one call at a time through the test hook cc_decode_attention), the per-element error bounds the GPU test
holds the kernels to (tests/test_gpu_decode_attention.py), float64 emulations of the defects those bounds must catch, a mirror of the
launch arithmetic (which kernel, union size, passes), and the case list both tests walk.  Plain torch, no GPU needed (every function runs
on whatever device its tensors are on); tests/test_decode_ref.py pins this module itself.  It stands to the decode attention as
tests/attn_ref.py stands to the training attention and reuses its constants.

Definition.  qkv [R*Tn][3 D] holds q | k | v of the Tn new positions of every row, the cache K, V [R][ctx_max][D] the older ones, D = H hd.
    key j < pos0 of row r          cache row row_map[r][j], position j          (row_map NULL: row r)
    key pos0 + u, u < Tn           the call's own: qkv row r * Tn + u
    query (r, t)                   sees keys 0 .. pos0 + t:   s_j = q . k_j / sqrt(hd),  A = softmax_j s,  out = A V
Afterwards (append = 1) slots pos0 .. pos0 + Tn - 1 of cache row r equal the k / v slices of qkv bit for bit, every other cache element
is unchanged, and out is written nowhere outside its R * Tn * D elements.  With append = 0 the caller has stored the new slices already
and the cache is not written at all.

Rounding model (attn_ref's fp32 VALU family: every kernel here accumulates in fp32 on the VALU).  u32 = 2^-24.
    score        2 hd roundings of u32 * sum_d |q||k| (one per product unless contracted, one per addition, any order), times the scale:
                 its own rounding and the multiplication, and the subtraction of the maximum: 3 u32 |s|
    weight       e_j = __expf(s_j - m): the argument's error carried through expm1 (first order: the error itself, the rest is
                 SECOND_ORDER's), plus attn_ref.EXP_ULPS * u32 * (1 + |x|), x = s_j - m — the same device function over the same range as
                 attention.hip's, so attn_ref's measured allowance holds.  The same weight enters numerator and denominator: out moves by
                 at most sum_j A_j rho_j (|v_j| + |out|) / (1 - max rho), the softmax's sensitivity (attn_ref.fwd_bounds).
    key sums     numerator sum_j e_j v_j and denominator sum_j e_j: n products and fewer than n additions each, in any order (lanes, key
                 groups, waves; keys a beam does not own carry weight exactly 0 and add nothing): 2 n roundings of u32 * sum |terms|
    division     k_decode_attn multiplies by 1 / sum, k_decode_attn_group divides: DIV_ROUNDINGS u32 |out|, counted as attn_ref counts its
                 own (the quotient or reciprocal within 4 u32, one multiplication); test_measured_allowances prints what the device does
                 (MI355X: 1 / n through k_decode_attn, n = 1 .. 200: 0.9688 u32 / n; v / n through k_decode_attn_group: 0.9375)
    store        one rounding to the stored type (none in the split-bf16 build, whose activations are fp32): gemm_ref.store_bound
Products of two of these relative errors are covered by attn_ref.SECOND_ORDER.  Nothing is tuned to what the kernels return."""
import torch

from tests import attn_ref as A
from tests import gemm_ref as G

U32 = G.U32
DT = A.DT
DIV_ROUNDINGS = 5.0                       # 1 / l within 4 u32 and one multiplication (attn_ref.fwd_bounds, "l"); v / l alone is inside it
LDS_LIMIT = 64 * 1024
PASS = 128                                # union entries per pass of k_decode_attn_group (4 waves x 32)


# ---- launch arithmetic (decode.hip: decode_attn_plan, k_group_union) ----------------------------------------------------------------------
def row_lds(ctx_max, hd):
    """k_decode_attn's LDS: per wave p[ctx_max] | srow[ctx_max] | red[8][hd], four waves"""
    return 4 * (2 * ctx_max + 8 * hd) * 4


def grp_cap(group, pos0):
    return (group * (pos0 + 1) + PASS - 1) // PASS * PASS


def grp_shm(group, pos0):
    """k_decode_attn_group's LDS: p[cap][8] | wmx[4][8] | wsum[8][8] | red2[8][G][64]"""
    return (grp_cap(group, pos0) * 8 + 96 + 8 * group * 64) * 4


def path(R, Tn, hd, pos0, group, npos):
    """0: k_decode_attn, 1: k_group_union + k_decode_attn_group (decode mode bit 0 set, workspace of cc_decode_ws_bytes)"""
    ents = R * npos + R * 128 if Tn == 1 else 0
    return int(Tn == 1 and 2 <= group <= 8 and hd == 64 and grp_shm(group, pos0) <= LDS_LIMIT and (R // group) * grp_cap(group, pos0) <= ents)


def union(rm, R, G_, pos0):
    """k_group_union's list for every group: [(cache row, position, owner bits)], positions ascending, at one position the distinct rows
    in order of the first beam that names them; then the G new keys (row r0 + b, position pos0, bit b).  rm: [R][>= pos0] table or None."""
    out = []
    t = None if rm is None else rm.tolist()
    for r0 in range(0, R, G_):
        ent = []
        for j in range(pos0):
            m = [t[r0 + b][j] if t is not None else r0 + b for b in range(G_)]
            for b in range(G_):
                if m[b] not in m[:b]:
                    ent.append((m[b], j, sum(1 << b2 for b2 in range(G_) if m[b2] == m[b])))
        ent += [(r0 + b, pos0, 1 << b) for b in range(G_)]
        out.append(ent)
    return out


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
TABLES = ("null", "random", "beam", "shared", "none", "prefix", "scattered", "cross")


class Case:
    """table: null (no row_map) | random (any row at every position) | beam (ancestry of a simulated beam search of width bw) | shared (a
    group's rows all name its first row) | none (identity) | prefix (the first k positions shared, then own) | scattered (shared at random
    positions) | cross (random rows of any group)."""

    def __init__(self, hd, R, Tn, pos0, ctx_max, table, group=1, append=1, k=0, bw=0, H=2, npos=0):
        assert table in TABLES and R % group == 0
        self.hd, self.R, self.Tn, self.pos0, self.ctx_max, self.table, self.group, self.append, self.k, self.H = hd, R, Tn, pos0, ctx_max, table, group, append, k, H
        self.bw = bw or (group if group > 1 else R)
        self.D = H * hd
        self.npos = npos or max(256, ctx_max)
        self.path = path(R, Tn, hd, pos0, group, self.npos)
        self.want_nU = None                               # union size the case was written for (largest group), where it matters

    @property
    def id(self):
        return f"hd{self.hd}-R{self.R}H{self.H}-pos{self.pos0}+{self.Tn}of{self.ctx_max}-{self.table}{self.k or ''}-g{self.group}-app{self.append}"

    @property
    def seed(self):
        return self.hd * 7919 + self.pos0 * 131 + self.Tn * 17 + self.group * 3 + self.append + TABLES.index(self.table) * 1009 + self.k

    def row_map(self):
        """int64 [R][ctx_max] on the CPU, or None.  Positions >= pos0 name the row itself, as cc_beam_advance leaves them."""
        if self.table == "null":
            return None
        g = torch.Generator().manual_seed(self.seed + 1)
        R, P, w = self.R, self.pos0, self.bw
        own = torch.arange(R).view(R, 1).expand(R, self.ctx_max).clone()
        first = (torch.arange(R) // w * w).view(R, 1)
        rm = own.clone()
        if self.table == "random" or self.table == "cross":
            rm[:, :P] = torch.randint(0, R, (R, P), generator=g)
        elif self.table == "shared":
            rm[:, :P] = first
        elif self.table == "prefix":
            rm[:, :min(self.k, P)] = first
        elif self.table == "scattered":
            sh = torch.rand(1, P, generator=g) < 0.5
            rm[:, :P] = torch.where(sh, first.expand(R, P), own[:, :P])
        elif self.table == "beam":
            for j in range(1, P + 1):             # before position j is written every row adopts the history of a row of its group
                src = first.view(R) + torch.randint(0, w, (R,), generator=g)
                if j % 3 == 0:
                    src = torch.arange(R)
                rm[:, :j] = rm[src, :j]
        return rm

    def inputs(self):
        """fp32 on the CPU: qkv [R*Tn][3 D], K and V caches [R][ctx_max][D] (EVERY slot holds its own random row: the defect emulations read
        slots the step must not), row_map.  N(0, 1) throughout: scores are N(0, 1) too, no key carries a row."""
        g = torch.Generator().manual_seed(self.seed)
        qkv = torch.randn(self.R * self.Tn, 3 * self.D, generator=g)
        kc = torch.randn(self.R, self.ctx_max, self.D, generator=g)
        vc = torch.randn(self.R, self.ctx_max, self.D, generator=g)
        return qkv, kc, vc, self.row_map()


def stored(c, op, dev="cpu"):
    """the buffers of a call in the build's stored type: dict(qkv, kc, vc, rm, named).  append = 0: the new slots of the cache hold the qkv
    slices (what the fused c_attn epilogue leaves).  named [R][ctx_max]: the cache slots the step may read."""
    qkv, kc, vc, rm = c.inputs()
    dt = DT[op]
    qkv, kc, vc = qkv.to(dt).to(dev), kc.to(dt).to(dev), vc.to(dt).to(dev)
    R, Tn, D, P = c.R, c.Tn, c.D, c.pos0
    named = torch.zeros(R, c.ctx_max, dtype=torch.bool)
    if P:
        cols = torch.arange(P).view(1, P).expand(R, P)
        named[(rm[:, :P] if rm is not None else torch.arange(R).view(R, 1).expand(R, P)), cols] = True
    if not c.append:
        x = qkv.view(R, Tn, 3, D)
        kc[:, P:P + Tn] = x[:, :, 1]
        vc[:, P:P + Tn] = x[:, :, 2]
        named[:, P:P + Tn] = True
    return dict(qkv=qkv, kc=kc, vc=vc, rm=None if rm is None else rm.to(dev), named=named.to(dev))


def expected_cache(c, S):
    """(K, V) the cache must hold after the call, given the buffers S as they were before it"""
    kc, vc = S["kc"].clone(), S["vc"].clone()
    if c.append:
        x = S["qkv"].view(c.R, c.Tn, 3, c.D)
        kc[:, c.pos0:c.pos0 + c.Tn] = x[:, :, 1]
        vc[:, c.pos0:c.pos0 + c.Tn] = x[:, :, 2]
    return kc, vc


# ---- reference and defect emulations --------------------------------------------------------------------------------------------------
DEFECTS = ("key64_dropped", "last_key_dropped", "tail_key_twice", "row_map_ignored", "stale_slot", "sibling_key", "second_pass_ignored",
           "union_lost_block")


def _keys(c, S, dtype):
    """gathered keys / values [R][ctx][D] of every row in `dtype`, and q [R][Tn][D]"""
    R, Tn, D, P = c.R, c.Tn, c.D, c.pos0
    ctx = P + Tn
    dev = S["qkv"].device
    x = S["qkv"].to(dtype).view(R, Tn, 3, D)
    kc, vc = S["kc"].to(dtype), S["vc"].to(dtype)
    rows = S["rm"][:, :ctx] if S["rm"] is not None else torch.arange(R, device=dev).view(R, 1).expand(R, ctx)
    cols = torch.arange(ctx, device=dev).view(1, ctx).expand(R, ctx)
    Kg, Vg = kc[rows, cols].clone(), vc[rows, cols].clone()
    Kg[:, P:], Vg[:, P:] = x[:, :, 1], x[:, :, 2]
    return x[:, :, 0], Kg, Vg


def _attend(c, q, Kg, Vg, mult):
    """q [R][Tn][D]; Kg, Vg [R][C][D]; mult [R][Tn][C]: how often query (r, t) counts key column j (0 = not visible).  -> dict"""
    R, Tn, H, hd = c.R, c.Tn, c.H, c.hd
    C = Kg.shape[1]
    qh, kh, vh = q.view(R, Tn, H, hd).transpose(1, 2), Kg.view(R, C, H, hd).transpose(1, 2), Vg.view(R, C, H, hd).transpose(1, 2)
    mu = mult.to(q.dtype).view(R, 1, Tn, C)
    live = mu > 0
    s = (qh @ kh.transpose(-1, -2)) * hd ** -0.5
    s = torch.where(live, s, torch.full_like(s, float("-inf")))
    m = s.max(-1, keepdim=True).values
    e = torch.where(live, torch.exp(s - m), torch.zeros_like(s)) * mu
    l = e.sum(-1, keepdim=True)
    Aw = e / l
    out = Aw @ vh
    return dict(out=out.transpose(1, 2).reshape(R, Tn, H * hd), oh=out, s=s, m=m, A=Aw, live=live, qh=qh, kh=kh, vh=vh)


def _causal(c, dev):
    t = torch.arange(c.Tn, device=dev).view(1, c.Tn, 1)
    j = torch.arange(c.pos0 + c.Tn, device=dev).view(1, 1, -1)
    return (j <= c.pos0 + t).expand(c.R, c.Tn, c.pos0 + c.Tn).to(torch.float64).clone()


def applicable(defect, c, S):
    n_max = c.pos0 + c.Tn
    if defect == "key64_dropped":
        return n_max > 64
    if defect in ("last_key_dropped", "tail_key_twice"):
        return n_max > 1
    if defect == "row_map_ignored":
        j = c.pos0 // 2
        return c.pos0 > 0 and S["rm"] is not None and bool((S["rm"][:, j].cpu() != torch.arange(c.R)).any())
    if defect == "stale_slot":
        return bool(c.append)
    if defect == "sibling_key":
        return c.path == 1
    if defect == "second_pass_ignored":
        return c.path == 1 and max(len(e) for e in union(S["rm"], c.R, c.group, c.pos0)) > PASS
    if defect == "union_lost_block":
        return c.path == 1 and c.pos0 > 64
    raise ValueError(defect)


def reference(c, S, defect=None, dtype=torch.float64):
    """the step on the stored buffers S (see stored()).  defect: one of DEFECTS — what a kernel with that one mistake would compute:
      key64_dropped        key 64, the first of a second trip of every 64-key loop, left out
      last_key_dropped     a query's newest key (its own position) left out
      tail_key_twice       the clamped tail load taken for a key of its own: the newest key counted twice
      row_map_ignored      at position pos0 // 2 every row reads its own cache row instead of the one its table names
      stale_slot           (append) key pos0 read from the cache slot, which still holds what was there before, instead of from qkv
      sibling_key          (group form) a beam also attends to the new key of the next beam of its group (an owner bit too many)
      second_pass_ignored  (group form) union entries 128 and up — the second and later passes — take no part
      union_lost_block     (group form) the union's running count not carried across 64-position blocks: only the last block's entries
                           and the new keys remain
    dtype float32 (defect None): the correct kernel's arithmetic in fp32, for the CPU test of the bounds."""
    dev = S["qkv"].device
    q, Kg, Vg = _keys(c, S, dtype)
    mult = _causal(c, dev)
    R, P, Gw = c.R, c.pos0, c.group
    if defect == "key64_dropped":
        mult[:, :, 64] = 0.0                              # (a query with 64 keys or fewer does not see it anyway)
    elif defect in ("last_key_dropped", "tail_key_twice"):
        t = torch.arange(c.Tn, device=dev)
        many = (P + t) > 0                                # a query with one key has nothing to lose
        mult[:, t[many], P + t[many]] = 0.0 if defect == "last_key_dropped" else 2.0
    elif defect == "row_map_ignored":
        j = P // 2
        Kg[:, j], Vg[:, j] = S["kc"].to(dtype)[:, j], S["vc"].to(dtype)[:, j]
    elif defect == "stale_slot":
        Kg[:, P], Vg[:, P] = S["kc"].to(dtype)[:, P], S["vc"].to(dtype)[:, P]
    elif defect == "sibling_key":
        sib = (torch.arange(R, device=dev) // Gw) * Gw + (torch.arange(R, device=dev) % Gw + 1) % Gw
        Kg, Vg = torch.cat([Kg, Kg[sib, P:P + 1]], 1), torch.cat([Vg, Vg[sib, P:P + 1]], 1)
        mult = torch.cat([mult, torch.ones(R, c.Tn, 1, dtype=mult.dtype, device=dev)], -1)
    elif defect == "second_pass_ignored":
        for s_, ent in enumerate(union(S["rm"], R, Gw, P)):
            for (_, j, bits) in ent[PASS:]:
                for b in range(Gw):
                    if (bits >> b) & 1:
                        mult[s_ * Gw + b, 0, j] = 0.0
    elif defect == "union_lost_block":
        mult[:, :, :64 * ((P - 1) // 64)] = 0.0
    elif defect is not None:
        raise ValueError(defect)
    return _attend(c, q, Kg, Vg, mult)


def bounds(c, Rf, op):
    """per-element bound [R][Tn][D] on |kernel - Rf['out']| (module docstring)"""
    qh, kh, vh, s, m, Aw, live, out = (Rf[x] for x in ("qh", "kh", "vh", "s", "m", "A", "live", "oh"))
    hd = c.hd
    sf = torch.where(live, s, torch.zeros_like(s))
    ds = hd ** -0.5 * 2.0 * hd * U32 * (qh.abs() @ kh.abs().transpose(-1, -2)) + 3.0 * U32 * sf.abs()
    x = torch.where(live, m - sf, torch.zeros_like(sf))
    rho = torch.where(live, ds + U32 * (A.EXP_ULPS + 1.0) * (1.0 + x), torch.zeros_like(sf))
    rmax = rho.max().item()
    assert rmax < 0.25, rmax
    Arho = Aw * rho
    e1 = (Arho @ vh.abs() + Arho.sum(-1, keepdim=True) * out.abs()) / (1.0 - rmax)
    n = live.sum(-1, keepdim=True).to(out.dtype)
    e3 = 2.0 * n * U32 * (Aw @ vh.abs() + out.abs())
    e4 = DIV_ROUNDINGS * U32 * out.abs()
    b = G.store_bound(out, A.SECOND_ORDER * (e1 + e3 + e4), DT[op]) + A.TINY
    return b.transpose(1, 2).reshape(c.R, c.Tn, c.D)


# ---- the cases both tests walk ------------------------------------------------------------------------------------------------------------
ROW_HD = (8, 16, 24, 40, 64, 96, 128, 256)
GROUP_POS = (0, 1, 63, 64, 65, 76, 128)
GROUP_TABLES = ("shared", "none", "prefix", "scattered", "cross")


def row_cases():
    """k_decode_attn.  Key counts per launch: 1 .. 66 | 31 .. 34 | 61 .. 68 | 77 | 125 .. 130 | 200; ctx_max equal to and beyond pos0 + Tn;
    tables null / random / beam-like; append 0 and 1; every lane layout (power-of-two chunk counts 1 .. 16: hd 8, 16, 64, 128; the scalar
    path: hd 24, 40, 96, 256; idle PV lanes: hd 24, 40, 96)."""
    out = []
    for hd in ROW_HD:
        out += [Case(hd, 2, 66, 0, 66, "null", append=1),
                Case(hd, 2, 4, 30, 40, "null", append=0),
                Case(hd, 3, 8, 60, 80, "random", append=0),
                Case(hd, 6, 1, 76, 77, "beam", append=1, bw=3),
                Case(hd, 3, 6, 124, 130, "random", append=1),
                Case(hd, 6, 1, 199, 256, "beam", append=0, bw=3)]
    out.append(Case(64, 6, 3, 70, 80, "beam", group=3, append=1))          # a group hint on a multi-position call: the per-row kernel
    return out


def lds_edge_cases():
    """head dim 64: ctx_max = 1792 is the last the per-row kernel's LDS admits (4 (2 ctx_max + 512) 4 = 64 KiB); 1793 is refused"""
    assert row_lds(1792, 64) == LDS_LIMIT
    return Case(64, 2, 4, 1788, 1792, "null", append=1, H=1, npos=2048), Case(64, 2, 4, 1788, 1793, "null", append=1, H=1, npos=2048)


def group_cases():
    """k_group_union + k_decode_attn_group, head dim 64, two groups: every G in 2 .. 8 at every pos0 of GROUP_POS, the five table kinds and
    append 0 / 1 rotating over them; union sizes 127 / 128 / 129 / 256 / 257 / 385 by sharing a prefix of k positions
    (nU = G (pos0 - k) + k + G); the LDS fallback edge of G = 8 (pos0 = 175: group form, 176: per-row kernel)."""
    out = []
    for G_ in range(2, 9):
        for i, pos0 in enumerate(GROUP_POS):
            tb = GROUP_TABLES[(G_ + i) % 5]
            out.append(Case(64, 2 * G_, 1, pos0, pos0 + 1 + (i % 2) * 7, tb, group=G_, append=(G_ + i // 2) % 2, k=pos0 // 3 if tb == "prefix" else 0))
    for (G_, pos0, k, nU, app) in ((2, 63, 1, 127, 1), (2, 63, 0, 128, 0), (2, 64, 0, 130, 1), (2, 64, 1, 129, 0), (2, 127, 0, 256, 1), (2, 128, 1, 257, 0),
                                   (5, 76, 0, 385, 1), (5, 76, 0, 385, 0)):
        c = Case(64, 2 * G_, 1, pos0, pos0 + 1, "prefix", group=G_, append=app, k=k)
        c.want_nU = nU
        out.append(c)
    for pos0, app in ((175, 1), (175, 0), (176, 1), (176, 0)):
        out.append(Case(64, 16, 1, pos0, 180, "scattered", group=8, append=app))
    return out


def all_cases():
    return row_cases() + [lds_edge_cases()[0]] + group_cases()
