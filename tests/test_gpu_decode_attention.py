"""The KV-cached attention step of one decode layer, one call at a time through the test hook cc_decode_attention (the product's own
dispatch: decode.hip's decode_attn_plan / decode_attn_run), against float64 (tests/decode_ref.py) in all three operand builds: the per-row
kernel k_decode_attn<APPEND> at every lane layout and on both sides of every loop boundary, k_group_union + k_decode_attn_group<G> for
every G, at one to four passes and at the LDS fallback edge.

Every call runs on poisoned buffers: each cache slot no table names, every position >= pos0 + Tnew (with append = 1 also the new slots,
which the kernel itself must fill), the output, and a guard band before and behind every buffer hold NaN.  (All buffers are dense — the
cache row stride is D, qkv's 3 D — so there is no pad inside a row to poison.)  A read of a slot the step must not read then shows as a
non-finite output; a stray write as a changed cache element or guard.  Asserted per case: the return code, the reported path (and for the
group form the union size and pass count the case was written for, from decode_ref's mirror of k_group_union), err <= bound for every
output element, and the cache post-condition bit for bit.  The bounds are derived in tests/decode_ref.py from the kernels' rounding
points, none tuned; tests/test_decode_ref.py shows on the CPU that they reject every emulated defect at these very cases."""
import ctypes as C

import pytest
import torch

from tests import decode_ref as R

pytestmark = pytest.mark.gpu

OPS = {"bf16": 0, "fp16": 1, "x3": 2}
ERR_ARG, ERR_SHAPE = -1, -2
GUARD = 256          # elements of NaN before and behind every buffer


def _lib():
    from clipcap_amd import _lib
    return _lib.lib()


def _cfg(c, op):
    from clipcap_amd._lib import Gpt2Cfg
    return Gpt2Cfg(c.D, c.H, 1, 128, 128, c.npos, OPS[op])


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


class Guarded:
    """a device buffer with a NaN band on either side"""

    def __init__(self, n, dt):
        self.flat = torch.full((n + 2 * GUARD,), float("nan"), dtype=dt, device="cuda")
        self.t = self.flat[GUARD:GUARD + n]
        self.ptr = C.c_void_p(self.t.data_ptr())

    def guards_intact(self):
        return bool(torch.isnan(self.flat[:GUARD]).all()) and bool(torch.isnan(self.flat[-GUARD:]).all())


class Call:
    """one case on the device: poisoned buffers, the hook call, what came back"""

    def __init__(self, op, c):
        self.op, self.c = op, c
        dt = R.DT[op]
        self.S = S = R.stored(c, op, "cuda")
        n = c.R * c.ctx_max * c.D
        self.qkv, self.kv, self.out = Guarded(S["qkv"].numel(), dt), Guarded(2 * n, dt), Guarded(c.R * c.Tn * c.D, dt)
        self.qkv.t.copy_(S["qkv"].view(-1))
        kv = self.kv.t.view(2, c.R, c.ctx_max, c.D)
        nan = torch.full((), float("nan"), dtype=dt, device="cuda")
        kv[0] = torch.where(S["named"].unsqueeze(-1), S["kc"], nan)
        kv[1] = torch.where(S["named"].unsqueeze(-1), S["vc"], nan)
        self.before = kv.clone()
        self.rm = None if S["rm"] is None else S["rm"].to(torch.int32).contiguous()
        self.cfg = _cfg(c, op)
        nb = _lib().cc_decode_ws_bytes(C.byref(self.cfg), c.R, c.Tn)
        assert nb > 0, nb
        self.ws = torch.zeros(nb + 256, dtype=torch.uint8, device="cuda")

    def run(self, **over):
        c = self.c
        a = dict(R=c.R, Tn=c.Tn, pos0=c.pos0, ctx_max=c.ctx_max, qkv=self.qkv.ptr, kv=self.kv.ptr, rm=None if self.rm is None else C.c_void_p(self.rm.data_ptr()),
                 group=c.group, append=c.append, ws=C.c_void_p(self.ws.data_ptr()), out=self.out.ptr)
        a.update(over)
        path = C.c_int32(-7)
        rc = _lib().cc_decode_attention(C.byref(self.cfg), a["R"], a["Tn"], a["pos0"], a["ctx_max"], a["qkv"], a["kv"], a["rm"], a["group"], a["append"],
                                        a["ws"], a["out"], C.byref(path), _st())
        torch.cuda.synchronize()
        return rc, path.value

    def untouched(self):
        kv = self.kv.t.view(2, self.c.R, self.c.ctx_max, self.c.D)
        return bool(torch.isnan(self.out.t).all()) and _same(kv, self.before) and self.guards()

    def guards(self):
        return self.qkv.guards_intact() and self.kv.guards_intact() and self.out.guards_intact() and _same(self.qkv.t, self.S["qkv"].view(-1))


class Report:
    def __init__(self, tag):
        self.tag, self.fail, self.worst = tag, [], 0.0

    def check(self, what, cond):
        if not cond:
            self.fail.append(what)

    def case(self, op, c):
        x = Call(op, c)
        rc, path = x.run()
        self.check(f"{c.id}: rc {rc}", rc == 0)
        if rc != 0:
            return
        self.check(f"{c.id}: path {path}, written for {c.path}", path == c.path)
        if c.path == 1:
            nU = max(len(e) for e in R.union(x.S["rm"], c.R, c.group, c.pos0))
            self.check(f"{c.id}: union of {nU} entries, written for {c.want_nU}", c.want_nU in (None, nU))
            self.check(f"{c.id}: {-(-nU // R.PASS)} passes in a list of {R.grp_cap(c.group, c.pos0)}", nU <= R.grp_cap(c.group, c.pos0))
        ref = R.reference(c, x.S)
        bound = R.bounds(c, ref, op)
        got = x.out.t.view(c.R, c.Tn, c.D).double()
        if not torch.isfinite(got).all():
            at = tuple(int(v) for v in (~torch.isfinite(got)).nonzero()[0])
            self.fail.append(f"{c.id}: non-finite output at (row, t, d) = {at}: a slot the step must not read was read")
        else:
            ratio = (got - ref["out"]).abs() / bound
            r = ratio.max().item()
            self.worst = max(self.worst, r)
            if r > 1.0:
                at = tuple(int(v) for v in torch.unravel_index(ratio.argmax(), ratio.shape))
                self.fail.append(f"{c.id}: error / bound = {r:.3f} at (row, t, d) = {at} (got {got[at].item():.6g}, float64 {ref['out'][at].item():.6g}, "
                                 f"bound {bound[at].item():.3g})")
        # the cache afterwards: the state before (NaN in every unnamed slot) with, under append, the new slots equal to the qkv slices
        want = x.before.clone()
        if c.append:
            q = x.S["qkv"].view(c.R, c.Tn, 3, c.D)
            want[0][:, c.pos0:c.pos0 + c.Tn], want[1][:, c.pos0:c.pos0 + c.Tn] = q[:, :, 1], q[:, :, 2]
        kv = x.kv.t.view(2, c.R, c.ctx_max, c.D)
        for i, name in enumerate("KV"):
            if not _same(kv[i], want[i]):
                bad = (kv[i].contiguous().view(torch.uint8) != want[i].contiguous().view(torch.uint8)).view(c.R, c.ctx_max, -1).any(-1).nonzero()[0]
                self.fail.append(f"{c.id}: {name} cache differs from its post-condition at (row, position) = {tuple(int(v) for v in bad)}")
        self.check(f"{c.id}: a guard band or qkv was written", x.guards())

    def done(self):
        print(f"RATIO {self.tag} out {self.worst:.4f}")
        assert not self.fail, f"{self.tag}: {len(self.fail)} failures: " + "; ".join(self.fail[:12])


@pytest.mark.parametrize("op", list(OPS))
def test_per_row_kernel(op):
    """k_decode_attn<APPEND>: head dims 8 .. 256 (every lane layout), 1 .. 200 keys, tables null / random / beam-like, append 0 / 1"""
    rep = Report(f"{op} per-row")
    for c in R.row_cases():
        rep.case(op, c)
    rep.done()


@pytest.mark.parametrize("op", list(OPS))
def test_group_form(op):
    """k_group_union<G> + k_decode_attn_group<G>: G 2 .. 8, pos0 on both sides of the 64-position block, unions of 127 .. 385 entries (one
    to four passes), every table kind, append 0 / 1, and the LDS fallback edge of G = 8"""
    rep = Report(f"{op} group")
    for c in R.group_cases():
        rep.case(op, c)
    rep.done()


@pytest.mark.parametrize("op", list(OPS))
def test_lds_edge_and_refusals(op):
    """ctx_max = 1792 at head dim 64 is the last the per-row kernel's 64 KiB admit and is right; 1793 returns CC_ERR_SHAPE; so does every
    other bad argument, with CC_ERR_ARG / CC_ERR_SHAPE as cc_decode_fwd_g — and nothing is launched: every output byte keeps its poison"""
    rep = Report(f"{op} edge")
    ok, over = R.lds_edge_cases()
    rep.case(op, ok)
    x = Call(op, over)
    rc, path = x.run()
    rep.check(f"{over.id}: rc {rc}, expected CC_ERR_SHAPE", rc == ERR_SHAPE and path == -7)
    rep.check(f"{over.id}: refused but something was written", x.untouched())
    c = R.Case(64, 6, 1, 9, 12, "beam", group=3, append=1)
    x = Call(op, c)
    for what, over, want in (("group does not divide R", dict(group=4), ERR_ARG), ("group 0", dict(group=0), ERR_ARG), ("R 0", dict(R=0), ERR_ARG),
                             ("Tnew 0", dict(Tn=0), ERR_ARG), ("pos0 < 0", dict(pos0=-1), ERR_ARG), ("append 2", dict(append=2), ERR_ARG),
                             ("qkv NULL", dict(qkv=None), ERR_ARG), ("cache NULL", dict(kv=None), ERR_ARG), ("ws NULL", dict(ws=None), ERR_ARG),
                             ("out NULL", dict(out=None), ERR_ARG), ("pos0 + Tnew > ctx_max", dict(pos0=12), ERR_SHAPE),
                             ("pos0 + Tnew > n_positions", dict(pos0=c.npos, ctx_max=c.npos + 1), ERR_SHAPE)):
        rc, path = x.run(**over)
        rep.check(f"{what}: rc {rc}, expected {want}", rc == want and path == -7)
        rep.check(f"{what}: refused but something was written", x.untouched())
    x.cfg.op_dtype = 7                       # no such operand build
    rc, path = x.run()
    rep.check(f"unknown op_dtype: rc {rc}", rc == ERR_ARG and path == -7 and x.untouched())
    x.cfg.op_dtype = OPS[op]
    # the A/B switch of cc_decode_fwd_g is honoured: bit 0 of cc_decode_mode off -> the per-row kernel, same result
    old = _lib().cc_decode_mode(-1)
    try:
        _lib().cc_decode_mode(old & ~1)
        c.path = 0
        rep.case(op, c)
    finally:
        _lib().cc_decode_mode(old)
    c.path = 1
    rep.case(op, c)
    rep.done()


def test_measured_allowances():
    """Prints (pytest -s) what the device's division really costs, the one figure tests/decode_ref.py counts by attn_ref's convention rather
    than derives (DIV_ROUNDINGS = 4 u32 for the quotient or reciprocal + one multiplication), and asserts it is inside the count.  Split-bf16
    build (fp32 in and out, no store rounding), q = 0 so every score is exactly 0 and every weight exactly 1, v = 1 at key 0 and 0 elsewhere:
    the numerator is exactly 1, the denominator exactly n, out = 1 / n with the division's rounding alone.
      * k_decode_attn (out = acc * (1 / sum)): one launch, head dim 8, pos0 = 0, Tnew = 200: n = 1 .. 200;
      * k_decode_attn_group (out = v / sum): G = 2, head dim 64, pos0 = 0, 3, 6 .. 198: n = pos0 + 1."""
    def measure(c):
        x = Call("x3", c)
        x.qkv.t.zero_()
        kv = x.kv.t.view(2, c.R, c.ctx_max, c.D)
        kv.zero_()
        if c.pos0 == 0:
            x.qkv.t.view(c.R, c.Tn, 3, c.D)[:, 0, 2] = 1.0
        else:
            kv[1][:, 0] = 1.0
        rc, path = x.run()
        assert rc == 0 and path == c.path
        n = torch.arange(c.pos0 + 1, c.pos0 + c.Tn + 1, device="cuda", dtype=torch.float64).view(1, c.Tn, 1)
        return ((x.out.t.view(c.R, c.Tn, c.D).double() - 1.0 / n).abs() * n / R.U32).max().item()

    w_row = measure(R.Case(8, 1, 200, 0, 200, "null", append=1, H=1))
    w_grp = max(measure(R.Case(64, 2, 1, p, p + 1, "null", group=2, append=1, H=1)) for p in range(0, 200, 3))
    print(f"MEASURED 1 / n through k_decode_attn, n = 1 .. 200: {w_row:.4f} x 2^-24 / n; v / n through k_decode_attn_group, n = 1, 4 .. 199: {w_grp:.4f} "
          f"(counted: {R.DIV_ROUNDINGS - 1.0} + 1 for the multiplication)")
    assert w_row <= R.DIV_ROUNDINGS - 1.0 and w_grp <= R.DIV_ROUNDINGS - 1.0


# ---- the KV append of the whole step (cc_decode_fwd_g): c_attn's fused epilogue, or k_decode_attn<APPEND> behind a plain c_attn ----------
SINGLE_MIN_TILES = 60        # gemm_api.h skinny_single_min_tiles(): c_attn grids of at least this many 128 x 128 tiles do not fuse the append


def _append_rows(D, Tn, many):
    """rows on either side of decode_fwd_impl's f_qkv = ceil(M / 128) ceil(3 D / 128) < SINGLE_MIN_TILES, M = rows * Tn"""
    col_tiles = -(-3 * D // 128)
    row_tiles = -(-SINGLE_MIN_TILES // col_tiles)
    rows = ((row_tiles - 1) * 128) // Tn + 1 if many else 4
    assert (-(-rows * Tn // 128) * col_tiles >= SINGLE_MIN_TILES) == many
    return rows


@pytest.mark.parametrize("many", [False, True], ids=["fused-epilogue", "kernel-append"])
@pytest.mark.parametrize("op", list(OPS))
def test_kv_append_of_the_whole_step(op, many):
    """One-layer engine, cc_decode_fwd_g with Tnew = 3 at pos0 = 5 on a cache full of NaN: afterwards slots 5 .. 7 of every cache row hold
    the K and V thirds of ln_1(x + wpe) W_attn + b, every other slot its NaN.  4 rows: c_attn's epilogue stores them (f_qkv); 1238 rows
    (60 tiles): c_attn writes qkv only and k_decode_attn<APPEND> copies.  Reference: float64 GEMM on the exact stored operands — x + wpe is
    one fp32 addition (reproduced bit for bit), ln_1's output is read through cc_layernorm_fwd (the same k_ln_fwd launch, checked against
    float64 LayerNorm here to fp32 accuracy + one stored rounding), W_attn is the operand arena's cast (split-bf16: the three-term product
    misses the exact one by gemm_ref.split_product_bound).  Bound: gemm_ref.acc_bound with the 16-deep MFMA step count (the most roundings
    of the kernels that can take this launch), one addition per K slice and one for the bias, then one stored-type rounding."""
    import math
    from clipcap_amd.engine import DecodeSession, Gpt2Engine
    from tests import gemm_ref as Gm
    D, H, Tn, pos0, ctx_max = 64, 2, 3, 5, 10
    rows = _append_rows(D, Tn, many)
    dt = R.DT[op]
    ge = Gpt2Engine(D, H, 1, 97, 16, device="cuda", precision={"bf16": "bf16", "fp16": 16, "x3": 32}[op])
    g = torch.Generator(device="cuda").manual_seed(5)
    vw = ge.views(ge.arena.w32)
    for k, v in vw.items():
        r = torch.randn(v.shape, generator=g, device="cuda")
        v.copy_(1.0 + 0.1 * r if ("ln_" in k and k.endswith("weight")) else 0.1 * r if k.endswith("bias") else 0.5 * r if "wpe" in k else r / math.sqrt(v.shape[0]))
    name = {k.split(".")[-2] + "." + k.split(".")[-1]: k for k in vw}
    sess = DecodeSession(ge, rows, ctx_max)
    sess.kv.fill_(float("nan"))
    sess.pos = pos0
    x = torch.randn(rows, Tn, D, generator=g, device="cuda") * 0.5
    sess.forward(x)
    torch.cuda.synchronize()
    kv = sess.kv.view(2, rows, ctx_max, D)
    # the stored operands
    M = rows * Tn
    xw = (x + vw[name["wpe.weight"]][pos0:pos0 + Tn].unsqueeze(0)).reshape(M, D).contiguous()
    gam, bet = vw[name["ln_1.weight"]], vw[name["ln_1.bias"]]
    xn = torch.full((M, D), float("nan"), dtype=dt, device="cuda")
    mean, rstd = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    assert _lib().cc_layernorm_fwd(OPS[op], p(xw), p(gam), p(bet), p(xn), p(mean), p(rstd), M, D, _st()) == 0
    torch.cuda.synchronize()
    xd = xw.double()
    xhat = (xd - xd.mean(-1, keepdim=True)) / torch.sqrt(xd.var(-1, unbiased=False, keepdim=True) + 1e-5)
    ln64 = xhat * gam.double() + bet.double()
    ln_b = Gm.store_bound(ln64, 2.0 * (D + 16) * Gm.U32 * ((xhat * gam.double()).abs() + bet.double().abs() + 1.0), dt)      # fp32 sums over D, rsqrt, affine
    assert bool(((xn.double() - ln64).abs() <= ln_b).all()), ((xn.double() - ln64).abs() / ln_b).max().item()
    W, b = vw[name["c_attn.weight"]], vw[name["c_attn.bias"]].double()
    ks = max(1, D // 128)
    if op == "x3":
        ahi, alo = Gm.split(xn)
        bhi, blo = Gm.split(W.t().contiguous())
        _, s3 = Gm.three_term(ahi, alo, bhi, blo)
        ref = xn.double() @ W.double() + b
        accb = Gm.split_product_bound(xn.double().abs() @ W.double().abs()) + Gm.acc_bound(s3 + b.abs(), 3 * D, 1, 1, ksplit=ks, extra=1)
    else:
        Wst = W.to(dt).double()
        ref = xn.double() @ Wst + b
        accb = Gm.acc_bound(xn.double().abs() @ Wst.abs() + b.abs(), D, 1, 1, ksplit=ks, extra=1)
    bound = Gm.store_bound(ref, accb, dt).view(rows, Tn, 3, D)
    ref = ref.view(rows, Tn, 3, D)
    worst = 0.0
    for i, nm in ((0, "K"), (1, "V")):
        got = kv[i][:, pos0:pos0 + Tn].double()
        assert bool(torch.isfinite(got).all()), f"{nm}: a new slot was not written"
        ratio = ((got - ref[:, :, 1 + i]).abs() / bound[:, :, 1 + i]).max().item()
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{nm} slots {pos0} .. {pos0 + Tn - 1}: error / bound = {ratio:.3f}"
        assert bool(torch.isnan(kv[i][:, :pos0]).all()) and bool(torch.isnan(kv[i][:, pos0 + Tn:]).all()), f"{nm}: a slot outside {pos0} .. {pos0 + Tn - 1} was written"
    print(f"RATIO {op} kv-append {'kernel' if many else 'epilogue'} {worst:.4f}")
