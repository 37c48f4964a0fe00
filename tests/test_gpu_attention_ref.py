"""The attention launchers attn_fwd / attn_bwd one call at a time through the test hooks cc_attention_fwd_x / cc_attention_bwd_x — with
attention-probability dropout and, in the split-bf16 build, the operand-image outputs — against float64 (tests/attn_ref.py) in all three
operand builds.  Outputs are NaN-filled before every call; every element must be finite and inside its own bound, and a failure names the
kernel and the worst element (b, h, row i or key j, d).  The bounds are derived in tests/attn_ref.py from the kernels' rounding points, none
tuned; the device exp / log allowances come from test_measured_allowances (run it with -s to see the raw figures).  tests/test_attn_ref.py
shows on the CPU that the same bounds reject every emulated defect at these very cases.

The backward is handed the float64 reference's lse (as fp32) and output (in the stored type), not the forward kernel's, so a forward defect
cannot hide in or be blamed on the backward.  The dropout mask is read with cc_dropout_mask at shape (B, H, S, S) and handed to the reference.

case -> kernel (attn_ref.paths; every S below in the families flat / peaked / rising / offset, causal and not, B, H in 2 .. 3):
  head dim 64 / 96 / 128, S in 1 31 32 33 64 65 97 160 200, forward:
      bf16, fp16: k_attn_fwd_mfma<HD, causal>                    split-bf16: k_attn_fwd_mfma3<HD, causal>
  backward with o and delta_ws, head dim 64: S 32 | 33 64 | 65 97 160, head dim 96: 32 | 33 64 | 65, head dim 128: 32 | 33:
      bf16, fp16: k_attn_bwd_fused<NBLK 1> | <NBLK 2> | k_attn_bwd_dq + k_attn_bwd_dkv
      split-bf16: k_attn_bwd_m3<1> | <2> (head dim 64 / 96) | k_attn_bwd (head dim 64 / 96 at S = 65, head dim 128 at 32 / 33) |
                  k_attn_bwd_rows_dq + _dkv (head dim 64 at S = 97 / 160; S = 89 and head dim 128 at S = 61 in test_images_x3)
  head dim 8 / 40, S in 7 31 | 32 50, o and delta_ws NULL: k_attn_fwd, k_attn_bwd_small | k_attn_bwd in every build
  dropout (causal; p 0.1 / 0.5, two seeds, layers 3 / 11): the <.., true, true> specialisations of all the MFMA and three-term kernels above
      at the same S lists, and in the split-bf16 build k_attn_fwd<true, true>, k_attn_bwd_small<true, true> (head dim 32, S = 17) and
      k_attn_bwd<true, true> (head dim 32 at S = 40; head dim 64 / 96 at S = 65, head dim 128 at 32 / 33); the row kernels carry none and
      refuse (test_refusals)
  images (split-bf16): k_attn_fwd_mfma3 / k_attn_bwd_m3 with img at head dim 64 / 96, S = 20, 33, 64; k_attn_bwd's image store at the
      legality edge (head dim 64: S = 88; head dim 128: S = 60, with k_attn_fwd_mfma3's image)."""
import ctypes as C

import pytest
import torch

from tests import attn_ref as R

pytestmark = pytest.mark.gpu

OPS = {"bf16": (0, torch.bfloat16), "fp16": (1, torch.float16), "x3": (2, torch.float32)}
ERR_ARG, ERR_SHAPE, ERR_STATE = -1, -2, -4
DROP_ATTN = 1


def _lib():
    from clipcap_amd import _lib
    return _lib.lib()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nan(shape, dt):
    return torch.full(shape, float("nan"), dtype=dt, device="cuda")


class Report:
    def __init__(self, tag):
        self.tag, self.fail, self.worst = tag, [], {}

    def bound(self, case, kernel, name, got, ref, bound):
        """got, ref, bound: [B][H][S][hd] or [B][H][S]"""
        got = got.double()
        if not torch.isfinite(got).all():
            idx = tuple(int(x) for x in (~torch.isfinite(got)).nonzero()[0])
            self.fail.append(f"{case} {kernel} {name}: non-finite at (b, h, row, d) = {idx}")
            return
        ratio = (got - ref).abs() / bound
        r = ratio.max().item()
        self.worst[name] = max(self.worst.get(name, 0.0), r)
        if r > 1.0:
            at = tuple(int(x) for x in torch.unravel_index(ratio.argmax(), ratio.shape))
            self.fail.append(f"{case} {kernel} {name}: error / bound = {r:.3f} at (b, h, row, d) = {at} "
                             f"(got {got[at].item():.6g}, float64 {ref[at].item():.6g}, bound {bound[at].item():.3g})")

    def check(self, what, cond):
        if not cond:
            self.fail.append(what)

    def done(self):
        print(f"RATIO {self.tag} " + " ".join(f"{k} {v:.4f}" for k, v in sorted(self.worst.items())))
        assert not self.fail, f"{self.tag}: {len(self.fail)} failures: " + "; ".join(self.fail[:12])


def dropout_mask(c):
    keep = torch.zeros(c.B, c.H, c.S, c.S, dtype=torch.uint8, device="cuda")
    assert _lib().cc_dropout_mask(c.seed, DROP_ATTN, c.layer, c.p, keep.numel(), _p(keep), _st()) == 0
    return keep


class Run:
    """one case on the device: stored inputs, float64 reference, and the two hook calls"""

    def __init__(self, op, c):
        self.op, self.c = op, c
        self.code, self.dt = OPS[op]
        qkv, dout = c.inputs()
        self.qkv, self.dout = qkv.cuda().to(self.dt), dout.cuda().to(self.dt)
        self.D = c.H * c.hd
        self.keep = dropout_mask(c) if c.p else None
        q, k, v = R.heads(self.qkv, c.B, c.S, c.H, c.hd)
        self.ref = R.reference(q, k, v, R.rows(self.dout, c.B, c.S, c.H, c.hd), c.causal, self.keep, c.p)
        (self.fk, self.ffam), (self.bk, self.bfam) = R.paths(op, c.S, c.hd, c.mfma_bwd)
        self.lse_in = self.ref["lse"].float().contiguous()
        self.o_in = R.unrows(self.ref["out"]).to(self.dt).contiguous()

    def fwd(self, p=None, layer=None, seed=None, causal=None, img=0, plain_hook=False):
        c = self.c
        out = _nan((c.B * c.S, 3 * self.D), torch.bfloat16) if img else _nan((c.B * c.S, self.D), self.dt)
        lse = _nan((c.B, c.H, c.S), torch.float32)
        causal = c.causal if causal is None else causal
        if plain_hook:
            rc = _lib().cc_attention_fwd(self.code, _p(self.qkv), c.B, c.S, c.H, c.hd, causal, _p(out), _p(lse), _st())
        else:
            rc = _lib().cc_attention_fwd_x(self.code, _p(self.qkv), c.B, c.S, c.H, c.hd, causal, _p(out), img, _p(lse), c.p if p is None else p,
                                           c.seed if seed is None else seed, c.layer if layer is None else layer, _st())
        torch.cuda.synchronize()
        return rc, out, lse

    def bwd(self, p=None, layer=None, causal=None, img=0, plain_hook=False, lse=None, o=None):
        c = self.c
        dqkv = _nan((c.B * c.S, 9 * self.D), torch.bfloat16) if img else _nan((c.B * c.S, 3 * self.D), self.dt)
        delta = _nan((c.B * c.H * c.S,), torch.float32) if c.mfma_bwd else None
        o = (self.o_in if o is None else o) if c.mfma_bwd else None
        lse = self.lse_in if lse is None else lse
        causal = c.causal if causal is None else causal
        if plain_hook:
            rc = _lib().cc_attention_bwd(self.code, _p(self.qkv), _p(self.dout), _p(o), _p(lse), _p(delta), c.B, c.S, c.H, c.hd, causal, _p(dqkv), _st())
        else:
            rc = _lib().cc_attention_bwd_x(self.code, _p(self.qkv), _p(self.dout), _p(o), _p(lse), _p(delta), c.B, c.S, c.H, c.hd, causal, _p(dqkv), img,
                                           c.p if p is None else p, c.seed, c.layer if layer is None else layer, _st())
        torch.cuda.synchronize()
        return rc, dqkv

    def check(self, rep):
        c = self.c
        rc, out, lse = self.fwd()
        rep.check(f"{c.id} {self.fk}: rc {rc}", rc == 0)
        if rc == 0:
            fb = R.fwd_bounds(self.ref, self.op, self.ffam)
            rep.bound(c.id, self.fk, "out", R.rows(out, c.B, c.S, c.H, c.hd), self.ref["out"], fb["out"])
            rep.bound(c.id, self.fk, "lse", lse, self.ref["lse"], fb["lse"])
        if not c.bwd:
            return
        rc, dqkv = self.bwd()
        rep.check(f"{c.id} {self.bk}: rc {rc}", rc == 0)
        if rc == 0:
            from_o = c.mfma_bwd and any(x in self.bk for x in ("fused", "dq+dkv", "rows"))
            bb = R.bwd_bounds(self.ref, self.op, self.bfam, from_o, self.lse_in, R.rows(self.o_in, c.B, c.S, c.H, c.hd))
            g = dqkv.view(c.B * c.S, 3, self.D)
            for t, name in enumerate(("dq", "dk", "dv")):
                rep.bound(c.id, self.bk, name, R.rows(g[:, t], c.B, c.S, c.H, c.hd), self.ref[name], bb[name])


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("op", list(OPS))
def test_plain(op, family):
    """no dropout: every forward and backward kernel at every shape of the table, causal and not"""
    rep = Report(f"{op} {family}")
    for c in R.plain_cases():
        if c.family == family:
            Run(op, c).check(rep)
    rep.done()


@pytest.mark.parametrize("op", list(OPS))
def test_dropout(op):
    """causal attention-probability dropout on every kernel that carries it, against float64 with the library's own mask stream"""
    rep = Report(f"{op} dropout")
    for c in R.dropout_cases(op):
        r = Run(op, c)
        kept = r.keep.float().mean().item()
        rep.check(f"{c.id}: kept fraction {kept:.3f}", c.S < 17 or abs(kept - (1 - c.p)) < 0.1)
        r.check(rep)
        if c.S in (33, 65, 40):              # bit-level properties, at a second-key-block shape of every kernel
            rc, out, lse = r.fwd()
            rc2, out2, lse2 = r.fwd()
            rep.check(f"{c.id}: forward twice", rc == 0 and rc2 == 0 and _same(out, out2) and _same(lse, lse2))
            rc3, out3, _ = r.fwd(layer=c.layer + 1)
            rep.check(f"{c.id}: another layer, same forward output", rc3 == 0 and not _same(out, out3))
            rc0, outp, lsep = r.fwd(plain_hook=True)
            rcx, out0, lse0 = r.fwd(p=0.0)
            rep.check(f"{c.id}: p = 0 forward differs from cc_attention_fwd", rc0 == 0 and rcx == 0 and _same(outp, out0) and _same(lsep, lse0))
            if c.bwd:
                rc, g = r.bwd()
                rc2, g2 = r.bwd()
                rep.check(f"{c.id}: backward twice", rc == 0 and rc2 == 0 and _same(g, g2))
                rc3, g3 = r.bwd(layer=c.layer + 1)
                rep.check(f"{c.id}: another layer, same backward output", rc3 == 0 and not _same(g, g3))
                rc0, gp = r.bwd(plain_hook=True)
                rcx, g0 = r.bwd(p=0.0)
                rep.check(f"{c.id}: p = 0 backward differs from cc_attention_bwd", rc0 == 0 and rcx == 0 and _same(gp, g0))
    rep.done()


@pytest.mark.parametrize("op", list(OPS))
def test_refusals(op):
    """what the hooks and the launchers refuse comes back as an error code with every output byte untouched"""
    rep = Report(f"{op} refusals")

    def untouched(what, rc, want, *bufs):
        rep.check(f"{what}: rc {rc}, expected {want}", rc == want)
        rep.check(f"{what}: an output was written", all(bool(torch.isnan(b.float()).all()) for b in bufs))

    for hd, S, mf in ((64, 40, True), (96, 33, True), (128, 70, True)) + (((32, 17, False), (32, 40, False)) if op == "x3" else ()):
        r = Run(op, R.Case("flat", hd, S, 1, True, mfma_bwd=mf, p=0.1, seed=5, layer=2))
        rc, out, lse = r.fwd(causal=0)
        untouched(f"hd {hd} S {S} forward dropout without causal", rc, ERR_SHAPE, out, lse)
        rc, g = r.bwd(causal=0)
        untouched(f"hd {hd} S {S} backward dropout without causal", rc, ERR_SHAPE, g)
        for p, layer in ((1.0, 2), (-0.1, 2), (float("nan"), 2), (0.1, 256), (0.1, -1)):
            rc, out, lse = r.fwd(p=p, layer=layer)
            untouched(f"forward p {p} layer {layer}", rc, ERR_ARG, out, lse)
            rc, g = r.bwd(p=p, layer=layer)
            untouched(f"backward p {p} layer {layer}", rc, ERR_ARG, g)
    if op == "x3":       # the row kernels (LDS tile too large, no MFMA head dim) carry no dropout
        r = Run(op, R.Case("flat", 32, 180, 1, True, p=0.1, seed=5, layer=2))
        assert r.fk == "k_attn_fwd_rows" and r.bk == "k_attn_bwd_rows"
        rc, out, lse = r.fwd()
        untouched("row-kernel forward with dropout", rc, ERR_SHAPE, out, lse)
        rc, g = r.bwd()
        untouched("row-kernel backward with dropout", rc, ERR_SHAPE, g)
        for S in (97, 160):       # head dim 64 past the LDS tile: the three-term forward carries dropout, the row-kernel backward refuses
            r = Run(op, R.Case("flat", 64, S, 1, True, p=0.1, seed=5, layer=2))
            assert r.bk == "k_attn_bwd_rows"
            rc, g = r.bwd()
            untouched(f"head dim 64 S {S} row-kernel backward with dropout", rc, ERR_SHAPE, g)
    else:                # images exist in the split-bf16 build only
        r = Run(op, R.Case("flat", 64, 20, 1, True))
        D = r.D
        out, lse, g = _nan((r.c.B * 20, 3 * D), torch.bfloat16), _nan((r.c.B, r.c.H, 20), torch.float32), _nan((r.c.B * 20, 9 * D), torch.bfloat16)
        rc = _lib().cc_attention_fwd_x(r.code, _p(r.qkv), r.c.B, 20, r.c.H, 64, 1, _p(out), D, _p(lse), 0.0, 0, 0, _st())
        torch.cuda.synchronize()
        untouched("image forward in a 16-bit build", rc, ERR_ARG, out, lse)
        rc = _lib().cc_attention_bwd_x(r.code, _p(r.qkv), _p(r.dout), _p(r.o_in), _p(r.lse_in), None, r.c.B, 20, r.c.H, 64, 1, _p(g), 3 * D, 0.0, 0, 0, _st())
        torch.cuda.synchronize()
        untouched("image backward in a 16-bit build", rc, ERR_ARG, g)
    rep.done()


def _split_rows(src, width):
    """cc_x3_split_rows form 0 of fp32 [rows][width] -> bf16 [rows][3 width]"""
    dst = _nan((src.shape[0], 3 * width), torch.bfloat16)
    assert _lib().cc_x3_split_rows(2, _p(src), width, src.shape[0], width, 0, _p(dst), _st()) == 0
    torch.cuda.synchronize()
    return dst


def test_images_x3():
    """split-bf16 build: with Act.img set, out / dqkv are bit for bit cc_x3_split_rows(form 0) of what the plain call writes — the image
    stores split the very fp32 accumulator values the plain stores write (k_attn_fwd_mfma3, k_attn_bwd_m3, k_attn_bwd), so nothing rounds
    differently between the two modes.  The legality edge of attn_bwd_can_image / attn_fwd_can_image is where attn_ref.attn_bwd_lds (the
    kernels' formula) crosses 160 KiB: the last legal S writes a correct image, the next returns CC_ERR_STATE and writes nothing."""
    rep = Report("x3 images")

    def pair(r, what):
        c = r.c
        rc, out, lse = r.fwd()
        rci, outi, lsei = r.fwd(img=r.D)
        ok = rc == 0 and rci == 0
        rep.check(f"{what} forward: rc {rc} / {rci}", ok)
        if ok:
            rep.check(f"{what} forward image differs from the split of the plain output", _same(outi, _split_rows(out, r.D)) and _same(lse, lsei))
        rc, g = r.bwd()
        rci, gi = r.bwd(img=3 * r.D)
        ok = rc == 0 and rci == 0
        rep.check(f"{what} backward: rc {rc} / {rci}", ok)
        if ok:
            rep.check(f"{what} backward image differs from the split of the plain output", _same(gi, _split_rows(g, 3 * r.D)))

    for hd in (64, 96):
        for S in (20, 33, 64):
            for p in (0.0, 0.1):
                r = Run("x3", R.Case("flat", hd, S, 1, True, p=p, seed=77, layer=5))
                pair(r, f"hd {hd} S {S} p {p}")
                if p == 0.0:
                    rc, out, _ = r.fwd(img=r.D + 8)
                    rep.check(f"hd {hd} S {S}: wrong image width accepted", rc == ERR_STATE and bool(torch.isnan(out.float()).all()))
    for hd in (64, 128):
        edge = R.bwd_lds_edge(hd)
        r = Run("x3", R.Case("flat", hd, edge, 1, True, BH_=(2, 2)))
        rep.check(f"hd {hd} S {edge}: expected the LDS-tile backward", r.bk == "k_attn_bwd")
        pair(r, f"hd {hd} S {edge} (edge)")
        r = Run("x3", R.Case("flat", hd, edge + 1, 1, True, BH_=(2, 2)))
        rc, out, lse = r.fwd(img=r.D)
        rep.check(f"hd {hd} S {edge + 1} forward image: rc {rc}", rc == ERR_STATE and bool(torch.isnan(out.float()).all()) and bool(torch.isnan(lse).all()))
        rc, g = r.bwd(img=3 * r.D)
        rep.check(f"hd {hd} S {edge + 1} backward image: rc {rc}", rc == ERR_STATE and bool(torch.isnan(g.float()).all()))
        r.check(rep)          # the plain call past the edge (row kernels) still computes attention
    rep.done()


def test_measured_allowances():
    """Re-measures the two figures tests/attn_ref.py cannot derive and prints them (pytest -s): after a compiler or ROCm update take the
    allowances as 4 x what this prints.  Asserts only that the raw figures are still inside the allowances in force.  Both go through the fp32
    LDS/VALU kernels of the split-bf16 build with q = 0 (every score exactly 0), where the device function's value reaches an output with no
    other rounding on the way:
      * __expf: k_attn_bwd_small, S = 31, hd = 32, dO row i = unit vector i: dv[j][d] = P[d][j] = __expf(-lse[d]) with lse handed in,
        arguments over [-80, 0] (below -87 the result leaves fp32's normal range), in units of 2^-24 exp(x) (1 + |x|);
      * __logf: k_attn_fwd, hd = 8, S = 1 .. 180: l = S exactly (S ones), lse = __logf(S), in units of 2^-24 max(1, log S)."""
    l = _lib()
    B, H, S, hd = 16, 16, 31, 32
    D = H * hd
    g = torch.Generator(device="cuda").manual_seed(3)
    qkv = torch.randn(B, S, 3, H, hd, device="cuda", generator=g)
    qkv[:, :, 0] = 0.0
    dout = torch.zeros(B, S, H, hd, device="cuda")
    dout[:, torch.arange(S), :, torch.arange(S)] = 1.0
    lse = torch.rand(B, H, S, device="cuda", generator=g) * 80.0
    lse[0, 0, 0] = 0.0
    dqkv = _nan((B * S, 3 * D), torch.float32)
    assert l.cc_attention_bwd_x(2, _p(qkv), _p(dout), None, _p(lse), None, B, S, H, hd, 0, _p(dqkv), 0, 0.0, 0, 0, _st()) == 0
    torch.cuda.synchronize()
    dv = dqkv.view(B, S, 3, H, hd)[:, :, 2].permute(0, 2, 1, 3)[..., :S].double()             # [B][H][key j][d = query]
    x = -lse.double().unsqueeze(2)                                                           # [B][H][1][query]
    worst_exp = ((dv - torch.exp(x)).abs() / (R.U32 * torch.exp(x) * (1.0 + x.abs()))).max().item()
    print(f"MEASURED __expf over [-80, 0], {B * H * S} arguments: {worst_exp:.4f} x 2^-24 exp(x) (1 + |x|)   (allowance {R.EXP_ULPS})")
    worst_log = 0.0
    for S in range(1, 181):
        qkv = torch.zeros(S, 3 * 8, device="cuda")
        out, ls = _nan((S, 8), torch.float32), _nan((1, 1, S), torch.float32)
        assert l.cc_attention_fwd_x(2, _p(qkv), 1, S, 1, 8, 0, _p(out), 0, _p(ls), 0.0, 0, 0, _st()) == 0
        torch.cuda.synchronize()
        want = torch.log(torch.tensor(float(S), dtype=torch.float64)).item()
        worst_log = max(worst_log, ((ls.double() - want).abs() / (R.U32 * max(1.0, want))).max().item())
    print(f"MEASURED __logf at l = 1 .. 180: {worst_log:.4f} x 2^-24 max(1, log l)   (allowance {R.LOG_ULPS})")
    assert worst_exp <= R.EXP_ULPS and worst_log <= R.LOG_ULPS
