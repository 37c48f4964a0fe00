"""The lm_head / cross-entropy chain one stage at a time against float64 (tests/lm_ref.py): cc_lmhead_ce_fwd, cc_lmhead_ce_bwd and
cc_lmhead_score on a residual stream the test puts into the workspace (cc_lmhead_put_x), their per-row state read back through
cc_lmhead_get.  All three builds run in this process (the ABI dispatches on op_dtype).  Every element is held to its own derived bound;
nothing here is tuned to what the kernels return.

Case -> kernels (lm_ref.paths; names of lm_ref.cases):
  every case      k_ce_targets, ln_fwd (row_map), then
  mode 1 / 2 bf16, mode 1 split-bf16 (exponential form): k_lm_tgt_ref, gemm_lmhead with EpiLMHeadExp (split-bf16: E as an operand image),
                  k_ce_rows, k_ce_stats; backward k_lm_rowfac, the input-gradient GEMM, [mode 2: k_lm_rows<1>, gemm_wgrad, scatter_rows], ln_bwd
  mode 1 / 2 fp16, mode 2 split-bf16 (logit form): gemm_lmhead with EpiLMHead, k_ce_rows, k_ce_stats; backward k_ce_dlogits, the
                  input-gradient GEMM, [mode 2: gemm_wgrad], ln_bwd
  score cases     k_score_keep, gemm_lmhead_score with EpiLMHeadScore, k_score_rows, k_score_samples
  -t4 / -t5 with D = 64, 256: the epilogue's `strip` entry point (256- and 320-row kernels); every other tile mode, and D = 96 (K % 64 != 0,
                  register-staged kernel): operator() on the 128 x 128 kernels
  V65601 (npart = 1026): the generic loop of ce_row_fold; V4099 (npart = 66): the second batch of the fast fold; V97 / V130: the first
  V4099 / V65601 with tile mode != 0: gemm_nt_deepk, two or more K slabs, k_deepk_finish_lm (exponential form) / k_splitk_finish;
                  tile mode 0 or V97 / V130: gemm_bf16out, then k_lm_rows<0> (lm_dgrad_fix) in the exponential form
  V130: a 64-column block with no real column (pmax = -inf, psum = 0); V97: a partly padded block."""
import ctypes as C
import math

import pytest
import torch

from tests import gemm_ref as G
from tests import lm_ref as LM

pytestmark = pytest.mark.gpu
CODE = {"bf16": 0, "fp16": 1, "x3": 2}
PREC = {"bf16": "bf16", "fp16": 16, "x3": 32}
LSE, TGT, ROW_LOSS, HF, DHF, DX32 = range(6)
ARG, SHAPE, STATE = -1, -2, -4


def _lib():
    from clipcap_amd import _lib as L
    return L.lib()


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Report:
    """worst |got - ref| / bound over everything one test checked; a failure names case, kernel, quantity and the worst element"""

    def __init__(self, case):
        self.case, self.worst, self.where = case, 0.0, ""

    def check(self, kernel, what, got, ref, bound, rows=None):
        got, ref, bound = got.double(), ref.double(), bound.double().expand_as(ref)
        if rows is not None:
            got, ref, bound = got[rows], ref[rows], bound[rows]
        if got.numel() == 0:
            return
        assert torch.isfinite(got).all(), f"{self.case}: {kernel}: {what} has non-finite elements"
        err = (got - ref).abs()
        exact = bound == 0
        assert not (exact & (err != 0)).any(), f"{self.case}: {kernel}: {what} differs where it must be exact"
        ratio = torch.where(exact, torch.zeros_like(err), err / bound.clamp_min(1e-300))
        i = int(ratio.argmax())
        r = ratio.reshape(-1)[i].item()
        if r > self.worst:
            self.worst, self.where = r, f"{kernel} {what}"
        assert r <= 1.0, (f"{self.case}: {kernel}: {what}[{i}] got {got.reshape(-1)[i].item():.9g} float64 {ref.reshape(-1)[i].item():.9g} "
                          f"bound {bound.reshape(-1)[i].item():.3g} (ratio {r:.2f})")

    def line(self):
        print(f"RATIO {self.case}: worst |err| / bound = {self.worst:.3f} ({self.where})")


class Pass:
    """a one-layer pass of the case's shape: weights synced, the case's residual stream put into the workspace"""

    def __init__(self, op, c, inputs=None):
        from clipcap_amd.engine import Gpt2Engine
        self.op, self.c = op, c
        x, gamma, beta, wte, tok = inputs if inputs is not None else LM.make_inputs(c, op)
        self.T = c.L + c.cap
        self.ge = ge = Gpt2Engine(c.D, 1, 1, c.V, self.T + 1, device="cuda", precision=PREC[op])
        v = ge.views(ge.arena.w32)
        v["transformer.wte.weight"].copy_(wte)
        v["transformer.ln_f.weight"].copy_(gamma)
        v["transformer.ln_f.bias"].copy_(beta)
        ge.arena.refresh_bf16()
        self.x, self.gamma, self.beta, self.wte, self.tok = x.cuda(), gamma.cuda(), beta.cuda(), wte.cuda(), tok.cuda().contiguous()
        self.Vp = ge.dims["Vp"]
        self.shp = ge.shape(c.B, c.L, self.T, c.cap, c.mode)
        self.ws = ge.workspace(self.shp)
        self.ws.fill_(255)                                   # NaN in every float format: nothing may rely on a zeroed workspace
        self.cfg = ge.cfg
        n = ge.arena.n
        self.g0 = 0.5 + 0.25 * torch.cos(0.37 * torch.arange(n, device="cuda", dtype=torch.float32))
        self.g32 = self.g0.clone()
        self.put()

    def put(self):
        assert _lib().cc_lmhead_put_x(C.byref(self.cfg), C.byref(self.shp), _p(self.ws), _p(self.x), _st()) == 0

    def get(self, field):
        c, Mc = self.c, self.c.B * self.c.cap
        sdt = LM.DT[self.op]
        shape, dt = {LSE: ((Mc,), torch.float32), TGT: ((Mc,), torch.float32), ROW_LOSS: ((Mc,), torch.float32), HF: ((Mc, c.D), sdt),
                     DHF: ((Mc, c.D), sdt), DX32: ((c.B * self.T, c.D), torch.float32)}[field]
        out = torch.empty(shape, dtype=dt, device="cuda")
        rc = _lib().cc_lmhead_get(C.byref(self.cfg), C.byref(self.shp), _p(self.ws), field, _p(out), out.numel() * out.element_size(), _st())
        assert rc == 0, (field, rc)
        return out

    def args(self):
        a = self.ge.arena
        return C.byref(self.cfg), C.byref(self.shp), _p(a.w32), _p(a.w16), _p(self.ws)

    def fwd(self):
        stats = torch.full((2,), float("nan"), device="cuda")
        rc = _lib().cc_lmhead_ce_fwd(*self.args(), _p(self.tok), _p(stats), _st())
        assert rc == 0, rc
        return stats

    def bwd(self, denom):
        d = torch.tensor([denom], dtype=torch.float32, device="cuda")
        ls = None if self.c.ls is None else torch.tensor([self.c.ls], dtype=torch.float32, device="cuda")
        rc = _lib().cc_lmhead_ce_bwd(*self.args(), _p(d), _p(ls), _p(self.g32), _st())
        assert rc == 0, rc

    def score(self):
        c = self.c
        lp = torch.full((c.B, c.cap), float("nan"), device="cuda")
        ss = torch.full((c.B, 2), float("nan"), device="cuda")
        rc = _lib().cc_lmhead_score(*self.args(), _p(self.tok), c.iz, _p(lp), _p(ss), _st())
        assert rc == 0, rc
        return lp, ss


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _ids(op):
    return [c.name for c in LM.cases(op)]


def _case(op, name):
    return {c.name: c for c in LM.cases(op)}[name]


def _run_case(op, c):
    l = _lib()
    rep = Report(f"{op} {c.name}")
    form, entry, fold, dgrad = LM.paths(c, op)
    old = l.cc_gemm_tile_mode(c.tile)
    try:
        P = Pass(op, c)
        denom = LM.denom_of(c, P.tok.cpu())
        T, Mc = P.T, c.B * c.cap
        ln = LM.ln_rows(P.x, P.gamma, P.beta, c.B, T, c.L, c.cap)
        if c.mode == 0:
            lp, ss = P.score()
            lp2, ss2 = P.score()
            lse = P.get(LSE)
            assert torch.equal(_bits(lp), _bits(lp2)) and torch.equal(_bits(ss), _bits(ss2)), f"{rep.case}: two calls differ"
        else:
            stats = P.fwd()
            lse = P.get(LSE)
            P.bwd(denom)
            dhf = P.get(DHF)
            g_once = P.g32.clone()
            stats2 = P.fwd()
            P.g32.copy_(P.g0)
            P.bwd(denom)
            assert torch.equal(_bits(stats), _bits(stats2)) and torch.equal(_bits(lse), _bits(P.get(LSE))) and \
                torch.equal(_bits(dhf), _bits(P.get(DHF))) and torch.equal(_bits(g_once), _bits(P.g32)), f"{rep.case}: two calls differ"
        torch.cuda.synchronize()
        hf = P.get(HF)
        rep.check("ln_fwd", "hf", hf, ln["hf"], LM.ln_bounds(ln, P.gamma, P.beta, op))
        R = LM.chain(hf, P.wte, P.tok, c, op, denom)
        Bd = LM.bounds(R, c, op)
        ok = ~R["beyond"]                                              # rows of the documented envelope: full bounds
        fwd_k = {"exp": "EpiLMHeadExp", "logit": "EpiLMHead", "score": "EpiLMHeadScore"}[form] + f"::{entry} + ce_row_fold({fold})"
        assert torch.isfinite(lse).all(), f"{rep.case}: {fwd_k}: lse not finite"
        rep.check(fwd_k, "lse", lse, R["lse"], Bd["lse"], ok)
        if (~ok).any():
            bad = ~ok
            assert (lse.double()[bad] >= (R["lse_c"] - Bd["lse"])[bad]).all(), f"{rep.case}: {fwd_k}: lse below the clamped sum's"
        rep.check("k_lm_tgt_ref" if form == "exp" else fwd_k, "target logit", P.get(TGT), R["tgt"], Bd["tgt"])
        if c.mode == 0:
            rep.check("k_score_rows", "token_logprob", lp.view(-1), R["tlp"], Bd["tlp"])
            rep.check("k_score_samples", "sample_stats", ss, R["sstats"], Bd["sstats"])
            rc = l.cc_lmhead_get(C.byref(P.cfg), C.byref(P.shp), _p(P.ws), ROW_LOSS, _p(lse), lse.numel() * 4, _st())
            assert rc == STATE, rc
            rep.line()
            return
        rep.check("k_ce_rows", "row_loss", P.get(ROW_LOSS), R["loss"], Bd["loss"], ok)
        assert torch.isfinite(stats).all(), f"{rep.case}: k_ce_stats: stats not finite"
        if ok.all():
            rep.check("k_ce_stats", "stats", stats, R["stats"], Bd["stats"])
        else:
            assert stats[1].item() == R["stats"][1].item()
        dg_k = {"deepk": "gemm_nt_deepk", "fallback": "gemm_bf16out" + (" + lm_dgrad_fix" if form == "exp" else "")}[dgrad]
        assert torch.isfinite(dhf.float()).all(), f"{rep.case}: {dg_k}: dhf not finite"
        rep.check(dg_k, "dhf", dhf, R["dhf"], Bd["dhf"], ok)
        ign = ~R["keep"]
        assert (dhf[ign] == 0).all(), f"{rep.case}: {dg_k}: dhf of an ignored row is not exactly zero"
        # ln_f backward from the device's own dhf
        W = LM.ln_bwd(ln, P.gamma, dhf)
        o = P.ge.offsets
        lw, lb = o[2 + 12], o[3 + 12]
        Bl = LM.ln_bwd_bounds(ln, W, P.gamma, dhf, P.g0[lw:lw + c.D], P.g0[lb:lb + c.D])
        dx = P.get(DX32)
        assert torch.isfinite(dx).all(), f"{rep.case}: ln_bwd: dx32 not finite"
        rows = ln["rows"]
        rep.check("ln_bwd", "dx32 (kept rows)", dx[rows], W["dx"], Bl["dx"])
        other = torch.ones(c.B * T, dtype=torch.bool, device=dx.device)
        other[rows[R["keep"]]] = False
        assert (dx[other] == 0).all(), f"{rep.case}: ln_bwd: dx32 of a row no kept caption row maps to is not exactly zero"
        diff = (P.g32.double() - P.g0.double())
        if c.mode == 1:
            assert torch.equal(_bits(P.g32), _bits(P.g0)), f"{rep.case}: a frozen-LM backward wrote into g32"
        else:
            dw = diff[:P.Vp * c.D].view(P.Vp, c.D)
            assert torch.equal(_bits(P.g32[c.V * c.D:P.Vp * c.D]), _bits(P.g0[c.V * c.D:P.Vp * c.D])), f"{rep.case}: gemm_wgrad: dwte rows >= V written"
            assert torch.isfinite(P.g32).all(), f"{rep.case}: g32 not finite"
            wg_k = "lm_scale_rows + gemm_wgrad + scatter_rows" if form == "exp" else "k_ce_dlogits + gemm_wgrad"
            if ok.all():
                rep.check(wg_k, "dwte", dw, R["dwte"], LM.dwte_bound(R, Bd, P.g0[:P.Vp * c.D].view(P.Vp, c.D)))
            rep.check("ln_bwd", "dgamma", diff[lw:lw + c.D], W["dgamma"], Bl["dgamma"])
            rep.check("ln_bwd", "dbeta", diff[lb:lb + c.D], W["dbeta"], Bl["dbeta"])
            mask = torch.ones_like(P.g0, dtype=torch.bool)
            mask[:P.Vp * c.D] = False
            mask[lw:lw + c.D] = False
            mask[lb:lb + c.D] = False
            assert torch.equal(_bits(P.g32[mask]), _bits(P.g0[mask])), f"{rep.case}: g32 written outside wte / ln_f"
        rep.line()
    finally:
        l.cc_gemm_tile_mode(old)


@pytest.mark.parametrize("name", _ids("bf16"))
def test_bf16(name):
    _run_case("bf16", _case("bf16", name))


@pytest.mark.parametrize("name", _ids("fp16"))
def test_fp16(name):
    _run_case("fp16", _case("fp16", name))


@pytest.mark.parametrize("name", _ids("x3"))
def test_split_bf16(name):
    _run_case("x3", _case("x3", name))


@pytest.mark.parametrize("op", LM.OPS)
def test_refusals_leave_the_outputs_alone(op):
    """the refusals the header documents return their codes before anything is written"""
    l = _lib()
    c = _case(op, LM.cases(op)[0].name)._replace(mode=2)
    P = Pass(op, c)
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    stats, lp, ss = nan(2), nan(c.B, c.cap), nan(c.B, 2)
    a = P.ge.arena

    def shape(**kw):
        d = dict(B=c.B, L=c.L, T=P.T, cap=c.cap, mode=2)
        d.update(kw)
        return P.ge.shape(d["B"], d["L"], d["T"], d["cap"], d["mode"])

    def fwd(s):
        return l.cc_lmhead_ce_fwd(C.byref(P.cfg), C.byref(s), _p(a.w32), _p(a.w16), _p(P.ws), _p(P.tok), _p(stats), _st())
    assert fwd(shape(mode=0)) == ARG
    assert fwd(shape(L=0, T=c.cap)) == ARG
    assert fwd(shape(cap=c.cap + 1)) == SHAPE
    one = torch.ones(1, device="cuda")
    assert l.cc_lmhead_ce_bwd(C.byref(P.cfg), C.byref(P.shp), _p(a.w32), _p(a.w16), _p(P.ws), _p(one), None, None, _st()) == ARG
    assert l.cc_lmhead_score(C.byref(P.cfg), C.byref(P.shp), _p(a.w32), _p(a.w16), _p(P.ws), _p(P.tok), 0, _p(lp), _p(ss), _st()) == ARG
    s0 = shape(mode=0, cap=c.cap + 1)
    assert l.cc_lmhead_score(C.byref(P.cfg), C.byref(s0), _p(a.w32), _p(a.w16), _p(P.ws), _p(P.tok), 0, _p(lp), _p(ss), _st()) == SHAPE
    buf = torch.empty(c.B * c.cap + 1, device="cuda")
    assert l.cc_lmhead_get(C.byref(P.cfg), C.byref(P.shp), _p(P.ws), LSE, _p(buf), buf.numel() * 4, _st()) == SHAPE
    assert l.cc_lmhead_get(C.byref(P.cfg), C.byref(P.shp), _p(P.ws), 6, _p(buf), 4, _st()) == ARG
    assert l.cc_lmhead_get(C.byref(P.cfg), C.byref(P.shp), _p(P.ws), LSE, None, 4, _st()) == ARG
    assert l.cc_lmhead_put_x(C.byref(P.cfg), C.byref(P.shp), _p(P.ws), None, _st()) == ARG
    torch.cuda.synchronize()
    assert torch.isnan(stats).all() and torch.isnan(lp).all() and torch.isnan(ss).all()
    assert torch.equal(_bits(P.g32), _bits(P.g0))


def test_measured_allowances():
    """prints the raw figures behind lm_ref.EXP2_POS_ULPS and LOGF_ULPS (run with -s) and checks that the recorded allowances cover them.
    ln_f weights gamma = 0, beta = (8, 0, ...): hf = (8, 0, ...) exactly, so logit v = 8 wte[v, 0] with no rounding anywhere before the
    device functions."""
    l = _lib()
    V, D = 97, 64
    gamma, beta = torch.zeros(D), torch.zeros(D)
    beta[0] = 8.0
    x = torch.randn(2, D)
    tok = torch.tensor([[1]])
    worst = {"exp2_pos": 0.0, "logf": 0.0}
    old = l.cc_gemm_tile_mode(-1)
    try:
        # exp2 at positive arguments (bf16 build, exponential form): cref = 0, one column at y, the rest 200 below
        P = Pass("bf16", LM.Case("measure", "flat", V, D, 1, 1, 1, 1, -1, "kept", None, 0), (x, gamma, beta, torch.zeros(V, D), tok))
        wv = P.ge.views(P.ge.arena.w32)["transformer.wte.weight"]
        for k in range(1, 161):
            y = 0.5 * k
            w = torch.full((V,), -25.0)
            w[1], w[2] = 0.0, y / 8.0
            wv[:, 0].copy_(w)
            P.ge.arena.refresh_bf16()
            P.fwd()
            lse = P.get(LSE).double().item()
            ref = torch.log1p(torch.exp(torch.tensor(y, dtype=torch.float64))).item()
            worst["exp2_pos"] = max(worst["exp2_pos"], abs(lse - ref) / (G.U32 * (1.0 + y)))
        # logf (scoring pass): k equal columns, the rest 200 below
        P = Pass("bf16", LM.Case("measure", "flat", V, D, 1, 1, 1, 0, -1, "kept", None, 0), (x, gamma, beta, torch.zeros(V, D), tok))
        wv = P.ge.views(P.ge.arena.w32)["transformer.wte.weight"]
        for k in range(1, V + 1):
            w = torch.full((V,), -25.0)
            w[:k] = 0.0
            wv[:, 0].copy_(w)
            P.ge.arena.refresh_bf16()
            P.score()
            lse = P.get(LSE).double().item()
            worst["logf"] = max(worst["logf"], abs(lse - math.log(k)) / (G.U32 * max(1.0, math.log(k))))
    finally:
        l.cc_gemm_tile_mode(old)
    print(f"MEASURED exp2 at positive arguments (with logf): worst |lse - y'| / (u32 (1 + y)) = {worst['exp2_pos']:.4f}; allowance {LM.EXP2_POS_ULPS}")
    print(f"MEASURED logf: worst |lse - log k| / (u32 max(1, log k)) = {worst['logf']:.4f}; allowance {LM.LOGF_ULPS}")
    assert LM.EXP2_POS_ULPS is not None and LM.LOGF_ULPS is not None, "write the figures above into tests/lm_ref.py"
    assert worst["exp2_pos"] <= LM.EXP2_POS_ULPS and worst["logf"] <= LM.LOGF_ULPS
