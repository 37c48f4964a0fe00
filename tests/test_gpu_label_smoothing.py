"""Label smoothing in the fused lm_head loss (cc_lmhead_ce_fwd_smooth, cc_lmhead_ce_bwd_smooth; clipcap_amd/csrc/smooth.hip) against the
float64 statement of tests/lm_smooth_ref.py, per operand build, in modes 1 and 2.  The same pass runs with and without smoothing on a
residual stream the test puts into the workspace (cc_lmhead_put_x / cc_lmhead_get, as tests/test_gpu_lm_head.py does): the DIFFERENCES
DHF(eps) - DHF(0) and g32(eps) - g32(0) are held to the statement's corrections within its derived bounds, which keeps the GEMMs' own
error out.  Nothing here is tuned to what the kernels return.

Shapes, the smallest at which each new kernel can go wrong (V, D, B x cap, L):
  97, 64, 5x1, 1        the smallest shape: one slice everywhere
  130, 96, 15x9, 4      Vp = 256 with 126 pad rows, which the test fills with non-zero values; D % 64 != 0
  4099, 256, 130x1, 1   loss scale 1024; the column mean over 33 slices
  65601, 64, 2x3, 1     the column mean over 256 slices of several row rounds
  130, 256, 257x9, 4    2313 rows: the row sum over 37 slices, the stats sum over three rounds of its block
  97, 1600, 3x2, 1      the widest row, if the plain chain takes that width (else the new entry points must refuse as it does)
Every case has ignored rows (target 0), -1 pads and repeated targets."""
import ctypes as C

import pytest
import torch

from tests import lm_ref as LM
from tests import lm_smooth_ref as SM
from tests.test_gpu_lm_head import DHF, DX32, HF, TGT, Pass, Report, _bits, _lib, _p, _st

pytestmark = pytest.mark.gpu
ARG = -1
# V D B cap L loss_scale
SHAPES = ((97, 64, 5, 1, 1, None), (130, 96, 15, 9, 4, None), (4099, 256, 130, 1, 1, 1024.0), (65601, 64, 2, 3, 1, None),
          (130, 256, 257, 9, 4, None), (97, 1600, 3, 2, 1, None))


def _case(V, D, B, cap, L, ls, mode):
    return LM.Case(f"V{V}-D{D}-B{B}x{cap}-L{L}-m{mode}", "flat", V, D, B, cap, L, mode, -1, "kept", ls, 0)


def _tokens(c):
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


_INPUTS = {}


def _inputs(c, op):
    """computed once per (shape, build) and shared, unchanged, by every test that needs them"""
    key = (op, c.V, c.D, c.B, c.cap, c.L)
    if key not in _INPUTS:
        x, gamma, beta, wte, _ = LM.make_inputs(c, op)
        tok = _tokens(c)
        flat = tok.reshape(-1)
        assert (flat == 0).any() and (flat == -1).any() and len(flat[flat > 0].unique()) < int((flat > 0).sum())
        _INPUTS[key] = (x, gamma, beta, wte, tok)
    return _INPUTS[key]


class SmoothPass(Pass):
    """Pass of tests/test_gpu_lm_head.py + the pad rows of wte filled, the caller's scratch, and the smoothed entry points"""

    def __init__(self, op, c, inputs):
        super().__init__(op, c, inputs)
        ge = self.ge
        pad = ge.arena.w32[c.V * c.D:self.Vp * c.D]
        pad.copy_(0.5 + 0.25 * torch.sin(0.61 * torch.arange(pad.numel(), device="cuda", dtype=torch.float32)))
        ge.arena.refresh_bf16()
        n = _lib().cc_lmhead_smooth_scratch_floats(C.byref(self.cfg), C.byref(self.shp))
        assert n > 0, n
        self.scratch = torch.full((n,), float("nan"), device="cuda")
        self.ls = None if c.ls is None else torch.tensor([c.ls], dtype=torch.float32, device="cuda")

    def fwd_s(self, eps, stats3=None, scratch="own"):
        stats3 = torch.full((3,), float("nan"), device="cuda") if stats3 is None else stats3
        sc = self.scratch if isinstance(scratch, str) else scratch
        rc = _lib().cc_lmhead_ce_fwd_smooth(*self.args(), _p(self.tok), eps, _p(sc), _p(stats3), _st())
        return rc, stats3

    def bwd_s(self, eps, denom, scratch="own"):
        d = torch.tensor([denom], dtype=torch.float32, device="cuda")
        sc = self.scratch if isinstance(scratch, str) else scratch
        return _lib().cc_lmhead_ce_bwd_smooth(*self.args(), _p(d), _p(self.ls), eps, _p(sc), _p(self.g32), _st())

    def state(self):
        return self.get(DHF), self.get(DX32), self.g32.clone()


def _run(op, c, eps):
    rep = Report(f"{op} {c.name} eps {eps}")
    inputs = _inputs(c, op)
    P = SmoothPass(op, c, inputs)
    denom = LM.denom_of(c, P.tok.cpu())
    T, V, D, Vp = P.T, c.V, c.D, P.Vp
    stats_nan = torch.full((2,), float("nan"), device="cuda")
    rc = _lib().cc_lmhead_ce_fwd(*P.args(), _p(P.tok), _p(stats_nan), _st())
    if rc != 0:      # the plain chain does not take this width at this vocabulary: the new entry points refuse the same way, nothing written
        rc2, s3 = P.fwd_s(eps)
        torch.cuda.synchronize()
        assert rc2 == rc and torch.isnan(s3).all(), (rc, rc2)
        print(f"REFUSED {rep.case}: the plain chain returns {rc}; so does the smoothed one")
        return
    # the plain chain
    stats = P.fwd()
    P.bwd(denom)
    dhf0, dx0, g_plain = P.state()
    tgt, hf = P.get(TGT), P.get(HF)
    # eps = 0 through the new entry points: every output bit-equal to the plain ones
    P.g32.copy_(P.g0)
    rc, s3 = P.fwd_s(0.0)
    assert rc == 0 and P.bwd_s(0.0, denom) == 0
    a, b, g = P.state()
    assert torch.equal(_bits(s3[:2]), _bits(stats)) and torch.equal(_bits(s3[2:]), _bits(stats[:1])), f"{rep.case}: eps = 0: stats3"
    assert torch.equal(_bits(a), _bits(dhf0)) and torch.equal(_bits(b), _bits(dx0)) and torch.equal(_bits(g), _bits(g_plain)), f"{rep.case}: eps = 0 differs"
    assert torch.isnan(P.scratch).all(), f"{rep.case}: eps = 0 wrote the scratch"
    # eps
    P.g32.copy_(P.g0)
    rc, s3 = P.fwd_s(eps)
    assert rc == 0 and P.bwd_s(eps, denom) == 0
    dhf1, dx1, g1 = P.state()
    torch.cuda.synchronize()
    S = SM.statement(hf, P.wte, P.tok, c, op, denom, eps, tgt=tgt, nll=stats[0].double())
    Bd = SM.bounds(S, c, op, dhf0, g0=g_plain[:Vp * D].view(Vp, D) if c.mode == 2 else None)
    assert torch.equal(_bits(s3[1:2]), _bits(stats[1:2])) and torch.equal(_bits(s3[2:]), _bits(stats[:1])), f"{rep.case}: stats3[1], [2] are not the plain chain's bits"
    rep.check("k_smooth_rows + k_smooth_stats", "stats3", s3, S["stats3"], Bd["stats3"])
    rep.check("k_smooth_dhf", "DHF(eps) - DHF(0)", dhf1.double() - dhf0.double(), S["d_dhf"], Bd["d_dhf"])
    assert (dhf1[~S["keep"]] == 0).all(), f"{rep.case}: k_smooth_dhf: dhf of an ignored row is not exactly zero"
    # ln_f backward from the device's own dhf, as tests/test_gpu_lm_head.py checks the plain chain
    ln = LM.ln_rows(P.x, P.gamma, P.beta, c.B, T, c.L, c.cap)
    W = LM.ln_bwd(ln, P.gamma, dhf1)
    o = P.ge.offsets
    lw, lb = o[2 + 12], o[3 + 12]
    Bl = LM.ln_bwd_bounds(ln, W, P.gamma, dhf1, P.g0[lw:lw + D], P.g0[lb:lb + D])
    assert torch.isfinite(dx1).all()
    rows = ln["rows"]
    rep.check("ln_bwd", "dx32 (kept rows)", dx1[rows], W["dx"], Bl["dx"])
    other = torch.ones(c.B * T, dtype=torch.bool, device="cuda")
    other[rows[S["keep"]]] = False
    assert (dx1[other] == 0).all(), f"{rep.case}: ln_bwd: dx32 of a row no kept caption row maps to is not exactly zero"
    if c.mode == 1:
        assert torch.equal(_bits(g1), _bits(P.g0)), f"{rep.case}: a frozen-LM backward wrote into g32"
    else:
        assert torch.isfinite(g1).all()
        assert torch.equal(_bits(g1[V * D:Vp * D]), _bits(P.g0[V * D:Vp * D])), f"{rep.case}: dwte rows >= V written"
        dd = (g1.double() - g_plain.double())[:Vp * D].view(Vp, D)
        rep.check("scatter_rows + smooth_dwte_bcast", "g32(eps) - g32(0)", dd, S["d_dwte"], Bd["d_dwte"])
        diff = g1.double() - P.g0.double()
        rep.check("ln_bwd", "dgamma", diff[lw:lw + D], W["dgamma"], Bl["dgamma"])
        rep.check("ln_bwd", "dbeta", diff[lb:lb + D], W["dbeta"], Bl["dbeta"])
        mask = torch.ones_like(P.g0, dtype=torch.bool)
        mask[:Vp * D] = False
        mask[lw:lw + D] = False
        mask[lb:lb + D] = False
        assert torch.equal(_bits(g1[mask]), _bits(P.g0[mask])), f"{rep.case}: g32 written outside wte / ln_f"
        # the same step again: bit for bit the same gradients (fixed-order sums, no atomics)
        P.g32.copy_(P.g0)
        rc, s3b = P.fwd_s(eps)
        assert rc == 0 and P.bwd_s(eps, denom) == 0
        assert torch.equal(_bits(s3b), _bits(s3)) and torch.equal(_bits(P.g32), _bits(g1)) and torch.equal(_bits(P.get(DHF)), _bits(dhf1)), \
            f"{rep.case}: two runs differ"
    rep.line()


_IDS = [f"V{s[0]}-D{s[1]}-B{s[2]}x{s[3]}" for s in SHAPES]


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=_IDS)
@pytest.mark.parametrize("op", LM.OPS)
def test_smoothing_corrections(op, shape, mode):
    _run(op, _case(*shape, mode), 0.1)


@pytest.mark.parametrize("op", LM.OPS)
def test_half_smoothing(op):
    _run(op, _case(*SHAPES[1], 2), 0.5)


@pytest.mark.parametrize("op", LM.OPS)
def test_refusals_leave_the_outputs_alone(op):
    c = _case(*SHAPES[0], 2)
    P = SmoothPass(op, c, _inputs(c, op))
    P.fwd()
    nan3 = torch.full((3,), float("nan"), device="cuda")
    for eps in (-0.1, 1.0, float("nan")):
        assert P.fwd_s(eps, nan3)[0] == ARG and P.bwd_s(eps, 3.0) == ARG
    assert P.fwd_s(0.1, nan3, scratch=None)[0] == ARG and P.bwd_s(0.1, 3.0, scratch=None) == ARG
    s0 = P.ge.shape(c.B, c.L, P.T, c.cap, 0)
    a = P.ge.arena
    l = _lib()
    assert l.cc_lmhead_ce_fwd_smooth(C.byref(P.cfg), C.byref(s0), _p(a.w32), _p(a.w16), _p(P.ws), _p(P.tok), 0.1, _p(P.scratch), _p(nan3), _st()) == ARG
    one = torch.ones(1, device="cuda")
    assert l.cc_lmhead_ce_bwd_smooth(C.byref(P.cfg), C.byref(s0), _p(a.w32), _p(a.w16), _p(P.ws), _p(one), None, 0.1, _p(P.scratch), _p(P.g32), _st()) == ARG
    assert l.cc_lmhead_ce_bwd_smooth(C.byref(P.cfg), C.byref(P.shp), _p(a.w32), _p(a.w16), _p(P.ws), _p(one), None, 0.1, _p(P.scratch), None, _st()) == ARG
    torch.cuda.synchronize()
    assert torch.isnan(nan3).all() and torch.isnan(P.scratch).all() and torch.equal(_bits(P.g32), _bits(P.g0))


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("op", LM.OPS)
def test_all_ignored_batch(op, mode):
    """a batch without a kept row: the divisor is clamped to 1 and every row's weight is 0, as lm_ref states the plain chain — the smoothed
    step equals the plain one bit for bit, the loss sums are 0, nothing is NaN"""
    c = _case(*SHAPES[1], mode)
    x, gamma, beta, wte, tok = _inputs(c, op)
    tok = tok.clone()
    tok[:] = -1
    tok[0, 0] = 0
    P = SmoothPass(op, c, (x, gamma, beta, wte, tok))
    stats = P.fwd()
    P.bwd(0.0)
    dhf0, dx0, g_plain = P.state()
    P.g32.copy_(P.g0)
    rc, s3 = P.fwd_s(0.1)
    assert rc == 0 and P.bwd_s(0.1, 0.0) == 0
    dhf1, dx1, g1 = P.state()
    torch.cuda.synchronize()
    assert (s3 == 0).all() and (stats == 0).all()
    assert (dhf1 == 0).all() and (dx1 == 0).all() and torch.isfinite(g1).all()
    assert torch.equal(_bits(dhf1), _bits(dhf0)) and torch.equal(_bits(dx1), _bits(dx0)) and torch.equal(_bits(g1), _bits(g_plain))
    S = SM.statement(P.get(HF), wte.cuda(), tok.cuda(), c, op, 0.0, 0.1, tgt=P.get(TGT), nll=stats[0].double())
    assert (S["stats3"] == 0).all() and (S["d_dhf"] == 0).all()


def test_engine_step_returns_the_smoothed_loss_and_keeps_the_plain_nll():
    """ClipCapEngine.forward_backward(label_smoothing=): the returned loss is stats3[0] / kept, last_nll the plain mean — equal, to the bit, to
    the loss the same engine returns without smoothing; 0.0 leaves the 2-float stats path untouched"""
    from clipcap_amd.engine import ClipCapEngine, Gpt2Engine, MapperEngine
    torch.manual_seed(0)
    E, D, P_, L, H, N, V, B, cap = 64, 128, 4, 4, 4, 1, 300, 4, 8
    me = MapperEngine(E, D, L, P_, H, N, device="cuda")
    ge = Gpt2Engine(D, 4, 1, V, 32, device="cuda")
    for eng in (me, ge):
        for k, v in eng.views(eng.arena.w32).items():
            v.copy_(torch.randn(v.shape) * 0.05 + (1.0 if k.endswith("weight") and ("ln_" in k or "norm" in k) else 0.0))
    tokens = torch.randint(1, V, (B, cap))
    tokens[0, 6:] = -1
    embeds = torch.randn(B, E)
    for train_lm in (False, True):
        eng = ClipCapEngine(me, ge, train_lm=train_lm)
        eng.zero_grad()
        plain = eng.forward_backward(tokens.cuda(), embeds.cuda()).clone()
        assert eng.stats3 is None and torch.equal(eng.last_nll, plain)
        eng.zero_grad()
        loss = eng.forward_backward(tokens.cuda(), embeds.cuda(), label_smoothing=0.1).clone()
        torch.cuda.synchronize()
        assert torch.equal(_bits(eng.last_nll.reshape(1)), _bits(plain.reshape(1)))
        s3 = eng.stats3
        assert torch.equal(loss, s3[0] / s3[1]) and s3[1].item() == float((tokens > 0).sum())
        assert torch.isfinite(loss) and loss.item() != plain.item()


# ---- the whole training step ---------------------------------------------------------------------------------------------------------
# bounds of the unsmoothed step in each build: the loss against the oracle at the build's rounding points 2e-3 (16-bit operands) / 5e-5
# (split-bf16, fp32 oracle), every gradient tensor in relative L2 3e-2 (tests/test_gpu_model.py's bound of a gradient against the oracle at
# equal rounding points) / 2e-3 (split-bf16: tests/test_gpu_edges.py)
STEP_TOL = {None: (2e-3, 3e-2), 16: (2e-3, 3e-2), 32: (5e-5, 2e-3)}
RB = {None: True, 16: "fp16", 32: "bf16x3"}


def _golden_engine(mode, precision):
    from clipcap_amd.engine import ClipCapEngine, Gpt2Engine, MapperEngine
    from tests.util import load_golden, sd_of
    g = load_golden(f"train_{mode}")
    E, D, P_, L, H, N, n_head, n_layer, V, npos = [int(v) for v in g["cfg"]]
    sd = {k: v for k, v in sd_of(g).items() if "lm_head" not in k}
    me = MapperEngine(E, D, L, P_, H, N, device="cuda", precision=precision)
    ge = Gpt2Engine(D, n_head, n_layer, V, npos, device="cuda", precision=precision)
    for k, v in me.views(me.arena.w32).items():
        v.copy_(sd["transformer_mapper." + k])
    for k, v in ge.views(ge.arena.w32).items():
        v.copy_(sd["language_model." + k])
    cfg = dict(projection_length=P_, prefix_length=L, heads=H, layers=N, n_head=n_head, n_layer=n_layer)
    tokens, embeds = torch.from_numpy(g["in.tokens"]), torch.from_numpy(g["in.embeds"])
    return ClipCapEngine(me, ge, train_lm=(mode == "full")), sd, cfg, tokens, embeds, V


def _oracle_step(sd, cfg, tokens, embeds, rb, train, eps):
    """float64 autograd of the oracle's forward (the build's rounding points) with F.cross_entropy(..., label_smoothing=eps)"""
    import torch.nn.functional as F
    from oracle import clipcap_oracle as O
    sdr = {k: (v.double().requires_grad_(True) if k in train else v.double()) for k, v in sd.items()}
    tok = tokens.clamp_min(0)
    logits = O.clipcap_logits(sdr, tok, embeds.double(), cfg=cfg, rb=rb)
    lg = logits[:, cfg["prefix_length"] - 1:-1]
    loss = F.cross_entropy(lg.reshape(-1, lg.shape[-1]), tok.flatten(), ignore_index=0, label_smoothing=eps)
    loss.backward()
    return loss.detach(), {k: sdr[k].grad for k in train}


@pytest.mark.parametrize("precision", [None, 16, 32])
@pytest.mark.parametrize("mode", ["prefix_only", "full"])
def test_one_optimizer_step_on_the_goldens(mode, precision):
    """loss and every gradient tensor of a step with eps = 0.1 against the oracle with the smoothed loss, at the bounds of the unsmoothed
    step; eps = 0 runs beside it and both figures are printed (-s).  Then the optimizer step itself: finite, and it moves the weights."""
    eng, sd, cfg, tokens, embeds, V = _golden_engine(mode, precision)
    train = [k for k in sd if mode == "full" or k.startswith("transformer_mapper.")]
    tol_loss, tol_grad = STEP_TOL[precision]
    figs = {}
    for eps in (0.0, 0.1):
        eng.zero_grad()
        loss = float(eng.forward_backward(tokens.cuda(), embeds.cuda(), label_smoothing=eps))
        ref, grads = _oracle_step(sd, cfg, tokens, embeds, RB[precision], train, SM.eps32(eps))
        unscale = 1.0 / float(eng.scaler.scale) if eng.scaler is not None else 1.0
        gm, gg = eng.mapper.views(eng.mapper.arena.g32), eng.gpt2.views(eng.gpt2.arena.g32) if mode == "full" else {}
        worst = ("", 0.0)
        for k in train:
            mine = gm[k[len("transformer_mapper."):]] if k.startswith("transformer_mapper.") else gg[k[len("language_model."):]]
            mine = mine.double().cpu() * unscale
            if k.endswith("wte.weight"):
                mine = mine[:V]
            r = ((mine - grads[k]).norm() / grads[k].norm().clamp_min(1e-12)).item()
            worst = max(worst, (k, r), key=lambda t: t[1])
        figs[eps] = (abs(loss - float(ref)), worst)
        print(f"STEP {mode} precision {precision} eps {eps}: |loss - oracle| {figs[eps][0]:.3e} (loss {loss:.6f}); worst gradient rel. L2 "
              f"{worst[1]:.3e} ({worst[0]}); bounds {tol_loss:g} / {tol_grad:g}")
    assert figs[0.1][0] <= tol_loss and figs[0.1][1][1] <= tol_grad, figs
    nll = float(eng.last_nll)
    eng.zero_grad()
    assert nll == float(eng.forward_backward(tokens.cuda(), embeds.cuda(), backward=False))
    eng.zero_grad()
    eng.forward_backward(tokens.cuda(), embeds.cuda(), label_smoothing=0.1)
    before = [a.w32.clone() for a in eng.arenas()]
    eng.optimizer_step(1e-3, 1, weight_decay=0.01)
    torch.cuda.synchronize()
    for a, w in zip(eng.arenas(), before):
        assert torch.isfinite(a.w32).all() and not torch.equal(a.w32, w)


def _ddp_worker(rank, world, port, mode, out):
    import os
    import numpy as np
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from clipcap_amd.train.ddp import GradReducer, shard_batch
    from tests.test_gpu_ddp import _build
    eng, tokens, embeds = _build(mode)
    arenas = eng.arenas()
    red = GradReducer([a.grads() for a in arenas])
    tk, em = shard_batch(tokens, embeds, rank, world)
    red.begin()
    loss = eng.forward_backward(tk.cuda(), em.cuda(), reduce_stats=red.reduce_stats, on_grads_ready=red.on_grads_ready, label_smoothing=0.1)
    red.finish()
    torch.cuda.synchronize()
    if rank == 0:
        np.savez(out, loss=float(loss), nll=float(eng.last_nll), **{f"g{i}": a.g32.cpu().numpy() for i, a in enumerate(arenas)})
    dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["prefix_only", "full"])
def test_two_rank_smoothed_step_equals_single_process(tmp_path, mode):
    """two ranks with half the batch each (sharing the box's GPU over gloo, as tests/test_gpu_ddp.py does) against one rank with the whole
    batch: reduce_stats sums the 3-float stats, so loss, nll and gradients agree at that test's bounds"""
    import numpy as np
    import torch.multiprocessing as mp
    from tests.test_ddp_gloo import _free_port
    from tests.test_gpu_ddp import _build
    out = str(tmp_path / "ddp.npz")
    mp.spawn(_ddp_worker, args=(2, _free_port(), mode, out), nprocs=2, join=True)
    res = np.load(out)
    eng, tokens, embeds = _build(mode)
    loss = eng.forward_backward(tokens.cuda(), embeds.cuda(), label_smoothing=0.1)
    torch.cuda.synchronize()
    assert abs(float(loss) - float(res["loss"])) <= 1e-5 and abs(float(eng.last_nll) - float(res["nll"])) <= 1e-5
    assert float(loss) != float(eng.last_nll)
    for i, a in enumerate(eng.arenas()):
        ref = a.g32.cpu().numpy()
        rel = np.linalg.norm(res[f"g{i}"] - ref) / np.linalg.norm(ref)
        assert rel <= 2e-2, (i, rel)
