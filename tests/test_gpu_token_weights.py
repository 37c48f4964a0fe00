"""Per-token loss weights in the fused lm_head loss (cc_lmhead_ce_fwd_w, cc_lmhead_ce_bwd_w; the <true> forms of k_ce_stats, k_ce_dlogits,
k_lm_rowfac, k_smooth_rows, k_smooth_stats, k_smooth_coef) per operand build, in modes 1 and 2, with eps 0 and 0.1, on a residual stream
the test puts into the workspace (cc_lmhead_put_x / cc_lmhead_get, as tests/test_gpu_lm_head.py does); then the engine's
forward_backward(token_weights=) on the golden models against the oracle, a two-rank step, and the self-critical step.

Properties (one pass per case and weight set, all on the same inputs):
  1  every weight 1.0 (NaN / inf on the rows that are not kept): stats3, DHF, dx32 and g32 bit-equal to the plain pair (eps 0) or to the
     smoothing pair (eps > 0).
  2  weights +-2^k, k = -2 .. 3, and 0: bf16 and split-bf16: every row of DHF(w) equals w[m] times the row of DHF(1) exactly (compared as
     values, so that -0 == 0 where w is 0 or negative); fp16, whose gradients can be subnormal: held to the float64 statement's bound
     like 3.
  3  general weights (mixed sign, three decades): stats3, DHF, the wte rows of g32 and the ln_f gradients against the float64 statement
     of tests/lm_weight_ref.py evaluated from the pass's own hf / lse / target logit, within its derived bounds.
Shapes (V, D, B x cap, L): tests/lm_weight_ref.py SHAPES, those of tests/test_gpu_label_smoothing.py that exercise these kernels.  Every
case has ignored rows, -1 pads, a repeated target, a kept row of weight 0, a negative weight, and NaN on an ignored row and on a pad."""
import ctypes as C

import pytest
import torch

from tests import lm_ref as LM
from tests import lm_smooth_ref as SM
from tests import lm_weight_ref as WR
from tests.test_gpu_label_smoothing import RB, STEP_TOL, SmoothPass, _golden_engine, _inputs
from tests.test_gpu_lm_head import HF, LSE, TGT, Report, _bits, _lib, _p, _st

pytestmark = pytest.mark.gpu
ARG = -1


class WeightPass(SmoothPass):
    """SmoothPass + the weighted entry points"""

    def fwd_w(self, w, eps, stats3=None, scratch="own"):
        stats3 = torch.full((3,), float("nan"), device="cuda") if stats3 is None else stats3
        sc = self.scratch if isinstance(scratch, str) else scratch
        rc = _lib().cc_lmhead_ce_fwd_w(*self.args(), _p(self.tok), _p(w), eps, _p(sc), _p(stats3), _st())
        return rc, stats3

    def bwd_w(self, w, eps, denom, scratch="own", g32="own"):
        d = torch.tensor([denom], dtype=torch.float32, device="cuda")
        sc = self.scratch if isinstance(scratch, str) else scratch
        g = self.g32 if isinstance(g32, str) else g32
        return _lib().cc_lmhead_ce_bwd_w(*self.args(), _p(d), _p(self.ls), _p(w), eps, _p(sc), _p(g), _st())

    def step_w(self, w, eps, denom):
        """g32 back to its pre-fill, a weighted forward + backward; (stats3, DHF, dx32, g32)"""
        self.g32.copy_(self.g0)
        rc, s3 = self.fwd_w(w, eps)
        assert rc == 0 and self.bwd_w(w, eps, denom) == 0, rc
        return (s3,) + self.state()


def _weights(tok, kind):
    return WR.make_weights(tok.cpu(), kind).cuda().contiguous()


def _against_statement(rep, P, c, op, eps, denom, w, got, what):
    s3, dhf, dx, g = got
    T, V, D, Vp = P.T, c.V, c.D, P.Vp
    W, R, S = WR.statement(P.get(HF), P.wte, P.tok, w, c, op, denom, eps, lse=P.get(LSE), tgt=P.get(TGT))
    pre = P.g0[:Vp * D].view(Vp, D) if c.mode == 2 else None
    Bd = WR.bounds(W, R, S, c, op, pre=pre, own_rows=True)
    rep.check("k_ce_stats<w> (+ k_smooth_rows<w>, k_smooth_stats<w>)", f"stats3 [{what}]", s3, W["stats3"], Bd["stats3"])
    rep.check("k_ce_dlogits<w> / k_lm_rowfac<w> (+ k_smooth_coef<w>) -> dgrad", f"DHF [{what}]", dhf, W["dhf"], Bd["dhf"])
    # ln_f backward from the device's own dhf, as tests/test_gpu_lm_head.py checks the plain chain
    ln = LM.ln_rows(P.x, P.gamma, P.beta, c.B, T, c.L, c.cap)
    Wl = LM.ln_bwd(ln, P.gamma, dhf)
    o = P.ge.offsets
    lw, lb = o[2 + 12], o[3 + 12]
    Bl = LM.ln_bwd_bounds(ln, Wl, P.gamma, dhf, P.g0[lw:lw + D], P.g0[lb:lb + D])
    assert torch.isfinite(dx).all(), f"{rep.case}: dx32 not finite [{what}]"
    rep.check("ln_bwd", f"dx32 (kept rows) [{what}]", dx[ln["rows"]], Wl["dx"], Bl["dx"])
    if c.mode == 1:
        assert torch.equal(_bits(g), _bits(P.g0)), f"{rep.case}: a frozen-LM backward wrote into g32 [{what}]"
        return
    assert torch.isfinite(g).all(), f"{rep.case}: g32 not finite [{what}]"
    assert torch.equal(_bits(g[V * D:Vp * D]), _bits(P.g0[V * D:Vp * D])), f"{rep.case}: dwte rows >= V written [{what}]"
    diff = g.double() - P.g0.double()
    rep.check("gemm_wgrad / scatter_rows (+ smooth_dwte_bcast)", f"g32 wte rows [{what}]", diff[:Vp * D].view(Vp, D), W["dwte"], Bd["dwte"])
    rep.check("ln_bwd", f"dgamma [{what}]", diff[lw:lw + D], Wl["dgamma"], Bl["dgamma"])
    rep.check("ln_bwd", f"dbeta [{what}]", diff[lb:lb + D], Wl["dbeta"], Bl["dbeta"])


def _reference_pass(op, c, eps):
    """the pass without weights on the case's inputs: (P, denom, kept rows, stats3, DHF, dx32, g32) of the plain pair (eps 0) or the smoothing pair"""
    P = WeightPass(op, c, _inputs(c, op))
    denom = LM.denom_of(c, P.tok.cpu())
    if eps == 0.0:
        stats = P.fwd()
        P.bwd(denom)
        s3_ref = torch.stack([stats[0], stats[1], stats[0]])
    else:
        rc, s3_ref = P.fwd_s(eps)
        assert rc == 0 and P.bwd_s(eps, denom) == 0
    return (P, denom, P.tok.reshape(-1) > 0, s3_ref) + P.state()


def _common(rep, got, keep, s3_ref):
    assert torch.isfinite(got[0]).all() and torch.equal(_bits(got[0][1:]), _bits(s3_ref[1:])), f"{rep.case}: stats3[1], [2] are not the unweighted pass's bits"
    assert (got[1][~keep] == 0).all(), f"{rep.case}: DHF of a row that is not kept is not exactly zero"
    assert torch.isfinite(got[2]).all() and torch.isfinite(got[3]).all(), f"{rep.case}: dx32 / g32 not finite"


_IDS = [f"V{s[0]}-D{s[1]}-B{s[2]}x{s[3]}" for s in WR.SHAPES]
_cases = pytest.mark.parametrize("op,shape,mode,eps", [(op, sh, m, e) for op in LM.OPS for sh in WR.SHAPES for m in (1, 2) for e in (0.0, 0.1)],
                                 ids=[f"{op}-{i}-m{m}-eps{e}" for op in LM.OPS for i in _IDS for m in (1, 2) for e in (0.0, 0.1)])


@_cases
def test_unit_weights_are_the_unweighted_pass(op, shape, mode, eps):
    """property 1: every weight 1.0, NaN / inf on the rows that are not kept"""
    c = WR.case(*shape, mode)
    rep = Report(f"{op} {c.name} eps {eps}")
    P, denom, keep, s3_ref, dhf1, dx1, g1 = _reference_pass(op, c, eps)
    s3, dhf, dx, g = P.step_w(_weights(P.tok, "ones"), eps, denom)
    assert torch.equal(_bits(s3), _bits(s3_ref)), f"{rep.case}: unit weights: stats3 {s3.tolist()} against {s3_ref.tolist()}"
    assert torch.equal(_bits(dhf), _bits(dhf1)) and torch.equal(_bits(dx), _bits(dx1)) and torch.equal(_bits(g), _bits(g1)), \
        f"{rep.case}: unit weights differ from the pass without weights"
    if eps == 0.0:
        assert torch.isnan(P.scratch).all(), f"{rep.case}: eps = 0 wrote the scratch"


@_cases
def test_power_of_two_weights(op, shape, mode, eps):
    """property 2.  In the logit form (fp16; split-bf16 mode 2) the weight's magnitude goes into d logits and its sign onto the rows of
    d hf after the GEMM (k_lm_rowsign): the matrix cores' accumulation is not symmetric under negation of an operand (cc_lmhead_ce_bwd
    with loss scale -4 against +4 differs in the split-bf16 logit form), so a signed operand could not give the negated row exactly."""
    c = WR.case(*shape, mode)
    rep = Report(f"{op} {c.name} eps {eps}")
    P, denom, keep, s3_ref, dhf1, dx1, g1 = _reference_pass(op, c, eps)
    w2 = _weights(P.tok, "pow2")
    got = P.step_w(w2, eps, denom)
    _common(rep, got, keep, s3_ref)
    if op == "fp16":
        _against_statement(rep, P, c, op, eps, denom, w2, got, "2^k")
        rep.line()
        return
    wk = torch.where(keep, w2.reshape(-1), torch.zeros_like(w2.reshape(-1)))
    want = wk.unsqueeze(1) * dhf1.float()
    bad = (got[1].float() != want).any(1)
    if bad.any():      # the figures, before the assertion
        d = (got[1].float() - want)[bad].abs()
        ulp = torch.finfo(dhf1.dtype).eps * want[bad].abs().clamp_min(1e-30)
        print(f"POW2 {rep.case}: {int(bad.sum())} of {int(keep.sum())} kept rows differ, {int((d != 0).sum())} elements, largest difference "
              f"{float((d / ulp).max()):.3g} ulp of the stored type; weights of those rows {sorted(set(wk[bad].tolist()))}")
    assert not bad.any(), f"{rep.case}: DHF(w) != w DHF(1) in rows {bad.nonzero().view(-1)[:8].tolist()} (weights {wk[bad][:8].tolist()})"


@_cases
def test_general_weights(op, shape, mode, eps):
    """property 3, and in mode 2 the same step twice: bit for bit the same (fixed-order sums, no atomics)"""
    c = WR.case(*shape, mode)
    rep = Report(f"{op} {c.name} eps {eps}")
    P, denom, keep, s3_ref, dhf1, dx1, g1 = _reference_pass(op, c, eps)
    wg = _weights(P.tok, "general")
    got = P.step_w(wg, eps, denom)
    _common(rep, got, keep, s3_ref)
    _against_statement(rep, P, c, op, eps, denom, wg, got, "general")
    if c.mode == 2:
        again = P.step_w(wg, eps, denom)
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, again)), f"{rep.case}: two runs differ"
    rep.line()


@pytest.mark.parametrize("op", LM.OPS)
def test_refusals_leave_the_outputs_alone(op):
    c = WR.case(*WR.SHAPES[0], 2)
    P = WeightPass(op, c, _inputs(c, op))
    P.fwd()
    w = _weights(P.tok, "general")
    nan3 = torch.full((3,), float("nan"), device="cuda")
    for eps in (0.0, 0.1):
        assert P.fwd_w(None, eps, nan3)[0] == ARG and P.bwd_w(None, eps, 3.0) == ARG
    for eps in (-0.1, 1.0, float("nan")):
        assert P.fwd_w(w, eps, nan3)[0] == ARG and P.bwd_w(w, eps, 3.0) == ARG
    assert P.fwd_w(w, 0.1, nan3, scratch=None)[0] == ARG and P.bwd_w(w, 0.1, 3.0, scratch=None) == ARG
    assert P.bwd_w(w, 0.0, 3.0, g32=None) == ARG                     # mode 2 without g32
    s0 = P.ge.shape(c.B, c.L, P.T, c.cap, 0)
    a = P.ge.arena
    l = _lib()
    one = torch.ones(1, device="cuda")
    assert l.cc_lmhead_ce_fwd_w(C.byref(P.cfg), C.byref(s0), _p(a.w32), _p(a.w16), _p(P.ws), _p(P.tok), _p(w), 0.1, _p(P.scratch), _p(nan3), _st()) == ARG
    assert l.cc_lmhead_ce_bwd_w(C.byref(P.cfg), C.byref(s0), _p(a.w32), _p(a.w16), _p(P.ws), _p(one), None, _p(w), 0.1, _p(P.scratch), _p(P.g32), _st()) == ARG
    torch.cuda.synchronize()
    assert torch.isnan(nan3).all() and torch.isnan(P.scratch).all() and torch.equal(_bits(P.g32), _bits(P.g0))
    # eps == 0 needs no scratch
    rc, s3 = P.fwd_w(w, 0.0, scratch=None)
    assert rc == 0 and P.bwd_w(w, 0.0, float(s3[1]), scratch=None) == 0 and torch.isfinite(s3).all() and torch.isfinite(P.g32).all()


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("op", LM.OPS)
def test_all_ignored_batch(op, mode, eps):
    """a batch without a kept row, every weight NaN or inf: loss sums 0, divisor clamped to 1, zero gradients, nothing NaN, and the bits of
    the same batch without weights"""
    c = WR.case(*WR.SHAPES[1], mode)
    x, gamma, beta, wte, tok = _inputs(c, op)
    tok = tok.clone()
    tok[:] = -1
    tok[0, 0] = 0
    P = WeightPass(op, c, (x, gamma, beta, wte, tok))
    P.fwd()
    P.bwd(0.0)
    dhf0, dx0, g_plain = P.state()
    w = torch.full((c.B, c.cap), float("nan"), device="cuda")
    w[1::2] = float("-inf")
    s3, dhf, dx, g = P.step_w(w, eps, 0.0)
    torch.cuda.synchronize()
    assert (s3 == 0).all() and (dhf == 0).all() and (dx == 0).all() and torch.isfinite(g).all()
    assert torch.equal(_bits(dhf), _bits(dhf0)) and torch.equal(_bits(dx), _bits(dx0)) and torch.equal(_bits(g), _bits(g_plain))


# ---- the engine ------------------------------------------------------------------------------------------------------------------------
def _engine_weights(tokens, seed=11):
    """fp32 (B, cap): magnitudes 0.25 .. 2 of either sign, one kept position of weight 0, NaN wherever the loss ignores the token"""
    g = torch.Generator().manual_seed(seed)
    w = (0.25 + 1.75 * torch.rand(tokens.shape, generator=g)) * torch.where(torch.rand(tokens.shape, generator=g) < 0.35, -1.0, 1.0)
    kept = (tokens.reshape(-1) > 0).nonzero().view(-1)
    w.view(-1)[kept[3]] = 0.0
    w[tokens <= 0] = float("nan")
    assert torch.isnan(w).any() and (w[tokens > 0] < 0).any()
    return w.float()


def _oracle_weighted_step(sd, cfg, tokens, embeds, w, rb, train, eps):
    """float64 autograd of the oracle's forward (the build's rounding points) with the weighted, smoothed loss written out in torch:
    sum over kept targets of w ((1 - eps) nll + eps mean over the classes of -log p) / the number of kept targets"""
    from oracle import clipcap_oracle as O
    sdr = {k: (v.double().requires_grad_(True) if k in train else v.double()) for k, v in sd.items()}
    tok = tokens.clamp_min(0)
    logits = O.clipcap_logits(sdr, tok, embeds.double(), cfg=cfg, rb=rb)
    lg = logits[:, cfg["prefix_length"] - 1:-1]
    logp = torch.log_softmax(lg.reshape(-1, lg.shape[-1]), 1)
    t = tok.flatten()
    keep = t != 0
    row = -(1.0 - eps) * logp.gather(1, t.view(-1, 1)).squeeze(1) - eps * logp.mean(1)
    n = keep.sum().clamp_min(1)
    loss = (w.flatten().double()[keep] * row[keep]).sum() / n
    loss.backward()
    nll = -logp.detach().gather(1, t.view(-1, 1)).squeeze(1)[keep].sum() / n
    return loss.detach(), nll, {k: sdr[k].grad for k in train}


@pytest.mark.parametrize("precision", [None, 16, 32])
@pytest.mark.parametrize("mode", ["prefix_only", "full"])
def test_weighted_step_on_the_goldens(mode, precision):
    """loss, plain NLL and every gradient tensor of forward_backward(token_weights=) with eps 0 and 0.1 against the oracle with the weighted
    loss, at the bounds tests/test_gpu_label_smoothing.py applies to the same quantities of the unweighted step; in the full finetune two
    runs are bit-equal.  Then the optimizer step itself: finite, and it moves the weights."""
    eng, sd, cfg, tokens, embeds, V = _golden_engine(mode, precision)
    train = [k for k in sd if mode == "full" or k.startswith("transformer_mapper.")]
    tol_loss, tol_grad = STEP_TOL[precision]
    w = _engine_weights(tokens)
    for eps in (0.0, 0.1):
        eng.zero_grad()
        loss = float(eng.forward_backward(tokens.cuda(), embeds.cuda(), label_smoothing=eps, token_weights=w.cuda()))
        nll = float(eng.last_nll)
        ref, ref_nll, grads = _oracle_weighted_step(sd, cfg, tokens, embeds, w, RB[precision], train, SM.eps32(eps))
        unscale = 1.0 / float(eng.scaler.scale) if eng.scaler is not None else 1.0
        gm, gg = eng.mapper.views(eng.mapper.arena.g32), eng.gpt2.views(eng.gpt2.arena.g32) if mode == "full" else {}
        worst = ("", 0.0)
        for k in train:
            mine = gm[k[len("transformer_mapper."):]] if k.startswith("transformer_mapper.") else gg[k[len("language_model."):]]
            mine = mine.double().cpu() * unscale
            if k.endswith("wte.weight"):
                mine = mine[:V]
            assert torch.isfinite(mine).all(), k
            r = ((mine - grads[k]).norm() / grads[k].norm().clamp_min(1e-12)).item()
            worst = max(worst, (k, r), key=lambda t: t[1])
        print(f"WEIGHTED STEP {mode} precision {precision} eps {eps}: |loss - oracle| {abs(loss - float(ref)):.3e} (loss {loss:.6f}); |nll - oracle| "
              f"{abs(nll - float(ref_nll)):.3e}; worst gradient rel. L2 {worst[1]:.3e} ({worst[0]}); bounds {tol_loss:g} / {tol_grad:g}")
        assert abs(loss - float(ref)) <= tol_loss and abs(nll - float(ref_nll)) <= tol_loss and worst[1] <= tol_grad, (eps, loss, float(ref), worst)
        if mode == "full":
            first = [a.g32.clone() for a in eng.arenas()]
            eng.zero_grad()
            again = eng.forward_backward(tokens.cuda(), embeds.cuda(), label_smoothing=eps, token_weights=w.cuda())
            assert float(again) == loss and all(torch.equal(_bits(a.g32), _bits(f)) for a, f in zip(eng.arenas(), first)), "two runs differ"
    # the plain NLL of the weighted step is the loss of the step without weights, to the bit
    eng.zero_grad()
    assert nll == float(eng.forward_backward(tokens.cuda(), embeds.cuda(), backward=False))
    eng.zero_grad()
    eng.forward_backward(tokens.cuda(), embeds.cuda(), label_smoothing=0.1, token_weights=w.cuda())
    before = [a.w32.clone() for a in eng.arenas()]
    eng.optimizer_step(1e-3, 1, weight_decay=0.01, max_grad_norm=1.0, ema_decay=0.9)      # with clipping and the weight average
    torch.cuda.synchronize()
    for a, w0 in zip(eng.arenas(), before):
        assert torch.isfinite(a.w32).all() and not torch.equal(a.w32, w0)
        assert a.ema is not None and torch.isfinite(a.ema).all()
    assert torch.isfinite(eng.last_grad_norm).all()


def _ddp_worker(rank, world, port, mode, out):
    import os
    import numpy as np
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from clipcap_amd.train.ddp import GradReducer, shard_batch, shard_range
    from tests.test_gpu_ddp import _build
    eng, tokens, embeds = _build(mode)
    w = _engine_weights(tokens)
    arenas = eng.arenas()
    red = GradReducer([a.grads() for a in arenas])
    tk, em = shard_batch(tokens, embeds, rank, world)
    lo, hi = shard_range(tokens.shape[0], rank, world)
    red.begin()
    loss = eng.forward_backward(tk.cuda(), em.cuda(), reduce_stats=red.reduce_stats, on_grads_ready=red.on_grads_ready, label_smoothing=0.1,
                                token_weights=w[lo:hi].cuda())
    red.finish()
    torch.cuda.synchronize()
    if rank == 0:
        np.savez(out, loss=float(loss), nll=float(eng.last_nll), **{f"g{i}": a.g32.cpu().numpy() for i, a in enumerate(arenas)})
    dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["prefix_only", "full"])
def test_two_rank_weighted_step_equals_single_process(tmp_path, mode):
    """two ranks with half the batch and half the weights each (sharing the box's GPU over gloo, as tests/test_gpu_ddp.py does) against one
    rank with the whole batch: reduce_stats sums the 3-float stats, the divisor is the global kept count, so loss, nll and gradients agree
    at that test's bounds"""
    import numpy as np
    import torch.multiprocessing as mp
    from tests.test_ddp_gloo import _free_port
    from tests.test_gpu_ddp import _build
    out = str(tmp_path / "ddp.npz")
    mp.spawn(_ddp_worker, args=(2, _free_port(), mode, out), nprocs=2, join=True)
    res = np.load(out)
    eng, tokens, embeds = _build(mode)
    loss = eng.forward_backward(tokens.cuda(), embeds.cuda(), label_smoothing=0.1, token_weights=_engine_weights(tokens).cuda())
    torch.cuda.synchronize()
    assert abs(float(loss) - float(res["loss"])) <= 1e-5 and abs(float(eng.last_nll) - float(res["nll"])) <= 1e-5
    assert float(loss) != float(eng.last_nll)
    for i, a in enumerate(eng.arenas()):
        ref = a.g32.cpu().numpy()
        rel = np.linalg.norm(res[f"g{i}"] - ref) / np.linalg.norm(ref)
        assert rel <= 2e-2, (i, rel)


# ---- the self-critical step ------------------------------------------------------------------------------------------------------------
def _scst_model():
    from clipcap_amd.encoders import EncoderConfig
    from clipcap_amd.model import ClipCapModel, Config, TrainingConfig
    from clipcap_amd.model.gpt2 import GPT2LM
    from tests.util import load_golden, sd_of
    g = load_golden("beam_tiny")
    D, n_layer, n_head, V, npos = [int(v) for v in g["cfg"]]
    eos = int(g["beam1.meta"][0])
    torch.manual_seed(3)
    lm = GPT2LM(n_embd=D, n_layer=n_layer, n_head=n_head, vocab_size=V, n_positions=npos)
    lm.load_state_dict(sd_of(g), strict=False)
    cfg = Config(language_model="unused", train_language_model=True, prefix_length=3, projection_length=2, transformer_layers=1,
                 transformer_attention_heads=2, encoder_config=EncoderConfig(encoder_embedding_size=16),
                 training_config=TrainingConfig(optimizer_lr=0.0, use_deepspeed_optimisers=False, scheduler_warmup_steps=1, total_steps=4))
    model = ClipCapModel(cfg, language_model=lm).to("cuda").eval()
    embeds = torch.randn(6, 16, generator=torch.Generator().manual_seed(4)).cuda()
    return model, embeds, eos, V, min(8, npos - 4)


def _reward_of(V, eos):
    def reward(ids):
        """minus the number of tokens from the lower half of the vocabulary, up to and including the first stop token"""
        hit = ids == eos
        upto = (hit.cumsum(1) - hit.long()) == 0
        return -((ids < V // 2) & upto).sum(1).float()
    return reward


def test_self_critical_step_equals_the_weighted_step_by_hand():
    """lr = 0 keeps the weights, so the same seed gives the same samples: the gradient arenas after self_critical_step are bit-equal to
    those of fused_step called by hand with the sampled tokens and the advantage; no sampled position is token 0"""
    from clipcap_amd.inference.base import sample_tokens
    from clipcap_amd.train import scst_tokens_and_weights, self_critical_step
    model, embeds, eos, V, entry = _scst_model()
    reward = _reward_of(V, eos)
    seen = {}

    def reward_fn(sampled, greedy):
        seen["sampled"], seen["greedy"] = sampled.clone(), greedy.clone()
        return reward(sampled), reward(greedy)

    gen = torch.Generator(device="cuda").manual_seed(7)
    loss, r_s, r_g = self_critical_step(model, embeds, reward_fn, 0.0, entry_length=entry, stop_token=eos, generator=gen)
    torch.cuda.synchronize()
    got = [a.g32.clone() for a in model.engine.arenas()]
    assert torch.isfinite(loss) and (seen["sampled"] != 0).all() and (seen["greedy"] != 0).all()
    # by hand
    gen = torch.Generator(device="cuda").manual_seed(7)
    with torch.no_grad():
        prefix = model.engine.mapper.forward(embeds, save=False)
        sampled, _ = sample_tokens(model, prefix, entry_length=entry, stop_token=eos, mode=0, top_p=1.0, generator=gen, suppress_tokens=[0])
        greedy, _ = sample_tokens(model, prefix, entry_length=entry, stop_token=eos, mode=0, top_p=1.0, top_k=1, suppress_tokens=[0])
    assert torch.equal(sampled, seen["sampled"]) and torch.equal(greedy, seen["greedy"])
    adv = reward(sampled) - reward(greedy)
    assert (adv != 0).any() and float(r_s) == float(reward(sampled).mean()) and float(r_g) == float(reward(greedy).mean())
    tokens, weights = scst_tokens_and_weights(sampled, adv, eos)
    by_hand = model.fused_step((tokens, embeds), 0.0, token_weights=weights)
    torch.cuda.synchronize()
    assert float(by_hand) == float(loss)
    for a, g in zip(model.engine.arenas(), got):
        assert torch.equal(_bits(a.g32), _bits(g)) and bool(g.ne(0).any())


def test_equal_rewards_give_exactly_zero_gradients():
    from clipcap_amd.train import self_critical_step
    model, embeds, eos, V, entry = _scst_model()
    gen = torch.Generator(device="cuda").manual_seed(7)
    loss, r_s, r_g = self_critical_step(model, embeds, lambda s, g: (torch.full((s.shape[0],), 2.5), torch.full((s.shape[0],), 2.5)), 0.0,
                                        entry_length=entry, stop_token=eos, generator=gen)
    torch.cuda.synchronize()
    assert float(loss) == 0.0 and float(r_s) == 2.5 == float(r_g) and float(model.last_nll) > 0.0
    for a in model.engine.arenas():
        assert (a.g32 == 0).all()
