"""No call reads a workspace byte it did not write this call (or that an earlier call of the same forward -> backward chain wrote for it).

The engines keep their workspaces between calls and reuse them across shapes (MapperEngine._ws, Gpt2Engine._ws "grown on demand",
_score_ws, smooth_scratch, _embed_bwd_ws, GradClipper.scratch), so a call normally starts on the leftovers of another call — after an
fp16 overflow on inf / NaN.  Every case below runs its chain twice from identical state: run A on workspaces filled with zeros, run B on
workspaces filled with 0xFF bytes (NaN in fp32 / bf16 / fp16, -1 as int32), both as framed buffers injected where the engine caches its
own (tests/ws_poison.py).  Everything the chain produces must be torch.equal between A and B and finite, the guards around every buffer
must be intact (nothing is written outside cc_*_ws_bytes), every buffer must have been written to, and the engine must still hold it.
First A is run twice and must equal itself.  No chain needed a tolerance: all of them repeat bit for bit.

Engines are built on "cuda:0": the engines compare a cached buffer's device with their own, and torch.device("cuda") != the
torch.device("cuda:0") a tensor reports, so an engine built on plain "cuda" never reuses its cached GPT-2 workspace (and could not keep
an injected one; Injection.verify would say so).

Integer buffers inside the workspaces, read as indices — each checked by reading the code to be written by the call's own chain before
anything reads it (so the -1 of the poison never becomes an address):
  * Gpt2WS.target, Gpt2WS.row_map [B*cap]: loss.hip k_ce_targets writes all B*cap entries first thing in cc_lmhead_ce_fwd / _smooth and
    cc_lmhead_score; read by ln_fwd / ln_bwd (row < rows), the lm_head epilogues (row < M: gemm.hip.h EpiLMHead*::load_row / operator()),
    ce_rows, ce_dlogits, lm_tgt_ref, lm_rowfac, lm_dgrad_fix, smooth_rows, smooth_dhf (all row < Mc) and scatter_rows (r < R).
    cc_lmhead_ce_bwd reads what the forward of the same chain wrote.  cc_gpt2_logits / cc_gpt2_logits_bwd pass no row_map and read no target.
  * Gpt2WS.keep [B*cap]: loss.hip k_score_keep writes all entries in cc_lmhead_score before score_rows reads them.
  * the scatter's index (reduce.hip sc_carve: tkeys, skeys, info, heads, mstarts, cnt): k_sc_sort_tile writes tkeys[0, R); k_sc_rank reads
    those and writes skeys / info at a permutation of [0, R) (keys are unique); k_sc_compact reads [0, R) and writes heads[0, cnt[0]),
    mstarts[0, cnt[1]) and cnt[0..1]; k_sc_sum / k_sc_fold read exactly those ranges; part is written by k_sc_sum before k_sc_fold.
    Token ids are clamped to [0, Vp) in k_sc_sort_tile.
  * beam scratch (beam.hip): pidx — every (sample, chunk, slot < width) written by beam_partial_body (k_beam_partial /
    k_beam_group_partial) before beam_final_body (k_beam_final / k_beam_group_final) reads them; picks — beam group g reads slots
    [0, row0) that the finals of groups < g wrote this step; the plain kernels have no picks.
  * MapperWS has no integer buffer.  DecodeSession.row_map is not scratch: it is built by arange at construction and never poisoned here.
The token inputs themselves (int64, -1 pads) are the caller's, not workspace; embed_concat and ce_targets clamp id < 0.

OUT OF SCOPE, DELIBERATELY: the decode workspace (DecodeSession._ws, decode.hip dec_carve).  It holds the arrival counters of the
persistent layer launch (pk_ctr), the control words of the XCD-team engine (xt_ctl) and a sticky error word; its contract is "starts
clear", engine.py allocates it with torch.zeros, and a nonzero counter could make a persistent launch wait forever.  Never fill it with
anything, and do not "complete" the coverage below by adding it."""
import pytest
import torch

from tests.ws_poison import (FILL_NAN, FILL_ZERO, embed_bwd_ws_bytes, gpt2_ws_bytes, grad_norm_scratch_bytes, injected_workspaces,
                             mapper_ws_bytes, smooth_scratch_bytes)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
S1 = dict(E=16, D=128, P=2, L=3, H=2, N=1, n_head=2, n_layer=2, V=157, npos=32, B=3, cap=7)      # T = 10: everything in one block
S2 = dict(S1, L=10, npos=96, B=40, cap=60)      # T = 70 > 64, M = 2800 rows (ragged 128-row tiles, folds over several blocks), Mc = 2400
SHAPES = {"S1": S1, "S2": S2}
DROP = (0.1, 0.15, 0.2, 0x1234_5678_9ABC)
LR = 1e-2


@pytest.fixture(autouse=True)
def _end_the_session_on_a_device_error():
    """A wrong value is a failed test; a device error ends the session, so that nothing more is started on a card that has faulted."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error during the workspace-poison tests: {e}", returncode=3)


# ------------------------------------------------------------------------------------------------ models and inputs
def _fill_weights(eng, gen):
    for k, v in eng.views(eng.arena.w32).items():
        if ("norm" in k or "ln_" in k) and k.endswith("weight"):
            t = 1.0 + 0.05 * torch.randn(v.shape, generator=gen)
        elif k.endswith(".bias"):
            t = 0.02 * torch.randn(v.shape, generator=gen)
        elif "prefix_const" in k or "pos_embeddings" in k:
            t = torch.randn(v.shape, generator=gen)
        else:
            t = torch.randn(v.shape, generator=gen) * (0.1 if ("wte" in k or "wpe" in k) else 0.5 / v.shape[-1] ** 0.5)
        v.copy_(t)


def _mapper(s, precision, W=1, use_pos=False):
    from clipcap_amd.engine import MapperEngine
    me = MapperEngine(s["E"], s["D"], s["L"], s["P"], s["H"], s["N"], window=W, use_pos=use_pos, device=DEV)
    _fill_weights(me, torch.Generator().manual_seed(11))
    if precision != "bf16":
        me.set_precision(precision)
    return me


def _gpt2(s, precision, npos=None):
    from clipcap_amd.engine import Gpt2Engine
    ge = Gpt2Engine(s["D"], s["n_head"], s["n_layer"], s["V"], npos or s["npos"], device=DEV)
    _fill_weights(ge, torch.Generator().manual_seed(12))
    if precision != "bf16":
        ge.set_precision(precision)
    return ge


def _engine(s, precision, train_lm, npos=None):
    """Seeded random weights with perturbed LayerNorm parameters and biases, as test_gpu_dropout.py::_build makes them; the same call
    gives the same engine, bit for bit."""
    from clipcap_amd.engine import ClipCapEngine
    return ClipCapEngine(_mapper(s, precision), _gpt2(s, precision, npos), train_lm=train_lm)


def _batch(s, seed, B=None, cap=None, W=1):
    """(tokens int64 (B, cap), embeds): ragged -1 tails on some samples, a few 0 tokens (the loss ignores them), one sample all pads."""
    B, cap = B or s["B"], cap or s["cap"]
    g = torch.Generator().manual_seed(seed)
    tokens = torch.randint(1, s["V"], (B, cap), generator=g)
    for b in range(1, B, 3):
        tokens[b, 1 + (5 * b + seed) % (cap - 1):] = -1
    tokens[0, 2] = 0
    tokens[0, cap - 1] = 0
    if B > 5:
        tokens[5, ::7] = 0
    tokens[2 if B <= 4 else 7] = -1
    embeds = torch.randn((B, s["E"]) if W == 1 else (B, W, s["E"]), generator=g)
    return tokens.to(DEV), embeds.to(DEV)


# ------------------------------------------------------------------------------------------------ comparing
def _keep(out, name, t):
    if t is not None:
        out[name] = t.detach().clone()


def _assert_finite(out, what):
    for k, v in out.items():
        if v.is_floating_point():
            bad = int((~torch.isfinite(v.float())).sum())
            assert bad == 0, f"{what}: {k} holds {bad} non-finite values of {v.numel()}"


def _assert_same(a, b, what):
    assert a.keys() == b.keys(), (what, sorted(a.keys() ^ b.keys()))
    for k in a:
        if not torch.equal(a[k], b[k]):
            x, y = a[k].double().flatten(), b[k].double().flatten()
            ne = (x != y) | (torch.isnan(x) != torch.isnan(y))
            raise AssertionError(f"{what}: {k} differs in {int(ne.sum())} of {x.numel()} elements; {int(torch.isnan(y).sum())} NaN in the second run; "
                                 f"largest finite difference {float((x - y)[torch.isfinite(x - y)].abs().max()) if bool(torch.isfinite(x - y).any()) else 0.0:.3e}")


def _three_runs(chain, what):
    """A, A again, B: the precondition (A repeats bit for bit), then zeros against 0xFF.  ``chain(fill)`` builds its own state."""
    a = chain(FILL_ZERO)
    _assert_finite(a, what + " [zero-filled workspaces]")
    _assert_same(a, chain(FILL_ZERO), what + " [precondition: the chain on zero-filled workspaces, run twice]")
    b = chain(FILL_NAN)
    _assert_finite(b, what + " [0xFF-filled workspaces]")
    _assert_same(a, b, what + " [zero-filled against 0xFF-filled workspaces]")
    return a


# ------------------------------------------------------------------------------------------------ case 1: the mapper
def _mapper_specs(me, B, saves=(0, 1)):
    return [(f"mapper ws (B={B}, save={sv})", me._ws, (B, sv), mapper_ws_bytes(me, B, sv), torch.uint8) for sv in saves]


MAPPER_CASES = [(sh, p, form) for sh, ps in (("S1", ("bf16", 16, 32)), ("S2", ("bf16", 32))) for p in ps for form in ("plain", "windowed")]


@pytest.mark.parametrize("shape,precision,form", MAPPER_CASES, ids=lambda v: str(v))
def test_mapper_forward_and_backward(shape, precision, form):
    """forward(save=False), then forward(save=True) + backward: the output of both and the whole g32 arena."""
    s = SHAPES[shape]
    W = 2 if form == "windowed" else 1

    def chain(fill):
        me = _mapper(s, precision, W=W, use_pos=W > 1)
        _, embeds = _batch(s, 3, W=W)
        dout = torch.randn(s["B"], s["L"], s["D"], generator=torch.Generator().manual_seed(4)).to(DEV)
        out = {}
        with injected_workspaces(_mapper_specs(me, s["B"]), fill, DEV):
            _keep(out, "out (save=False)", me.forward(embeds, save=False))
            _keep(out, "out (save=True)", me.forward(embeds, save=True))
            me.backward(dout)
            _keep(out, "mapper g32", me.arena.g32)
        return out

    out = _three_runs(chain, f"mapper {shape} {precision} {form}")
    assert bool(out["mapper g32"].ne(0).any())


def test_negative_control_poison_between_forward_and_backward_reaches_the_gradients():
    """The injected buffer IS the one the library reads: filled with 0xFF between forward(save=True) and backward, it puts NaN into the
    gradients — so the other cases cannot pass on a buffer the engine allocated for itself."""
    me = _mapper(S1, "bf16")
    _, embeds = _batch(S1, 3)
    dout = torch.randn(S1["B"], S1["L"], S1["D"], generator=torch.Generator().manual_seed(4)).to(DEV)
    with injected_workspaces(_mapper_specs(me, S1["B"], saves=(1,)), FILL_ZERO, DEV) as inj:
        me.forward(embeds, save=True)
        inj.slots[0].framed.refill(FILL_NAN)
        me.backward(dout)
    assert bool(torch.isnan(me.arena.g32).any())


# ------------------------------------------------------------------------------------------------ case 2: the training step
def _train_specs(eng, shp, eps=0.0, clip=None, mapper_B=()):
    from clipcap_amd.engine import GradClipper
    specs = [(f"gpt2 ws (mode {shp.mode})", eng.gpt2._ws, shp.mode, gpt2_ws_bytes(eng.gpt2, shp), torch.uint8)]
    for B in mapper_B or (shp.B,):
        specs += _mapper_specs(eng.mapper, B, saves=(1,))
    if eps > 0.0:
        specs.append(("smooth_scratch", eng, "smooth_scratch", smooth_scratch_bytes(eng.gpt2, shp), torch.float32))
    if clip is not None:
        eng.clipper = GradClipper(eng.mapper.arena.device, clip)
        eng.last_grad_norm = eng.clipper.norm
        specs.append(("GradClipper.scratch", eng.clipper, "scratch", grad_norm_scratch_bytes(), torch.float32))
    return specs


def _shape_of(eng, s, B=None, cap=None, dropout=None):
    B, cap, L = B or s["B"], cap or s["cap"], eng.mapper.dims["L"]
    return eng.gpt2.shape(B, L, L + cap, cap, 2 if eng.train_lm else 1, dropout)


def _keep_grads(out, eng, tag):
    _keep(out, f"{tag} mapper g32", eng.mapper.arena.g32)
    _keep(out, f"{tag} gpt2 g32", eng.gpt2.arena.g32)


def _keep_arenas(out, eng, tag):
    for name, a in zip(("mapper", "gpt2"), eng.arenas()):
        for f in ("w32", "m", "v", "w16"):
            _keep(out, f"{tag} {name} {f}", getattr(a, f))


def _step(out, eng, tag, batch, i, *, dropout=None, eps=0.0, clip=None, hook=False):
    eng.zero_grad()
    loss = eng.forward_backward(*batch, dropout=dropout, label_smoothing=eps, on_grads_ready=(lambda a, lo, hi: None) if hook else None)
    _keep(out, f"{tag} loss", loss)
    _keep(out, f"{tag} nll", eng.last_nll)
    _keep_grads(out, eng, tag)
    eng.optimizer_step(LR, i + 1, max_grad_norm=clip)
    _keep_arenas(out, eng, tag)
    if clip is not None:
        _keep(out, f"{tag} grad norm", eng.last_grad_norm)


def _variant(**kw):
    return dict(dict(dropout=None, eps=0.0, clip=None, hook=False), **kw)


TRAIN_CASES = []
for _sh, _ps in (("S1", ("bf16", 16, 32)), ("S2", ("bf16", 32))):
    for _p in _ps:
        TRAIN_CASES += [(_sh, _p, False, "plain", _variant()), (_sh, _p, True, "plain", _variant()),
                        (_sh, _p, True, "dropout", _variant(dropout=DROP)),
                        (_sh, _p, True, "smooth", _variant(eps=0.1))]
TRAIN_CASES += [("S1", "bf16", False, "smooth", _variant(eps=0.1)), ("S2", "bf16", False, "smooth", _variant(eps=0.1)),
                ("S1", 16, False, "smooth", _variant(eps=0.1)),
                ("S1", "bf16", True, "clip", _variant(clip=1.0)),
                ("S1", "bf16", False, "sliced", _variant(hook=True)), ("S1", "bf16", True, "sliced", _variant(hook=True)),
                ("S1", 16, True, "sliced", _variant(hook=True)),
                ("S2", "bf16", True, "sliced+dropout", _variant(hook=True, dropout=DROP)), ("S2", 32, True, "sliced", _variant(hook=True))]


@pytest.mark.parametrize("shape,precision,train_lm,name,kw", TRAIN_CASES, ids=[f"{c[0]}-{c[1]}-{'full' if c[2] else 'frozen'}-{c[3]}" for c in TRAIN_CASES])
def test_training_step(shape, precision, train_lm, name, kw):
    """Two consecutive forward_backward + optimizer_step: the loss, both g32 arenas, and after each optimizer_step w32, m, v and w16 of
    every trained arena.  sliced: with on_grads_ready, i.e. through cc_gpt2_bwd_range / cc_mapper_bwd_range."""
    s = SHAPES[shape]

    def chain(fill):
        eng = _engine(s, precision, train_lm)
        out = {}
        with injected_workspaces(_train_specs(eng, _shape_of(eng, s, dropout=kw["dropout"]), kw["eps"], kw["clip"]), fill, DEV):
            for i in range(2):
                _step(out, eng, f"step {i}", _batch(s, 20 + i), i, **kw)
        return out

    out = _three_runs(chain, f"training step {shape} {precision} {'full' if train_lm else 'frozen'} {name}")
    assert bool(out["step 1 mapper g32"].ne(0).any()) and not torch.equal(out["step 0 mapper w32"], out["step 1 mapper w32"])


# ------------------------------------------------------------------------------------------------ case 3: a stale shape
@pytest.mark.parametrize("precision", ["bf16", 16, 32], ids=str)
@pytest.mark.parametrize("train_lm", [False, True], ids=["frozen", "full"])
def test_small_step_on_the_leftovers_of_a_large_one(precision, train_lm):
    """What real training produces: in ONE set of buffers sized for S2 (0xFF-filled), an S2 step, zero_grad, then a step with S1's batch
    shape (B = 3, cap = 7; the models are S2's, so the prefix has 10 rows and T = 17) — twice, the second time with other inputs.  Each
    small step must equal, bit for bit, the same step on zero-filled buffers of the same size that have seen no other call.  The
    mapper's workspace is per batch size: its B = 3 buffer serves two different inputs."""
    s, Bs, caps = S2, S1["B"], S1["cap"]

    def specs(eng, stale):
        return _train_specs(eng, _shape_of(eng, s), mapper_B=(s["B"], Bs) if stale else (Bs,))

    def small_step(out, eng, seed):
        eng.zero_grad()
        _keep(out, "loss", eng.forward_backward(*_batch(s, seed, B=Bs, cap=caps)))
        _keep_grads(out, eng, "small step")

    eng = _engine(s, precision, train_lm)
    stale = []
    with injected_workspaces(specs(eng, True), FILL_NAN, DEV):
        for big_seed, small_seed in ((30, 31), (32, 33)):
            eng.zero_grad()
            eng.forward_backward(*_batch(s, big_seed))
            stale.append({})
            small_step(stale[-1], eng, small_seed)
    for i, small_seed in enumerate((31, 33)):
        fresh = {}
        twin = _engine(s, precision, train_lm)
        with injected_workspaces(specs(twin, False), FILL_ZERO, DEV):
            small_step(fresh, twin, small_seed)
        _assert_finite(fresh, f"fresh small step {i}")
        _assert_finite(stale[i], f"small step {i} after a large one")
        _assert_same(fresh, stale[i], f"small step {i}: fresh zero-filled buffers against the leftovers of an S2 step on 0xFF")
    assert not torch.equal(stale[0]["small step mapper g32"], stale[1]["small step mapper g32"])


# ------------------------------------------------------------------------------------------------ case 4: the step after an fp16 overflow
def test_the_step_after_an_fp16_overflow_is_unaffected():
    """fp16 operands, full finetune, the engine's LossScaler.  Step 1 takes embeds * 1e6: the activations overflow, found_inf is raised
    and the step is skipped on the device, leaving inf / NaN all over the workspaces.  Step 2 with normal inputs must equal step 2 of a
    twin with the same weights and scaler state on zero-filled workspaces."""
    from clipcap_amd.engine import LossScaler
    s = S1
    eng = _engine(s, 16, True)
    shp = _shape_of(eng, s)
    tokens, embeds = _batch(s, 40)
    got, want = {}, {}
    with injected_workspaces(_train_specs(eng, shp), FILL_NAN, DEV):
        w0 = [a.w32.clone() for a in eng.arenas()]
        eng.zero_grad()
        loss = eng.forward_backward(tokens, embeds * 1e6)
        assert not bool(torch.isfinite(loss)), float(loss)
        assert any(not bool(torch.isfinite(a.g32).all()) for a in eng.arenas())
        state0 = eng.scaler.state.clone()
        eng.optimizer_step(LR, 1)
        for a, w in zip(eng.arenas(), w0):      # skipped: weights and moments unchanged, scale halved, no applied step counted
            assert torch.equal(a.w32, w) and not bool(a.m.any()) and not bool(a.v.any())
        assert float(eng.scaler.state[0]) == 0.5 * float(state0[0]) and float(eng.scaler.state[2]) == float(state0[2]) == 0.0
        assert float(eng.scaler.found_inf) == 0.0
        state1 = eng.scaler.state.clone()
        _step(got, eng, "step 2", _batch(s, 41), 1)
    twin = _engine(s, 16, True)
    twin.scaler = LossScaler(twin.gpt2.arena.device)
    twin.scaler.state.copy_(state1)
    with injected_workspaces(_train_specs(twin, shp), FILL_ZERO, DEV):
        _step(want, twin, "step 2", _batch(s, 41), 1)
    _assert_finite(want, "twin step 2")
    _assert_finite(got, "step 2 after the overflow")
    _assert_same(want, got, "step 2: twin on zero-filled workspaces against the engine whose step 1 overflowed")
    assert not torch.equal(got["step 2 mapper w32"], w0[0]) and float(twin.scaler.state[2]) == 1.0 == float(eng.scaler.state[2])


# ------------------------------------------------------------------------------------------------ case 5: logits and scoring
LOGITS_CASES = [(sh, p, m) for sh, ps in (("S1", ("bf16", 16, 32)), ("S2", ("bf16", 32))) for p in ps for m in (0, 1, 2)]


@pytest.mark.parametrize("shape,precision,save_mode", LOGITS_CASES, ids=str)
def test_logits_and_logits_backward(shape, precision, save_mode):
    """Gpt2Engine.logits at save_mode 0 / 1 / 2 and logits_backward: the logits, dx0, and for mode 2 the accumulated g32."""
    s = SHAPES[shape]
    B, T = s["B"], s["L"] + s["cap"]
    g = torch.Generator().manual_seed(50)
    x = (0.5 * torch.randn(B, T, s["D"], generator=g)).to(DEV)
    dlogits = (1e-3 * torch.randn(B, T, s["V"], generator=g)).to(DEV)

    def chain(fill):
        ge = _gpt2(s, precision)
        shp = ge.shape(B, T, T, 0, 0) if not save_mode else ge.shape(B, 0, T, T, save_mode)
        out = {}
        with injected_workspaces([(f"gpt2 ws (mode {save_mode})", ge._ws, save_mode, gpt2_ws_bytes(ge, shp), torch.uint8)], fill, DEV):
            _keep(out, "logits", ge.logits(x, save_mode))
            if save_mode:
                _keep(out, "dx0", ge.logits_backward(dlogits))
                _keep(out, "gpt2 g32", ge.arena.g32)
        return out

    out = _three_runs(chain, f"logits {shape} {precision} save_mode {save_mode}")
    assert ("gpt2 g32" in out) == (save_mode == 2)


@pytest.mark.parametrize("shape,precision", [("S1", "bf16"), ("S1", 16), ("S1", 32), ("S2", "bf16"), ("S2", 32)], ids=str)
@pytest.mark.parametrize("ignore_zero", [False, True], ids=["all", "ignore_zero"])
def test_score(shape, precision, ignore_zero):
    """ClipCapEngine.score: token log-probabilities and per-sample sums and counts, on its own workspace and the mapper's save = 0 one."""
    s = SHAPES[shape]

    def chain(fill):
        eng = _engine(s, precision, False)
        L = s["L"]
        shp = eng.gpt2.shape(s["B"], L, L + s["cap"], s["cap"], 0)
        specs = [("_score_ws", eng, "_score_ws", gpt2_ws_bytes(eng.gpt2, shp), torch.uint8)] + _mapper_specs(eng.mapper, s["B"], saves=(0,))
        out = {}
        with injected_workspaces(specs, fill, DEV):
            lp, ssum, cnt = eng.score(*_batch(s, 60), ignore_zero=ignore_zero)
            _keep(out, "token_logprob", lp)
            _keep(out, "sample_sum", ssum)
            _keep(out, "sample_count", cnt)
        return out

    out = _three_runs(chain, f"score {shape} {precision} ignore_zero={ignore_zero}")
    assert bool(out["sample_count"].eq(0).any()) and bool(out["sample_count"].gt(0).any())       # the all-pads sample, and real ones


@pytest.mark.parametrize("R", [21, 2400], ids=lambda r: f"R{r}")
def test_embed_tokens_bwd_bridge(R):
    """engine.embed_tokens_bwd (cc_embed_tokens_bwd_ws, the scatter of reduce.hip) on its cached index scratch: duplicate ids (a list longer
    than one chunk at R = 2400, which also spans two sort tiles), pad ids (-1) and ids of 0."""
    from clipcap_amd.engine import embed_tokens_bwd
    s = S1
    g = torch.Generator().manual_seed(70 + R)
    tokens = torch.randint(0, s["V"], (R,), generator=g).to(torch.int32)
    tokens[::5] = 9
    tokens[3::11] = -1
    tokens[1] = 0
    dout = torch.randn(R, s["D"], generator=g).to(DEV)
    tokens = tokens.to(DEV)

    def chain(fill):
        ge = _gpt2(s, "bf16")
        out = {}
        with injected_workspaces([("_embed_bwd_ws", ge, "_embed_bwd_ws", embed_bwd_ws_bytes(ge, R), torch.uint8)], fill, DEV):
            _keep(out, "d wte", embed_tokens_bwd(ge, tokens, dout))
        return out

    out = _three_runs(chain, f"embed_tokens_bwd R={R}")
    keep = tokens >= 0
    want = torch.zeros(s["V"], s["D"], dtype=torch.float64, device=DEV).index_add_(0, tokens[keep].long(), dout[keep].double())
    want[0] += dout[~keep].double().sum(0)      # pad ids are clamped to 0, as the training path's scatter does
    assert float((out["d wte"].double() - want).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max()))


# ------------------------------------------------------------------------------------------------ case 6: decoder scratch that is plain data
# (the decode workspace itself — DecodeSession._ws — is out of scope, deliberately: see the module docstring.  It is never filled here.)
# The sampling step (engine.sample_step / cc_sample_step_lp) takes no scratch from its caller — tokens and probabilities are outputs it
# writes in full — so there is nothing of it to fill.
STOP = 17


def _step_logits(R, ld, seed, steps=3):
    """As test_gpu_beam_group.py::_inputs: randn * 3, from step 1 on +25 on the stop logit of every third row (stopped beams)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for step in range(steps):
        buf = torch.randn(R, ld, generator=g) * 3.0
        if step >= 1:
            buf[::3, STOP] += 25.0
        out.append(buf.to(DEV))
    return out


def _fill_bufs(bufs, byte):
    for t in bufs:
        t.view(torch.uint8).fill_(byte)
    return bufs


@pytest.mark.parametrize("beam,groups,V,ld", [(5, 1, 4099, 4104), (6, 1, 1001, 1001), (6, 3, 4099, 4104), (4, 2, 1001, 1001), (12, 2, 130, 136)],
                         ids=lambda v: str(v))
def test_beam_scratch(beam, groups, V, ld):
    """beam_buffers / beam_group_buffers (outputs and scratch alike) filled with 0xFF against zeros: three steps through stopped beams;
    tokens, source rows and state must be equal."""
    from clipcap_amd.engine import beam_buffers, beam_group_buffers, beam_group_step, beam_step
    S = 3
    logits = _step_logits(S * beam, ld, beam * 1000 + V + groups)

    def chain(byte):
        bufs = _fill_bufs(beam_buffers(DEV, S, beam, V) if groups == 1 else beam_group_buffers(DEV, S, beam, groups, V), byte)
        scores, seql, stopped = torch.zeros(S * beam, device=DEV), torch.ones(S * beam, device=DEV), torch.zeros(S * beam, dtype=torch.uint8, device=DEV)
        out = {}
        for i, lg in enumerate(logits):
            if groups == 1:
                nt, sr = beam_step(lg[:, :V], S, beam, 0.9, i == 0, STOP, scores, seql, stopped, bufs)
            else:
                nt, sr = beam_group_step(lg[:, :V], S, beam, groups, 0.9, 0.7, i == 0, STOP, scores, seql, stopped, bufs)
            for name, t in (("tokens", nt), ("src", sr), ("scores", scores), ("lengths", seql), ("stopped", stopped)):
                _keep(out, f"step {i} {name}", t)
        return out

    a, b = chain(0x00), chain(0xFF)
    _assert_finite(b, "beam scratch 0xFF")
    _assert_same(a, b, f"beam {beam} groups {groups}: zeroed against 0xFF-filled buffers")
    assert bool(a["step 2 stopped"].any())


def test_contrastive_scratch():
    """contrastive_buffers: the fields a step only writes (cand_tok, cand_prob, sel, src_rows, skip_rows) and the history rows beyond the
    context filled with 0xFF against the zeros the constructor gives; the state fields (stopped, lengths, captions, scores) start at
    zero by contract and keep it.  Three steps of top-k + select on synthetic logits and unit vectors."""
    from clipcap_amd.engine import contrastive_buffers, contrastive_select, contrastive_topk
    S, k, D, V, L0, steps = 3, 4, 128, 1001, 2, 3
    g = torch.Generator().manual_seed(80)
    unit = lambda *shape: torch.nn.functional.normalize(torch.randn(*shape, generator=g), dim=-1).to(DEV)      # noqa: E731
    prefix_h, cand_h = unit(S, L0, D), [unit(S * k, D) for _ in range(steps)]
    logits0 = (torch.randn(S, V, generator=g) * 3.0).to(DEV)
    logits = _step_logits(S * k, V, 81, steps)

    def chain(byte):
        b = contrastive_buffers(DEV, S, k, D, L0 + steps, steps)
        for t in (b.cand_tok, b.cand_prob, b.cand_h, b.sel, b.src_rows, b.skip_rows, b.hist):
            t.view(torch.uint8).fill_(byte)
        b.hist[:, :L0] = prefix_h
        out = {}
        contrastive_topk(logits0, S, 1, None, k, None, b.cand_tok, b.cand_prob)
        for i in range(steps):
            b.cand_h.copy_(cand_h[i])
            contrastive_select(b, k, 0, L0 + i, 0.6, STOP, i)
            contrastive_topk(logits[i], S, k, b.sel, k, b.stopped, b.cand_tok, b.cand_prob)
            for name in ("cand_tok", "cand_prob", "sel", "src_rows", "skip_rows", "stopped", "lengths", "captions", "scores"):
                _keep(out, f"step {i} {name}", getattr(b, name))
            _keep(out, f"step {i} hist", b.hist[:, :L0 + i + 1])
        return out

    a, b = chain(0x00), chain(0xFF)
    _assert_finite(b, "contrastive scratch 0xFF")
    _assert_same(a, b, "contrastive search: zeroed against 0xFF-filled buffers")


def _poison_session(sess, byte):
    """KV cache, logits and softmax partials of a DecodeSession — everything but its decode workspace (out of scope: module docstring) and
    its ancestry table (data, built at construction).  Cache positions below sess.pos hold what expand() copied: they stay."""
    import ctypes as C

    from clipcap_amd import _lib
    d = sess.g.dims
    if sess.pos == 0:
        sess.kv.view(torch.uint8).fill_(byte)
    else:
        sess.kv.view(d["NL"], 2, sess.R, sess.ctx_max, d["D"])[:, :, :, sess.pos:, :] = float("nan") if byte else 0.0
    sess._logits = torch.empty(sess.R, d["Vp"], dtype=torch.float32, device=sess.kv.device)
    sess._logits.view(torch.uint8).fill_(byte)
    n = _lib.check(_lib.lib().cc_decode_part_floats(C.byref(sess.g.cfg), sess.R), "cc_decode_part_floats")
    sess._lpart = torch.empty(n, dtype=torch.float32, device=sess.kv.device)
    sess._lpart.view(torch.uint8).fill_(byte)
    return sess


@pytest.mark.parametrize("precision", ["bf16", 32], ids=str)
def test_decode_session_on_a_poisoned_cache(precision):
    """A short greedy decode and a short beam decode on S1's GPT-2 with the session's KV cache, _logits and _lpart filled with 0xFF after
    construction and before the first forward (and after the beam fan-out, beyond the copied prefix): same tokens, logits and scores as
    on zeroed ones.  The decode workspace is left exactly as DecodeSession allocates it."""
    from clipcap_amd.engine import DecodeSession, beam_buffers, beam_step, embed_tokens
    s = S1
    S, L0, steps, beam = 2, 4, 5, 3
    prefix = (0.5 * torch.randn(S, L0, s["D"], generator=torch.Generator().manual_seed(90))).to(DEV)

    def chain(byte):
        ge = _gpt2(s, precision)
        wte = ge.views(ge.arena.w32)["transformer.wte.weight"]
        V, D = s["V"], s["D"]
        out = {}
        # greedy
        sess = _poison_session(DecodeSession(ge, S, L0 + steps), byte)
        logits = sess.forward(prefix)
        x = torch.empty(S, 1, D, dtype=torch.float32, device=DEV)
        for i in range(steps):
            _keep(out, f"greedy logits {i}", logits)
            tok = logits.argmax(dim=-1).to(torch.int32)
            _keep(out, f"greedy token {i}", tok)
            if i + 1 < steps:
                logits = sess.forward(embed_tokens(ge, tok, x))
        # beam (the decoders' loop, inference/base.py generate_beam_rounds: prefill, fan out, one forward + update + advance per step)
        R = S * beam
        scores, seql, stopped = torch.zeros(R, device=DEV), torch.ones(R, device=DEV), torch.zeros(R, dtype=torch.uint8, device=DEV)
        sess = _poison_session(DecodeSession(ge, S, L0 + steps), byte)
        lg = torch.zeros(R, V, dtype=torch.float32, device=DEV)
        lg[::beam] = sess.forward(prefix)
        bufs = _fill_bufs(beam_buffers(DEV, S, beam, V), byte)
        nt, src = beam_step(lg, S, beam, 1.0, True, STOP, scores, seql, stopped, bufs)
        base = torch.arange(S, device=DEV, dtype=torch.int32).repeat_interleave(beam)
        sess = _poison_session(sess.expand(base, R), byte)
        tok = [torch.zeros(R, steps, dtype=torch.int32, device=DEV) for _ in range(2)]
        x = torch.empty(R, 1, D, dtype=torch.float32, device=DEV)
        sess.beam_advance(beam, nt, None, wte, 0, tok[1], tok[0], x)
        for n in range(1, steps):
            logits = sess.forward(x, partials=True, group=beam)
            _keep(out, f"beam logits {n}", logits)
            nt, src = beam_step(logits, S, beam, 1.0, False, STOP, scores, seql, stopped, bufs, sess.lpart)
            sess.beam_advance(beam, nt, src, wte, n, tok[(n - 1) & 1], tok[n & 1], x)
            _keep(out, f"beam scores {n}", scores)
            _keep(out, f"beam src {n}", src)
        _keep(out, "beam tokens", tok[(steps - 1) & 1])
        _keep(out, "beam lengths", seql)
        return out

    a, b = chain(0x00), chain(0xFF)
    _assert_finite(b, "decode on a 0xFF cache")
    _assert_same(a, b, f"decode {precision}: zeroed against 0xFF-filled cache, logits and partials")
