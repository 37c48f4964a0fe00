"""Caption scoring on the GPU: ClipCapEngine.score / cc_lmhead_score (forward-only pass, store-free lm_head epilogue, per-sample fold)
and its public surface (clipcap_amd.inference.score_captions / rerank_captions, generate_nucleus_sampling(rerank=), clipcap_amd.train.evaluate).

Yardsticks: the CPU oracle with the operand mode's rounding points; the route to the same numbers that existed before scoring
(ClipCapModel.forward(...).logits + torch log_softmax / gather), measured in the same test; and the training loss of
ClipCapEngine.forward_backward, whose objective scoring with ignore_zero reproduces."""
import os

import numpy as np
import pytest
import torch

from oracle import clipcap_oracle as O
from tests.util import load_golden, sd_of, seeded_full_model

pytestmark = pytest.mark.gpu

PRECISIONS = ["bf16", 16, 32]
RB = {"bf16": True, 16: "fp16", 32: "bf16x3"}                 # the oracle's rounding points per operand mode
LOSS_TOL = {"bf16": 2e-3, 16: 5e-3, 32: 2e-5}                # the project's per-mode loss bounds


def _tiny_model(precision, mode="prefix_only"):
    from clipcap_amd.encoders import EncoderConfig
    from clipcap_amd.model import ClipCapModel, ClipCapModelPrefixOnly, Config, TrainingConfig
    from clipcap_amd.model.gpt2 import GPT2LM
    g = load_golden(f"train_{mode}")
    E, D, P, L, H, N, n_head, n_layer, V, npos = [int(v) for v in g["cfg"]]
    lm = GPT2LM(n_embd=D, n_layer=n_layer, n_head=n_head, vocab_size=V, n_positions=npos, embd_pdrop=0.0, attn_pdrop=0.0, resid_pdrop=0.0)
    cfg = Config(language_model="unused", train_language_model=(mode == "full"), prefix_length=L, projection_length=P, transformer_layers=N,
                 transformer_attention_heads=H, encoder_config=EncoderConfig(encoder_embedding_size=E),
                 training_config=TrainingConfig(optimizer_lr=1e-3, use_deepspeed_optimisers=False, scheduler_warmup_steps=2, total_steps=6))
    m = (ClipCapModel if mode == "full" else ClipCapModelPrefixOnly)(cfg, language_model=lm)
    m.load_state_dict(sd_of(g), strict=True)
    m = m.set_precision(precision).to("cuda")
    m.eval()
    dims = dict(E=E, D=D, P=P, L=L, H=H, N=N, n_head=n_head, n_layer=n_layer, V=V, npos=npos)
    ocfg = dict(projection_length=P, prefix_length=L, heads=H, layers=N, n_head=n_head, n_layer=n_layer)
    return m, g, dims, ocfg


def _fixture_batch(g):
    """The training fixture's batch: ragged captions, -1 pads, and a row with an explicit token 0."""
    tokens, embeds = torch.from_numpy(g["in.tokens"]), torch.from_numpy(g["in.embeds"])
    assert (tokens == 0).any() and (tokens < 0).any() and (tokens >= 0).sum(dim=1).unique().numel() > 1
    return tokens, embeds


def _random_batch(B, cap, V, E, seed):
    gen = torch.Generator().manual_seed(seed)
    tokens = torch.randint(1, V, (B, cap), generator=gen)
    lengths = torch.randint(1, cap + 1, (B,), generator=gen)
    tokens[torch.arange(cap).view(1, -1) >= lengths.view(-1, 1)] = -1
    tokens[::7, 0] = 0                                        # explicit token 0 inside captions
    return tokens, torch.randn(B, E, generator=gen)


def _gathered(logits, tokens, L):
    """log_softmax(logits[:, L-1:-1]) at the tokens (pads read position 0; callers mask them)."""
    return torch.log_softmax(logits[:, L - 1:-1].float(), dim=-1).gather(2, tokens.clamp_min(0).unsqueeze(-1)).squeeze(-1)


def _errors_vs_oracle(m, g, dims, ocfg, precision, tokens, embeds):
    """(max error of the scoring pass, max error of the logits + torch route, scores) against the oracle at the kept positions."""
    from clipcap_amd.inference import score_captions
    L = dims["L"]
    kept = tokens >= 0
    with torch.no_grad():
        ref = _gathered(O.clipcap_logits(sd_of(g), tokens.clamp_min(0), embeds, cfg=ocfg, rb=RB[precision]), tokens, L)
        s = score_captions(m, embeds.cuda(), tokens.cuda())
        old = _gathered(m(tokens.clamp_min(0).cuda(), embeds.cuda(), kept.cuda()).logits, tokens.cuda(), L)
    e_new = float((s.token_logprobs.cpu() - ref)[kept].abs().max())
    e_old = float((old.cpu() - ref)[kept].abs().max())
    return e_new, e_old, s


@pytest.mark.parametrize("precision", PRECISIONS)
def test_token_logprobs_against_the_oracle(precision):
    """The scoring pass is at most twice as far from the oracle as the logits + log_softmax + gather route: both read the same fp32
    accumulators, the factor covers the different fold order of the 64-column partials."""
    m, g, dims, ocfg = _tiny_model(precision)
    tokens, embeds = _fixture_batch(g)
    e_new, e_old, s = _errors_vs_oracle(m, g, dims, ocfg, precision, tokens, embeds)
    print(f"score vs oracle ({precision}): scoring pass {e_new:.3e}, logits + torch route {e_old:.3e}")
    assert s.token_logprobs.shape == tokens.shape and s.logprob.shape == s.num_tokens.shape == (tokens.shape[0],)
    assert s.token_logprobs.is_cuda and s.token_logprobs.dtype == torch.float32
    assert e_new <= 2.0 * e_old, (e_new, e_old)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_ignore_zero_reproduces_the_training_loss_tiny(precision):
    from clipcap_amd.inference import score_captions
    m, g, dims, _ = _tiny_model(precision)
    tokens, embeds = _fixture_batch(g)
    loss = float(m.engine.forward_backward(tokens.cuda(), embeds.cuda(), backward=False))
    s = score_captions(m, embeds.cuda(), tokens.cuda(), ignore_zero=True)
    mine = float(-s.logprob.sum() / s.num_tokens.sum())
    print(f"tiny ({precision}): -sum logprob / tokens {mine:.7f}, training loss {loss:.7f}, diff {abs(mine - loss):.3e}")
    assert int(s.num_tokens.sum()) == int((tokens > 0).sum())
    assert abs(mine - loss) <= LOSS_TOL[precision], (mine, loss)


@pytest.fixture(scope="module")
def small_engines():
    """GPT-2-small width (config2_full's seeded parameters), built once for the three precisions."""
    from clipcap_amd.engine import ClipCapEngine, Gpt2Engine, MapperEngine
    sd, _, dims = seeded_full_model(load_golden("config2_full"))
    me = MapperEngine(dims["E"], dims["D"], dims["L"], dims["P"], dims["H"], dims["N"], device="cuda")
    ge = Gpt2Engine(dims["D"], dims["n_head"], dims["NL"], dims["V"], dims["NPOS"], device="cuda")
    for pre, eng in (("transformer_mapper.", me), ("language_model.", ge)):
        for k, v in eng.views(eng.arena.w32).items():
            v.copy_(sd[pre + k])
    del sd
    yield me, ge, dims
    del me, ge
    torch.cuda.empty_cache()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_ignore_zero_reproduces_the_training_loss_gpt2_small_b256(small_engines, precision):
    """B = 256, cap = 40 (10 240 lm_head rows x 50 304 columns: the 320 x 256 tile kernel with the store-free epilogue)."""
    from clipcap_amd.engine import ClipCapEngine
    me, ge, dims = small_engines
    me.set_precision(precision)
    ge.set_precision(precision)
    eng = ClipCapEngine(me, ge, train_lm=False)
    tokens, embeds = _random_batch(256, 40, dims["V"], dims["E"], seed=40)
    tokens, embeds = tokens.cuda(), embeds.cuda()
    loss = float(eng.forward_backward(tokens, embeds, backward=False))
    ge._ws.clear()                                             # the training workspace is not needed any more
    lp, ssum, cnt = eng.score(tokens, embeds, ignore_zero=True)
    mine = float(-ssum.sum() / cnt.sum())
    print(f"GPT-2 small B=256 cap=40 ({precision}): -sum logprob / tokens {mine:.7f}, training loss {loss:.7f}, diff {abs(mine - loss):.3e}")
    assert int(cnt.sum()) == int((tokens > 0).sum()) and bool(torch.isfinite(lp).all())
    assert abs(mine - loss) <= LOSS_TOL[precision], (mine, loss)
    eng._score_ws = None


@pytest.mark.parametrize("precision", PRECISIONS)
def test_mask_semantics_and_causality(precision):
    from clipcap_amd.inference import score_captions
    m, g, dims, ocfg = _tiny_model(precision)
    tokens, embeds = _fixture_batch(g)
    _, e_old, s = _errors_vs_oracle(m, g, dims, ocfg, precision, tokens, embeds)
    bound = 2.0 * e_old                                        # the bound of test_token_logprobs_against_the_oracle
    for flag, kept in ((False, tokens >= 0), (True, tokens > 0)):
        r = score_captions(m, embeds.cuda(), tokens.cuda(), ignore_zero=flag)
        lp = r.token_logprobs.cpu()
        assert bool((lp[~kept] == 0.0).all()), "dropped positions read exactly 0"
        assert bool((lp[kept] < 0.0).all()), "kept positions hold a log-probability"
        assert torch.equal(r.num_tokens.cpu(), kept.sum(dim=1).float())
        assert torch.equal(lp[kept], s.token_logprobs.cpu()[kept])      # the flag only masks: the kept values are the same numbers
        assert torch.allclose(r.logprob.cpu(), lp.sum(dim=1), rtol=1e-6, atol=1e-6)
    # a longer -1 tail (larger cap) leaves the kept positions' values where they were: the pass is causal
    wide = torch.cat((tokens, torch.full((tokens.shape[0], 5), -1, dtype=torch.int64)), dim=1)
    w = score_captions(m, embeds.cuda(), wide.cuda())
    kept = tokens >= 0
    d = float((w.token_logprobs.cpu()[:, : tokens.shape[1]] - s.token_logprobs.cpu())[kept].abs().max())
    print(f"causality ({precision}): max change of kept log-probs under 5 more pad columns {d:.3e} (bound {bound:.3e})")
    assert bool((w.token_logprobs.cpu()[:, tokens.shape[1]:] == 0.0).all()) and torch.equal(w.num_tokens, s.num_tokens)
    assert d <= bound


@pytest.mark.parametrize("precision", PRECISIONS)
def test_scoring_is_bit_reproducible(precision):
    m, g, dims, _ = _tiny_model(precision)
    tokens, embeds = _random_batch(37, 9, dims["V"], dims["E"], seed=3)
    tokens, embeds = tokens.cuda(), embeds.cuda()
    a = [t.clone() for t in m.engine.score(tokens, embeds)]
    b = [t.clone() for t in m.engine.score(tokens, embeds)]
    m.engine.zero_grad()
    m.engine.forward_backward(tokens, embeds)
    c = m.engine.score(tokens, embeds)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_scoring_between_backward_and_optimizer_step_changes_nothing(precision):
    """forward_backward -> score -> optimizer_step leaves the parameters and engine.stats bit-identical to the step without the score call."""
    results = []
    for with_score in (False, True):
        m, g, dims, _ = _tiny_model(precision, "full")
        m.train()
        tokens, embeds = _fixture_batch(g)
        tokens, embeds = tokens.cuda(), embeds.cuda()
        eng = m.engine
        eng.zero_grad()
        loss = eng.forward_backward(tokens, embeds).clone()
        stats = eng.stats.clone()
        if with_score:
            other = _random_batch(6, 11, dims["V"], dims["E"], seed=9)
            eng.score(other[0].cuda(), other[1].cuda(), ignore_zero=True)
            assert torch.equal(eng.stats, stats), "engine.stats belongs to the training step"
        eng.optimizer_step(1e-3, 1)
        torch.cuda.synchronize()
        results.append((loss, eng.stats.clone(), m.transformer_mapper.engine.arena.w32.clone(), m.language_model.engine.arena.w32.clone(),
                        m.transformer_mapper.engine.arena.g32.clone(), m.language_model.engine.arena.g32.clone()))
    for x, y in zip(*results):
        assert torch.equal(x, y)
    assert not torch.equal(results[0][3], torch.zeros_like(results[0][3]))


def test_scoring_between_a_saved_mapper_forward_and_its_backward():
    """score(embeds=...) runs the mapper without saving: the activations and the input a forward(save=True) holds for backward stay."""
    grads = []
    for with_score in (False, True):
        m, g, dims, _ = _tiny_model("bf16")
        tokens, embeds = _fixture_batch(g)
        me = m.transformer_mapper.engine
        x = embeds.cuda().clone()
        out = me.forward(x, save=True)
        held = me._last
        del x
        if with_score:
            other = _random_batch(9, 5, dims["V"], dims["E"], seed=2)
            m.engine.score(other[0].cuda(), other[1].cuda(), chunk=4)
            assert me._last is held
        me.arena.grads().zero_()
        me.backward(torch.ones_like(out))
        grads.append(me.arena.g32.clone())
    assert torch.equal(grads[0], grads[1]) and float(grads[0].abs().max()) > 0


@pytest.mark.parametrize("precision", PRECISIONS)
def test_chunked_scoring_equals_one_call(precision):
    m, g, dims, ocfg = _tiny_model(precision)
    tokens, embeds = _fixture_batch(g)
    _, e_old, _ = _errors_vs_oracle(m, g, dims, ocfg, precision, tokens, embeds)
    bound = 2.0 * e_old
    tokens, embeds = _random_batch(256, 8, dims["V"], dims["E"], seed=5)
    tokens, embeds = tokens.cuda(), embeds.cuda()
    one = m.engine.score(tokens, embeds)
    ws_one = m.engine._score_ws.numel()
    m.engine._score_ws = None
    four = m.engine.score(tokens, embeds, chunk=64)
    assert m.engine._score_ws.numel() < ws_one, "a chunk's workspace is smaller than the whole batch's"
    d = float((one[0] - four[0]).abs().max())
    print(f"chunk = 64 over B = 256 ({precision}): max |diff| of token log-probs {d:.3e} (bound {bound:.3e})")
    assert d <= bound
    assert torch.equal(one[2], four[2])
    assert float((one[1] - four[1]).abs().max()) <= bound * tokens.shape[1]
    ragged = m.engine.score(tokens[:100], embeds[:100], chunk=64)          # a last chunk of another size
    assert float((ragged[0] - one[0][:100]).abs().max()) <= bound


@pytest.mark.parametrize("precision", PRECISIONS)
def test_text_prefix_and_from_prefix(precision):
    from clipcap_amd.inference import score_captions
    m, g, dims, _ = _tiny_model(precision)
    tokens, embeds = _fixture_batch(g)
    tokens, embeds = tokens.cuda(), embeds.cuda()
    t = torch.tensor([[5, 17, 3]])
    a = score_captions(m, embeds, tokens, text_prefix_tokens=t)
    with torch.no_grad():
        mapped = m.transformer_mapper(embeds)
        wte = m.language_model.get_input_embeddings().weight.detach()
        by_hand = torch.cat((mapped, wte[t.cuda()].expand(tokens.shape[0], -1, -1)), dim=1)
    b = score_captions(m, by_hand, tokens, from_prefix=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    plain = score_captions(m, embeds, tokens)
    assert not torch.equal(plain.token_logprobs, a.token_logprobs), "the text prefix conditions the caption"
    c = score_captions(m, mapped, tokens, from_prefix=True)                # from_prefix alone == scoring from the embeddings
    for x, y in zip(plain, c):
        assert torch.equal(x, y)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_rerank_orders_by_length_normalised_likelihood(precision):
    from clipcap_amd.inference import rerank_captions, score_captions
    m, g, dims, _ = _tiny_model(precision)
    B, N, n = 3, 5, 7
    gen = torch.Generator().manual_seed(12)
    cand = torch.randint(1, dims["V"], (B, N, n), generator=gen)
    lengths = torch.randint(2, n + 1, (B, N), generator=gen)
    cand[torch.arange(n).view(1, 1, -1) >= lengths.unsqueeze(-1)] = -1
    with torch.no_grad():
        prefix = m.transformer_mapper(torch.from_numpy(g["in.embeds"])[:B].cuda())
    order, scores = rerank_captions(m, prefix, cand.cuda())
    s = score_captions(m, prefix.repeat_interleave(N, dim=0), cand.view(B * N, n).cuda(), from_prefix=True)
    assert torch.equal(s.num_tokens.cpu().view(B, N), lengths.float())
    assert torch.equal(scores, (s.logprob / s.num_tokens).view(B, N))
    assert torch.equal(order, torch.argsort(scores, dim=1, descending=True, stable=True))
    assert bool((scores.gather(1, order).diff(dim=1) <= 0).all())
    order_raw, raw = rerank_captions(m, prefix, cand.cuda(), length_normalise=False)
    assert torch.equal(raw, s.logprob.view(B, N)) and bool((raw.gather(1, order_raw).diff(dim=1) <= 0).all())


@pytest.mark.parametrize("precision", PRECISIONS)
def test_beam_scores_are_the_beams_likelihoods(precision):
    """generate_beam_tokens accumulates log-softmax of KV-cached logits; scoring re-forwards the whole sequence.  Bound, written down before
    any run: the decode tests hold KV-cached logits to 4 x tol x max(1, |logits|) of the re-forward, tol = 2e-3 with 16-bit operands and
    1e-4 with split-bf16 operands (tests/test_gpu_decode_group.py; tests/test_gpu_beam.py itself only bounds the beam update on given
    logits, to 3e-5); a log-softmax moves by at most twice the largest logit change, and a beam sums one such term per token.  The
    logit scale is taken over every position of every beam's re-forwarded sequence."""
    from clipcap_amd.inference import generate_beam_tokens, rerank_captions, score_captions
    m, g, dims, _ = _tiny_model(precision)
    S, beam, stop = 3, 4, 11
    tol = 1e-4 if precision == 32 else 2e-3
    with torch.no_grad():
        prefix = m.transformer_mapper(torch.from_numpy(g["in.embeds"])[:S].cuda())
        toks, scores, lengths = generate_beam_tokens(m, prefix, beam_size=beam, entry_length=12, temperature=1.0, stop_token=stop)
        n = toks.shape[2]
        cand = torch.where(torch.arange(n, device=toks.device).view(1, 1, -1) < lengths.unsqueeze(-1), toks, torch.full_like(toks, -1))
        rows = prefix.repeat_interleave(beam, dim=0)
        s = score_captions(m, rows, cand.view(S * beam, n), from_prefix=True)
        wte = m.language_model.get_input_embeddings().weight.detach()
        scale = max(1.0, float(m.language_model.engine.logits(torch.cat((rows, wte[toks.view(S * beam, n)]), dim=1)).abs().max()))
    assert torch.equal(s.num_tokens.view(S, beam), lengths)
    want = scores * lengths
    d = (s.logprob.view(S, beam) - want).abs()
    per_token = 2.0 * 4 * tol * scale
    bound = lengths * per_token
    print(f"beam ({precision}): max |logprob - scores x lengths| {float(d.max()):.3e} (bound {float(bound.min()):.3e} .. {float(bound.max()):.3e}, "
          f"logit scale {scale:.2f})")
    assert bool((d <= bound).all()), (d, bound)
    order, norm = rerank_captions(m, prefix, cand)
    assert float((norm - scores).abs().max()) <= per_token


def test_generate_nucleus_sampling_rerank():
    """rerank=False: the tokens sample_tokens draws with the same generator, in sampling order; rerank=True: the same texts per prefix
    row, ordered by rerank_captions' score."""
    from clipcap_amd.inference import generate_nucleus_sampling, rerank_captions
    from clipcap_amd.inference.base import _rows_for, sample_tokens
    from tests.test_api_surface import FakeTokenizer
    m, g, dims, _ = _tiny_model("bf16")
    tok = FakeTokenizer(vocab=dims["V"], eos=5)
    S, N, n = 2, 4, 10
    with torch.no_grad():
        prefix = m.transformer_mapper(torch.from_numpy(g["in.embeds"])[:S].cuda())

    def gen():
        return torch.Generator(device="cuda").manual_seed(77)
    toks, stop_pos = sample_tokens(m, _rows_for(prefix, N), n, 5, mode=0, top_p=0.8, top_k=None, temperature=1.0, generator=gen())
    texts = [tok.decode(toks[r, :min(int(stop_pos[r]) + 1, toks.shape[1])].tolist()) for r in range(S * N)]
    assert generate_nucleus_sampling(m, tok, prefix, number_to_generate=N, entry_length=n, generator=gen()) == texts
    assert generate_nucleus_sampling(m, tok, prefix, number_to_generate=N, entry_length=n, generator=gen(), rerank=False) == texts
    ranked = generate_nucleus_sampling(m, tok, prefix, number_to_generate=N, entry_length=n, generator=gen(), rerank=True)
    keep = torch.arange(toks.shape[1], device="cuda").view(1, -1) <= stop_pos.view(-1, 1)
    cand = torch.where(keep, toks, torch.full_like(toks, -1)).view(S, N, -1)
    order, scores = rerank_captions(m, prefix, cand)
    assert ranked == [texts[s * N + int(j)] for s in range(S) for j in order[s]]
    assert len(set(map(float, scores.flatten()))) > 1


@pytest.mark.parametrize("precision", PRECISIONS)
def test_evaluate_is_the_token_weighted_training_loss(tmp_path, precision):
    pa = pytest.importorskip("pyarrow")
    import pyarrow.parquet as pq
    from clipcap_amd.train import evaluate
    from clipcap_amd.train.dataloader import DevicePrefetcher, get_dataloader

    class Tok:
        def encode(self, c):
            p = c.split()
            return [int(p[1])] + [7] * (len(p) - 2)

    m, g, dims, _ = _tiny_model(precision)
    cnt, E = 150, dims["E"]
    os.makedirs(tmp_path / "embeddings")
    os.makedirs(tmp_path / "captions")
    np.save(tmp_path / "embeddings" / "e000.npy", np.random.default_rng(0).standard_normal((cnt, E)).astype(np.float32))
    pq.write_table(pa.table({"caption": [f"cap {i} " + "w " * (i % 9) for i in range(cnt)]}), tmp_path / "captions" / "c000.parquet")
    out = evaluate(m, str(tmp_path), batch_size=64, tokenizer=Tok(), max_token_length=16)
    ds, _ = get_dataloader(str(tmp_path), "unused", 64, tokenizer=Tok(), max_token_length=16)
    tot, n, batches = 0.0, 0.0, 0
    for tokens, embeds in DevicePrefetcher(ds, "cuda"):
        loss = float(m.engine.forward_backward(tokens, embeds, backward=False))
        k = float(m.engine.stats[1])
        tot += loss * k
        n += k
        batches += 1
    ds.close()
    print(f"evaluate ({precision}): loss {out['loss']:.7f} over {out['tokens']} tokens; training-loss mean {tot / n:.7f}")
    assert batches == 3 and out["tokens"] == int(n) > 0
    assert abs(out["loss"] - tot / n) <= LOSS_TOL[precision]
    assert abs(out["perplexity"] - float(np.exp(out["loss"]))) <= 1e-6 * out["perplexity"]
    first = evaluate(m, str(tmp_path), batch_size=64, max_batches=1, tokenizer=Tok(), max_token_length=16)
    assert 0 < first["tokens"] < out["tokens"]
