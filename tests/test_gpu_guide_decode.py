"""Classifier-free guidance in the beam and sampling decoders (clipcap_amd/inference/base.py), end to end on the beam_tiny golden model in
split-bf16 operands (precision 32, as tests/test_gpu_contrastive.py), against a guided beam search for one prefix on the CPU
(tests/guide_ref.guided_beam_search_ref: the oracle's full re-forward of both streams, the combination in float64, oracle.beam_update).

A search is compared only where the reference's smallest kept / rejected gap is at least (|g| + |1-g|) * 2e-3 — the suite's end-to-end
margin scaled by what guidance amplifies; every case below asserts that on the reference first.  negative_embeds = wte[50] (one
position), stop token 50, entry length 10.  The cases (tests/test_guide_ref.py pins them on the CPU) all move the caption off the unguided
one, and that is asserted too: a guided decoder that ignores the scale fails here.
"""
import pytest
import torch

from tests.guide_ref import guided_beam_search_ref
from tests.util import load_golden, sd_of

pytestmark = pytest.mark.gpu

STOP, ENTRY = 50, 10
BANS = dict(no_repeat_ngram_size=2, min_length=3)


def _margin_needed(g):
    return (abs(g) + abs(1 - g)) * 2e-3


def _score_tol(g):
    return (abs(g) + abs(1 - g)) * 1e-3


_MODELS = {}


def _tiny(precision=32, cases=("1", "3")):
    from types import SimpleNamespace
    from clipcap_amd.model.gpt2 import GPT2LM
    g = load_golden("beam_tiny")
    D, n_layer, n_head, V, npos = [int(v) for v in g["cfg"]]
    if precision not in _MODELS:
        lm = GPT2LM(n_embd=D, n_layer=n_layer, n_head=n_head, vocab_size=V, n_positions=npos, precision=precision)
        lm.load_state_dict(sd_of(g), strict=False)
        _MODELS[precision] = SimpleNamespace(language_model=lm.to("cuda"))
    sd = {"language_model." + k: v for k, v in sd_of(g).items()}
    pref = torch.cat([torch.from_numpy(g[f"beam{c}.prefix"]) for c in cases])
    neg = sd["language_model.transformer.wte.weight"][50].view(1, 1, -1).clone()
    return _MODELS[precision], sd, pref, neg, dict(n_head=n_head, n_layer=n_layer), V


_REFS = {}


def _reference(case, g, beam, neg_key="wte50", neg=None, **kw):
    """The CPU search of one case, computed once per configuration and shared; -> ([(tokens, scores, lengths) per round], margin)."""
    key = (case, g, beam, neg_key, tuple(sorted(kw.items())))
    if key not in _REFS:
        _, sd, pref, neg0, dims, _ = _tiny(32, (case,))
        _REFS[key] = guided_beam_search_ref(sd, pref, neg0 if neg is None else neg, scale=g, beam=beam, entry_length=ENTRY, stop_token=STOP, **dims, **kw)
    return _REFS[key]


def _assert_equals_reference(out, s, ref, g):
    """Prefix s of a device result (tokens (S, beam, n), scores, lengths) against one round of the CPU search."""
    toks, scores, lens = (t.cpu() for t in out)
    rt, rs, rl = ref
    assert torch.equal(lens[s].double(), rl.double()), (s, lens[s].tolist(), rl.tolist())
    for b in range(rt.shape[0]):
        n = int(rl[b])
        assert toks[s, b, :n].tolist() == rt[b, :n].tolist(), (s, b, toks[s, b].tolist(), rt[b].tolist())
    err = (scores[s].double() - rs.double()).abs().max().item()
    print(f"  prefix {s}: score error {err:.3e} (bar {_score_tol(g):.1e})")
    assert err <= _score_tol(g), (s, err)


def _best(toks, scores, lens, s=0):
    b = int(scores[s].argmax())
    return toks[s, b, :int(lens[s, b])].tolist()


@pytest.mark.parametrize("beam", [3, 1])
def test_guided_beam_search_equals_the_cpu_search(beam):
    from clipcap_amd.inference import generate_beam_tokens
    g = 3.0
    model, _, pref, neg, _, _ = _tiny(32)
    out = generate_beam_tokens(model, pref.cuda(), beam, ENTRY, 1.0, STOP, guidance_scale=g, negative_embeds=neg.cuda())
    plain = [t.cpu() for t in generate_beam_tokens(model, pref.cuda(), beam, ENTRY, 1.0, STOP)]
    for s, case in enumerate(("1", "3")):
        ref, margin = _reference(case, g, beam)
        print(f"case {case} beam {beam}: reference margin {margin:.3e}")
        assert margin >= _margin_needed(g), (case, margin)
        _assert_equals_reference(out, s, ref[0], g)
        if (beam, case) != (1, "3"):                                                    # (greedy on case 3 finds [14, 14, 14, 14, 50] either way)
            assert _best(*[t.cpu() for t in out], s) != _best(*plain, s), case         # guidance moved the caption
    assert _best(*[t.cpu() for t in out], 0) == [40, 1, 1, 1, 50] and _best(*plain, 0) == ([29, 29, 29, 29, 50] if beam == 3 else [40, 40, 40, 40, 50])


def test_guided_greedy_on_the_case_that_stops_at_once_unguided():
    from clipcap_amd.inference import generate_beam_tokens
    g = 1.5
    model, _, pref, neg, _, _ = _tiny(32, ("T",))
    out = generate_beam_tokens(model, pref.cuda(), 1, ENTRY, 1.0, STOP, guidance_scale=g, negative_embeds=neg.cuda())
    ref, margin = _reference("T", g, 1)
    assert margin >= _margin_needed(g), margin
    _assert_equals_reference(out, 0, ref[0], g)
    plain = [t.cpu() for t in generate_beam_tokens(model, pref.cuda(), 1, ENTRY, 1.0, STOP)]
    assert _best(*[t.cpu() for t in out]) == [29, 29, 29, 29, 50] and _best(*plain) == [50]


def _well_formed(toks, scores, lens, V):
    toks, scores, lens = toks.cpu(), scores.cpu(), lens.cpu()
    assert toks.min() >= 0 and toks.max() < V and torch.isfinite(scores).all()
    for s in range(toks.shape[0]):
        for b in range(toks.shape[1]):
            n = int(lens[s, b])
            seq = toks[s, b].tolist()
            assert 1 <= n <= toks.shape[2] and STOP not in seq[:n - 1], (s, b, seq, n)
            assert seq[n - 1] == STOP or n == toks.shape[2], (s, b, seq, n)


def _same_bits(a, b):
    return all(torch.equal(x.cpu(), y.cpu()) if not x.is_floating_point() else torch.equal(x.cpu().view(torch.int32), y.cpu().view(torch.int32))
               for x, y in zip(a, b))


def test_live_rounds_under_guidance():
    """generate_beam_rounds(rounds=2), beam 3, g = 3: the reference's margin holds over both rounds on both cases (3.4e-2 and 2.9e-2 against the
    1e-2 needed), so both rounds are compared with the CPU search; well-formedness and run-to-run bit identity besides."""
    from clipcap_amd.inference.base import generate_beam_rounds
    g = 3.0
    model, _, pref, neg, _, V = _tiny(32)
    run = lambda: generate_beam_rounds(model, pref.cuda(), 3, ENTRY, 1.0, STOP, 2, guidance_scale=g, negative_embeds=neg.cuda())  # noqa: E731
    out, again = run(), run()
    assert len(out) == 2
    for r in range(2):
        _well_formed(*out[r], V)
        assert _same_bits(out[r], again[r])
    for s, case in enumerate(("1", "3")):
        ref, margin = _reference(case, g, 3, rounds=2)
        print(f"rounds, case {case}: reference margin {margin:.3e}")
        assert margin >= _margin_needed(g), (case, margin)
        for r in range(2):
            _assert_equals_reference(out[r], s, ref[r], g)


def test_beam_groups_under_guidance():
    """num_beam_groups = 3, diversity_penalty = 1, beam 3, g = 3: the reference's margin holds on both cases (3.8e-2 and 2.9e-2), so the result
    is compared with the CPU search; well-formedness and run-to-run bit identity besides."""
    from clipcap_amd.inference import generate_beam_tokens
    g = 3.0
    model, _, pref, neg, _, V = _tiny(32)
    run = lambda: generate_beam_tokens(model, pref.cuda(), 3, ENTRY, 1.0, STOP, num_beam_groups=3, diversity_penalty=1.0, guidance_scale=g,  # noqa: E731
                                       negative_embeds=neg.cuda())
    out, again = run(), run()
    _well_formed(*out, V)
    assert _same_bits(out, again)
    for s, case in enumerate(("1", "3")):
        ref, margin = _reference(case, g, 3, groups=3, penalty=1.0)
        print(f"beam groups, case {case}: reference margin {margin:.3e}")
        assert margin >= _margin_needed(g), (case, margin)
        _assert_equals_reference(out, s, ref[0], g)


def test_sampling_with_one_candidate_is_the_guided_greedy_search():
    from clipcap_amd.inference.base import sample_tokens
    g = 3.0
    model, _, pref, neg, _, _ = _tiny(32)
    toks, stop_pos = (t.cpu() for t in sample_tokens(model, pref.cuda(), ENTRY, STOP, mode=0, top_k=1, top_p=0, guidance_scale=g,
                                                      negative_embeds=neg.cuda()))
    for s, case in enumerate(("1", "3")):
        ref, margin = _reference(case, g, 1)
        assert margin >= _margin_needed(g)
        rt, _, rl = ref[0]
        n = int(rl[0])
        assert int(rt[0, n - 1]) == STOP and int(stop_pos[s]) == n - 1
        assert toks[s, :n].tolist() == rt[0, :n].tolist(), (case, toks[s].tolist(), rt[0].tolist())


def test_bans_apply_after_the_combination():
    from clipcap_amd.inference import generate_beam_tokens
    g = 3.0
    model, _, pref, neg, _, _ = _tiny(32)
    out = generate_beam_tokens(model, pref.cuda(), 3, ENTRY, 1.0, STOP, guidance_scale=g, negative_embeds=neg.cuda(), **BANS)
    for s, case in enumerate(("1", "3")):
        ref, margin = _reference(case, g, 3, **BANS)
        print(f"bans, case {case}: reference margin {margin:.3e}")
        assert margin >= _margin_needed(g), (case, margin)
        _assert_equals_reference(out, s, ref[0], g)
        seq = _best(*[t.cpu() for t in out], s)
        assert STOP not in seq[:3] and len({tuple(seq[i:i + 2]) for i in range(len(seq) - 1)}) == len(seq) - 1, seq


def test_scale_one_is_the_unguided_decoder_and_makes_no_guidance_call(monkeypatch):
    from clipcap_amd import engine
    from clipcap_amd.inference.base import generate_beam_tokens, sample_tokens
    model, _, pref, neg, _, _ = _tiny(32)
    calls = []
    real = engine.guide_logits
    monkeypatch.setattr(engine, "guide_logits", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    a = generate_beam_tokens(model, pref.cuda(), 3, ENTRY, 1.0, STOP)
    b = generate_beam_tokens(model, pref.cuda(), 3, ENTRY, 1.0, STOP, guidance_scale=1.0, negative_embeds=neg.cuda())
    c = generate_beam_tokens(model, pref.cuda(), 3, ENTRY, 1.0, STOP, guidance_scale=1.0)
    assert _same_bits(a, b) and _same_bits(a, c)
    gen = lambda: torch.Generator(device="cuda").manual_seed(3)  # noqa: E731
    sa = sample_tokens(model, pref.cuda(), ENTRY, STOP, generator=gen())
    sb = sample_tokens(model, pref.cuda(), ENTRY, STOP, generator=gen(), guidance_scale=1.0, negative_embeds=neg.cuda())
    assert _same_bits(sa, sb)
    assert not calls
    generate_beam_tokens(model, pref.cuda(), 3, ENTRY, 1.0, STOP, guidance_scale=3.0, negative_embeds=neg.cuda())
    assert len(calls) >= 2                                                                 # the counter does see a guided decode


def test_guided_decodes_are_bit_identical_from_run_to_run_and_broadcast_the_negative_context():
    from clipcap_amd.inference import generate_beam_tokens
    model, _, pref, neg, _, _ = _tiny(32)
    run = lambda n: generate_beam_tokens(model, pref.cuda(), 3, ENTRY, 1.0, STOP, guidance_scale=3.0, negative_embeds=n.cuda(), **BANS)  # noqa: E731
    a, b = run(neg), run(neg)
    assert _same_bits(a, b)
    assert _same_bits(a, run(neg.expand(pref.shape[0], -1, -1).contiguous()))              # (1, Ln, D) and (S, Ln, D) with equal rows


def test_a_negative_context_of_three_positions():
    """Ln = 3 on case 1.  The context wte[50, 29, 40] was chosen on the CPU among five tried for the reference's margin (1.1e-1; wte[50, 7, 21]
    leaves 2.9e-3, below the condition); it also changes the caption, to [16, 1, 1, 1, 50]: the second stream's own positions matter."""
    from clipcap_amd.inference import generate_beam_tokens
    g = 3.0
    model, sd, pref, _, _, _ = _tiny(32, ("1",))
    neg3 = sd["language_model.transformer.wte.weight"][[50, 29, 40]].view(1, 3, -1).clone()
    ref, margin = _reference("1", g, 3, neg_key="wte50-29-40", neg=neg3)
    print(f"Ln = 3: reference margin {margin:.3e}")
    assert margin >= _margin_needed(g), margin
    out = generate_beam_tokens(model, pref.cuda(), 3, ENTRY, 1.0, STOP, guidance_scale=g, negative_embeds=neg3.cuda())
    _assert_equals_reference(out, 0, ref[0], g)
    assert _best(*[t.cpu() for t in out]) == [16, 1, 1, 1, 50]


def test_guided_decode_in_bf16_operands_is_well_formed():
    from clipcap_amd.inference import generate_beam_tokens
    model, _, pref, neg, _, V = _tiny("bf16")
    out = generate_beam_tokens(model, pref.cuda(), 3, ENTRY, 1.0, STOP, guidance_scale=3.0, negative_embeds=neg.cuda())
    _well_formed(*out, V)
    assert _same_bits(out, generate_beam_tokens(model, pref.cuda(), 3, ENTRY, 1.0, STOP, guidance_scale=3.0, negative_embeds=neg.cuda()))


def test_tokenizer_level_decoders_build_the_default_negative_context():
    """generate_beam and generate_nucleus_sampling under guidance with negative_embeds = None: the texts are those of the token-level
    decoders given the bos embedding (followed by the text prefix, as the prefix is) as the unconditional context."""
    from tests.test_api_surface import FakeTokenizer
    from clipcap_amd.inference import generate_beam, generate_beam_tokens, generate_nucleus_sampling
    from clipcap_amd.inference.base import sample_tokens
    g = 3.0
    model, sd, pref, _, _, V = _tiny(32)
    tk = FakeTokenizer(V, STOP)
    wte = sd["language_model.transformer.wte.weight"]
    bos = wte[tk.encode(tk.bos_token)[0]].view(1, 1, -1)
    texts = generate_beam(model, tk, pref.cuda(), beam_size=3, entry_length=ENTRY, guidance_scale=g)
    toks, scores, lens = (t.cpu() for t in generate_beam_tokens(model, pref.cuda(), 3, ENTRY, 1.0, STOP, guidance_scale=g, negative_embeds=bos.cuda()))
    assert texts == [tk.decode(_best(toks, scores, lens, s)) for s in range(pref.shape[0])]
    assert texts != generate_beam(model, tk, pref.cuda(), beam_size=3, entry_length=ENTRY)
    head = torch.tensor([[7, 9]])
    texts = generate_nucleus_sampling(model, tk, pref.cuda(), number_to_generate=2, text_prefix_tokens=head.cuda(), entry_length=ENTRY, top_k=1,
                                      guidance_scale=g)
    with_head = lambda e: torch.cat((e, wte[head[0]].view(1, 2, -1).expand(e.shape[0], -1, -1)), dim=1)  # noqa: E731
    st, sp = (t.cpu() for t in sample_tokens(model, with_head(pref).repeat_interleave(2, dim=0).cuda(), ENTRY, STOP, mode=0, top_p=0.8, top_k=1,
                                              guidance_scale=g, negative_embeds=with_head(bos).cuda()))
    assert texts == [tk.decode([7, 9] + st[r, :min(int(sp[r]) + 1, st.shape[1])].tolist()) for r in range(4)]
