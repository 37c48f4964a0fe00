"""CPU side of lexically constrained beam search (inference/lexical.py): cc_beam_lex_step and cc_beam_lex_ws_bytes are declared, bound and
exported under ABI version 3; their argument errors need no device; the decoders take the options keyword-only; the phrase validation
errors; the order and the cut of the returned texts on a stubbed search."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"cc_beam_lex_ws_bytes": 4, "cc_beam_lex_step": 19}


def _declared(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clipcap_hip.h")).read(), flags=re.S)
    m = re.search(r"^(int|int64_t)\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr, flags=re.M)
    assert m, f"{name} is not declared in include/clipcap_hip.h"
    return m.group(1), [p.strip() for p in " ".join(m.group(2).split()).split(",")]


@pytest.mark.parametrize("name", sorted(NAMES))
def test_header_binding_and_library_carry_the_entry_point(name):
    from clipcap_amd import _lib
    ret, params = _declared(name)
    assert len(params) == NAMES[name]
    res, args = _lib.SIGNATURES[name]
    assert res is (_lib._L if ret == "int64_t" else _lib._I) and len(args) == len(params)
    for p, a in zip(params, args):
        want = _lib._P if "*" in p else _lib._L if p.startswith("int64_t") else _lib._F if p.startswith("float") else _lib._I
        assert a is want, (p, a)
    l = _lib.lib()
    assert hasattr(l, name) and l.cc_abi_version() == 3 and _lib.ABI_VERSION == 3


def test_step_signature_is_the_documented_one():
    _, params = _declared("cc_beam_lex_step")
    assert [p.split()[-1].lstrip("*") for p in params] == ["S", "beam", "V", "logits", "ldl", "temperature", "first", "stop_token", "phrases", "n_phr",
                                                          "phr_len", "scores", "seq_lengths", "has_stopped", "lex_state", "next_tokens", "src_rows",
                                                          "ws", "stream"]
    _, params = _declared("cc_beam_lex_ws_bytes")
    assert [p.split()[-1] for p in params] == ["S", "beam", "n_phr", "V"]


def test_generated_abi_files_are_current_and_name_them():
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_abi.py"), "--check"]).returncode == 0
    csrc = os.path.join(ROOT, "clipcap_amd", "csrc")
    for f in ("abi_dispatch.cpp", "exports.map", "exports_lab.map"):
        text = open(os.path.join(csrc, f)).read()
        for name in NAMES:
            assert name in text, (f, name)
    # built once, like beam.hip and gumbel.hip: no per-operand-type variants are declared
    disp = open(os.path.join(csrc, "abi_dispatch.cpp")).read()
    for name in NAMES:
        assert name + "_bf16" in disp and name + "_f16" not in disp and name + "_x3" not in disp
    mk = open(os.path.join(csrc, "Makefile")).read()
    once = re.search(r"^SRCS_ONCE\s*=(.*)$", mk, flags=re.M).group(1).split()
    hdrs = re.search(r"^HDRS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "lexbeam.hip" in once and "lex_state.h" in hdrs and "beam.hip.h" in hdrs


def test_argument_errors_need_no_device():
    """The argument checks come before anything touches the device: error codes for bad arguments with pointers that are never followed."""
    from clipcap_amd import _lib
    f = _lib.lib().cc_beam_lex_step
    ptr = [C.c_void_p(4096 * (i + 1)) for i in range(9)]

    def call(S=2, beam=6, V=130, logits=ptr[0], ldl=136, temp=1.0, first=0, stop=5, phrases=ptr[1], n_phr=3, phr_len=4, scores=ptr[2], seql=ptr[3],
             stopped=ptr[4], state=ptr[5], nt=ptr[6], src=ptr[7], ws=ptr[8]):
        return f(S, beam, V, logits, ldl, temp, first, stop, phrases, n_phr, phr_len, scores, seql, stopped, state, nt, src, ws, None)

    for kw in (dict(logits=None), dict(phrases=None), dict(scores=None), dict(seql=None), dict(stopped=None), dict(state=None), dict(nt=None),
               dict(src=None), dict(ws=None)):
        assert call(**kw) == -1, kw
    assert call(S=-1) == -1
    assert call(beam=0) == -1 and call(beam=17) == -1 and call(beam=-3) == -1
    assert call(V=0, ldl=0) == -1 and call(V=-1) == -1
    assert call(ldl=129) == -1
    assert call(n_phr=-1) == -1 and call(n_phr=9) == -1
    assert call(phr_len=0) == -1 and call(phr_len=9) == -1 and call(phr_len=-1) == -1
    assert call(temp=float("nan")) == -1
    assert call(V=2097153, ldl=2097160) == -2                                   # CC_ERR_SHAPE
    assert call(V=2097153, ldl=2097160, beam=17) == -1                          # an argument error comes first
    # S == 0: ok, and nothing is launched (there is no device here to launch on); without phrases neither the table nor phr_len is looked at
    assert call(S=0) == 0 and call(S=0, n_phr=0, phrases=None, phr_len=0) == 0 and call(S=0, n_phr=8, phr_len=8, beam=16) == 0
    assert call(S=0, n_phr=0, phrases=None, phr_len=99) == 0
    assert call(S=0, temp=0.0) == 0 and call(S=0, temp=-1.0) == 0               # a temperature <= 0 means 1, as in cc_beam_step
    w = _lib.lib().cc_beam_lex_ws_bytes
    assert w(-1, 6, 3, 130) < 0 and w(2, 0, 3, 130) < 0 and w(2, 17, 3, 130) < 0 and w(2, 6, -1, 130) < 0 and w(2, 6, 9, 130) < 0
    assert w(2, 6, 3, 0) < 0 and w(2, 6, 3, 2097153) == -2
    assert w(0, 6, 3, 130) >= 0
    # the row statistics and, per parent row, beam + n_phr + 1 (value, token) pairs: no smaller than that, and monotone in beam and n_phr
    assert w(3, 6, 3, 50257) >= 3 * 6 * 8 + 3 * 6 * (6 + 3 + 1) * 8
    for n_phr in range(9):
        assert all(w(3, b, n_phr, 50257) < w(3, b + 1, n_phr, 50257) for b in range(1, 16))
    for beam in range(1, 17):
        assert all(w(3, beam, n, 50257) < w(3, beam, n + 1, 50257) for n in range(8))


OPTIONS = [("no_repeat_ngram_size", 0), ("min_length", 0), ("suppress_tokens", None), ("guidance_scale", 1.0), ("negative_embeds", None)]


@pytest.mark.parametrize("fn", ["generate_constrained_beam_tokens", "generate_constrained_beam"])
def test_decoders_take_the_options_keyword_only(fn):
    from clipcap_amd import inference
    from clipcap_amd.inference import lexical
    assert getattr(inference, fn) is getattr(lexical, fn)
    p = inspect.signature(getattr(lexical, fn)).parameters
    for k, d in OPTIONS + ([("num_return_sequences", 1)] if fn == "generate_constrained_beam" else []):
        assert k in p, (fn, k)
        assert p[k].kind is inspect.Parameter.KEYWORD_ONLY and p[k].default == d and type(p[k].default) is type(d), (fn, k)
    names = list(p)
    if fn == "generate_constrained_beam_tokens":
        assert names[:7] == ["model", "embeds", "phrases", "beam_size", "entry_length", "temperature", "stop_token"]
        assert [p[k].default for k in names[3:7]] == [5, 67, 1.0, 50256] and "num_return_sequences" not in p
    else:
        assert names[:8] == ["model", "tokenizer", "embeds", "force_words", "text_prefix_tokens", "beam_size", "entry_length", "temperature"]
        assert [p[k].default for k in names[4:8]] == [None, 5, 67, 1.0]
        assert "leading space" in lexical.generate_constrained_beam.__doc__
    assert inference.ConstrainedBeams._fields == ("tokens", "scores", "seq_lengths", "tokens_met", "all_met")
    assert inference.best_constrained_beams is lexical.best_constrained_beams


def test_engine_wrappers_have_the_documented_signatures():
    from clipcap_amd import engine
    assert list(inspect.signature(engine.beam_lex_step).parameters) == ["logits", "samples", "beam", "temperature", "first", "stop_token", "scores",
                                                                       "seq_lengths", "has_stopped", "lex_state", "phrases", "bufs"]
    assert inspect.signature(engine.beam_lex_step).parameters["bufs"].default is None
    assert list(inspect.signature(engine.beam_lex_buffers).parameters) == ["device", "samples", "beam", "n_phr", "V"]


def test_validate_phrases_forms_and_errors():
    from clipcap_amd.inference.utils import validate_phrases
    V, stop = 50, 7
    one = validate_phrases([[1, 2, 3], [4]], 2, V, stop)                              # one list for all prefixes
    assert one.dtype == torch.int32 and one.tolist() == [[[1, 2, 3], [4, -1, -1]]] * 2
    per = validate_phrases([[[1, 2]], [[3], [4, 5, 6]]], 2, V, stop)                  # one list per prefix: padded to the most and the longest
    assert per.tolist() == [[[1, 2, -1], [-1, -1, -1]], [[3, -1, -1], [4, 5, 6]]]
    ten = validate_phrases(torch.tensor([[[1, 2, -1], [-1, -1, -1], [9, -1, -1]]]), 3, V, stop)      # (1, C, L) for all prefixes; an all -1 row is no phrase
    assert ten.tolist() == [[[1, 2], [9, -1]]] * 3
    assert validate_phrases(torch.tensor([[[1, 2]], [[3, -1]]], dtype=torch.int32), 2, V, stop).tolist() == [[[1, 2]], [[3, -1]]]
    for none in (None, [], [[], []], torch.full((2, 3, 4), -1)):
        assert tuple(validate_phrases(none, 2, V, stop).shape) == (2, 0, 1)
    assert validate_phrases([[1]], 2, V, stop, suppress_tokens=[2, 3]).tolist() == [[[1]]] * 2
    for bad, match in (([[i + 1] for i in range(9)], "at most 8"),                     # more than 8 phrases
                       ([[1, 2], []], "1 to 8 tokens"),                               # an empty phrase
                       ([list(range(10, 19))], "1 to 8 tokens"),                      # longer than 8
                       ([[1, V]], "outside"), ([[-2, 1]], "outside"),                 # an id outside [0, V)
                       ([[1, stop, 2]], "stop token"),                                # the stop token inside a phrase
                       ([[1, 2], [1, 2]], "twice"),                                   # the same phrase twice for one prefix
                       ([[[1]], [[2]], [[3]]], "prefixes"),                            # a wrong batch dimension
                       (torch.zeros(3, 1, 2, dtype=torch.int64), "prefixes"),
                       (torch.zeros(2, 2), "int tensor"), (torch.zeros(2, 1, 2), "int tensor"),
                       (torch.tensor([[[1, -1, 2]]]), "after its padding")):
        with pytest.raises(ValueError, match=match):
            validate_phrases(bad, 2, V, stop)
    with pytest.raises(ValueError, match="suppress_tokens"):                          # a phrase token in suppress_tokens
        validate_phrases([[1, 2]], 2, V, stop, suppress_tokens=torch.tensor([9, 2]))
    assert validate_phrases([[[1, 2]], [[1, 2]]], 2, V, stop).shape == (2, 1, 2)      # the same phrase for two prefixes is fine


def test_unpack_lex_state():
    from clipcap_amd.inference.utils import unpack_lex_state, validate_phrases
    from tests.lexbeam_ref import pack, tokens_met
    ph = [[[1, 2, 3], [4]], [[5, 6]]]
    table = validate_phrases(ph, 2, 50, 7)
    states = [[0, pack(0b01, -1, 0), pack(0b10, 0, 2), pack(0b11, -1, 0)], [0, pack(0, 0, 1), pack(1, -1, 0), 0]]
    met, done = unpack_lex_state(torch.tensor(states, dtype=torch.int32).view(-1), table)
    assert met.dtype == torch.int32 and done.dtype == torch.bool
    assert met.tolist() == [[tokens_met(s, ph[i]) for s in row] for i, row in enumerate(states)] == [[0, 3, 3, 4], [0, 1, 2, 0]]
    assert done.tolist() == [[False, False, False, True], [False, False, True, False]]
    met, done = unpack_lex_state(torch.zeros(6, dtype=torch.int32), validate_phrases(None, 2, 50, 7))
    assert met.tolist() == [[0] * 3] * 2 and done.tolist() == [[True] * 3] * 2        # nothing to produce: met


def test_decoders_validate_before_touching_the_device():
    """A bad option raises ValueError from the decoder itself (no GPU here: anything later would fail differently)."""
    from types import SimpleNamespace
    from clipcap_amd.inference import generate_constrained_beam, generate_constrained_beam_tokens
    from clipcap_amd.model.gpt2 import GPT2LM
    from tests.test_api_surface import FakeTokenizer
    lm = GPT2LM(n_embd=32, n_layer=1, n_head=2, vocab_size=97, n_positions=16)
    model = SimpleNamespace(language_model=lm)
    emb, tk = torch.zeros(2, 2, 32), FakeTokenizer(97, 5)
    for kw, match in ((dict(beam_size=0), "beam_size"), (dict(beam_size=17), "beam_size")):
        with pytest.raises(ValueError, match=match):
            generate_constrained_beam_tokens(model, emb, [[1, 2]], **kw)
        with pytest.raises(ValueError, match=match):
            generate_constrained_beam(model, tk, emb, [" a"], **kw)
    for bad, match in (([[1, 97]], "outside"), ([[1, 5]], "stop token"), ([[1], [1]], "twice"), ([[[1]]] * 3, "prefixes")):
        with pytest.raises(ValueError, match=match):
            generate_constrained_beam_tokens(model, emb, bad, 4, 4, 1.0, 5)
    with pytest.raises(ValueError, match="suppress_tokens"):
        generate_constrained_beam_tokens(model, emb, [[1, 2]], 4, 4, 1.0, 5, suppress_tokens=[2])
    with pytest.raises(ValueError, match="negative_embeds"):
        generate_constrained_beam_tokens(model, emb, [[1, 2]], 4, 4, 1.0, 5, guidance_scale=1.5)
    with pytest.raises(ValueError, match="num_return_sequences"):
        generate_constrained_beam(model, tk, emb, [" a"], beam_size=4, num_return_sequences=5)
    with pytest.raises(ValueError, match="1 to 8 tokens"):
        generate_constrained_beam(model, tk, emb, ["a word of more than eight tokens"], beam_size=4)
    with pytest.raises(ValueError, match="twice"):
        generate_constrained_beam(model, tk, emb, [[" a"], [" b", " b"]], beam_size=4)


def test_generate_constrained_beam_returns_the_texts_in_best_constrained_beams_order(monkeypatch):
    """generate_constrained_beam on a stubbed search: 2 prefixes, 4 beams -> n texts per prefix, contiguous, most constraint tokens first, then
    the score, each cut at its own length; an empty slot is skipped; the words reach the search as tokenizer.encode gives them."""
    from clipcap_amd.inference import ConstrainedBeams, lexical
    from tests.test_api_surface import FakeTokenizer
    tokens = torch.arange(2 * 4 * 5).view(2, 4, 5)
    stub = ConstrainedBeams(tokens, torch.tensor([[-2.0, -1.0, -1.0, -0.1], [-0.5, float("-inf"), -0.7, -0.6]]),
                            torch.tensor([[5.0, 2.0, 3.0, 1.0], [1.0, 1.0, 2.0, 4.0]]), torch.tensor([[3, 3, 3, 1], [2, 0, 1, 2]], dtype=torch.int32),
                            torch.tensor([[True, True, True, False], [True, False, False, True]]))
    seen = {}

    def fake_search(model, embeds, phrases, beam_size, entry_length, temperature, stop, **kw):
        seen.update(kw, phrases=phrases, beam_size=beam_size, entry_length=entry_length, stop=stop)
        return stub

    monkeypatch.setattr(lexical, "generate_constrained_beam_tokens", fake_search)
    tk = FakeTokenizer(157, 5)
    out = lexical.generate_constrained_beam(None, tk, torch.zeros(2, 1, 8), [" dog", " a"], None, 4, 9, 1.0, num_return_sequences=3,
                                            no_repeat_ngram_size=2, min_length=1)
    assert out == ["5 6", "10 11 12", "0 1 2 3 4",                                 # prefix 0: beams 1, 2 (tie: lower first), 0; beam 3 met less
                   "20", "35 36 37 38", "30 31"]                                   # prefix 1: beams 0, 3 (both 2 met, by score), then 2
    assert seen["phrases"] == [tk.encode(" dog"), tk.encode(" a")] and seen["beam_size"] == 4 and seen["entry_length"] == 9 and seen["stop"] == 5
    assert seen["no_repeat_ngram_size"] == 2 and seen["min_length"] == 1 and seen["guidance_scale"] == 1.0 and seen["negative_embeds"] is None
    assert lexical.generate_constrained_beam(None, tk, torch.zeros(2, 1, 8), [[" dog"], [" a", " b"]], beam_size=4) == ["5 6", "20"]
    assert seen["phrases"] == [[tk.encode(" dog")], [tk.encode(" a"), tk.encode(" b")]]
    out = lexical.generate_constrained_beam(None, tk, torch.zeros(2, 1, 8), [" dog"], beam_size=4, num_return_sequences=4)
    assert len(out) == 7 and out[3] == "15" and out[4:] == ["20", "35 36 37 38", "30 31"]      # the empty slot of prefix 1 is skipped
