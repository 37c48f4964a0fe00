"""CPU side of diverse beam search (num_beam_groups / diversity_penalty / num_return_sequences): cc_beam_group_step and
cc_beam_group_ws_bytes are declared, bound and exported under ABI version 3; their argument errors need no device; the beam decoders take
the options keyword-only; the validation errors; the order of the returned beams on a stub."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"cc_beam_group_ws_bytes": 4, "cc_beam_group_step": 17}


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
    _, params = _declared("cc_beam_group_step")
    assert [p.split()[-1].lstrip("*") for p in params] == ["S", "beam", "groups", "V", "logits", "ldl", "temperature", "diversity_penalty", "first",
                                                          "stop_token", "scores", "seq_lengths", "has_stopped", "next_tokens", "src_rows", "ws",
                                                          "stream"]
    _, params = _declared("cc_beam_group_ws_bytes")
    assert [p.split()[-1] for p in params] == ["S", "beam", "groups", "V"]


def test_generated_abi_files_are_current_and_name_them():
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_abi.py"), "--check"]).returncode == 0
    csrc = os.path.join(ROOT, "clipcap_amd", "csrc")
    for f in ("abi_dispatch.cpp", "exports.map", "exports_lab.map"):
        text = open(os.path.join(csrc, f)).read()
        for name in NAMES:
            assert name in text, (f, name)
    # built once, like the rest of beam.hip: no per-operand-type variants are declared
    disp = open(os.path.join(csrc, "abi_dispatch.cpp")).read()
    assert "cc_beam_group_step_bf16" in disp and "cc_beam_group_step_f16" not in disp and "cc_beam_group_step_x3" not in disp


def test_argument_errors_need_no_device():
    """The argument checks come before anything touches the device: error codes for bad arguments with pointers that are never followed."""
    from clipcap_amd import _lib
    f = _lib.lib().cc_beam_group_step
    ptr = [C.c_void_p(4096 * (i + 1)) for i in range(7)]

    def call(S=2, beam=6, groups=3, V=130, logits=ptr[0], ldl=136, temp=1.0, pen=0.5, first=0, stop=5, scores=ptr[1], seql=ptr[2], stopped=ptr[3],
             nt=ptr[4], src=ptr[5], ws=ptr[6]):
        return f(S, beam, groups, V, logits, ldl, temp, pen, first, stop, scores, seql, stopped, nt, src, ws, None)

    for kw in (dict(logits=None), dict(scores=None), dict(seql=None), dict(stopped=None), dict(nt=None), dict(src=None), dict(ws=None)):
        assert call(**kw) == -1, kw
    assert call(beam=17, groups=1) == -1 and call(beam=32, groups=2) == -1
    assert call(groups=0) == -1 and call(groups=-1) == -1
    assert call(beam=6, groups=4) == -1 and call(beam=4, groups=8) == -1
    assert call(ldl=129) == -1
    assert call(pen=-0.5) == -1 and call(pen=float("inf")) == -1 and call(pen=float("nan")) == -1
    assert call(S=-1) == -1 and call(beam=0, groups=1) == -1 and call(V=0, ldl=0) == -1
    # S == 0: ok, and nothing is launched (there is no device here to launch on)
    assert call(S=0) == 0 and call(S=0, groups=1, pen=0.0) == 0
    w = _lib.lib().cc_beam_group_ws_bytes
    assert w(2, 6, 4, 130) < 0 and w(2, 17, 1, 130) < 0 and w(2, 6, 0, 130) < 0 and w(0, 6, 3, 130) < 0
    # row statistics + one beam group's chunk winners + the picks: no smaller than that, and the winners shrink with the group width
    assert w(3, 6, 3, 50257) >= 3 * 6 * 8 + 3 * 16 * 2 * 8 + 3 * 6 * 4
    assert w(3, 6, 6, 50257) < w(3, 6, 3, 50257) < w(3, 6, 1, 50257)


BEAM_DECODERS = ["generate_beam_rounds", "generate_beam_tokens", "generate_beam"]


@pytest.mark.parametrize("fn", BEAM_DECODERS)
def test_beam_decoders_take_the_options_keyword_only(fn):
    from clipcap_amd.inference import base
    p = inspect.signature(getattr(base, fn)).parameters
    want = [("num_beam_groups", 1), ("diversity_penalty", 0.0)] + ([("num_return_sequences", 1)] if fn == "generate_beam" else [])
    for k, d in want:
        assert k in p, (fn, k)
        assert p[k].kind is inspect.Parameter.KEYWORD_ONLY and p[k].default == d and type(p[k].default) is type(d), (fn, k)
    if fn != "generate_beam":
        assert "num_return_sequences" not in p


def test_engine_wrappers_have_the_documented_signatures():
    from clipcap_amd import engine
    assert list(inspect.signature(engine.beam_group_step).parameters) == ["logits", "samples", "beam", "groups", "temperature", "diversity_penalty",
                                                                         "first", "stop_token", "scores", "seq_lengths", "has_stopped", "bufs"]
    assert inspect.signature(engine.beam_group_step).parameters["bufs"].default is None
    assert list(inspect.signature(engine.beam_group_buffers).parameters) == ["device", "samples", "beam", "groups", "V"]


def test_validation_errors():
    from clipcap_amd.inference.utils import validate_beam_groups
    assert validate_beam_groups(5) is None and validate_beam_groups(6, 3, 0.5) is None and validate_beam_groups(6, 6, 2.0, 6) is None
    assert validate_beam_groups(5, 1, 0.0, 5) is None
    for args in ((6, 0, 0.0), (6, -2, 1.0),                   # num_beam_groups >= 1
                 (6, 4, 1.0), (5, 2, 1.0), (4, 8, 1.0),       # a divisor of beam_size
                 (6, 3, -0.5), (6, 3, float("inf")), (6, 3, float("nan")), (6, 1, float("nan")),   # finite and >= 0
                 (6, 3, 0.0),                                 # beam groups need a penalty
                 (6, 1, 0.5),                                 # a penalty needs beam groups
                 (6, 1, 0.0, 0), (6, 1, 0.0, 7), (6, 3, 1.0, -1)):                                 # 1 <= num_return_sequences <= beam_size
        with pytest.raises(ValueError):
            validate_beam_groups(*args)


def test_decoders_validate_before_touching_the_device():
    """A bad option raises ValueError from the decoder itself (no GPU here: anything later would fail differently)."""
    from types import SimpleNamespace
    from clipcap_amd.inference import base
    from clipcap_amd.model.gpt2 import GPT2LM
    lm = GPT2LM(n_embd=32, n_layer=1, n_head=2, vocab_size=97, n_positions=16)
    model = SimpleNamespace(language_model=lm)
    emb = torch.zeros(1, 2, 32)
    with pytest.raises(ValueError, match="multiple"):
        base.generate_beam_tokens(model, emb, 4, 4, 1.0, 5, num_beam_groups=3, diversity_penalty=1.0)
    with pytest.raises(ValueError, match="diversity_penalty"):
        base.generate_beam_tokens(model, emb, 4, 4, 1.0, 5, num_beam_groups=2)
    with pytest.raises(ValueError, match="num_beam_groups"):
        base.generate_beam_rounds(model, emb, 4, 4, 1.0, 5, 1, diversity_penalty=0.5)
    tok = SimpleNamespace(eos_token="<eos>", encode=lambda s: [5], decode=lambda ids: " ".join(str(int(i)) for i in ids))
    with pytest.raises(ValueError, match="num_return_sequences"):
        base.generate_beam(model, tok, emb, beam_size=4, entry_length=4, num_return_sequences=5)


def test_best_beams_order_on_a_stub():
    from clipcap_amd.inference.base import best_beams
    scores = torch.tensor([[-1.0, -0.5, -0.5, -3.0], [-2.0, -2.0, -2.0, -2.0], [-4.0, -3.0, -2.0, -1.0]])
    assert best_beams(scores, 1).tolist() == [[1], [0], [3]]                       # today's argmax: ties to the first beam
    assert best_beams(scores, 3).tolist() == [[1, 2, 0], [0, 1, 2], [3, 2, 1]]     # best first, ties to the lower beam index
    assert best_beams(scores, 4).tolist() == [[1, 2, 0, 3], [0, 1, 2, 3], [3, 2, 1, 0]]


def test_generate_beam_returns_the_n_best_texts_of_every_prefix_together(monkeypatch):
    """generate_beam on a stubbed search: 2 prefixes, 2 rounds, 3 beams -> n texts per (round, prefix), contiguous, best first, each cut at
    its own length; n == 1 is the best beam only."""
    from types import SimpleNamespace
    from clipcap_amd.inference import base
    tokens = torch.arange(2 * 3 * 4).view(2, 3, 4)
    rounds = [(tokens, torch.tensor([[-2.0, -1.0, -1.0], [-0.5, -3.0, -0.7]]), torch.tensor([[4.0, 2.0, 3.0], [1.0, 4.0, 2.0]])),
              (tokens + 100, torch.tensor([[-1.0, -2.0, -3.0], [-3.0, -2.0, -1.0]]), torch.tensor([[2.0, 2.0, 2.0], [3.0, 3.0, 3.0]]))]
    seen = {}

    def fake_rounds(model, embeds, beam_size, entry_length, temperature, stop, n_rounds, **kw):
        seen.update(kw, beam_size=beam_size, rounds=n_rounds)
        return rounds

    monkeypatch.setattr(base, "generate_beam_rounds", fake_rounds)
    tok = SimpleNamespace(eos_token="<eos>", encode=lambda s: [5], decode=lambda ids: " ".join(str(int(i)) for i in ids))
    out = base.generate_beam(None, tok, torch.zeros(2, 1, 8), 2, None, 3, 4, 1.0, num_beam_groups=3, diversity_penalty=0.5, num_return_sequences=2)
    assert out == ["4 5", "8 9 10", "12", "20 21",                                 # round 0: prefix 0 beams 1, 2 (tie: lower first); prefix 1 beams 0, 2
                   "100 101", "104 105", "120 121 122", "116 117 118"]             # round 1: prefix 0 beams 0, 1; prefix 1 beams 2, 1
    assert seen["num_beam_groups"] == 3 and seen["diversity_penalty"] == 0.5 and seen["beam_size"] == 3 and seen["rounds"] == 2
    assert base.generate_beam(None, tok, torch.zeros(2, 1, 8), 2, None, 3, 4, 1.0) == ["4 5", "12", "100 101", "120 121 122"]
    assert seen["num_beam_groups"] == 1 and seen["diversity_penalty"] == 0.0
