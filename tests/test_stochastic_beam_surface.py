"""CPU side of stochastic beam search: cc_beam_gumbel_ws_bytes, cc_beam_gumbel_step and the noise hooks cc_gumbel_noise /
cc_gumbel_from_bits are declared, bound and exported under ABI version 3; gumbel.hip is built once; the argument checks need no device;
the decoders take their options keyword-only at the off values and validate before they touch a device.  The kernels and the decoder are
tested on the device in tests/test_gpu_gumbel.py."""
import inspect
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLS = {
    "cc_beam_gumbel_ws_bytes": ("int64_t", ["int32_t S", "int32_t beam", "int32_t V"]),
    "cc_beam_gumbel_step": ("int", ["int32_t S", "int32_t beam", "int32_t V", "const float* logits", "int64_t ldl", "float temperature",
                                    "int32_t first", "int32_t stop_token", "uint64_t seed", "int32_t step", "float* scores", "float* gumbels",
                                    "float* seq_lengths", "uint8_t* has_stopped", "int32_t* next_tokens", "int32_t* src_rows", "void* ws",
                                    "void* stream"]),
    "cc_gumbel_noise": ("int", ["uint64_t seed", "int32_t step", "int32_t row", "int32_t V", "float* out", "void* stream"]),
    "cc_gumbel_from_bits": ("int", ["const uint32_t* h", "int32_t n", "float* out", "void* stream"]),
}


def test_header_binding_and_library_carry_the_entry_points():
    import ctypes as C
    from clipcap_amd import _lib
    raw = open(os.path.join(ROOT, "include", "clipcap_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    added = raw[raw.index("ADDED since (still 3"):raw.index("#define CC_ABI_VERSION")]
    l = _lib.lib()
    assert l.cc_abi_version() == 3 and _lib.ABI_VERSION == 3
    for name, (ret, want) in DECLS.items():
        m = re.search(r"^" + ret + r"\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr, flags=re.M)
        assert m, f"{name} is not declared in include/clipcap_hip.h"
        params = [p.strip() for p in " ".join(m.group(1).split()).split(",")]
        assert params == want, name
        res, args = _lib.SIGNATURES[name]
        assert res is (_lib._L if ret == "int64_t" else _lib._I) and len(args) == len(params)
        for p, a in zip(params, args):
            exp = _lib._P if "*" in p else C.c_uint64 if p.startswith("uint64_t") else _lib._L if p.startswith("int64_t") else \
                _lib._F if p.startswith("float") else _lib._I
            assert a is exp, (name, p, a)
        assert hasattr(l, name) and name in added, name


def test_generated_abi_files_are_current_and_the_unit_is_built_once():
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_abi.py"), "--check"]).returncode == 0
    csrc = os.path.join(ROOT, "clipcap_amd", "csrc")
    for f in ("abi_dispatch.cpp", "exports.map", "exports_lab.map"):
        text = open(os.path.join(csrc, f)).read()
        for name in DECLS:
            assert name in text, (f, name)
    mk = open(os.path.join(csrc, "Makefile")).read()
    once = next(line for line in mk.splitlines() if line.startswith("SRCS_ONCE"))
    assert "gumbel.hip" in once
    assert "philox.h" in next(line for line in mk.splitlines() if line.startswith("HDRS"))
    src = open(os.path.join(csrc, "gumbel.hip")).read()
    assert '#include "select.hip.h"' in src and '#include "philox.h"' in src
    for piece in ("cand_better", "struct SoftmaxPair", "struct SortedList", "void block_argmax", "void pick_from_list"):
        assert piece.split()[-1] in src and not re.search(piece + r"\b[^;]*\{", src), piece      # used, not defined a second time
    assert "#include" not in open(os.path.join(csrc, "philox.h")).read().replace("#include <stdint.h>", "")   # no HIP header


def test_argument_errors_need_no_device():
    """The argument checks come before anything touches the device: return codes for bad arguments with pointers that are never followed;
    with no samples nothing is launched at all."""
    import ctypes as C
    from clipcap_amd import _lib
    l = _lib.lib()
    p = C.c_void_p(4096)
    nan = float("nan")

    def step(S=2, beam=5, V=130, logits=p, ldl=136, T=1.0, first=0, stop=17, seed=7, step=3, scores=p, gumbels=p, lens=p, stopped=p, nt=p, sr=p,
             ws=p):
        return l.cc_beam_gumbel_step(S, beam, V, logits, ldl, T, first, stop, seed, step, scores, gumbels, lens, stopped, nt, sr, ws, None)

    assert step(S=0) == 0 and step(S=0, first=1, T=0.0, seed=2 ** 64 - 1) == 0          # no samples: CC_OK, nothing launched
    assert step(S=-1) == -1 and step(beam=0) == -1 and step(beam=17) == -1 and step(V=0) == -1 and step(ldl=129) == -1 and step(step=-1) == -1
    assert step(T=nan) == -1
    for k in ("logits", "scores", "gumbels", "lens", "stopped", "nt", "sr", "ws"):
        assert step(**{k: None}) == -1, k
        assert step(S=0, **{k: None}) == -1, k                                          # a bad argument is one whatever S is
    assert step(S=0, beam=16) == 0 and step(S=0, beam=1) == 0
    vmax = 2097152
    assert step(S=0, V=vmax, ldl=vmax) == 0 and step(V=vmax + 1, ldl=vmax + 1) == -2 and step(S=0, V=vmax + 1, ldl=vmax + 1) == -2
    assert step(V=vmax + 1, ldl=vmax) == -1                                              # argument errors come first
    ws = l.cc_beam_gumbel_ws_bytes
    assert ws(64, 5, 50257) >= 64 * 5 * 4 * 5 and ws(0, 1, 1) >= 0 and ws(3, 16, vmax) > 0
    assert ws(-1, 5, 130) == -1 and ws(2, 0, 130) == -1 and ws(2, 17, 130) == -1 and ws(2, 5, 0) == -1 and ws(2, 5, vmax + 1) == -2
    assert l.cc_gumbel_noise(1, -1, 0, 8, p, None) == -1 and l.cc_gumbel_noise(1, 0, -1, 8, p, None) == -1
    assert l.cc_gumbel_noise(1, 0, 0, 0, p, None) == -1 and l.cc_gumbel_noise(1, 0, 0, 8, None, None) == -1
    assert l.cc_gumbel_from_bits(p, -1, p, None) == -1 and l.cc_gumbel_from_bits(None, 4, p, None) == -1
    assert l.cc_gumbel_from_bits(p, 4, None, None) == -1 and l.cc_gumbel_from_bits(p, 0, p, None) == 0


def test_decoder_signatures():
    from clipcap_amd import engine, inference
    from clipcap_amd.inference import stochastic_beam
    assert inference.generate_stochastic_beam is stochastic_beam.generate_stochastic_beam
    assert inference.generate_stochastic_beam_tokens is stochastic_beam.generate_stochastic_beam_tokens
    assert inference.sbs_importance_weights is stochastic_beam.sbs_importance_weights and inference.StochasticBeams._fields == (
        "tokens", "logprobs", "gumbels", "seq_lengths")
    p = inspect.signature(stochastic_beam.generate_stochastic_beam_tokens).parameters
    assert list(p) == ["model", "embeds", "beam_size", "entry_length", "temperature", "stop_token", "seed", "generator", "no_repeat_ngram_size",
                       "min_length", "suppress_tokens", "guidance_scale", "negative_embeds"]
    assert [p[k].default for k in list(p)[2:]] == [5, 67, 1.0, 50256, None, None, 0, 0, None, 1.0, None]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[6:])
    assert all(p[k].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for k in list(p)[:6])
    q = inspect.signature(stochastic_beam.generate_stochastic_beam).parameters
    assert list(q) == ["model", "tokenizer", "embeds", "text_prefix_tokens", "beam_size", "entry_length", "temperature", "num_return_sequences",
                       "seed", "generator", "no_repeat_ngram_size", "min_length", "suppress_tokens", "guidance_scale", "negative_embeds"]
    assert [q[k].default for k in list(q)[3:]] == [None, 5, 67, 1.0, None, None, None, 0, 0, None, 1.0, None]
    assert all(q[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(q)[7:])
    w = inspect.signature(stochastic_beam.sbs_importance_weights).parameters
    assert list(w) == ["logprobs", "gumbels", "normalise"] and w["normalise"].default is True
    e = inspect.signature(engine.beam_gumbel_step).parameters
    assert list(e) == ["logits", "samples", "beam", "temperature", "first", "stop_token", "seed", "step", "scores", "gumbels", "seq_lengths",
                       "has_stopped", "bufs"] and e["bufs"].default is None
    assert list(inspect.signature(engine.beam_gumbel_buffers).parameters) == ["device", "samples", "beam", "V"]
    for text in (stochastic_beam.generate_stochastic_beam_tokens.__doc__, stochastic_beam.__doc__):
        assert "renormalised constrained / guided" in text                                # what bans and guidance do to the sample


def test_validate_stochastic_beam():
    from clipcap_amd.inference.utils import validate_stochastic_beam
    assert validate_stochastic_beam(5) is None and validate_stochastic_beam(16, 16, 2 ** 64 - 1) is None and validate_stochastic_beam(1, 1, 0) is None
    for b in (0, 17, -1, 2.0, "5", None, True):
        with pytest.raises(ValueError, match="beam_size"):
            validate_stochastic_beam(b)
    for n in (0, 6, -1, 1.0, True):
        with pytest.raises(ValueError, match="num_return_sequences"):
            validate_stochastic_beam(5, n)
    for s in (-1, 2 ** 64, 1.5, "7", True):
        with pytest.raises(ValueError, match="seed"):
            validate_stochastic_beam(5, None, s)


def test_decoders_validate_before_touching_the_device():
    """A bad option raises ValueError from the decoder itself (no GPU here: anything later would fail differently)."""
    from types import SimpleNamespace
    from clipcap_amd.inference import generate_stochastic_beam, generate_stochastic_beam_tokens
    from clipcap_amd.model.gpt2 import GPT2LM
    from tests.test_api_surface import FakeTokenizer
    lm = GPT2LM(n_embd=32, n_layer=1, n_head=2, vocab_size=97, n_positions=16)
    model = SimpleNamespace(language_model=lm)
    emb, tk = torch.zeros(2, 2, 32), FakeTokenizer(97, 5)
    for kw, match in ((dict(beam_size=0), "beam_size"), (dict(beam_size=17), "beam_size"), (dict(seed=-1), "seed"), (dict(seed=2 ** 64), "seed")):
        with pytest.raises(ValueError, match=match):
            generate_stochastic_beam_tokens(model, emb, **kw)
        with pytest.raises(ValueError, match=match):
            generate_stochastic_beam(model, tk, emb, **kw)
    with pytest.raises(ValueError, match="num_return_sequences"):
        generate_stochastic_beam(model, tk, emb, beam_size=4, num_return_sequences=5)


def test_seed_is_drawn_from_the_generator_and_manual_seed_reproduces_it():
    from clipcap_amd.inference.stochastic_beam import _draw_seed
    g = torch.Generator().manual_seed(11)
    a = _draw_seed(g)
    assert 0 <= a < 2 ** 62 and _draw_seed(torch.Generator().manual_seed(11)) == a and _draw_seed(g) != a
    torch.manual_seed(5)
    b = _draw_seed(None)
    torch.manual_seed(5)
    assert _draw_seed(None) == b
