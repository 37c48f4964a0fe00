"""CPU side of classifier-free guidance at decode time (guidance_scale / negative_embeds): cc_logits_guide is declared, bound and exported
under ABI version 3; its argument checks need no device; every beam and sampling decoder takes the two options keyword-only, after the
existing ones; the validation errors; engine.guide_logits's signature.  The kernel and the decoders are tested on the device in
tests/test_gpu_guide.py and tests/test_gpu_guide_decode.py."""
import inspect
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cc_logits_guide"
PARAMS = ["const float* cond", "int64_t ld_c", "const float* uncond", "int64_t ld_u", "int32_t R", "int32_t V", "float scale", "float* out",
          "int64_t ld_o", "const uint8_t* skip_rows", "void* stream"]


def test_header_binding_and_library_carry_the_entry_point():
    from clipcap_amd import _lib
    raw = open(os.path.join(ROOT, "include", "clipcap_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"^int\s+" + NAME + r"\s*\(([^;]*)\)\s*;", hdr, flags=re.M)
    assert m, f"{NAME} is not declared in include/clipcap_hip.h"
    params = [p.strip() for p in " ".join(m.group(1).split()).split(",")]
    assert params == PARAMS
    res, args = _lib.SIGNATURES[NAME]
    assert res is _lib._I and len(args) == len(params) == 11
    for p, a in zip(params, args):
        want = _lib._P if "*" in p else _lib._L if p.startswith("int64_t") else _lib._F if p.startswith("float") else _lib._I
        assert a is want, (p, a)
    l = _lib.lib()
    assert hasattr(l, NAME) and l.cc_abi_version() == 3 and _lib.ABI_VERSION == 3
    assert "#define CC_ABI_VERSION 3" in raw
    added = raw[raw.index("ADDED since (still 3"):raw.index("#define CC_ABI_VERSION")]
    assert NAME in added                                                                   # the list of entry points added without a bump


def test_generated_abi_files_are_current_and_name_it():
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_abi.py"), "--check"]).returncode == 0
    csrc = os.path.join(ROOT, "clipcap_amd", "csrc")
    for f in ("abi_dispatch.cpp", "exports.map", "exports_lab.map"):
        assert NAME in open(os.path.join(csrc, f)).read(), f
    assert "guide.hip" in open(os.path.join(csrc, "Makefile")).read()


def test_argument_errors_need_no_device():
    """The argument checks come before anything touches the device: return codes for bad arguments with pointers that are never followed."""
    import ctypes as C
    from clipcap_amd import _lib
    f = _lib.lib().cc_logits_guide
    c, u, o = C.c_void_p(4096), C.c_void_p(65536), C.c_void_p(1 << 20)

    def call(cond=c, ld_c=136, uncond=u, ld_u=130, R=2, V=130, scale=1.5, out=o, ld_o=131):
        return f(cond, ld_c, uncond, ld_u, R, V, scale, out, ld_o, None, None)

    assert call(R=0) == 0 and call(R=0, out=None) == 0 and call(R=0, cond=None, uncond=None, out=None) == 0      # nothing is launched
    assert call(V=0) == -1 and call(V=-3) == -1 and call(R=-1) == -1
    assert call(ld_c=129) == -1 and call(ld_u=129) == -1 and call(ld_o=129) == -1
    assert call(scale=-0.5) == -1 and call(scale=float("inf")) == -1 and call(scale=float("nan")) == -1
    assert call(cond=None) == -1 and call(uncond=None) == -1
    assert call(R=0, V=0) == -1 and call(R=0, scale=float("nan")) == -1                   # a bad argument is one whatever R is


DECODERS = ["base.generate_beam_rounds", "base.generate_beam_tokens", "base.generate_beam", "base.sample_tokens",
            "base.generate_nucleus_sampling", "base.generate_no_beam", "no_beam.generate_no_beam", "nucleus_sampling.generate_nucleus_sampling",
            "generate.generate"]


@pytest.mark.parametrize("where", DECODERS)
def test_every_decoder_takes_the_two_options_keyword_only_after_the_others(where):
    import importlib
    mod, fn = where.split(".")
    p = inspect.signature(getattr(importlib.import_module("clipcap_amd.inference." + mod), fn)).parameters
    assert list(p)[-2:] == ["guidance_scale", "negative_embeds"], where
    assert p["guidance_scale"].kind is inspect.Parameter.KEYWORD_ONLY and p["guidance_scale"].default == 1.0
    assert p["negative_embeds"].kind is inspect.Parameter.KEYWORD_ONLY and p["negative_embeds"].default is None


def test_engine_guide_logits_signature():
    from clipcap_amd import engine
    p = inspect.signature(engine.guide_logits).parameters
    assert list(p) == ["cond", "uncond", "scale", "out", "skip_rows"]
    assert all(p[k].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for k in ("cond", "uncond", "scale"))
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY and p[k].default is None for k in ("out", "skip_rows"))


def test_validate_guidance():
    from clipcap_amd.inference.utils import validate_guidance
    assert validate_guidance() == 1.0 and validate_guidance(0) == 0.0 and validate_guidance(7.5) == 7.5
    for bad in (-0.1, float("inf"), float("-inf"), float("nan"), "much", None):
        with pytest.raises(ValueError, match="guidance_scale"):
            validate_guidance(bad)


def test_decoders_validate_before_touching_the_device():
    """A bad option raises ValueError from the decoder itself (no GPU here: anything later would fail differently)."""
    from types import SimpleNamespace
    from clipcap_amd.inference import base, no_beam, nucleus_sampling
    from clipcap_amd.model.gpt2 import GPT2LM
    from tests.test_api_surface import FakeTokenizer
    lm = GPT2LM(n_embd=32, n_layer=1, n_head=2, vocab_size=97, n_positions=16)
    model = SimpleNamespace(language_model=lm)
    emb, tk = torch.zeros(2, 2, 32), FakeTokenizer(97, 5)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="guidance_scale"):
            base.generate_beam_tokens(model, emb, 2, 4, 1.0, 5, guidance_scale=bad, negative_embeds=torch.zeros(1, 1, 32))
        with pytest.raises(ValueError, match="guidance_scale"):
            base.sample_tokens(model, emb, 4, 5, guidance_scale=bad, negative_embeds=torch.zeros(1, 1, 32))
        for fn in (base.generate_beam, base.generate_nucleus_sampling, base.generate_no_beam, no_beam.generate_no_beam,
                   nucleus_sampling.generate_nucleus_sampling):
            with pytest.raises(ValueError, match="guidance_scale"):
                fn(model, tk, emb, guidance_scale=bad)
    # a token-level function has no tokenizer to build the default context from
    with pytest.raises(ValueError, match="negative_embeds"):
        base.generate_beam_rounds(model, emb, 2, 4, 1.0, 5, guidance_scale=2.0)
    with pytest.raises(ValueError, match="negative_embeds"):
        base.generate_beam_tokens(model, emb, 2, 4, 1.0, 5, guidance_scale=2.0)
    with pytest.raises(ValueError, match="negative_embeds"):
        base.sample_tokens(model, emb, 4, 5, guidance_scale=0.0)
    for shape in ((3, 1, 32), (1, 0, 32), (1, 1, 16), (1, 32)):                            # rows, Ln >= 1, D, rank
        with pytest.raises(ValueError, match="negative_embeds"):
            base.generate_beam_tokens(model, emb, 2, 4, 1.0, 5, guidance_scale=2.0, negative_embeds=torch.zeros(*shape))


def test_the_default_negative_context_is_the_bos_embedding_followed_by_the_text_prefix():
    from types import SimpleNamespace
    from clipcap_amd.inference.base import _negative_context
    from clipcap_amd.model.gpt2 import GPT2LM
    from tests.test_api_surface import FakeTokenizer
    lm = GPT2LM(n_embd=32, n_layer=1, n_head=2, vocab_size=97, n_positions=16)
    model = SimpleNamespace(language_model=lm)
    tk = FakeTokenizer(97, 5)
    wte = lm.get_input_embeddings().weight.detach()
    bos = tk.encode(tk.bos_token)[0]
    assert _negative_context(model, tk, None, None, 1.0) is None and _negative_context(model, tk, torch.ones(1, 2, 32), None, 1.0) is None
    assert torch.equal(_negative_context(model, tk, None, None, 2.0), wte[bos].view(1, 1, 32))
    text = torch.tensor([[7, 9, 11]])
    got = _negative_context(model, tk, None, text, 2.0)
    assert got.shape == (1, 4, 32) and torch.equal(got[0, 0], wte[bos]) and torch.equal(got[0, 1:], wte[text[0]])
    mine = torch.randn(2, 3, 32)
    got = _negative_context(model, tk, mine, text, 0.5)
    assert got.shape == (2, 6, 32) and torch.equal(got[:, :3], mine) and torch.equal(got[1, 3:], wte[text[0]])
