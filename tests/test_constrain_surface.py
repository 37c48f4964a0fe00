"""CPU side of constrained decoding (no_repeat_ngram_size / min_length / suppress_tokens): cc_logits_constrain is declared, bound and
exported under ABI version 3; every decoder takes the three options keyword-only; ``banned_tokens`` (the CPU statement of the no-repeat
rule the kernel is tested against, tests/test_gpu_constrain.py) on hand-written cases; the validation errors."""
import inspect
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cc_logits_constrain"


def test_header_binding_and_library_carry_the_entry_point():
    from clipcap_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clipcap_hip.h")).read(), flags=re.S)
    m = re.search(r"^int\s+" + NAME + r"\s*\(([^;]*)\)\s*;", hdr, flags=re.M)
    assert m, f"{NAME} is not declared in include/clipcap_hip.h"
    params = [p.strip() for p in " ".join(m.group(1).split()).split(",")]
    assert len(params) == 16 and params[0] == "float* logits" and params[-1] == "void* stream"
    res, args = _lib.SIGNATURES[NAME]
    assert res is _lib._I and len(args) == len(params)
    # pointer / 64-bit / 32-bit classes of the ctypes signature follow the declaration
    for p, a in zip(params, args):
        want = _lib._P if "*" in p else _lib._L if p.startswith("int64_t") else _lib._I
        assert a is want, (p, a)
    l = _lib.lib()
    assert hasattr(l, NAME) and l.cc_abi_version() == 3 and _lib.ABI_VERSION == 3
    assert "#define CC_ABI_VERSION 3" in open(os.path.join(ROOT, "include", "clipcap_hip.h")).read()
    # (the lab library's export list is exports_lab.map, checked below)


def test_generated_abi_files_are_current_and_name_it():
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_abi.py"), "--check"]).returncode == 0
    csrc = os.path.join(ROOT, "clipcap_amd", "csrc")
    for f in ("abi_dispatch.cpp", "exports.map", "exports_lab.map"):
        assert NAME in open(os.path.join(csrc, f)).read(), f


def test_argument_errors_need_no_device():
    """The argument checks come before anything touches the device: error codes for bad shapes with pointers that are never followed."""
    import ctypes as C
    from clipcap_amd import _lib
    f = _lib.lib().cc_logits_constrain
    lg, hist, sup = C.c_void_p(4096), C.c_void_p(8192), C.c_void_p(12288)

    def call(logits=lg, R=2, V=130, ldl=136, lpart=None, npart=0, history=hist, he=4, hs=8, hl=4, g=2, ban=-1, suppress=None, ns=0):
        return f(logits, R, V, ldl, lpart, npart, history, he, hs, hl, g, ban, suppress, ns, None, None)

    assert call(logits=None) == -1 and call(V=0) == -1 and call(ldl=129) == -1 and call(R=-1) == -1
    assert call(g=-1) == -1 and call(hl=-1) == -1 and call(ns=-1) == -1
    assert call(ban=130) == -1 and call(ban=-2) == -1
    assert call(he=2) == -1 and call(history=None) == -1 and call(hs=3) == -1
    assert call(suppress=None, ns=3) == -1
    assert call(lpart=C.c_void_p(16384), npart=2) == -1                 # 2 * 64 < 130
    assert call(hl=1025, hs=2048) == -2 and call(suppress=sup, ns=1024) == -2
    # nothing to ban: ok, and nothing is launched (there is no device here to launch on)
    assert call(g=0, history=None, hl=0) == 0 and call(g=3, hl=2) == 0 and call(R=0, ban=5) == 0


DECODERS = ["base.generate_beam_rounds", "base.generate_beam_tokens", "base.generate_beam", "base.sample_tokens",
            "base.generate_nucleus_sampling", "base.generate_no_beam", "no_beam.generate_no_beam", "nucleus_sampling.generate_nucleus_sampling",
            "generate.generate"]


@pytest.mark.parametrize("where", DECODERS)
def test_every_decoder_takes_the_three_options_keyword_only(where):
    import importlib
    mod, fn = where.split(".")
    p = inspect.signature(getattr(importlib.import_module("clipcap_amd.inference." + mod), fn)).parameters
    for k, d in (("no_repeat_ngram_size", 0), ("min_length", 0), ("suppress_tokens", None)):
        assert k in p, (where, k)
        assert p[k].kind is inspect.Parameter.KEYWORD_ONLY and (p[k].default is d or p[k].default == d), (where, k)


def test_reference_positional_calls_keep_their_order():
    """The options come after the reference's parameters: the positional prefixes of the reference signatures are unchanged."""
    import importlib
    from clipcap_amd.inference import base, no_beam, nucleus_sampling
    generate = importlib.import_module("clipcap_amd.inference.generate")       # the package attribute of that name is the function
    names = lambda f: [k for k, v in inspect.signature(f).parameters.items() if v.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]  # noqa: E731
    assert names(base.generate_beam) == ["model", "tokenizer", "embeds", "number_to_generate", "text_prefix_tokens", "beam_size", "entry_length",
                                         "temperature"]
    assert names(base.generate_nucleus_sampling)[:9] == ["model", "tokenizer", "embeds", "number_to_generate", "text_prefix_tokens", "entry_length",
                                                         "top_p", "top_k", "temperature"]
    assert names(base.generate_no_beam)[:10] == ["model", "tokenizer", "embeds", "text_prefix_tokens", "top_p", "top_k", "entry_length", "temperature",
                                                 "repetition_penalty", "desired_sentence_length"]
    assert names(no_beam.generate_no_beam)[:5] == ["model", "tokenizer", "embeds", "number_to_generate", "text_prefix_tokens"]
    assert names(nucleus_sampling.generate_nucleus_sampling)[:5] == ["model", "tokenizer", "embeds", "number_to_generate", "text_prefix_tokens"]
    assert names(generate.generate)[:9] == ["model", "tokenizer", "embeddings", "top_p", "top_k", "temperature", "number_to_generate", "text_prefix",
                                            "stop_token"]
    assert names(base.generate_beam_rounds) == ["model", "embeds", "beam_size", "entry_length", "temperature", "stop_token", "rounds"]


@pytest.mark.parametrize("history,g,want", [
    ([3, 5, 3, 9], 1, {3, 5, 9}),                       # g = 1: every token of the history
    ([], 1, set()),
    ([3, 5, 8, 3], 2, {5}),                             # the last token 3 was followed by 5
    ([3, 5, 8, 3, 5], 3, {8}),                          # ... (3, 5) by 8
    ([1, 2, 3, 9, 1, 2, 3], 4, {9}),
    ([1, 2, 3, 9, 1, 2, 4], 4, set()),                  # the last three tokens occur nowhere else
    ([4, 6], 3, set()),                                 # n < g
    ([4], 3, set()),
    ([4, 6], 2, set()),                                 # n == g: one window, whose prefix (4) is not the last token (6)
    ([6, 6], 2, {6}),                                   # n == g and it matches
    ([4, 6, 7], 4, set()),                              # n == g - 1
    ([6], 2, set()),                                    # n == g - 1, g = 2
    ([1, 2, 7, 1, 2, 7, 1, 2], 3, {7}),                 # the same n-gram twice, same continuation
    ([1, 2, 7, 1, 2, 8, 1, 2], 3, {7, 8}),              # the same n-gram twice, different continuations
    ([7, 7, 7], 2, {7}),                                # an n-gram overlapping itself
    ([7, 7, 7, 7], 3, {7}),
    ([1, 2, 3], 0, set()),                              # off
])
def test_banned_tokens_hand_cases(history, g, want):
    from clipcap_amd.inference.utils import banned_tokens
    assert banned_tokens(history, g) == want
    assert banned_tokens(torch.tensor(history, dtype=torch.int64), g) == want
    assert banned_tokens(torch.tensor(history, dtype=torch.int32), g) == want


def test_banned_tokens_means_no_repeated_ngram():
    """The rule's purpose, by brute force: t is banned exactly when appending it would make the last g tokens an n-gram seen before."""
    from clipcap_amd.inference.utils import banned_tokens
    gen = torch.Generator().manual_seed(4)
    for _ in range(200):
        n, g = int(torch.randint(0, 12, (1,), generator=gen)), int(torch.randint(1, 5, (1,), generator=gen))
        h = torch.randint(0, 4, (n,), generator=gen).tolist()
        seen = {tuple(h[i:i + g]) for i in range(n - g + 1)}
        want = {t for t in range(4) if tuple((h + [t])[-g:]) in seen}            # seen holds g-tuples only: a shorter tail matches nothing
        assert banned_tokens(h, g) == want, (h, g)


def test_validation_errors():
    from clipcap_amd.inference.utils import MAX_SUPPRESS_TOKENS, validate_constraints
    V, stop = 211, 7
    assert validate_constraints(V, stop) == []
    assert validate_constraints(V, stop, 3, 5, [1, 2, 210]) == [1, 2, 210]
    assert validate_constraints(V, stop, 0, 1, torch.tensor([stop, 0])) == [stop, 0]          # with min_length > 0 the caller asked for it
    for kw in (dict(no_repeat_ngram_size=-1), dict(min_length=-2), dict(suppress_tokens=[-1]), dict(suppress_tokens=[V]),
               dict(suppress_tokens=[0] * (MAX_SUPPRESS_TOKENS + 1))):
        with pytest.raises(ValueError):
            validate_constraints(V, stop, **kw)
    assert MAX_SUPPRESS_TOKENS == 1023 and len(validate_constraints(V, stop, suppress_tokens=[1] * 1023)) == 1023
    with pytest.raises(ValueError, match="never stop"):
        validate_constraints(V, stop, 0, 0, [3, stop])
    with pytest.raises(ValueError):
        validate_constraints(V, V + 5, min_length=2)                                           # a stop token the vocabulary does not have


def test_decoders_validate_before_touching_the_device():
    """A bad option raises ValueError from the decoder itself (no GPU here: anything later would fail differently)."""
    from types import SimpleNamespace
    from clipcap_amd.inference import base
    from clipcap_amd.model.gpt2 import GPT2LM
    lm = GPT2LM(n_embd=32, n_layer=1, n_head=2, vocab_size=97, n_positions=16)
    model = SimpleNamespace(language_model=lm)
    with pytest.raises(ValueError, match="never stop"):
        base.generate_beam_tokens(model, torch.zeros(1, 2, 32), 2, 4, 1.0, 5, suppress_tokens=[5])
    with pytest.raises(ValueError):
        base.sample_tokens(model, torch.zeros(1, 2, 32), 4, 5, no_repeat_ngram_size=-1)
