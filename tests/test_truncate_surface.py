"""CPU side of the sampling truncation rules (min_p / typical_p / epsilon_cutoff / eta_cutoff): cc_logits_truncate is declared, bound and
exported under ABI version 3; its argument checks need no device; the sampling decoders and self_critical_step take the four options
keyword-only at their off values; engine.truncate_logits validates before it touches a device and launches nothing with every rule off.
The kernel and the decoders are tested on the device in tests/test_gpu_truncate.py."""
import inspect
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cc_logits_truncate"
PARAMS = ["float* logits", "int32_t R", "int32_t V", "int64_t ldl", "float temperature", "const int64_t* history", "int32_t hist_len",
          "int32_t hist_ld", "float repetition_penalty", "float min_p", "float typical_p", "float epsilon_cutoff", "float eta_cutoff", "void* stream"]
OFF = dict(min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)


def test_header_binding_and_library_carry_the_entry_point():
    from clipcap_amd import _lib
    raw = open(os.path.join(ROOT, "include", "clipcap_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"^int\s+" + NAME + r"\s*\(([^;]*)\)\s*;", hdr, flags=re.M)
    assert m, f"{NAME} is not declared in include/clipcap_hip.h"
    params = [p.strip() for p in " ".join(m.group(1).split()).split(",")]
    assert params == PARAMS
    res, args = _lib.SIGNATURES[NAME]
    assert res is _lib._I and len(args) == len(params) == 14
    for p, a in zip(params, args):
        want = _lib._P if "*" in p else _lib._L if p.startswith("int64_t") else _lib._F if p.startswith("float") else _lib._I
        assert a is want, (p, a)
    l = _lib.lib()
    assert hasattr(l, NAME) and l.cc_abi_version() == 3 and _lib.ABI_VERSION == 3
    added = raw[raw.index("ADDED since (still 3"):raw.index("#define CC_ABI_VERSION")]
    assert NAME in added                                                                   # the list of entry points added without a bump


def test_generated_abi_files_are_current_and_name_it():
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_abi.py"), "--check"]).returncode == 0
    csrc = os.path.join(ROOT, "clipcap_amd", "csrc")
    for f in ("abi_dispatch.cpp", "exports.map", "exports_lab.map"):
        assert NAME in open(os.path.join(csrc, f)).read(), f
    mk = open(os.path.join(csrc, "Makefile")).read()
    once = next(line for line in mk.splitlines() if line.startswith("SRCS_ONCE"))
    assert "truncate.hip" in once                                                          # fp32 / integer work: built once


def test_argument_errors_need_no_device():
    """The argument checks come before anything touches the device: return codes for bad arguments with pointers that are never followed;
    with every rule off, or no rows, nothing is launched at all."""
    import ctypes as C
    from clipcap_amd import _lib
    f = _lib.lib().cc_logits_truncate
    x, h = C.c_void_p(4096), C.c_void_p(65536)
    nan, inf = float("nan"), float("inf")

    def call(logits=x, R=2, V=130, ldl=136, T=1.0, hist=h, hl=3, hld=5, rep=1.2, min_p=0.1, typ=0.9, eps=3e-4, eta=6e-4):
        return f(logits, R, V, ldl, T, hist, hl, hld, rep, min_p, typ, eps, eta, None)

    assert call(R=0) == 0 and call(R=0, logits=None) == 0                                  # no rows
    assert call(min_p=0.0, typ=1.0, eps=0.0, eta=0.0) == 0                                 # every rule off
    assert call(R=-1) == -1 and call(V=0) == -1 and call(V=-3) == -1 and call(ldl=129) == -1
    assert call(min_p=-0.1) == -1 and call(min_p=1.5) == -1 and call(min_p=nan) == -1
    assert call(typ=0.0) == -1 and call(typ=-0.5) == -1 and call(typ=1.5) == -1 and call(typ=nan) == -1
    assert call(eps=-1e-3) == -1 and call(eps=1.0) == -1 and call(eps=nan) == -1 and call(eps=inf) == -1
    assert call(eta=-1e-3) == -1 and call(eta=1.0) == -1 and call(eta=nan) == -1
    assert call(hist=None) == -1 and call(hld=2) == -1 and call(hl=-1) == -1
    assert call(hist=None, hl=0, R=0) == 0 and call(logits=None) == -1
    assert call(R=0, V=0) == -1 and call(R=0, eta=nan) == -1                               # a bad argument is one whatever R is
    assert call(min_p=0.0, typ=1.0, eps=0.0, eta=0.0, V=0) == -1                           # ... and whatever the rules are
    vmax = (150 * 1024 - 16928) // 4 * 32                                                  # the history bitmap's share of LDS (header)
    assert call(R=0, V=vmax + 1, ldl=vmax + 1) == 0                                        # nothing to launch: no shape to refuse
    assert call(V=vmax + 1, ldl=vmax + 1) == -2
    assert f"V <= {vmax}" in open(os.path.join(ROOT, "include", "clipcap_hip.h")).read()


DECODERS = ["inference.base.sample_tokens", "inference.base.generate_nucleus_sampling", "inference.base.generate_no_beam",
            "inference.no_beam.generate_no_beam", "inference.nucleus_sampling.generate_nucleus_sampling", "inference.generate.generate",
            "train.self_critical.self_critical_step"]


@pytest.mark.parametrize("where", DECODERS)
def test_every_sampling_decoder_takes_the_four_options_keyword_only_at_their_off_values(where):
    import importlib
    mod, fn = where.rsplit(".", 1)
    p = inspect.signature(getattr(importlib.import_module("clipcap_amd." + mod), fn)).parameters
    for k, off in OFF.items():
        assert k in p, (where, k)
        assert p[k].kind is inspect.Parameter.KEYWORD_ONLY and p[k].default == off, (where, k)


def test_engine_truncate_logits_signature():
    from clipcap_amd import engine
    p = inspect.signature(engine.truncate_logits).parameters
    assert list(p) == ["logits", "temperature", "history", "hist_len", "repetition_penalty", "min_p", "typical_p", "epsilon_cutoff", "eta_cutoff"]
    assert p["logits"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(p)[1:])
    assert [p[k].default for k in list(p)[1:]] == [1.0, None, 0, 1.0, 0.0, 1.0, 0.0, 0.0]


def test_validate_truncation():
    from clipcap_amd.inference.utils import truncation_is_on, validate_truncation
    assert validate_truncation() == OFF and not truncation_is_on(validate_truncation())
    got = validate_truncation(1, 0.5, 0.25, 0.125)
    assert got == dict(min_p=1.0, typical_p=0.5, epsilon_cutoff=0.25, eta_cutoff=0.125) and truncation_is_on(got)
    for k, on in (("min_p", 0.05), ("typical_p", 0.9), ("epsilon_cutoff", 3e-4), ("eta_cutoff", 3e-4)):
        assert truncation_is_on(validate_truncation(**{k: on}))
    bad = dict(min_p=(-0.1, 1.01), typical_p=(0.0, -1.0, 1.01), epsilon_cutoff=(-1e-3, 1.0), eta_cutoff=(-1e-3, 1.0, 2.0))
    for k, vals in bad.items():
        for v in vals + (float("nan"), float("inf"), "much", None, True):
            with pytest.raises(ValueError, match=k):
                validate_truncation(**{k: v})


def test_engine_truncate_logits_validates_on_cpu_tensors_and_launches_nothing_when_off():
    from clipcap_amd import engine
    x = torch.randn(3, 11)
    keep = x.clone()
    hist = torch.zeros(3, 4, dtype=torch.int64)
    assert engine.truncate_logits(x) is x and torch.equal(x, keep)                          # every rule off: no device is needed
    assert engine.truncate_logits(x, temperature=0.7, history=hist, hist_len=4, repetition_penalty=1.2) is x and torch.equal(x, keep)
    for k, v in (("min_p", 1.5), ("typical_p", 0.0), ("epsilon_cutoff", 1.0), ("eta_cutoff", float("nan"))):
        with pytest.raises(ValueError, match=k):
            engine.truncate_logits(x, **{k: v})
    with pytest.raises(ValueError, match="hist_len"):
        engine.truncate_logits(x, hist_len=2, min_p=0.1)
    with pytest.raises(ValueError, match="hist_len"):
        engine.truncate_logits(x, history=hist, hist_len=-1, min_p=0.1)
    for bad in (lambda: engine.truncate_logits(x.double(), min_p=0.1), lambda: engine.truncate_logits(x[0], min_p=0.1),
                lambda: engine.truncate_logits(x.t(), min_p=0.1), lambda: engine.truncate_logits(x, history=hist.int(), hist_len=2, min_p=0.1),
                lambda: engine.truncate_logits(x, history=hist[:2], hist_len=2, min_p=0.1),
                lambda: engine.truncate_logits(x, history=hist, hist_len=5, min_p=0.1)):
        with pytest.raises(AssertionError):
            bad()
    assert torch.equal(x, keep)


def test_decoders_validate_the_options_before_touching_the_device():
    """A bad option raises ValueError from the decoder itself (no GPU here: anything later would fail differently)."""
    from types import SimpleNamespace
    from clipcap_amd.inference import base, no_beam, nucleus_sampling
    from clipcap_amd.model.gpt2 import GPT2LM
    from tests.test_api_surface import FakeTokenizer
    lm = GPT2LM(n_embd=32, n_layer=1, n_head=2, vocab_size=97, n_positions=16)
    model = SimpleNamespace(language_model=lm)
    emb, tk = torch.zeros(2, 2, 32), FakeTokenizer(97, 5)
    for k, v in (("min_p", -0.5), ("typical_p", 0.0), ("epsilon_cutoff", 1.0), ("eta_cutoff", float("nan"))):
        with pytest.raises(ValueError, match=k):
            base.sample_tokens(model, emb, 4, 5, **{k: v})
        for fn in (base.generate_nucleus_sampling, base.generate_no_beam, no_beam.generate_no_beam, nucleus_sampling.generate_nucleus_sampling):
            with pytest.raises(ValueError, match=k):
                fn(model, tk, emb, **{k: v})
