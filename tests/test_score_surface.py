"""CPU tests of the caption-scoring surface: cc_lmhead_score is declared, exported, bound and refuses bad calls before any HIP call;
the public Python entry points exist; and the workspace layout of every shape that existed before scoring is byte-identical
(tests/golden/gpt2_ws_bytes.json: cc_gpt2_ws_bytes recorded from the commit before cc_lmhead_score), while the scoring shape itself
never holds a [B cap, Vp] logits matrix."""
import ctypes as C
import inspect
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPT2_SMALL = dict(D=768, H=12, NL=12, V=50257, Vp=50304, NPOS=1024)


def _nm(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_header_declares_cc_lmhead_score():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "clipcap_hip.h")).read(), flags=re.S)
    m = re.search(r"^int\s+cc_lmhead_score\s*\(([^;]*?)\)\s*;", hdr, flags=re.M | re.S)
    assert m, "cc_lmhead_score is not declared in include/clipcap_hip.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["const cc_gpt2_cfg* cfg", "const cc_gpt2_shape* shp", "const float* w32", "const uint16_t* w16", "void* ws",
                      "const int64_t* tokens", "int32_t ignore_zero", "float* token_logprob", "float* sample_stats", "void* stream"]


def test_both_libraries_export_cc_lmhead_score():
    if shutil.which("nm") is None:
        pytest.skip("binutils nm not available")
    for name in ("libclipcap_hip.so", "libclipcap_hip_lab.so"):
        lib = os.path.join(ROOT, "clipcap_amd", name)
        assert os.path.exists(lib), f"{name} has not been built"
        exported = _nm(lib)
        assert "cc_lmhead_score" in exported, f"{name} does not export cc_lmhead_score"
        assert not {n for n in exported if n.startswith("cc_lmhead_score_")}, "the per-operand-type variants stay local"


def test_ctypes_signature_and_abi_version():
    from clipcap_amd import _lib
    assert "cc_lmhead_score" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["cc_lmhead_score"]
    assert res is C.c_int32 and len(args) == 10 and args[6] is C.c_int32
    l = _lib.lib()
    assert hasattr(l, "cc_lmhead_score")
    assert l.cc_abi_version() == 3 and _lib.ABI_VERSION == 3          # additive change: the version stays


def test_generated_abi_files_are_current_and_carry_the_entry_point():
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_abi.py"), "--check"]).returncode == 0
    csrc = os.path.join(ROOT, "clipcap_amd", "csrc")
    for f in ("abi_dispatch.cpp", "exports.map", "exports_lab.map"):
        assert "cc_lmhead_score" in open(os.path.join(csrc, f)).read(), f


def test_public_python_surface():
    import clipcap_amd.inference as inf
    import clipcap_amd.train as tr
    from clipcap_amd.engine import ClipCapEngine
    assert callable(inf.score_captions) and callable(inf.rerank_captions) and callable(tr.evaluate)
    sig = inspect.signature(inf.generate_nucleus_sampling)
    assert "rerank" in sig.parameters and sig.parameters["rerank"].default is False
    p = inspect.signature(inf.score_captions).parameters
    assert list(p)[:3] == ["model", "embeds", "tokens"]
    for k, d in (("text_prefix_tokens", None), ("ignore_zero", False), ("from_prefix", False)):
        assert p[k].kind is inspect.Parameter.KEYWORD_ONLY and p[k].default is d
    p = inspect.signature(inf.rerank_captions).parameters
    assert list(p)[:3] == ["model", "prefix", "candidates"] and p["length_normalise"].default is True
    p = inspect.signature(tr.evaluate).parameters
    assert list(p)[:4] == ["model", "dataset_path", "batch_size", "max_batches"] and p["batch_size"].default == 256 and p["max_batches"].default is None
    p = inspect.signature(ClipCapEngine.score).parameters
    assert list(p)[:3] == ["self", "tokens", "embeds"]
    for k, d in (("prefix", None), ("ignore_zero", False), ("chunk", None)):
        assert p[k].kind is inspect.Parameter.KEYWORD_ONLY and p[k].default is d
    assert inf.CaptionScores._fields == ("token_logprobs", "logprob", "num_tokens")
    # evaluate() is a function, not a flag: the trainer's flag set stays the reference's (tests/test_api_surface.py pins it)
    import argparse
    from clipcap_amd.train import add_training_args
    flags = {o for a in add_training_args(argparse.ArgumentParser())._actions for o in a.option_strings}
    assert not {f for f in flags if "eval" in f or "score" in f or "rerank" in f}


def _cfg_shape(op=0, mode=0, B=4, L=4, T=12, cap=8, **cfg):
    from clipcap_amd._lib import Gpt2Cfg, Gpt2Shape
    d = dict(D=128, H=4, NL=2, V=300, Vp=384, NPOS=32)
    d.update(cfg)
    return Gpt2Cfg(op_dtype=op, **d), Gpt2Shape(B, L, T, cap, mode, 0.0, 0.0, 0.0, 0)


@pytest.mark.parametrize("op", [0, 1, 2])
def test_bad_arguments_are_refused_before_any_hip_call(op):
    from clipcap_amd import _lib
    l = _lib.lib()
    ARG, SHAPE = -1, -2
    buf = C.create_string_buffer(64)          # never dereferenced: every call below must return before touching the device
    p = C.cast(buf, C.c_void_p)
    c, s = _cfg_shape(op)

    def call(cfg=c, shp=s, w32=p, w16=p, ws=p, tok=p, out=p, st=p):
        return l.cc_lmhead_score(C.byref(cfg) if cfg is not None else None, C.byref(shp) if shp is not None else None, w32, w16, ws, tok, 0, out,
                                 st, None)
    for kw in ({"w32": None}, {"w16": None}, {"ws": None}, {"tok": None}, {"out": None}, {"st": None}, {"shp": None}):
        assert call(**kw) == ARG, kw
    assert l.cc_lmhead_score(None, C.byref(s), p, p, p, p, 0, p, p, None) == ARG
    for mode in (1, 2):                                                   # the training modes keep the training entry points
        assert call(shp=_cfg_shape(op, mode=mode)[1]) == ARG
    assert call(shp=_cfg_shape(op, L=0, T=8, cap=8)[1]) == ARG           # no prefix row to predict the first token from
    assert call(shp=_cfg_shape(op, L=12, T=12, cap=0)[1]) == SHAPE       # no caption rows
    assert call(shp=_cfg_shape(op, L=4, T=12, cap=9)[1]) == SHAPE        # cap must be T - L: every token column is scored


@pytest.mark.parametrize("op", [0, 1, 2])
def test_workspace_layout(op):
    """Shapes that existed before scoring (mode >= 1, and mode 0 without caption rows) keep the byte counts the commit before
    cc_lmhead_score returned; the scoring shape adds the softmax partials and four per-row vectors to the forward-only pass, and
    never a [B cap, Vp] logits matrix."""
    from clipcap_amd import _lib
    from clipcap_amd._lib import Gpt2Cfg, Gpt2Shape
    rows = [r for r in json.load(open(os.path.join(ROOT, "tests", "golden", "gpt2_ws_bytes.json"))) if r["cfg"]["op_dtype"] == op]
    assert len([r for r in rows if r["shape"]["mode"] >= 1]) >= 12 and [r for r in rows if r["shape"]["mode"] == 0]
    l = _lib.lib()
    for r in rows:
        sh = r["shape"]
        assert sh["mode"] >= 1 or sh["cap"] == 0 == sh["T"] - sh["L"]
        s = Gpt2Shape(sh["B"], sh["L"], sh["T"], sh["cap"], sh["mode"], sh.get("p_embd", 0.0), sh.get("p_attn", 0.0), sh.get("p_resid", 0.0),
                      sh.get("drop_seed", 0))
        got = l.cc_gpt2_ws_bytes(C.byref(Gpt2Cfg(**r["cfg"])), C.byref(s))
        assert got == r["bytes"], (r["cfg"], sh, got, r["bytes"])
    B, L, T = 256, 10, 50
    cap = T - L
    c, s = _cfg_shape(op, mode=0, B=B, L=L, T=T, cap=cap, **GPT2_SMALL)
    n = l.cc_gpt2_ws_bytes(C.byref(c), C.byref(s))
    # the matrix the training pass stores and this pass must not: 2 bytes per element with 16-bit operands; the split-bf16 build keeps
    # fp32 activations (its forward-only pass without any caption rows is already larger than the 16-bit matrix), so there the
    # yardstick is that build's own smallest form of the matrix, 4 bytes per element
    logits_bytes = B * cap * GPT2_SMALL["Vp"] * (4 if op == 2 else 2)
    assert 0 < n < logits_bytes, (n, logits_bytes)
    c0, s0 = _cfg_shape(op, mode=0, B=B, L=T, T=T, cap=0, **GPT2_SMALL)
    n0 = l.cc_gpt2_ws_bytes(C.byref(c0), C.byref(s0))
    extra = B * cap * (2 * (GPT2_SMALL["Vp"] // 64) + 3) * 4
    assert 0 <= n - n0 - extra <= 5 * 256, (n, n0, extra)                # (256-byte alignment of the five buffers)
    # the training shape of the same batch does hold the matrix
    c1, s1 = _cfg_shape(op, mode=1, B=B, L=L, T=T, cap=cap, **GPT2_SMALL)
    assert l.cc_gpt2_ws_bytes(C.byref(c1), C.byref(s1)) > n + logits_bytes
