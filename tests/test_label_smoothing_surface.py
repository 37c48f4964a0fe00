"""CPU tests of the label-smoothing surface: the three entry points are declared, exported and bound with the header's types (the ABI
version stays), the Python keywords and their defaults, the ValueError on values outside [0, 1), the refusals of the C entry points that
return before the first HIP call, and train() picking the value up from the namespace (no new CLI flag)."""
import argparse
import ctypes as C
import importlib
import inspect
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

from tests.test_api_surface import FakeTokenizer
from tests.test_grad_clip_surface import _args
from tests.test_score_surface import _cfg_shape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cc_lmhead_smooth_scratch_floats", "cc_lmhead_ce_fwd_smooth", "cc_lmhead_ce_bwd_smooth")
ARG, SHAPE = -1, -2


def test_symbols_are_declared_exported_and_bound_with_the_headers_types():
    from clipcap_amd import _lib
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_abi
    finally:
        sys.path.pop(0)
    hdr = open(gen_abi.HDR).read()
    protos = {name: (ret, plist) for ret, name, plist in gen_abi.prototypes(hdr)}
    l = _lib.lib()
    for name in NEW:
        assert name in protos, f"{name} is not declared in include/clipcap_hip.h"
        ret, plist = protos[name]
        res, args = _lib.SIGNATURES[name]
        assert len(args) == len(plist), (name, len(args), len(plist))
        assert res is (_lib._L if ret == "int64_t" else _lib._I)
        for a, p in zip(args, plist):
            want = _lib._GC if "cc_gpt2_cfg" in p else _lib._GS if "cc_gpt2_shape" in p else _lib._P if "*" in p else \
                _lib._F if p.startswith("float ") else _lib._L if p.startswith("int64_t ") else _lib._I
            assert a is want, (name, p)
        assert hasattr(l, name)
        assert name in hdr[hdr.index("ADDED since (still 3"):hdr.index("#define CC_ABI_VERSION")]      # named in the header's list
    assert "#define CC_ABI_VERSION 3" in hdr and l.cc_abi_version() == _lib.ABI_VERSION == 3           # additive change: the version stays
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_abi.py"), "--check"]).returncode == 0
    for f in ("exports.map", "exports_lab.map", "abi_dispatch.cpp"):
        text = open(os.path.join(ROOT, "clipcap_amd", "csrc", f)).read()
        assert all(name in text for name in NEW), f


def test_python_surface_has_the_keywords():
    from clipcap_amd.engine import ClipCapEngine
    from clipcap_amd.model import ClipCapModel, ClipCapModelPrefixOnly
    assert inspect.signature(ClipCapEngine.forward_backward).parameters["label_smoothing"].default == 0.0
    assert inspect.signature(ClipCapModel.fused_step).parameters["label_smoothing"].default is None
    assert ClipCapModel.label_smoothing == 0.0 and ClipCapModelPrefixOnly.label_smoothing == 0.0
    assert isinstance(ClipCapModel.last_nll, property)
    eng = ClipCapEngine(None, None, train_lm=False)
    assert eng.last_nll is None and eng.stats3 is None and eng.smooth_scratch is None


@pytest.mark.parametrize("bad", [-0.1, 1.0, float("nan"), 2.0, float("inf")])
def test_values_outside_the_interval_raise_before_any_launch(bad):
    """engine, fused_step and training_step refuse before they touch an engine, a library or a device (there is none here)"""
    from clipcap_amd.engine import ClipCapEngine, check_label_smoothing
    from clipcap_amd.model import ClipCapModel
    with pytest.raises(ValueError):
        check_label_smoothing(bad)
    with pytest.raises(ValueError):
        ClipCapEngine(None, None, train_lm=False).forward_backward(None, None, label_smoothing=bad)
    with pytest.raises(ValueError):
        ClipCapModel.fused_step(SimpleNamespace(label_smoothing=0.0), (None, None), lr=0.0, label_smoothing=bad)
    with pytest.raises(ValueError):
        ClipCapModel.fused_step(SimpleNamespace(label_smoothing=bad), (None, None), lr=0.0)
    assert check_label_smoothing(0) == 0.0 and check_label_smoothing(0.1) == 0.1


@pytest.mark.parametrize("op", [0, 1, 2])
def test_bad_arguments_are_refused_before_any_hip_call(op):
    from clipcap_amd import _lib
    l = _lib.lib()
    buf = (C.c_char * 64)()                   # never dereferenced: every call below must return before touching the device
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    odd = C.c_void_p(p.value + 4)
    c, s = _cfg_shape(op, mode=1)

    def fwd(eps=0.1, shp=s, scratch=p, **kw):
        a = dict(w32=p, w16=p, ws=p, tok=p, stats=p)
        a.update(kw)
        return l.cc_lmhead_ce_fwd_smooth(C.byref(c), C.byref(shp), a["w32"], a["w16"], a["ws"], a["tok"], eps, scratch, a["stats"], None)

    def bwd(eps=0.1, shp=s, scratch=p, **kw):
        a = dict(w32=p, w16=p, ws=p, denom=p)
        a.update(kw)
        return l.cc_lmhead_ce_bwd_smooth(C.byref(c), C.byref(shp), a["w32"], a["w16"], a["ws"], a["denom"], None, eps, scratch, None, None)
    for f in (fwd, bwd):
        for eps in (-0.1, 1.0, float("nan"), float("inf"), -0.0 - 1e-30):
            assert f(eps=eps) == ARG, (f.__name__, eps)
        assert f(scratch=None) == ARG and f(scratch=odd) == ARG
        assert f(shp=_cfg_shape(op, mode=0)[1]) == ARG
        for eps in (0.0, 0.1):                                            # what the plain entry points refuse is refused here too
            assert f(eps=eps, w32=None) == ARG and f(eps=eps, ws=None) == ARG
    assert fwd(tok=None) == ARG and fwd(stats=None) == ARG and bwd(denom=None) == ARG
    assert fwd(shp=_cfg_shape(op, mode=1, L=0, T=8, cap=8)[1]) == ARG
    assert fwd(shp=_cfg_shape(op, mode=1, cap=9)[1]) == SHAPE
    assert bwd(shp=_cfg_shape(op, mode=2)[1]) == ARG                      # mode 2 without g32
    # the scratch: wbar, hsum, three per-row vectors + the coefficient pairs, the column mean's slice partials; the workspace does not grow
    n = l.cc_lmhead_smooth_scratch_floats(C.byref(c), C.byref(s))
    rows = (s.B * (s.T - s.L) + 3) // 4 * 4
    assert n == 2 * c.D + 4 * rows + min((c.V + 127) // 128, 256) * c.D
    assert l.cc_lmhead_smooth_scratch_floats(C.byref(c), C.byref(_cfg_shape(op, mode=3)[1])) == SHAPE


@pytest.mark.parametrize("value,expect", [(None, 0.0), (0.0, 0.0), (0.1, 0.1)])
def test_train_picks_label_smoothing_up_from_the_namespace(tmp_path, monkeypatch, capsys, value, expect):
    """label_smoothing on the namespace -> the model's attribute, read by fused_step; one line on rank 0 and `nll` in the log when on"""
    T = importlib.import_module("clipcap_amd.train.train")
    from clipcap_amd.model import ClipCapModel
    seen = []

    def fused_step(self, batch, lr, reducer=None, **kw):
        seen.append((self.label_smoothing, kw))
        return torch.tensor(1.25)

    monkeypatch.setattr(ClipCapModel, "fused_step", fused_step)
    monkeypatch.setattr(ClipCapModel, "last_nll", property(lambda self: torch.tensor(0.75)))
    monkeypatch.setattr(ClipCapModel, "to", lambda self, *a, **k: self)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(T, "DevicePrefetcher", lambda it, device: iter(it))
    args, lm = _args(tmp_path, **({} if value is None else {"label_smoothing": value}))
    assert T.train(args, tokenizer=FakeTokenizer(), language_model=lm) == 0
    assert seen == [(expect, {}), (expect, {})]
    out = capsys.readouterr().out.splitlines()
    lines = [ln for ln in out if ln.startswith("epoch ")]
    notes = [ln for ln in out if "label smoothing" in ln]
    assert len(lines) == 2
    if expect > 0:
        assert len(notes) == 1 and "0.1" in notes[0] and all(ln.endswith("loss 1.2500 nll 0.7500") for ln in lines)
    else:
        assert not notes and all("nll" not in ln for ln in lines)


def test_train_refuses_a_bad_value(tmp_path, monkeypatch):
    T = importlib.import_module("clipcap_amd.train.train")
    from clipcap_amd.model import ClipCapModel
    monkeypatch.setattr(ClipCapModel, "to", lambda self, *a, **k: self)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    args, lm = _args(tmp_path, label_smoothing=1.0)
    with pytest.raises(ValueError):
        T.train(args, tokenizer=FakeTokenizer(), language_model=lm)


def test_no_cli_flag_and_no_config_field_were_added():
    from clipcap_amd.model import Config, TrainingConfig, add_model_args
    from clipcap_amd.train import add_training_args
    ns = add_model_args(add_training_args(argparse.ArgumentParser())).parse_args([])
    assert not hasattr(ns, "label_smoothing")
    for cls in (Config, TrainingConfig):
        assert "label_smoothing" not in inspect.signature(cls).parameters
