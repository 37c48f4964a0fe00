"""CPU tests of the per-token loss weights' surface: the two entry points are declared, exported and bound with the header's types (the ABI
version stays), their refusals that return before the first HIP call, the Python keywords and their ValueErrors (raised from types and
shapes alone, before an engine or a device is touched), sample_weights x token_weights, and the self-critical step's construction of
tokens and weights from fixed sampled / greedy ids and a fake reward, with no device."""
import ctypes as C
import inspect
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

from tests.test_score_surface import _cfg_shape

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cc_lmhead_ce_fwd_w", "cc_lmhead_ce_bwd_w")
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
        assert ret == "int" and res is _lib._I
        for a, p in zip(args, plist):
            want = _lib._GC if "cc_gpt2_cfg" in p else _lib._GS if "cc_gpt2_shape" in p else _lib._P if "*" in p else \
                _lib._F if p.startswith("float ") else _lib._L if p.startswith("int64_t ") else _lib._I
            assert a is want, (name, p)
        assert any("row_weight" in p and "const float*" in p for p in plist), name
        assert hasattr(l, name)
        assert name in hdr[hdr.index("ADDED since (still 3"):hdr.index("#define CC_ABI_VERSION")]      # named in the header's list
    assert "#define CC_ABI_VERSION 3" in hdr and l.cc_abi_version() == _lib.ABI_VERSION == 3           # additive change: the version stays
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_abi.py"), "--check"]).returncode == 0
    for f in ("exports.map", "exports_lab.map", "abi_dispatch.cpp"):
        text = open(os.path.join(ROOT, "clipcap_amd", "csrc", f)).read()
        assert all(name in text for name in NEW), f


@pytest.mark.parametrize("op", [0, 1, 2])
def test_bad_arguments_are_refused_before_any_hip_call(op):
    from clipcap_amd import _lib
    l = _lib.lib()
    buf = (C.c_char * 64)()                   # never dereferenced: every call below must return before touching the device
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    odd = C.c_void_p(p.value + 4)
    c, s = _cfg_shape(op, mode=1)

    def fwd(eps=0.1, shp=s, scratch=p, rw=p, **kw):
        a = dict(w32=p, w16=p, ws=p, tok=p, stats=p)
        a.update(kw)
        return l.cc_lmhead_ce_fwd_w(C.byref(c), C.byref(shp), a["w32"], a["w16"], a["ws"], a["tok"], rw, eps, scratch, a["stats"], None)

    def bwd(eps=0.1, shp=s, scratch=p, rw=p, **kw):
        a = dict(w32=p, w16=p, ws=p, denom=p)
        a.update(kw)
        return l.cc_lmhead_ce_bwd_w(C.byref(c), C.byref(shp), a["w32"], a["w16"], a["ws"], a["denom"], None, rw, eps, scratch, None, None)
    for f in (fwd, bwd):
        for eps in (0.0, 0.1):
            assert f(eps=eps, rw=None) == ARG, (f.__name__, eps)                  # the weights are not optional here
            assert f(eps=eps, w32=None) == ARG and f(eps=eps, ws=None) == ARG    # what the plain entry points refuse
            assert f(eps=eps, scratch=odd) == ARG
            assert f(eps=eps, shp=_cfg_shape(op, mode=0)[1]) == ARG
        for eps in (-0.1, 1.0, float("nan"), float("inf")):
            assert f(eps=eps) == ARG, (f.__name__, eps)
        assert f(eps=0.1, scratch=None) == ARG                                    # a NULL scratch only with eps == 0 ...
        assert f(eps=0.0, scratch=None, w32=None) == ARG                          # ... where the next check is the plain chain's
    assert fwd(tok=None) == ARG and fwd(stats=None) == ARG and bwd(denom=None) == ARG
    assert fwd(shp=_cfg_shape(op, mode=1, cap=9)[1]) == SHAPE
    assert fwd(eps=0.0, scratch=None, shp=_cfg_shape(op, mode=1, cap=9)[1]) == SHAPE      # eps == 0 without a scratch gets past the argument check
    assert bwd(shp=_cfg_shape(op, mode=2)[1]) == ARG                              # mode 2 without g32


def test_python_surface_has_the_keywords():
    import clipcap_amd.train as T
    from clipcap_amd.engine import ClipCapEngine
    from clipcap_amd.model import ClipCapModel
    assert inspect.signature(ClipCapEngine.forward_backward).parameters["token_weights"].default is None
    fs = inspect.signature(ClipCapModel.fused_step).parameters
    assert fs["token_weights"].default is None and fs["sample_weights"].default is None
    sc = inspect.signature(T.self_critical_step).parameters
    assert list(sc)[:4] == ["model", "batch_embeds", "reward_fn", "lr"]
    for k in ("temperature", "top_k", "top_p", "entry_length", "generator"):
        assert sc[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    assert sc["temperature"].default == 1.0 and sc["top_k"].default is None and sc["generator"].default is None
    assert any(p.kind is inspect.Parameter.VAR_KEYWORD for p in sc.values())
    assert "suppress_tokens=[0]" in T.self_critical_step.__doc__ and "ignore_index" in T.self_critical_step.__doc__


def _fake_model():
    return SimpleNamespace(label_smoothing=0.0, ema_decay=None)


@pytest.mark.parametrize("bad,kw", [
    (torch.ones(3, 5, dtype=torch.float64), "token_weights"), (torch.ones(3, 5, dtype=torch.float16), "token_weights"),
    (torch.ones(3, 4), "token_weights"), (torch.ones(15), "token_weights"), (torch.ones(3, 5, dtype=torch.int64), "token_weights"),
    ([[1.0] * 5] * 3, "token_weights"), (1.0, "token_weights"),
    (torch.ones(3, dtype=torch.float64), "sample_weights"), (torch.ones(4), "sample_weights"), (torch.ones(3, 1), "sample_weights"),
    ([1.0, 1.0, 1.0], "sample_weights")], ids=lambda v: str(getattr(v, "shape", v)) + str(getattr(v, "dtype", "")) if not isinstance(v, str) else v)
def test_shape_and_dtype_mismatches_raise_before_anything_touches_the_device(bad, kw):
    """engine and fused_step refuse on type, dtype and shape alone: there is no engine, library or device behind these objects, so
    anything that got further would raise something other than ValueError"""
    from clipcap_amd.engine import ClipCapEngine
    from clipcap_amd.model import ClipCapModel
    tokens = torch.zeros(3, 5, dtype=torch.int64)
    with pytest.raises(ValueError, match=kw):
        ClipCapModel.fused_step(_fake_model(), (tokens, None), lr=0.0, **{kw: bad})
    if kw == "token_weights":
        with pytest.raises(ValueError, match=kw):
            ClipCapEngine(None, None, train_lm=False).forward_backward(tokens, None, token_weights=bad)
    ok = torch.ones(3, 5)
    with pytest.raises(ValueError):                                   # a good tensor does not rescue a bad one
        ClipCapModel.fused_step(_fake_model(), (tokens, None), lr=0.0, token_weights=ok if kw == "sample_weights" else bad,
                                sample_weights=bad if kw == "sample_weights" else torch.ones(3))


def test_values_are_not_inspected():
    """NaN, inf, negative and zero weights pass the checks: no value is read (a read would be a host sync on a device tensor)"""
    from clipcap_amd.engine import check_token_weights
    from clipcap_amd.model.model import combine_loss_weights
    w = torch.tensor([[float("nan"), float("inf"), -3.0, 0.0, 1e30]] * 3)
    check_token_weights(w, (3, 5))
    assert combine_loss_weights((3, 5), w, None) is w
    assert combine_loss_weights((3, 5), None, None) is None


def test_sample_weights_and_token_weights_multiply():
    """what fused_step hands the engine: sample_weights broadcast over the caption, times token_weights where both are given"""
    from clipcap_amd.model import ClipCapModel
    tokens = torch.zeros(3, 5, dtype=torch.int64)
    tw = torch.arange(15, dtype=torch.float32).reshape(3, 5) - 4.0
    sw = torch.tensor([2.0, -0.5, 0.0])
    seen = []

    class Stop(Exception):
        pass

    class Eng:
        def zero_grad(self):
            pass

        def forward_backward(self, tok, emb, **kw):
            seen.append(kw)
            raise Stop

    for kw in (dict(token_weights=tw), dict(sample_weights=sw), dict(token_weights=tw, sample_weights=sw), {}):
        m = _fake_model()
        m.engine, m._dropout = Eng(), lambda: None
        with pytest.raises(Stop):
            ClipCapModel.fused_step(m, (tokens, None), lr=0.0, **kw)
    assert torch.equal(seen[0]["token_weights"], tw)
    assert torch.equal(seen[1]["token_weights"], sw.reshape(3, 1).expand(3, 5)) and seen[1]["token_weights"].is_contiguous()
    assert torch.equal(seen[2]["token_weights"], tw * sw.reshape(3, 1))
    assert seen[2]["token_weights"].dtype == torch.float32 and seen[2]["token_weights"].shape == (3, 5)
    assert "token_weights" not in seen[3]                             # neither: exactly the call of a step without the option


STOP = 9
SAMPLED = torch.tensor([[4, 7, STOP, 3, 3], [5, 5, 5, 5, 5], [STOP, 2, STOP, 1, 6], [8, 1, 2, 3, STOP]])
GREEDY = torch.tensor([[4, STOP, 0, 0], [5, 6, 7, STOP], [1, 1, 1, 1], [STOP, 3, 3, 3]])


def _count_reward(ids):
    """minus the number of 5s up to and including the first stop token"""
    hit = ids == STOP
    upto = (hit.cumsum(1) - hit.long()) == 0
    return -((ids == 5) & upto).sum(1).float()


def test_tokens_and_weights_of_a_self_critical_step():
    from clipcap_amd.train import scst_tokens_and_weights
    adv = torch.tensor([1.5, -4.0, 0.0, 0.25])
    tokens, weights = scst_tokens_and_weights(SAMPLED, adv, STOP)
    assert tokens.dtype == torch.int64 and weights.dtype == torch.float32 and weights.is_contiguous()
    assert tokens.tolist() == [[4, 7, STOP, -1, -1], [5, 5, 5, 5, 5], [STOP, -1, -1, -1, -1], [8, 1, 2, 3, STOP]]
    assert torch.equal(weights, adv.reshape(4, 1).expand(4, 5))
    with pytest.raises(ValueError):
        scst_tokens_and_weights(SAMPLED, adv[:3], STOP)


def test_self_critical_step_without_a_device(monkeypatch):
    """the step's plumbing with the decodes replaced by fixed ids: both decodes suppress token 0, the greedy one is top_k = 1 and takes no
    generator, reward_fn gets (sampled, greedy), the loss's tokens stop after the first stop token, the weight is the advantage on every
    position, fused_step's keywords pass through, and the means of the rewards come back"""
    import clipcap_amd.train.self_critical as SC
    calls = []

    def fake_sample_tokens(model, embeds, **kw):
        calls.append(kw)
        ids = GREEDY if kw.get("top_k") == 1 else SAMPLED
        return ids, None

    monkeypatch.setattr(SC, "sample_tokens", fake_sample_tokens)
    steps = []

    def fused_step(batch, lr, **kw):
        steps.append((batch, lr, kw))
        return torch.tensor(0.5)

    gen = torch.Generator().manual_seed(1)
    embeds = torch.zeros(4, 6)
    prefix = torch.zeros(4, 2, 8)
    model = SimpleNamespace(engine=SimpleNamespace(mapper=SimpleNamespace(forward=lambda e, save: prefix)), fused_step=fused_step)
    seen = []

    def reward_fn(sampled, greedy):
        seen.append((sampled, greedy))
        return _count_reward(sampled), _count_reward(greedy)

    loss, r_s, r_g = SC.self_critical_step(model, embeds, reward_fn, 3e-5, temperature=0.7, top_k=40, top_p=0.9, entry_length=5,
                                           stop_token=STOP, generator=gen, max_grad_norm=1.0, label_smoothing=0.1)
    assert len(calls) == 2 and all(c["suppress_tokens"] == [0] and c["entry_length"] == 5 and c["stop_token"] == STOP for c in calls)
    assert calls[0]["generator"] is gen and calls[0]["temperature"] == 0.7 and calls[0]["top_k"] == 40 and calls[0]["top_p"] == 0.9
    assert calls[1]["top_k"] == 1 and calls[1].get("generator") is None and calls[1]["mode"] == 0
    assert seen[0][0] is SAMPLED and seen[0][1] is GREEDY
    rs, rg = torch.tensor([0.0, -5.0, 0.0, 0.0]), torch.tensor([0.0, -1.0, 0.0, 0.0])
    (tokens, emb), lr, kw = steps[0]
    assert emb is embeds and lr == 3e-5 and kw["max_grad_norm"] == 1.0 and kw["label_smoothing"] == 0.1
    assert tokens.tolist() == [[4, 7, STOP, -1, -1], [5, 5, 5, 5, 5], [STOP, -1, -1, -1, -1], [8, 1, 2, 3, STOP]]
    assert torch.equal(kw["token_weights"], (rs - rg).reshape(4, 1).expand(4, 5))
    assert float(loss) == 0.5 and float(r_s) == float(rs.mean()) and float(r_g) == float(rg.mean())
    with pytest.raises(ValueError):
        SC.self_critical_step(model, embeds, reward_fn, 3e-5, token_weights=torch.ones(4, 5))
