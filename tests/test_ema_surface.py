"""CPU tests of the weight-average surface: cc_adamw_step_ema is declared, exported and bound with the header's types (the ABI version
stays), its refusals return before the first HIP call, the Python keywords and their defaults, train() picking the value up from the
namespace (no CLI flag, no keyword to fused_step), the checkpoint keys and files, and the sharded average on 3 gloo ranks."""
import argparse
import ctypes as C
import importlib
import inspect
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import ema_ref as R
from tests.test_api_surface import FakeTokenizer
from tests.test_ddp_gloo import _free_port
from tests.test_grad_clip_surface import _args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cc_adamw_step_ema",)
ARG, SHAPE = -1, -2


def test_symbol_is_declared_exported_and_bound_with_the_headers_types():
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
            want = _lib._P if "*" in p else _lib._F if p.startswith("float ") else _lib._L if p.startswith("int64_t ") else _lib._I
            assert a is want, (name, p)
        assert hasattr(l, name)
        assert name in hdr[hdr.index("ADDED since (still 3"):hdr.index("#define CC_ABI_VERSION")]      # named in the header's list
    # cc_adamw_step_clip's parameters, then the average and its decay in front of the stream
    clip, ema = protos["cc_adamw_step_clip"][1], protos["cc_adamw_step_ema"][1]
    assert [p.split()[-1] for p in ema] == [p.split()[-1] for p in clip[:-1]] + ["ema", "ema_decay", "stream"]
    assert "#define CC_ABI_VERSION 3" in hdr and l.cc_abi_version() == _lib.ABI_VERSION == 3           # additive change: the version stays
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_abi.py"), "--check"]).returncode == 0
    for f in ("exports.map", "exports_lab.map", "abi_dispatch.cpp"):
        text = open(os.path.join(ROOT, "clipcap_amd", "csrc", f)).read()
        assert all(name in text for name in NEW), f


def test_no_cli_flag_and_no_config_field_were_added():
    from clipcap_amd.model import Config, TrainingConfig, add_model_args
    from clipcap_amd.train import add_training_args
    ns = add_model_args(add_training_args(argparse.ArgumentParser())).parse_args([])
    for name in ("ema_decay", "ema_warmup"):
        assert not hasattr(ns, name)
        for cls in (Config, TrainingConfig):
            assert name not in inspect.signature(cls).parameters


@pytest.mark.parametrize("bad", [-0.1, 1.0, 1.5, float("nan"), float("inf")])
def test_values_outside_the_interval_raise_before_anything_is_touched(bad):
    from clipcap_amd.engine import _Arena, check_ema_decay
    from clipcap_amd.model import ClipCapModel
    from clipcap_amd.model.optim import ArenaAdamW
    with pytest.raises(ValueError):
        check_ema_decay(bad)
    with pytest.raises(ValueError):
        ClipCapModel.fused_step(SimpleNamespace(label_smoothing=0.0, ema_decay=None), (None, None), lr=0.0, ema_decay=bad)
    with pytest.raises(ValueError):
        ClipCapModel.fused_step(SimpleNamespace(label_smoothing=0.0, ema_decay=bad), (None, None), lr=0.0)
    a = _Arena(16, "cpu")
    with pytest.raises(ValueError):
        a.adamw_step(1e-3, 1, ema_decay=bad)
    assert a.ema is None and a.m is None                 # refused before the average or the moments were created
    with pytest.raises(ValueError):
        ArenaAdamW([], ema_decay=bad)


def test_accepted_values_and_the_python_surface():
    from clipcap_amd.engine import ClipCapEngine, _Arena, check_ema_decay
    from clipcap_amd.model import ClipCapModel, ClipCapModelPrefixOnly
    from clipcap_amd.model.optim import ArenaAdamW
    from clipcap_amd.train.train import evaluate
    assert check_ema_decay(None) is None and check_ema_decay(0) == 0.0 and check_ema_decay(0.999) == 0.999
    assert isinstance(check_ema_decay(0), float)
    assert inspect.signature(ClipCapModel.fused_step).parameters["ema_decay"].default is None
    assert inspect.signature(_Arena.adamw_step).parameters["ema_decay"].default is None
    assert inspect.signature(ArenaAdamW.__init__).parameters["ema_decay"].default is None
    ev = inspect.signature(evaluate).parameters["ema"]
    assert ev.default is False and ev.kind is inspect.Parameter.KEYWORD_ONLY
    for cls in (ClipCapModel, ClipCapModelPrefixOnly):
        assert cls.ema_decay is None and cls.ema_warmup is False and cls.ema_updates == 0
    assert "ema_decay" in ClipCapEngine.optimizer_step.__doc__
    for name in ("ema_state_dict", "ema_weights"):
        assert callable(getattr(ClipCapModel, name))
    a = _Arena(64, "cpu")
    assert a.ema is None and a.full_ema() is None and a.ema_on_device() is None
    a.w32.copy_(torch.arange(64.0))
    a.enable_ema()
    assert torch.equal(a.ema, a.w32) and a.ema.data_ptr() != a.w32.data_ptr()
    assert a.full_ema() is a.ema and a.ema_on_device() is a.ema                  # replicated state: the tensor itself
    first = a.ema
    a.enable_ema()
    assert a.ema is first                                                          # already enabled: kept
    b = a.moved_to("cpu", None)
    assert torch.equal(b.ema, a.ema) and torch.equal(b.w32, a.w32)                # moved_to carries the average


@pytest.mark.parametrize("op", [0, 1, 2])
def test_bad_arguments_are_refused_before_any_hip_call(op):
    from clipcap_amd import _lib
    l = _lib.lib()
    buf = (C.c_char * 512)()                  # never dereferenced: every call below must return before touching the device
    base = (C.addressof(buf) + 15) & ~15
    p, e = C.c_void_p(base), C.c_void_p(base + 256)
    scale = C.c_void_p(base + 128)

    def step(n=8, ema=e, d=0.9, w16=None, stp=3, ls=None, **kw):
        a = dict(p=p, g=p, m=p, v=p)
        a.update(kw)
        return l.cc_adamw_step_ema(op, a["p"], a["g"], a["m"], a["v"], n, 1e-3, 0.9, 0.999, 1e-8, 0.01, stp, 1.0, ls, None, None, w16, ema, d, None)
    assert step(ema=None) == ARG
    assert step(ema=C.c_void_p(e.value + 4)) == ARG and step(ema=C.c_void_p(e.value + 8)) == ARG            # misaligned
    assert step(ema=p) == ARG                                                                              # the parameters themselves
    assert step(ema=C.c_void_p(p.value + 16)) == ARG and step(n=16, ema=C.c_void_p(p.value + 48)) == ARG   # overlapping them
    assert step(p=C.c_void_p(e.value + 16), n=8) == ARG                                                    # ... from the other side
    for d in (-0.1, 1.0, 1.5, float("nan"), float("inf"), -float("inf")):
        assert step(d=d) == ARG, d
    assert step(n=6) == SHAPE and step(n=6, d=0.0) == SHAPE
    assert step(n=6, ema=None) == ARG and step(n=6, d=1.0) == ARG              # the argument checks come first
    assert step(n=0) == 0 and step(n=0, d=0.0) == 0                              # no-op
    assert step(n=-4) == ARG and step(p=None) == ARG and step(g=None) == ARG and step(m=None) == ARG and step(v=None) == ARG
    assert step(stp=-1) == ARG and step(stp=0) == ARG                            # step 0 needs the loss scaler's state
    assert step(n=0, stp=0, ls=scale) == 0
    if op == 2:
        assert step(w16=p) == ARG                                                # no flat cast in the split-bf16 mode, as cc_adamw_step_clip
    else:
        assert step(n=0, w16=p) == 0


@pytest.mark.parametrize("value,warm", [(None, False), (0.999, False), (0.999, True)])
def test_train_picks_ema_up_from_the_namespace(tmp_path, monkeypatch, capsys, value, warm):
    """ema_decay / ema_warmup on the namespace -> the model's attributes, read by fused_step; fused_step itself sees no keyword; one line
    on rank 0 when the average is on, none when it is off; with the step mocked no average exists, so no file is added"""
    T = importlib.import_module("clipcap_amd.train.train")
    from clipcap_amd.model import ClipCapModel
    seen = []

    def fused_step(self, batch, lr, reducer=None, **kw):
        seen.append((self.ema_decay, self.ema_warmup, kw))
        return torch.tensor(1.25)

    monkeypatch.setattr(ClipCapModel, "fused_step", fused_step)
    monkeypatch.setattr(ClipCapModel, "to", lambda self, *a, **k: self)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(T, "DevicePrefetcher", lambda it, device: iter(it))
    extra = {} if value is None else {"ema_decay": value}
    if warm:
        extra["ema_warmup"] = True
    args, lm = _args(tmp_path, **extra)
    assert T.train(args, tokenizer=FakeTokenizer(), language_model=lm) == 0
    assert seen == [(value, warm, {})] * 2
    out = capsys.readouterr().out.splitlines()
    notes = [ln for ln in out if ln.startswith("clipcap_amd:") and " ema " in ln]
    if value is None:
        assert not notes
    else:
        assert len(notes) == 1 and "0.999" in notes[0] and ("warm-up" in notes[0]) == warm
    assert sorted(os.listdir(tmp_path / "out")) == ["t_config.yaml", "t_epoch_0.ckpt", "t_final.ckpt"]
    assert "ema_state" not in torch.load(tmp_path / "out" / "t_final.ckpt", map_location="cpu")


def test_train_refuses_a_bad_value(tmp_path, monkeypatch):
    T = importlib.import_module("clipcap_amd.train.train")
    from clipcap_amd.model import ClipCapModel
    monkeypatch.setattr(ClipCapModel, "to", lambda self, *a, **k: self)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    args, lm = _args(tmp_path, ema_decay=1.0)
    with pytest.raises(ValueError):
        T.train(args, tokenizer=FakeTokenizer(), language_model=lm)


def _cpu_model(tmp_path, full):
    from clipcap_amd.encoders import EncoderConfig
    from clipcap_amd.model import ClipCapModel, ClipCapModelPrefixOnly, Config, TrainingConfig
    from clipcap_amd.model.gpt2 import GPT2LM
    lm = GPT2LM(n_embd=64, n_layer=2, n_head=4, vocab_size=157, n_positions=40)
    lm_dir = tmp_path / "lm"
    lm.save_pretrained(str(lm_dir))
    cfg = Config(language_model=str(lm_dir), train_language_model=full, prefix_length=3, projection_length=2, transformer_layers=2,
                 transformer_attention_heads=4, encoder_config=EncoderConfig(encoder_embedding_size=24), training_config=TrainingConfig(total_steps=3))
    return (ClipCapModel if full else ClipCapModelPrefixOnly)(cfg), cfg


@pytest.mark.parametrize("full", [False, True])
def test_checkpoints_carry_the_average_and_load_reads_the_averaged_file(tmp_path, full):
    """CheckpointSaver on a CPU model whose trained arenas carry a hand-filled average: ema_state in every .ckpt, <prefix>_final_ema.ckpt
    whose state_dict is ema_state_dict(), read by load() with no change; resume() restores the average and its step count"""
    from clipcap_amd.model import load
    from clipcap_amd.train.callback import CheckpointSaver, resume
    m, cfg = _cpu_model(tmp_path, full)
    ma, la = m.transformer_mapper.engine.arena, m.language_model.engine.arena
    saver = CheckpointSaver(str(tmp_path / "off"), "demo")
    saver.save_config(cfg.to_dict())
    saver.on_epoch_end(m, 0)
    saver.save_final_checkpoint(m)
    assert sorted(os.listdir(tmp_path / "off")) == ["demo_config.yaml", "demo_epoch_0.ckpt", "demo_final.ckpt"]      # the reference's three names
    assert "ema_state" not in torch.load(tmp_path / "off" / "demo_final.ckpt", map_location="cpu")
    plain = {k: v.clone() for k, v in m.state_dict().items()}
    assert all(torch.equal(v, plain[k]) for k, v in m.ema_state_dict().items())                                    # no average: the weights

    m.ema_decay, m.ema_warmup, m.ema_updates = 0.99, True, 7
    ma.enable_ema()
    ma.ema.mul_(0.5).add_(0.25)
    la.enable_ema()                                        # a frozen language model's average (should one exist) is never used
    la.ema.mul_(-2.0).sub_(0.125)
    avg = m.ema_state_dict()
    assert list(avg) == list(plain) and all(avg[k].shape == plain[k].shape for k in plain)
    for k in plain:
        if k.startswith("transformer_mapper."):
            assert torch.equal(avg[k], plain[k] * 0.5 + 0.25), k
        elif full:
            assert torch.equal(avg[k], plain[k] * -2.0 - 0.125), k
        else:
            assert torch.equal(avg[k], plain[k]), k
    assert all(torch.equal(v, plain[k]) for k, v in m.state_dict().items())                                        # the weights are untouched
    saver = CheckpointSaver(str(tmp_path / "on"), "demo")
    saver.save_config(cfg.to_dict())
    saver.on_epoch_end(m, 0)
    saver.save_final_checkpoint(m)
    assert sorted(os.listdir(tmp_path / "on")) == ["demo_config.yaml", "demo_epoch_0.ckpt", "demo_final.ckpt", "demo_final_ema.ckpt"]
    for f in ("demo_epoch_0.ckpt", "demo_final.ckpt"):
        ck = torch.load(tmp_path / "on" / f, map_location="cpu")
        es = ck["ema_state"]
        assert sorted(es) == sorted(["mapper", "decay", "warmup", "updates"] + (["lm"] if full else []))
        assert es["decay"] == 0.99 and es["warmup"] is True and es["updates"] == 7
        assert torch.equal(es["mapper"], ma.ema) and (not full or torch.equal(es["lm"], la.ema))
        assert all(torch.equal(v, plain[k]) for k, v in ck["state_dict"].items())
    m2, _ = load(str(tmp_path / "on" / "demo_final_ema.ckpt"), str(tmp_path / "on" / "demo_config.yaml"), device="cpu", from_checkpoint=True,
                 tokenizer=FakeTokenizer())
    got = m2.state_dict()
    for k in plain:
        assert torch.equal(got[k], avg[k]), k
    # resume: the average and its count come back; a checkpoint without one clears an average enabled before (it restarts at the weights)
    m3, _ = _cpu_model(tmp_path, full)
    resume(m3, str(tmp_path / "on" / "demo_final.ckpt"))
    a3 = m3.transformer_mapper.engine.arena
    assert torch.equal(a3.ema, ma.ema) and m3.ema_updates == 7
    assert (m3.language_model.engine.arena.ema is not None) == full
    resume(m3, str(tmp_path / "off" / "demo_final.ckpt"))
    assert a3.ema is None and m3.language_model.engine.arena.ema is None


def test_ema_weights_swaps_and_restores_on_a_cpu_model(tmp_path):
    m, _ = _cpu_model(tmp_path, True)
    ma, la = m.transformer_mapper.engine.arena, m.language_model.engine.arena
    ma.enable_ema()
    ma.ema.add_(1.0)
    keep_m, keep_l = ma.w32.clone(), la.w32.clone()
    with m.ema_weights() as inner:
        assert inner is m
        assert torch.equal(ma.w32, ma.ema) and torch.equal(la.w32, keep_l)          # no average on the language model: its weights stay
        inside, avg = m.state_dict(), m.ema_state_dict()
        assert all(torch.equal(inside[k], avg[k]) for k in avg)
    assert torch.equal(ma.w32, keep_m) and torch.equal(la.w32, keep_l)
    with pytest.raises(KeyError):
        with m.ema_weights():
            raise KeyError("inside")
    assert torch.equal(ma.w32, keep_m) and torch.equal(ma.ema, keep_m + 1.0)


def _emulate(n, steps, d):
    """the replicated run: 'parameters' move by a seeded step, the average follows in torch fp32 (the kernel's convex form)"""
    gen = torch.Generator().manual_seed(31)
    w = torch.randn(n, generator=gen)
    ema = w.clone()
    for _ in range(steps):
        w = w + 0.1 * torch.randn(n, generator=gen)
        ema = R.ema_convex_f32(ema, w, d)
    return w, ema


def _shard_worker(rank, world, port, out, enable_first):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from clipcap_amd.engine import _Arena
    from clipcap_amd.train.ddp import ZeroShard
    n, d = 1003, 0.9
    gen = torch.Generator().manual_seed(31)
    a = _Arena(n, "cpu")
    a.w32.copy_(torch.randn(n, generator=gen))
    if enable_first:
        a.enable_ema()                                   # full-size: shard_optimizer_state cuts it down to the own range
        assert a.ema.numel() == n
    ZeroShard(rank, world).apply([a])
    if not enable_first:
        a.enable_ema()                                   # after sharding: the own range only
    _, ranges, gather = a.zero
    lo, hi = ranges[rank]
    assert a.ema.numel() == hi - lo and torch.equal(a.ema, a.w32[lo:hi])
    for _ in range(3):
        step = 0.1 * torch.randn(n, generator=gen)      # the same on every rank
        a.w32[lo:hi] += step[lo:hi]                      # the own slice is stepped and averaged, then the owners' slices travel
        a.ema.copy_(R.ema_convex_f32(a.ema, a.w32[lo:hi], d))
        gather(a.w32, ranges)
    own = a.ema.clone()
    full, dev = a.full_ema(), a.ema_on_device()          # collectives
    assert torch.equal(a.ema, own) and dev.numel() == n and full.numel() == n
    np.savez(f"{out}.{rank}.npz", full=full.numpy(), dev=dev.numpy(), w=a.w32.numpy(), lo=lo, hi=hi)
    dist.destroy_process_group()


@pytest.mark.parametrize("enable_first", [False, True])
def test_sharded_average_three_ranks(tmp_path, enable_first):
    """3 gloo ranks with uneven slices: each rank averages its own slice; full_ema() and ema_on_device() equal the replicated average bit
    for bit on every rank, whether the average was enabled before or after sharding"""
    out = str(tmp_path / "ema")
    mp.spawn(_shard_worker, args=(3, _free_port(), out, enable_first), nprocs=3, join=True)
    w, ema = _emulate(1003, 3, 0.9)
    spans = []
    for rank in range(3):
        res = np.load(f"{out}.{rank}.npz")
        assert np.array_equal(res["w"], w.numpy())
        assert np.array_equal(res["full"], ema.numpy()) and np.array_equal(res["dev"], ema.numpy()), rank
        spans.append((int(res["lo"]), int(res["hi"])))
    assert spans[0][0] == 0 and spans[-1][1] == 1003 and len({hi - lo for lo, hi in spans}) > 1       # uneven slices
