"""CPU tests of the gradient-clipping surface: the ctypes signatures follow the header, train() takes Lightning's gradient_clip_val
from the namespace (no new CLI flag) and hands it to fused_step, and the generated ABI files are current."""
import argparse
import inspect
import os
import subprocess
import sys

import pytest
import torch

from tests.test_api_surface import FakeTokenizer, _write_dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cc_grad_norm_scratch_floats", "cc_grad_sqnorm", "cc_grad_clip_coef", "cc_adamw_step_clip")


def test_ctypes_signatures_follow_the_header():
    from clipcap_amd import _lib
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_abi
    finally:
        sys.path.pop(0)
    protos = {name: (ret, plist) for ret, name, plist in gen_abi.prototypes(open(gen_abi.HDR).read())}
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
    assert l.cc_grad_norm_scratch_floats() == 1024
    assert l.cc_abi_version() == _lib.ABI_VERSION            # additive change: the version stays


def test_python_surface_has_the_keywords():
    from clipcap_amd.engine import ClipCapEngine, GradClipper, _Arena
    from clipcap_amd.model import ClipCapModel
    from clipcap_amd.model.optim import ArenaAdamW
    assert inspect.signature(ClipCapModel.fused_step).parameters["max_grad_norm"].default is None
    ps = inspect.signature(ClipCapEngine.optimizer_step).parameters
    assert ps["max_grad_norm"].default is None and ps["sync_norm"].default is None
    assert inspect.signature(_Arena.adamw_step).parameters["clip"].default is None
    assert inspect.signature(ArenaAdamW.__init__).parameters["max_grad_norm"].default is None
    assert isinstance(ClipCapModel.last_grad_norm, property)
    assert list(inspect.signature(GradClipper.__init__).parameters)[1:] == ["device", "max_norm"]
    # owned range of partitioned gradients: the slice whose moments the rank holds; whole arena otherwise
    a = _Arena(64, "cpu")
    assert a.grad_range(False) == (0, 64) and a.grad_range(True) == (0, 64)
    a.shard_optimizer_state(1, 2, gather=None)
    assert a.grad_range(True) == (32, 64) and a.grad_range(False) == (0, 64)


def _args(tmp_path, **extra):
    from clipcap_amd.model import add_model_args
    from clipcap_amd.model.gpt2 import GPT2LM
    from clipcap_amd.train import add_training_args
    _write_dataset(tmp_path / "ds", n=16, E=24, shards=(16,))
    lm = GPT2LM(n_embd=64, n_layer=1, n_head=4, vocab_size=157, n_positions=96)
    args = add_model_args(add_training_args(argparse.ArgumentParser())).parse_args([
        "--input-dataset", str(tmp_path / "ds"), "--output-folder", str(tmp_path / "out"), "--language-model", "unused",
        "--batch-size", "8", "--epochs", "1", "--scheduler-warmup-steps", "1", "--checkpoint-filename-prefix", "t",
        "--prefix-length", "4", "--projection-length", "4", "--transformer-layers", "1", "--transformer-attention-heads", "4",
        "--logging-frequency", "1", "--fp-precision", "bf16"])
    for k, v in extra.items():
        setattr(args, k, v)
    return args, lm


@pytest.mark.parametrize("value,expect", [(None, None), (0, None), (0.0, None), (0.5, 0.5), (float("inf"), float("inf"))])
def test_train_hands_gradient_clip_val_to_fused_step(tmp_path, monkeypatch, capsys, value, expect):
    """gradient_clip_val (Lightning's name) on the namespace -> fused_step(max_grad_norm=...); None / 0 = off: the call carries no
    such keyword and the log line no grad_norm."""
    import importlib
    T = importlib.import_module("clipcap_amd.train.train")       # (the package re-exports the function under the same name)
    from clipcap_amd.model import ClipCapModel
    calls = []

    def fused_step(self, batch, lr, reducer=None, **kw):
        calls.append(kw)
        return torch.tensor(1.25)

    monkeypatch.setattr(ClipCapModel, "fused_step", fused_step)
    monkeypatch.setattr(ClipCapModel, "last_grad_norm", property(lambda self: torch.tensor([2.5])))
    monkeypatch.setattr(ClipCapModel, "to", lambda self, *a, **k: self)                 # no GPU here: the model stays where it is
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(T, "DevicePrefetcher", lambda it, device: iter(it))
    args, lm = _args(tmp_path, **({} if value is None else {"gradient_clip_val": value}))
    assert T.train(args, tokenizer=FakeTokenizer(), language_model=lm) == 0
    assert len(calls) == 2
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("epoch ")]
    assert len(lines) == 2
    if expect is None:
        assert all(kw == {} for kw in calls) and all("grad_norm" not in ln for ln in lines)
    else:
        assert all(kw == {"max_grad_norm": expect} for kw in calls) and all(ln.endswith("grad_norm 2.5000") for ln in lines)


def test_no_cli_flag_was_added():
    from clipcap_amd.model import add_model_args
    from clipcap_amd.train import add_training_args
    ns = add_model_args(add_training_args(argparse.ArgumentParser())).parse_args([])
    assert sorted(vars(ns)) == sorted([
        "batch_size", "epochs", "optimizer_lr", "scheduler_warmup_steps", "fp_precision", "checkpoint_save_frequency",
        "checkpoint_filename_prefix", "device", "input_dataset", "output_folder", "reader_max_piece_size", "reader_parallel_pieces",
        "enable_deepspeed", "deepspeed_strategy", "enable_wandb", "wandb_project", "logging_frequency", "language_model", "prefix_length",
        "projection_length", "train_language_model", "transformer_layers", "transformer_attention_heads", "use_positional_embeddings",
        "resume_from"])
    assert not hasattr(ns, "gradient_clip_val")


def test_generated_abi_files_are_current_and_name_the_new_entry_points():
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_abi.py"), "--check"]).returncode == 0
    for f in ("exports.map", "exports_lab.map", "abi_dispatch.cpp"):
        text = open(os.path.join(ROOT, "clipcap_amd", "csrc", f)).read()
        assert all(name in text for name in NEW), f
