"""CPU tests of the MLP mapping network's surface: arena layout and refusals of the C ABI, the nn.Module's state-dict keys, the Config
switch and its yaml schema, the converter for original ClipCap state dicts, the header / binding bookkeeping, and the launch plans the
weight gradients get at the real shape (tests/mlp_plan_check.cpp, compiled with the host compiler alone)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
from argparse import Namespace

import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cc_mlp_param_count", "cc_mlp_param_offsets", "cc_mlp_ws_bytes", "cc_mlp_sync_weights", "cc_mlp_transpose_weights", "cc_mlp_fwd",
       "cc_mlp_bwd", "cc_mlp_bwd_part", "cc_mlp_get", "cc_gemm_tanh"]


def _cfg(E, D, L, Hd=None, op=0):
    from clipcap_amd import _lib
    return _lib.MlpCfg(E=E, D=D, L=L, Hd=(L * D) // 2 if Hd is None else Hd, op_dtype=op)


@pytest.mark.parametrize("E,D,L", [(24, 32, 3), (16, 40, 10), (512, 768, 10)])
@pytest.mark.parametrize("op", [0, 1, 2])
def test_param_count_and_offsets(E, D, L, op):
    from clipcap_amd import _lib
    l = _lib.lib()
    c = _cfg(E, D, L, op=op)
    Hd, LD = L * D // 2, L * D
    n = l.cc_mlp_param_count(C.byref(c))
    assert n == Hd * E + Hd + LD * Hd + LD
    if (E, D, L) == (512, 768, 10):
        assert n == 31_468_800
    offs = (C.c_int64 * 4)()
    assert l.cc_mlp_param_offsets(C.byref(c), offs) == 0
    assert list(offs) == [0, Hd * E, Hd * E + Hd, Hd * E + Hd + LD * Hd]
    assert all(o % 8 == 0 for o in offs)                       # 16-byte starts in the 16-bit arena
    small, big = l.cc_mlp_ws_bytes(C.byref(c), 4, 0), l.cc_mlp_ws_bytes(C.byref(c), 4, 1)
    assert 0 < small < big and small % 256 == 0 and big % 256 == 0
    assert big >= l.cc_wgrad_scratch_bytes() + 4 * l.cc_red_scratch_floats()


def test_refusals():
    from clipcap_amd import _lib
    l = _lib.lib()
    offs = (C.c_int64 * 4)()
    bad = [_cfg(20, 32, 3), _cfg(24, 36, 3), _cfg(24, 40, 3),      # E, D not multiples of 8; L D = 120 not a multiple of 16
           _cfg(24, 32, 3, Hd=40), _cfg(24, 32, 3, Hd=96), _cfg(24, 32, 0, Hd=8), _cfg(24, 32, 3, op=3)]
    for c in bad:
        assert l.cc_mlp_param_count(C.byref(c)) == -2 and l.cc_mlp_param_offsets(C.byref(c), offs) == -2
        assert l.cc_mlp_ws_bytes(C.byref(c), 4, 1) == -2
        assert l.cc_mlp_sync_weights(C.byref(c), None, None, None) == -1 and l.cc_mlp_fwd(C.byref(c), 4, None, None, None, None, None, 0, None) == -1
        assert l.cc_mlp_bwd(C.byref(c), 4, None, None, None, None, None, None) == -1
    good = _cfg(24, 32, 3)
    for B in (0, -1, -2 ** 31):
        assert l.cc_mlp_ws_bytes(C.byref(good), B, 0) == -2 and l.cc_mlp_ws_bytes(C.byref(good), B, 1) == -2
    assert l.cc_mlp_param_count(None) == -2 and l.cc_mlp_param_offsets(C.byref(good), None) == -2
    # NULL buffers and undersized calls return before anything is launched (no GPU here: a launch would fail differently)
    assert l.cc_mlp_fwd(C.byref(good), 4, None, None, None, None, None, 1, None) == -1
    assert l.cc_mlp_bwd_part(C.byref(good), 4, None, None, None, None, None, 1, None) == -1
    assert l.cc_mlp_get(C.byref(good), 4, None, 0, None, 0, None) == -1
    assert l.cc_gemm_tanh(0, 0, 0, None, 0, 8, None, 8, 8, 8, 8, None, 0, 8, None, None, 0, None, 0, None) == -1
    from clipcap_amd.engine import MlpMapperEngine
    for E, D, Lp in ((20, 32, 3), (24, 36, 3), (24, 40, 3), (24, 8, 3)):
        with pytest.raises(_lib.CCError):
            MlpMapperEngine(E, D, Lp)


def test_module_state_dict_on_a_cpu_arena():
    from clipcap_amd.model import MLPMapper
    from clipcap_amd.model.arena_module import ArenaModule
    torch.manual_seed(0)
    m = MLPMapper(24, 32, 3)
    assert isinstance(m, ArenaModule)
    sd = m.state_dict()
    assert list(sd) == ["model.0.weight", "model.0.bias", "model.2.weight", "model.2.bias"]
    assert [tuple(v.shape) for v in sd.values()] == [(48, 24), (48,), (96, 48), (96,)]
    e = m.engine
    assert e.dims == dict(E=24, D=32, L=3, Hd=48, W=1) and e.arena.n == 48 * 24 + 48 + 96 * 48 + 96 and e.arena.w16 is None
    # nn.Linear defaults: U(+-1/sqrt(fan_in)) for weight and bias, nothing left at zero
    for k, fan in (("model.0.weight", 24), ("model.0.bias", 24), ("model.2.weight", 48), ("model.2.bias", 48)):
        assert 0.5 / fan ** 0.5 < sd[k].abs().max().item() <= 1.0 / fan ** 0.5
    # the parameters ARE the arena, and an original nn.Sequential's tensors load by name
    seq = torch.nn.Sequential(torch.nn.Linear(24, 48), torch.nn.Tanh(), torch.nn.Linear(48, 96))
    m.load_state_dict({"model." + k: v for k, v in seq.state_dict().items()})
    assert torch.equal(e.arena.w32[:48 * 24].view(48, 24), seq[0].weight.detach()) and torch.equal(e.arena.w32[-96:], seq[2].bias.detach())
    with pytest.raises(RuntimeError):
        m(torch.randn(2, 24))                      # no CPU fallback
    with pytest.raises(ValueError):
        e.forward(torch.randn(2, 3, 24))           # windowed input is refused before anything else


def test_config_switch_and_yaml_schema(tmp_path):
    from clipcap_amd.encoders import EncoderConfig
    from clipcap_amd.model import Config
    reference_keys = ["language_model", "train_language_model", "prefix_length", "projection_length", "transformer_layers",
                      "transformer_attention_heads", "use_positional_embeddings", "encoder_config", "training_config"]
    assert list(Config().to_dict()) == reference_keys and Config().mapping_type == "transformer"
    assert list(Config(mapping_type="transformer", encoder_config=EncoderConfig()).to_dict()) == reference_keys
    cfg = Config(language_model="gpt2", train_language_model=True, prefix_length=10, mapping_type="mlp",
                 encoder_config=EncoderConfig(encoder_embedding_size=512))
    d = cfg.to_dict()
    assert list(d) == reference_keys + ["mapping_type"] and d["mapping_type"] == "mlp"
    p = tmp_path / "c.yaml"
    p.write_text(yaml.dump(d, default_flow_style=False))
    raw = yaml.safe_load(p.read_text())                       # load()'s parsing
    raw["encoder_config"] = EncoderConfig(**raw["encoder_config"])
    assert Config(**raw) == cfg
    with pytest.raises(ValueError):
        Config(mapping_type="linear")
    with pytest.raises(ValueError):
        Config(**dict(raw, mapping_type="MLP"))
    args = Namespace(language_model="gpt2", train_language_model=False, prefix_length=4, projection_length=4, transformer_layers=2,
                     transformer_attention_heads=4, use_positional_embeddings=True)
    assert Config.from_args(args).mapping_type == "transformer"
    args.mapping_type = "mlp"
    assert Config.from_args(args).mapping_type == "mlp"
    # no CLI flag
    import argparse
    from clipcap_amd.model import add_model_args
    from clipcap_amd.train import add_training_args
    assert "mapping_type" not in vars(add_model_args(add_training_args(argparse.ArgumentParser())).parse_args([]))


def _tiny_lm(D=32):
    from clipcap_amd.model.gpt2 import GPT2LM
    return GPT2LM(n_embd=D, n_layer=1, n_head=2, vocab_size=61, n_positions=16)


def test_model_builds_the_mlp_mapper_and_refuses_windows():
    from clipcap_amd.encoders import EncoderConfig
    from clipcap_amd.model import ClipCapModel, ClipCapModelPrefixOnly, Config, MLPMapper
    cfg = Config(language_model="unused", prefix_length=3, mapping_type="mlp", encoder_config=EncoderConfig(encoder_embedding_size=24))
    for cls in (ClipCapModelPrefixOnly, ClipCapModel):
        m = cls(cfg, language_model=_tiny_lm())
        assert isinstance(m.transformer_mapper, MLPMapper) and m.transformer_mapper.engine.dims["Hd"] == 48
        keys = [k for k in m.state_dict() if k.startswith("transformer_mapper.")]
        assert keys == ["transformer_mapper.model.0.weight", "transformer_mapper.model.0.bias", "transformer_mapper.model.2.weight",
                        "transformer_mapper.model.2.bias"]
        assert m.hparams["mapping_type"] == "mlp"
    assert len(list(ClipCapModelPrefixOnly(cfg, language_model=_tiny_lm()).parameters())) == 4
    win = Config(language_model="unused", prefix_length=3, mapping_type="mlp",
                 encoder_config=EncoderConfig(encoder_embedding_size=24, use_windowed_embeddings=True))
    with pytest.raises(ValueError):
        ClipCapModel(win, language_model=_tiny_lm())


def _original_state_dict(kind, E=24, D=32, L=3, hidden=None):
    """a synthetic state dict with the key names of the original ClipCap's ClipCaptionModel: clip_project.* + gpt.*"""
    g = torch.Generator().manual_seed(1)
    lm = _tiny_lm(D)
    sd = {"gpt." + k: v.detach().clone() for k, v in lm.state_dict().items()}
    if kind == "mlp":
        hidden = L * D // 2 if hidden is None else hidden
        sd.update({"clip_project.model.0.weight": torch.randn(hidden, E, generator=g), "clip_project.model.0.bias": torch.randn(hidden, generator=g),
                   "clip_project.model.2.weight": torch.randn(L * D, hidden, generator=g), "clip_project.model.2.bias": torch.randn(L * D, generator=g)})
    else:
        from clipcap_amd.model.mapper import TransformerMapper
        tm = TransformerMapper(E, D, L, 2, num_heads=8, num_layers=2)
        sd.update({"clip_project." + k: v.detach().clone() for k, v in tm.state_dict().items()})
    return sd


@pytest.mark.parametrize("kind", ["mlp", "transformer"])
def test_original_state_dicts_convert_and_load(kind):
    from clipcap_amd.model import ClipCapModel, config_from_original_state_dict, convert_original_state_dict
    from clipcap_amd.model.mapper import MLPMapper, TransformerMapper
    D = 32 if kind == "mlp" else 64          # (the transformer mapper's 8 heads need a head dim that is a multiple of 8)
    sd = _original_state_dict(kind, D=D)
    sd["unrelated.buffer"] = torch.zeros(1)
    conv = convert_original_state_dict(sd)
    assert len(conv) == len(sd) and "unrelated.buffer" in conv
    assert not any(k.startswith(("clip_project.", "gpt.")) for k in conv)
    assert sum(k.startswith("transformer_mapper.") for k in conv) == sum(k.startswith("clip_project.") for k in sd)
    assert conv["language_model.transformer.wte.weight"] is sd["gpt.transformer.wte.weight"]
    for src in (sd, conv):                                    # inference works on either naming
        cfg = config_from_original_state_dict(src, "unused")
        assert cfg.mapping_type == ("mlp" if kind == "mlp" else "transformer") and cfg.train_language_model is True
        assert cfg.prefix_length == 3 and cfg.encoder_config.encoder_embedding_size == 24 and cfg.language_model == "unused"
        if kind == "transformer":
            assert cfg.projection_length == 2 and cfg.transformer_layers == 2
    assert config_from_original_state_dict(sd, "unused", train_language_model=False).train_language_model is False
    m = ClipCapModel(cfg, language_model=_tiny_lm(D))
    assert isinstance(m.transformer_mapper, MLPMapper if kind == "mlp" else TransformerMapper)
    res = m.load_state_dict(conv, strict=False)
    assert not [k for k in res.missing_keys if k.startswith("transformer_mapper.")], res.missing_keys
    name = "model.2.weight" if kind == "mlp" else "linear.weight"
    assert torch.equal(m.state_dict()["transformer_mapper." + name], sd["clip_project." + name])


def test_config_inference_refusals():
    from clipcap_amd.model import config_from_original_state_dict
    with pytest.raises(ValueError):
        config_from_original_state_dict(_original_state_dict("mlp", hidden=40), "unused")        # hidden width != L D / 2
    sd = _original_state_dict("mlp")
    with pytest.raises(ValueError):
        config_from_original_state_dict({k: v for k, v in sd.items() if "wte" not in k}, "unused")
    with pytest.raises(ValueError):
        config_from_original_state_dict({k: v for k, v in sd.items() if not k.startswith("clip_project.")}, "unused")


def test_header_binding_and_generated_files():
    from clipcap_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "clipcap_hip.h")).read()
    added = hdr[hdr.index("ADDED since (still 3"):hdr.index("#define CC_ABI_VERSION")]
    l = _lib.lib()
    for name in NEW:
        assert name in added, f"{name} missing from the header's ADDED list"
        assert name in _lib.SIGNATURES and hasattr(l, name)
        assert re.search(r"^(?:int|int64_t)\s+" + name + r"\s*\(", hdr, flags=re.M), f"{name} not declared"
    assert "#define CC_ABI_VERSION 3" in hdr and l.cc_abi_version() == 3 and _lib.ABI_VERSION == 3
    assert "#define CC_MLP_TENSORS 4" in hdr and "} cc_mlp_cfg;" in hdr
    assert C.sizeof(_lib.MlpCfg) == 20 and [f[0] for f in _lib.MlpCfg._fields_] == ["E", "D", "L", "Hd", "op_dtype"]
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_abi.py"), "--check"]).returncode == 0
    disp = open(os.path.join(ROOT, "clipcap_amd", "csrc", "abi_dispatch.cpp")).read()
    assert "cc_mlp_fwd_x3(" in disp and "cfg ? cfg->op_dtype" in disp and "cc_gemm_tanh_f16(" in disp
    for f in ("exports.map", "exports_lab.map"):
        text = open(os.path.join(ROOT, "clipcap_amd", "csrc", f)).read()
        assert all(f"    {n};" in text for n in NEW)
    mk = open(os.path.join(ROOT, "clipcap_amd", "csrc", "Makefile")).read()
    assert "gemm_inst_tanh.hip" in mk and "mlp.hip" in mk


CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


def test_wgrad_plans_at_the_real_shape(tmp_path):
    """model.2.weight's fp32 slab (118 MB) exceeds the 96 MiB weight-gradient scratch: plan_wgrad must give a one-slice direct form"""
    assert CXX, "no host C++ compiler"
    api = open(os.path.join(ROOT, "clipcap_amd", "csrc", "gemm_api.h")).read()
    assert "WGRAD_SCRATCH_BYTES = size_t(96) << 20" in api      # the size the check below assumes
    exe = str(tmp_path / "mlp_plan_check")
    flags = ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-g", "-I", os.path.join(ROOT, "clipcap_amd", "csrc")]
    subprocess.run([CXX, *flags, os.path.join(ROOT, "tests", "mlp_plan_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1].startswith("ok:")
