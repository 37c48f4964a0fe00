"""``load(model_path, config_path, device, from_checkpoint)`` -> (model.eval(), tokenizer) — reference clipcap/model/load.py:9-42.
Reads the same ``*_config.yaml`` schema and the same state-dict keys (``strict=False``), so reference checkpoints load.

The publicly distributed checkpoints of the original ClipCap (``clip_project.*`` + ``gpt.*``, no config file) load in two steps:
``convert_original_state_dict`` renames the keys, ``config_from_original_state_dict`` infers the Config from the tensors."""
from __future__ import annotations

from typing import Callable, Dict, Tuple, Union

import torch
import yaml

from clipcap_amd.encoders.config import EncoderConfig
from clipcap_amd.model.config import Config
from clipcap_amd.model.model import ClipCapModel, ClipCapModelPrefixOnly, get_tokenizer


def load(model_path: str, config_path: str, device: str = "cpu", from_checkpoint: bool = False,
         tokenizer: Union[None, Callable] = None) -> Tuple[Union[ClipCapModel, ClipCapModelPrefixOnly], Callable]:
    with open(config_path, "r") as f:
        raw = yaml.safe_load(f)
    if from_checkpoint and raw.get("training_config") is not None:
        raw["training_config"] = None                       # stale schedule of a finished run (load.py:15-16)
    raw["encoder_config"] = EncoderConfig(**raw["encoder_config"])
    if isinstance(raw.get("training_config"), dict):
        from clipcap_amd.model.config import TrainingConfig
        raw["training_config"] = TrainingConfig(**raw["training_config"])
    config = Config(**raw)
    model = (ClipCapModel if config.train_language_model else ClipCapModelPrefixOnly)(config)
    state = torch.load(model_path, map_location="cpu")
    if from_checkpoint:
        state = state["state_dict"]
    model.load_state_dict(state, strict=False)
    model = model.eval().to(device)
    if tokenizer is None:
        tokenizer = get_tokenizer(config.language_model)
    return model, tokenizer


def convert_original_state_dict(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """State dict of an original ClipCap model (``ClipCaptionModel``: ``clip_project.*``, ``gpt.*``) -> this package's keys
    (``transformer_mapper.*``, ``language_model.*``).  Both of the original's mapping networks keep their inner names — the MLP's
    ``model.0.*`` / ``model.2.*`` and the transformer mapper's ``linear.*`` / ``prefix_const`` / ``transformer.layers.*`` are the
    names used here.  Every other key passes through; tensors are not copied."""
    renames = (("clip_project.", "transformer_mapper."), ("gpt.", "language_model."))
    out = {}
    for k, v in sd.items():
        for old, new in renames:
            if k.startswith(old):
                k = new + k[len(old):]
                break
        out[k] = v
    return out


def config_from_original_state_dict(sd: Dict[str, torch.Tensor], language_model: str, train_language_model: bool = True) -> Config:
    """The Config an original ClipCap state dict (converted or not) was trained with, as far as its tensors tell: the mapping type from
    the key names, E / prefix_length / D from the shapes and ``wte``.  ``language_model`` names the GPT-2 the ``gpt.*`` tensors belong
    to (the file does not say).  MLP mapper: ValueError unless the hidden width is prefix_length * D / 2 (the only width the
    original builds, and the only one the kernels run).  Transformer mapper: layers and projection_length from the tensors; the head
    count leaves no trace in them and is left at the original's default of 8."""
    sd = convert_original_state_dict(sd)
    m, lm = "transformer_mapper.", "language_model."
    wte = sd.get(lm + "transformer.wte.weight")
    if wte is None:
        raise ValueError("no gpt.transformer.wte.weight / language_model.transformer.wte.weight in the state dict: cannot infer lm_embedding_size")
    D = int(wte.shape[1])
    kw = dict(language_model=language_model, train_language_model=bool(train_language_model))
    if m + "model.0.weight" in sd and m + "model.2.weight" in sd:
        w1, w2 = sd[m + "model.0.weight"], sd[m + "model.2.weight"]
        hidden, E, out = int(w1.shape[0]), int(w1.shape[1]), int(w2.shape[0])
        if out % D or int(w2.shape[1]) != hidden:
            raise ValueError(f"MLP mapper shapes {tuple(w1.shape)}, {tuple(w2.shape)} do not end in a multiple of lm_embedding_size {D}")
        L = out // D
        if 2 * hidden != L * D:
            raise ValueError(f"MLP mapper hidden width {hidden} is not prefix_length * lm_embedding_size / 2 = {L} * {D} / 2")
        return Config(prefix_length=L, mapping_type="mlp", encoder_config=EncoderConfig(encoder_embedding_size=E), **kw)
    if m + "linear.weight" in sd and m + "prefix_const" in sd:
        lin, pc = sd[m + "linear.weight"], sd[m + "prefix_const"]
        layers = {int(k[len(m + "transformer.layers."):].split(".")[0]) for k in sd if k.startswith(m + "transformer.layers.")}
        return Config(prefix_length=int(pc.shape[0]), projection_length=int(lin.shape[0]) // D, transformer_layers=len(layers),
                      transformer_attention_heads=8, use_positional_embeddings=False,
                      encoder_config=EncoderConfig(encoder_embedding_size=int(lin.shape[1])), **kw)
    raise ValueError("neither an MLP mapper (clip_project.model.0/2.*) nor a transformer mapper (clip_project.linear.*, prefix_const) in the state dict")
