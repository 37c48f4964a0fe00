"""The MLP mapping network inside the model: ClipCapModelPrefixOnly / ClipCapModel with Config.mapping_type = "mlp" on the tiny language model
of tests/test_gpu_x3.py's full-finetune test (D = 128, 2 heads, 2 layers, V = 157, 32 positions), E = 16, L = 3, B = 3, cap = 7, one ragged row.

Reference: tests/mlp_ref.py's prefix, then oracle.clipcap_oracle.gpt2_logits and the loss formula of clipcap_loss, under torch autograd.
  * precision 32 (split-bf16 operands) against the plain fp32 reference: loss within 2e-5, every mapper gradient within 2e-3 relative
    Frobenius — the figures tests/test_gpu_x3.py asserts for this language model;
  * bf16 / fp16 operands against the same reference with its rounding points on: 3e-2 relative Frobenius, the like-for-like bar of
    tests/test_gpu_model.py.
Then the training surface: fused_step with clipping, label smoothing and the weight average; bit-reproducible frozen-LM steps; the decoders
and the scorer; a train() -> checkpoint -> load() round trip; two gloo ranks with the overlapped reducer against one process."""
import argparse
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F
import yaml

from oracle import clipcap_oracle as O
from tests import mlp_ref as MR
from tests.test_api_surface import FakeTokenizer, _write_dataset
from tests.test_ddp_gloo import _free_port

pytestmark = pytest.mark.gpu

E, D, L, N_HEAD, N_LAYER, V, NPOS, B, CAP = 16, 128, 3, 2, 2, 157, 32, 3, 7
RB = {32: False, "bf16": True, 16: "fp16"}


def _state_dict(seed=0):
    """random parameters of the whole model under this package's state-dict names"""
    from clipcap_amd.engine import Gpt2Engine, MlpMapperEngine
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for pre, eng in (("transformer_mapper.", MlpMapperEngine(E, D, L)), ("language_model.", Gpt2Engine(D, N_HEAD, N_LAYER, V, NPOS))):
        for k, v in eng.views(eng.arena.w32).items():
            if "ln_" in k and k.endswith("weight"):
                t = 1.0 + 0.05 * torch.randn(v.shape, generator=g)
            elif k.endswith(".bias"):
                t = 0.1 * torch.randn(v.shape, generator=g)
            else:
                t = torch.randn(v.shape, generator=g) * (0.1 if ("wte" in k or "wpe" in k) else 0.8 / v.shape[-1] ** 0.5)
            sd[pre + k] = t
    return sd


def _model(full, precision, seed=0):
    from clipcap_amd.encoders import EncoderConfig
    from clipcap_amd.model import ClipCapModel, ClipCapModelPrefixOnly, Config, MLPMapper, TrainingConfig
    from clipcap_amd.model.gpt2 import GPT2LM
    lm = GPT2LM(n_embd=D, n_layer=N_LAYER, n_head=N_HEAD, vocab_size=V, n_positions=NPOS, embd_pdrop=0.0, attn_pdrop=0.0, resid_pdrop=0.0)
    cfg = Config(language_model="unused", train_language_model=full, prefix_length=L, mapping_type="mlp",
                 encoder_config=EncoderConfig(encoder_embedding_size=E),
                 training_config=TrainingConfig(optimizer_lr=1e-3, use_deepspeed_optimisers=False, scheduler_warmup_steps=2, total_steps=6))
    m = (ClipCapModel if full else ClipCapModelPrefixOnly)(cfg, language_model=lm)
    assert isinstance(m.transformer_mapper, MLPMapper)
    sd = _state_dict(seed)
    res = m.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and all("lm_head" in k for k in res.missing_keys), res
    m = m.to("cuda")
    m.set_precision(precision)
    return m, sd


def _batch():
    g = torch.Generator().manual_seed(1)
    tokens, embeds = torch.randint(1, V, (B, CAP), generator=g), torch.randn(B, E, generator=g)
    tokens[1, 5:] = -1
    return tokens, embeds


def _reference(sd, tokens, embeds, rb, train_lm):
    """(loss, {name: gradient}) of the torch-autograd reference"""
    p = {k: v.clone().requires_grad_(k.startswith("transformer_mapper.") or train_lm) for k, v in sd.items()}
    tok = tokens.clone()
    tok[tok < 0] = 0
    pre = MR.prefix(p, embeds, L, pre="transformer_mapper.", rb=rb)
    x = torch.cat((pre, p["language_model.transformer.wte.weight"][tok]), dim=1)
    logits = O.gpt2_logits(p, x, N_HEAD, N_LAYER, pre="language_model.", rb=rb)
    lg = logits[:, L - 1:-1]
    loss = F.cross_entropy(lg.reshape(-1, lg.shape[-1]), tok.flatten(), ignore_index=0)
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in p.items() if v.grad is not None}


@pytest.mark.parametrize("full", [False, True], ids=["prefix_only", "full"])
@pytest.mark.parametrize("precision", [32, "bf16", 16])
def test_loss_and_mapper_gradients_against_the_reference(precision, full):
    m, sd = _model(full, precision)
    tokens, embeds = _batch()
    eng = m.engine
    eng.zero_grad()
    loss = float(eng.forward_backward(tokens.cuda(), embeds.cuda()))
    torch.cuda.synchronize()
    scale = float(eng.scaler.scale) if eng.scaler is not None else 1.0
    ref, grads = _reference(sd, tokens, embeds, RB[precision], full)
    me = m.transformer_mapper.engine
    worst = ("", 0.0)
    for k, v in me.views(me.arena.g32).items():
        r = grads["transformer_mapper." + k]
        rel = ((v.cpu() / scale - r).norm() / r.norm().clamp_min(1e-20)).item()
        worst = max(worst, (k, rel), key=lambda t: t[1])
    print(f"MLP mapper model, precision {precision}, full {full}: loss {loss:.6f} vs reference {ref:.6f}; worst mapper gradient {worst[1]:.3e} ({worst[0]})")
    if precision == 32:
        assert abs(loss - ref) <= 2e-5, (loss, ref)
        assert worst[1] <= 2e-3, worst
    else:
        assert abs(loss - ref) <= 3e-2 * max(1.0, abs(ref)), (loss, ref)
        assert worst[1] <= 3e-2, worst


def _four_steps(full, precision):
    m, _ = _model(full, precision)
    m.train()
    tokens, embeds = _batch()
    losses = [float(m.fused_step((tokens.clone().cuda(), embeds.cuda()), lr=2e-3, max_grad_norm=1.0, label_smoothing=0.1, ema_decay=0.9)) for _ in range(4)]
    torch.cuda.synchronize()
    a = m.transformer_mapper.engine.arena
    return m, losses, a.w32.clone(), a.ema.clone()


@pytest.mark.parametrize("full", [False, True], ids=["prefix_only", "full"])
def test_fused_steps_with_clipping_smoothing_and_average(full):
    m, losses, w, ema = _four_steps(full, "bf16")
    print("MLP mapper fused_step losses", losses, "grad norm", float(m.last_grad_norm))
    assert all(np.isfinite(losses)) and losses[3] < losses[0]
    assert float(m.last_grad_norm) > 0 and float(m.last_nll) > 0
    assert torch.isfinite(ema).all() and not torch.equal(ema, w) and float((ema - w).abs().max()) < 0.2
    if not full:      # frozen LM: the whole step is bit-reproducible
        _, losses2, w2, ema2 = _four_steps(full, "bf16")
        assert losses2 == losses and torch.equal(w2, w) and torch.equal(ema2, ema)


def test_decoders_and_scorer_run_on_the_model():
    from clipcap_amd.inference import generate_beam
    from clipcap_amd.inference.score import score_captions
    m, sd = _model(False, "bf16")
    m.eval()
    tokens, embeds = _batch()
    tok = FakeTokenizer(V, 96)
    with torch.no_grad():
        prefix = m.transformer_mapper(embeds[:1].cuda())
    assert prefix.shape == (1, L, D)
    ref = MR.prefix({k: v for k, v in sd.items()}, embeds[:1], L, pre="transformer_mapper.", rb=True)
    assert ((prefix.cpu() - ref).norm() / ref.norm()).item() <= 3e-2
    text = generate_beam(m, tok, prefix, beam_size=3, entry_length=6)
    assert isinstance(text, list) and len(text) == 1 and isinstance(text[0], str)
    sc = score_captions(m, embeds.cuda(), tokens.cuda())
    assert torch.isfinite(sc.token_logprobs).all() and float(sc.logprob.sum()) < 0 and sc.num_tokens.tolist() == [7.0, 5.0, 7.0]
    # the module's autograd bridge: the same gradients as the engine's backward
    m.train()
    out = m.transformer_mapper(embeds.cuda())
    up = torch.randn(out.shape, generator=torch.Generator().manual_seed(2)).cuda()
    (out * up).sum().backward()
    me = m.transformer_mapper.engine
    me.forward(embeds.cuda(), save=True)
    me.arena.grads().zero_()
    me.backward(up)
    for k, p in m.transformer_mapper._arena_params.items():
        assert torch.equal(p.grad, me.views(me.arena.g32)[k]), k


def test_train_checkpoint_and_load_round_trip(tmp_path):
    """train() with args.mapping_type = "mlp": the written config carries the key, load(from_checkpoint=True) rebuilds an MLPMapper with the
    checkpoint's weights and reproduces the prefix"""
    import clipcap_amd
    from clipcap_amd.model import MLPMapper, add_model_args
    from clipcap_amd.model.gpt2 import GPT2LM
    from clipcap_amd.train import add_training_args, train
    emb, _ = _write_dataset(tmp_path / "ds", n=32, E=24, shards=(12, 20))
    GPT2LM(n_embd=64, n_layer=2, n_head=4, vocab_size=157, n_positions=96).save_pretrained(str(tmp_path / "lm"))
    args = add_model_args(add_training_args(argparse.ArgumentParser())).parse_args([
        "--input-dataset", str(tmp_path / "ds"), "--output-folder", str(tmp_path / "out"), "--language-model", str(tmp_path / "lm"),
        "--batch-size", "16", "--epochs", "1", "--optimizer-lr", "2e-3", "--scheduler-warmup-steps", "1", "--checkpoint-filename-prefix",
        "t", "--prefix-length", "4", "--logging-frequency", "1000"])
    args.mapping_type = "mlp"
    tok = FakeTokenizer()
    assert train(args, tokenizer=tok) == 0
    raw = yaml.safe_load(open(tmp_path / "out" / "t_config.yaml"))
    assert raw["mapping_type"] == "mlp" and raw["prefix_length"] == 4
    ckpt = torch.load(str(tmp_path / "out" / "t_final.ckpt"), map_location="cpu")["state_dict"]
    keys = [k for k in ckpt if k.startswith("transformer_mapper.")]
    assert keys == ["transformer_mapper." + n for n in ("model.0.weight", "model.0.bias", "model.2.weight", "model.2.bias")]
    assert tuple(ckpt["transformer_mapper.model.2.weight"].shape) == (256, 128)
    model, _ = clipcap_amd.load(str(tmp_path / "out" / "t_final.ckpt"), str(tmp_path / "out" / "t_config.yaml"), device="cuda",
                                from_checkpoint=True, tokenizer=tok)
    assert isinstance(model.transformer_mapper, MLPMapper) and model.config.mapping_type == "mlp"
    for k in keys:
        assert torch.equal(model.state_dict()[k].cpu(), ckpt[k]), k
    x = torch.from_numpy(emb[:5])
    with torch.no_grad():
        prefix = model.transformer_mapper(x.cuda())
    ref = MR.prefix(ckpt, x, 4, pre="transformer_mapper.", rb=True)
    assert prefix.shape == (5, 4, 64) and ((prefix.cpu() - ref).norm() / ref.norm()).item() <= 3e-2


def _ddp_engine():
    from clipcap_amd.engine import ClipCapEngine
    m, _ = _model(False, "bf16", seed=3)
    g = torch.Generator().manual_seed(5)
    tokens = torch.randint(1, V, (8, 8), generator=g)
    tokens[1, 4:] = -1
    tokens[6, 2:] = -1
    embeds = torch.randn(8, E, generator=g)
    eng = m.engine
    assert isinstance(eng, ClipCapEngine)
    return m, eng, tokens, embeds


def _ddp_worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from clipcap_amd.train.ddp import GradReducer, shard_batch
    m, eng, tokens, embeds = _ddp_engine()
    arenas = eng.arenas()
    red = GradReducer([a.grads() for a in arenas])
    tk, em = shard_batch(tokens, embeds, rank, world)
    red.begin()
    loss = eng.forward_backward(tk.cuda(), em.cuda(), reduce_stats=red.reduce_stats, on_grads_ready=red.on_grads_ready)
    red.finish()
    torch.cuda.synchronize()
    if rank == 0:
        np.savez(out, loss=float(loss), **{f"g{i}": a.g32.cpu().numpy() for i, a in enumerate(arenas)})
    dist.destroy_process_group()


def test_two_rank_step_equals_single_process(tmp_path):
    out = str(tmp_path / "ddp.npz")
    mp.spawn(_ddp_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    res = np.load(out)
    m, eng, tokens, embeds = _ddp_engine()
    eng.zero_grad()
    loss = eng.forward_backward(tokens.cuda(), embeds.cuda())
    torch.cuda.synchronize()
    assert abs(float(loss) - float(res["loss"])) <= 1e-5
    for i, a in enumerate(eng.arenas()):
        ref = a.g32.cpu().numpy()
        rel = np.linalg.norm(res[f"g{i}"] - ref) / np.linalg.norm(ref)
        assert rel <= 2e-2, (i, rel)
