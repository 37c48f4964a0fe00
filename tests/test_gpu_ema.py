"""The weight average inside the AdamW step on the device: cc_adamw_step_ema leaves p, m, v and w16 with cc_adamw_step_clip's bits and
the average within tests/ema_ref.py's bound of the float64 update (a one-step statement against the device's own new p, so nothing
accumulates); a skipped step skips it; then the engine, the model's ema_weights / ema_state_dict, evaluate(ema=True), checkpoints, resume,
the training driver, and two ranks with sharded state."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import ema_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HP = (1e-2, 0.9, 0.999, 1e-8, 0.01)


def _lib():
    from clipcap_amd import _lib as L
    return L.lib()


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _grid_cap_floats():
    """elements one trip of the AdamW launch covers at its grid cap, read from the launch itself: blocks cap x threads x 4 floats"""
    src = open(os.path.join(ROOT, "clipcap_amd", "csrc", "kernels.hip")).read()
    body = src[src.index("int adamw("):]
    m = re.search(r"flat_grid\(n4,\s*(\d+),\s*(\d+)\)", body)
    threads, cap = int(m.group(1)), int(m.group(2))
    assert threads == 256
    return cap * threads * 4


SIZES = [8, 1028, _grid_cap_floats() + 8]          # one group per thread of one wave's corner; not a multiple of the block; a second grid-stride trip
_INPUTS = {}


def _inputs(n):
    """fresh device copies of the same five tensors for every call at this size (made once): p, g, m, v and an average that is NOT p"""
    if n not in _INPUTS:
        gen = torch.Generator().manual_seed(n)
        p = torch.randn(n, generator=gen)
        g = torch.randn(n, generator=gen) * 3.0
        m = torch.randn(n, generator=gen) * 0.1
        v = torch.rand(n, generator=gen) * 0.01
        e = p + 0.05 * torch.randn(n, generator=gen)
        e[: min(n, 64)] = -p[: min(n, 64)]                     # e = -p: the cancelling corner of the convex form
        _INPUTS[n] = [t.cuda() for t in (p, g, m, v, e)]
    return [t.clone() for t in _INPUTS[n]]


def _bits(ts):
    return [None if t is None else (t.view(torch.int32) if t.dtype == torch.float32 else t).clone() for t in ts]


def _call(n, op, entry, cast, clip, step, state, found, d=0.9):
    """one launch on fresh copies; returns (p, m, v, w16, ema) as left on the device"""
    p, g, m, v, e = _inputs(n)
    w16 = torch.full((n,), 0x1234, dtype=torch.int16, device="cuda") if cast else None
    l = _lib()
    if entry == "clip":
        rc = l.cc_adamw_step_clip(op, _p(p), _p(g), _p(m), _p(v), n, *HP, step, 1.0, _p(state), _p(found), _p(clip), _p(w16), _st())
    else:
        rc = l.cc_adamw_step_ema(op, _p(p), _p(g), _p(m), _p(v), n, *HP, step, 1.0, _p(state), _p(found), _p(clip), _p(w16), _p(e), d, _st())
    assert rc == 0
    torch.cuda.synchronize()
    return p, m, v, w16, e


@pytest.mark.parametrize("op", [0, 1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_adamw_step_ema_kernel(n, op):
    quarter = torch.tensor([0.25], device="cuda")
    state = torch.tensor([1024.0, 3.0, 5.0], device="cuda")
    clear, raised = torch.zeros(1, device="cuda"), torch.ones(1, device="cuda")
    start = _inputs(n)
    worst = 0.0
    for cast in ([True, False] if op != 2 else [False]):          # split-bf16 operands have no flat cast
        for clip in (None, quarter):
            for step, st, fi in ((3, None, None), (0, state, clear)):
                ref = _call(n, op, "clip", cast, clip, step, st, fi)
                got = _call(n, op, "ema", cast, clip, step, st, fi)
                what = (n, op, cast, clip is not None, step)
                assert not torch.equal(ref[0], start[0]), what                                   # the step really moved the parameters
                for a, b in zip(_bits(ref[:4]), _bits(got[:4])):                                 # p, m, v, w16: cc_adamw_step_clip's bits
                    assert (a is None and b is None) or torch.equal(a, b), what
                worst = max(worst, R.assert_ema_step(got[4], start[4], got[0], 0.9, str(what)))  # from the DEVICE's new p and the old average
                assert not torch.equal(got[4], start[4])
        # d = 0: the average becomes the parameters, as numbers
        got = _call(n, op, "ema", cast, None, 3, None, None, d=0.0)
        assert torch.equal(got[4], got[0])
        # found_inf raised: the bits of all five buffers stay
        got = _call(n, op, "ema", cast, quarter, 0, state, raised)
        untouched = [start[0], start[2], start[3], torch.full((n,), 0x1234, dtype=torch.int16, device="cuda") if cast else None, start[4]]
        for a, b in zip(_bits(got), _bits(untouched)):
            assert (a is None and b is None) or torch.equal(a, b), (n, op, cast)
    print(f"n {n} op {op}: worst |ema - float64| / bound = {worst:.3f}")
    assert worst > 0.0                                            # the comparison saw rounding, i.e. it is not vacuous


# ---- the engine --------------------------------------------------------------------------------------------------------------------------
def _model(mode, precision):
    from tests.test_gpu_fp16 import _tiny_model
    m, g = _tiny_model(mode, precision)
    m.train()
    return m, (torch.from_numpy(g["in.tokens"]).cuda(), torch.from_numpy(g["in.embeds"]).cuda())


def _weights(m):
    return [mod.engine.arena.w32.view(torch.int32).clone() for mod in (m.transformer_mapper, m.language_model)]


@pytest.mark.parametrize("precision", ["bf16", 32])
@pytest.mark.parametrize("mode", ["prefix_only", "full"])
def test_four_steps_with_the_average_equal_four_steps_without(mode, precision):
    lr, d = 1e-3, 0.9
    plain, batch = _model(mode, precision)
    avg, _ = _model(mode, precision)
    ma, la = avg.transformer_mapper.engine.arena, avg.language_model.engine.arena
    trained = [ma] + ([la] if mode == "full" else [])
    start = [a.w32.clone() for a in trained]
    worst = 0.0
    for s in range(4):
        l0 = plain.fused_step((batch[0].clone(), batch[1]), lr)
        prev = [a.ema.clone() if a.ema is not None else a.w32.clone() for a in trained]       # ema_0 = p_0
        l1 = avg.fused_step((batch[0].clone(), batch[1]), lr, ema_decay=d)
        torch.cuda.synchronize()
        assert torch.equal(l0.view(torch.int32), l1.view(torch.int32)), s                     # the loss and every parameter, bit for bit
        assert all(torch.equal(x, y) for x, y in zip(_weights(plain), _weights(avg))), s
        for a, e0 in zip(trained, prev):
            assert a.ema.numel() == a.n and a.ema.data_ptr() != a.w32.data_ptr()
            worst = max(worst, R.assert_ema_step(a.ema, e0, a.w32, d, f"{mode} {precision} step {s}"))
    assert (la.ema is None) == (mode == "prefix_only")            # a frozen language model keeps no average
    assert plain.transformer_mapper.engine.arena.ema is None and plain.ema_updates == 0 and avg.ema_updates == 4
    for a, p0 in zip(trained, start):                              # and the average is a real average: between the start and the last iterate
        assert not torch.equal(a.ema, a.w32) and not torch.equal(a.ema, p0)
    print(f"{mode} {precision}: worst |ema - float64| / bound over 4 steps = {worst:.3f}")


def test_warmup_uses_the_hosts_step_count():
    m, batch = _model("prefix_only", "bf16")
    m.ema_decay, m.ema_warmup = 0.999, True
    a = m.transformer_mapper.engine.arena
    prev = a.w32.clone()
    for t, d in ((1, 2 / 11), (2, 3 / 12), (3, 4 / 13)):
        m.fused_step((batch[0].clone(), batch[1]), 1e-3)           # the attributes alone switch it on
        assert m._opt_step == t
        R.assert_ema_step(a.ema, prev, a.w32, d, f"warm-up step {t}")
        with pytest.raises(AssertionError):
            R.assert_ema_step(a.ema, prev, a.w32, 0.999)           # ... and not the configured decay
        prev = a.ema.clone()
    m.ema_warmup = False
    m.fused_step((batch[0].clone(), batch[1]), 1e-3)
    R.assert_ema_step(a.ema, prev, a.w32, 0.999, "warm-up off")


@pytest.mark.parametrize("mode", ["prefix_only", "full"])
def test_fp16_skipped_step_leaves_the_average_alone(mode):
    lr = 1e-3
    m, batch = _model(mode, 16)
    m.fused_step((batch[0].clone(), batch[1]), lr, ema_decay=0.9)
    eng = m.engine
    arenas = eng.arenas()
    assert all(a.ema is not None for a in arenas)
    before = [(a.w32.clone(), a.ema.clone(), a.m.clone()) for a in arenas]
    applied = float(eng.scaler.state[2])
    eng.zero_grad()
    eng.forward_backward(batch[0].clone(), batch[1])
    arenas[-1].g32[5] = float("inf")
    eng.optimizer_step(lr, 2, weight_decay=m._weight_decay(), ema_decay=0.9)
    torch.cuda.synchronize()
    for a, (w, e, mo) in zip(arenas, before):                      # skipped on the device, every arena, with no host synchronisation
        assert torch.equal(a.w32.view(torch.int32), w.view(torch.int32)) and torch.equal(a.ema.view(torch.int32), e.view(torch.int32))
        assert torch.equal(a.m, mo)
    assert float(eng.scaler.state[2]) == applied
    m.fused_step((batch[0].clone(), batch[1]), lr, ema_decay=0.9)  # the next clean step updates both
    assert float(eng.scaler.state[2]) == applied + 1
    for a, (w, e, _) in zip(arenas, before):
        assert not torch.equal(a.w32, w) and not torch.equal(a.ema, e)
        R.assert_ema_step(a.ema, e, a.w32, 0.9, f"fp16 {mode}")


def test_ema_weights_swaps_the_average_in_and_back():
    m, batch = _model("full", "bf16")
    for _ in range(3):
        m.fused_step((batch[0].clone(), batch[1]), 5e-3, ema_decay=0.9)
    m.eval()
    x = batch[1]
    before_w = _weights(m)
    with torch.no_grad():
        before_out = m.transformer_mapper(x).clone()
        before_logits = m.language_model.engine.logits(before_out).clone()
    avg = m.ema_state_dict()
    plain = {k: v.clone() for k, v in m.state_dict().items()}
    assert list(avg) == list(plain) and any(not torch.equal(avg[k], plain[k]) for k in plain)
    with m.ema_weights():
        inside = m.state_dict()
        assert all(torch.equal(inside[k], avg[k]) for k in avg)
        assert all(torch.equal(v, avg[k]) for k, v in m.ema_state_dict().items())
        with torch.no_grad():
            out = m.transformer_mapper(x)
            logits = m.language_model.engine.logits(before_out)
        assert not torch.equal(out, before_out) and not torch.equal(logits, before_logits)     # the operand copies follow the swap
    assert all(torch.equal(a, b) for a, b in zip(_weights(m), before_w))
    with torch.no_grad():
        assert torch.equal(m.transformer_mapper(x), before_out) and torch.equal(m.language_model.engine.logits(before_out), before_logits)
    with pytest.raises(KeyError):
        with m.ema_weights():
            raise KeyError("inside the block")
    assert all(torch.equal(a, b) for a, b in zip(_weights(m), before_w))
    with torch.no_grad():
        assert torch.equal(m.transformer_mapper(x), before_out)


def test_checkpoint_resume_restores_the_average(tmp_path):
    """two averaged steps, save, a third; a fresh model resumed from the file takes the third step and has the same average (the bar the
    existing resume test holds the weights to)"""
    from clipcap_amd.train.callback import CheckpointSaver, resume
    m, batch = _model("prefix_only", "bf16")
    m.ema_decay = 0.9
    for _ in range(2):
        m.fused_step((batch[0].clone(), batch[1]), 1e-3)
    CheckpointSaver(str(tmp_path), "r").save_final_checkpoint(m)
    assert sorted(os.listdir(tmp_path)) == ["r_final.ckpt", "r_final_ema.ckpt"]
    ck = torch.load(tmp_path / "r_final.ckpt", map_location="cpu")
    a = m.transformer_mapper.engine.arena
    assert sorted(ck["ema_state"]) == ["decay", "mapper", "updates", "warmup"] and torch.equal(ck["ema_state"]["mapper"], a.ema.cpu())
    averaged = torch.load(tmp_path / "r_final_ema.ckpt", map_location="cpu")["state_dict"]
    assert all(torch.equal(v.cpu(), averaged[k]) for k, v in m.ema_state_dict().items())
    m.fused_step((batch[0].clone(), batch[1]), 1e-3)
    m2, _ = _model("prefix_only", "bf16")
    m2.ema_decay = 0.9
    resume(m2, str(tmp_path / "r_final.ckpt"))
    a2 = m2.transformer_mapper.engine.arena
    assert m2.ema_updates == 2 and a2.ema.is_cuda and torch.equal(a2.ema.cpu(), ck["ema_state"]["mapper"])
    m2.fused_step((batch[0].clone(), batch[1]), 1e-3)
    assert m2.ema_updates == m.ema_updates == 3
    assert torch.allclose(a2.ema, a.ema, atol=1e-7, rtol=0) and torch.allclose(a2.w32, a.w32, atol=1e-7, rtol=0)
    # a checkpoint without an average: one enabled afterwards starts from the resumed weights
    m3, _ = _model("prefix_only", "bf16")
    m3.transformer_mapper.engine.arena.enable_ema()
    plain, _ = _model("prefix_only", "bf16")
    plain.fused_step((batch[0].clone(), batch[1]), 1e-3)
    CheckpointSaver(str(tmp_path / "plain"), "p").save_final_checkpoint(plain)
    assert sorted(os.listdir(tmp_path / "plain")) == ["p_final.ckpt"]
    resume(m3, str(tmp_path / "plain" / "p_final.ckpt"))
    a3 = m3.transformer_mapper.engine.arena
    assert a3.ema is None
    a3.enable_ema()
    assert torch.equal(a3.ema, plain.transformer_mapper.engine.arena.w32)


def test_train_driver_writes_the_averaged_checkpoint_and_evaluate_reads_the_average(tmp_path):
    import argparse
    import clipcap_amd
    from clipcap_amd.inference import generate_beam
    from clipcap_amd.model import add_model_args
    from clipcap_amd.model.gpt2 import GPT2LM
    from clipcap_amd.train import add_training_args, train
    from clipcap_amd.train.train import evaluate
    from tests.test_api_surface import FakeTokenizer, _write_dataset
    _write_dataset(tmp_path / "ds", n=48, E=24, shards=(20, 28))
    GPT2LM(n_embd=64, n_layer=2, n_head=4, vocab_size=157, n_positions=96).save_pretrained(str(tmp_path / "lm"))
    args = add_model_args(add_training_args(argparse.ArgumentParser())).parse_args([
        "--input-dataset", str(tmp_path / "ds"), "--output-folder", str(tmp_path / "out"), "--language-model", str(tmp_path / "lm"),
        "--batch-size", "16", "--epochs", "1", "--optimizer-lr", "2e-3", "--scheduler-warmup-steps", "2", "--checkpoint-filename-prefix",
        "t", "--prefix-length", "4", "--projection-length", "4", "--transformer-layers", "2", "--transformer-attention-heads", "4",
        "--logging-frequency", "1000"])
    args.ema_decay = 0.99
    tok = FakeTokenizer()
    seen = {}
    assert train(args, tokenizer=tok, step_hook=lambda step, model: seen.update(model=model, step=step)) == 0
    assert sorted(os.listdir(tmp_path / "out")) == ["t_config.yaml", "t_epoch_0.ckpt", "t_final.ckpt", "t_final_ema.ckpt"]
    trained = seen["model"]
    assert trained.ema_decay == 0.99 and trained.ema_updates == seen["step"] == 3
    es = torch.load(tmp_path / "out" / "t_epoch_0.ckpt", map_location="cpu")["ema_state"]
    assert es["updates"] == 3 and es["decay"] == 0.99 and es["warmup"] is False and "lm" not in es
    model, _ = clipcap_amd.load(str(tmp_path / "out" / "t_final_ema.ckpt"), str(tmp_path / "out" / "t_config.yaml"), device="cuda",
                                from_checkpoint=True, tokenizer=tok)
    averaged = trained.ema_state_dict()
    assert all(torch.equal(v, averaged[k]) for k, v in model.state_dict().items())
    text = generate_beam(model, tok, model.transformer_mapper(torch.randn(1, 24, device="cuda")), beam_size=3, entry_length=6)
    assert isinstance(text, list) and len(text) == 1 and isinstance(text[0], str)
    # evaluate(ema=True): the held-out loss of the average, through the unchanged scoring pass
    last = evaluate(trained, str(tmp_path / "ds"), batch_size=16, tokenizer=tok)
    w = _weights(trained)
    mean = evaluate(trained, str(tmp_path / "ds"), batch_size=16, tokenizer=tok, ema=True)
    assert all(torch.equal(a, b) for a, b in zip(_weights(trained), w))
    assert np.isfinite(mean["loss"]) and mean["tokens"] == last["tokens"] and mean["loss"] != last["loss"]


# ---- two ranks on one GPU ----------------------------------------------------------------------------------------------------------------
def _rank_worker(rank, world, port, out):
    """both ranks on the one GPU (gloo on device tensors, as tests/test_gpu_ddp.py's _zero_worker): replicated state, ZeRO stage 1 and
    stage 2.  gloo cannot reduce a device tensor onto one rank, so the stage-2 reducer all-reduces each owner's piece instead — the owner
    reads the same sum, the others never read theirs."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from clipcap_amd.train.ddp import GradReducer, ZeroShard, shard_batch

    class Reducer(GradReducer):
        def _collective(self, t, root, side=None):
            return super()._collective(t, None, side)

    res = {}
    for stage in (0, 1, 2):
        m, batch = _model("full", "bf16")
        arenas = m.engine.arenas()
        red = Reducer([a.grads() for a in arenas])
        if stage >= 1:
            owners = ZeroShard(rank, world).apply(arenas)
            if stage >= 2:
                red.set_owners(owners, rank)
        gen = torch.Generator().manual_seed(5)                             # 8 samples, 4 per rank, two of them padded
        tokens = torch.randint(1, m.language_model.config.vocab_size, (8, batch[0].shape[1]), generator=gen)
        tokens[1, 4:] = -1
        tokens[6, 2:] = -1
        tk, em = shard_batch(tokens, torch.randn(8, batch[1].shape[1], generator=gen), rank, world)
        for _ in range(3):
            m.fused_step((tk.cuda(), em.cuda()), 1e-3, reducer=red, ema_decay=0.9)
        if stage >= 1:
            lo, hi = arenas[0].zero[1][rank]
            assert arenas[0].ema.numel() == hi - lo < arenas[0].n          # this rank averages its own slice only
        avg = m.ema_state_dict()                                          # a collective when the state is sharded
        with m.ema_weights():                                             # every rank enters
            inside = m.state_dict()
            assert all(torch.equal(inside[k].cpu(), avg[k].cpu()) for k in avg), stage
        torch.cuda.synchronize()
        for k, v in avg.items():
            res[f"{stage}:{k}"] = v.cpu().numpy()
        for i, a in enumerate(arenas):
            res[f"{stage}:w{i}"] = a.w32.cpu().numpy()
    np.savez(out.format(rank), **res)
    dist.destroy_process_group()


def test_two_ranks_sharded_average_equals_the_replicated_average(tmp_path):
    from tests.test_ddp_gloo import _free_port
    from tests.test_gpu_grad_clip import _spawn
    out = str(tmp_path / "ema_rank{}.npz")
    _spawn(_rank_worker, (2, _free_port(), out), 2, limit=240)
    ranks = [np.load(out.format(r)) for r in range(2)]
    keys = [k for k in ranks[0].files if k.startswith("0:")]
    assert any("transformer_mapper" in k for k in keys) and any("language_model" in k for k in keys)
    for k in keys:
        ref = ranks[0][k]
        for stage in (0, 1, 2):
            for r in ranks:
                assert np.array_equal(r[f"{stage}:{k[2:]}"], ref), (stage, k)            # bit for bit, on every rank
    # the average is not the last iterate (linear.weight sits at the front of the mapper's arena)
    lw = ranks[0]["0:transformer_mapper.linear.weight"].ravel()
    assert not np.array_equal(lw, ranks[0]["0:w0"][: lw.size])
