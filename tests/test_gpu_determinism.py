"""Bit reproducibility of the training step (the cross-block gradient reductions fold per-block partials in a fixed order, kernels.h
RED_SCRATCH_FLOATS): the same seeded model, inputs and step count give the same loss, gradients and weights bit for bit, at the bench's
configs[1] (frozen GPT-2-small, B = 256) in bf16 and split-bf16 operands — the sizes at which LayerNorm dgamma / dbeta, the bias column
sums and the prefix batch sum all reduce over many blocks."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _run(precision, steps=4):
    import bench
    c = dict(bench.CONFIGS["2"])
    dev = torch.device("cuda", 0)
    me, ge, eng = bench.init_engines(c, dev)
    if precision != "bf16":
        me.set_precision(precision)
        ge.set_precision(precision)
    gen = torch.Generator(device=dev).manual_seed(99)
    embeds = torch.randn(c["B"], c["E"], generator=gen, device=dev)
    tokens = torch.randint(1, c["V"], (c["B"], c["cap"]), generator=gen, device=dev)
    tokens[::5, 33:] = -1
    losses = []
    for i in range(steps):
        eng.zero_grad()
        losses.append(eng.forward_backward(tokens, embeds).clone())
        eng.optimizer_step(1e-3, i + 1)
    torch.cuda.synchronize()
    out = (torch.stack(losses).cpu(), me.arena.g32.cpu().clone(), me.arena.w32.cpu().clone())
    del me, ge, eng
    torch.cuda.empty_cache()
    return out


@pytest.mark.parametrize("precision", ["bf16", 32])
def test_training_steps_are_bit_reproducible(precision):
    a, b = _run(precision), _run(precision)
    assert torch.isfinite(a[0]).all() and torch.isfinite(a[1]).all()
    for name, x, y in zip(("losses", "gradients", "weights"), a, b):
        assert torch.equal(x, y), f"{name}: max |diff| {(x - y).abs().max().item():.3e}"
