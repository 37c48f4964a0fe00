"""The weighted entry points (cc_lmhead_ce_fwd_w / cc_lmhead_ce_bwd_w) read no workspace byte they did not write this call: the training
step with token_weights, with and without label smoothing, on zero-filled against 0xFF-filled injected workspaces, with the helpers and
the rules of tests/test_gpu_workspace_poison.py (whose module docstring says why every integer buffer is safe to fill: the weighted forms
read target / row_map exactly where the plain forms do, after k_ce_targets has written them).  The weights themselves are the caller's
input, not workspace; on the positions the loss ignores they are NaN here, so a weight that leaked would show as well."""
import pytest
import torch

from tests.test_gpu_workspace_poison import (DEV, DROP, LR, SHAPES, _batch, _end_the_session_on_a_device_error, _engine, _keep,  # noqa: F401
                                             _keep_arenas, _keep_grads, _shape_of, _three_runs, _train_specs)
from tests.ws_poison import injected_workspaces

pytestmark = pytest.mark.gpu


def _weights(tokens, seed):
    g = torch.Generator().manual_seed(seed)
    w = (4.0 * torch.rand(tokens.shape, generator=g) - 1.5).float()
    w[0, 0] = 0.0
    w = w.to(DEV)
    w[tokens <= 0] = float("nan")
    return w


# shape, precision, full finetune, eps, GPT-2 dropout + gradient clipping + weight average on top
CASES = [("S1", "bf16", False, 0.0, False), ("S1", "bf16", True, 0.0, False), ("S1", "bf16", False, 0.1, False), ("S1", "bf16", True, 0.1, True),
         ("S1", 16, True, 0.1, True), ("S1", 32, False, 0.0, False), ("S1", 32, True, 0.1, True), ("S2", "bf16", True, 0.1, True),
         ("S2", 32, True, 0.0, False)]


@pytest.mark.parametrize("shape,precision,train_lm,eps,more", CASES,
                         ids=[f"{c[0]}-{c[1]}-{'full' if c[2] else 'frozen'}-eps{c[3]}{'-dropout-clip-ema' if c[4] else ''}" for c in CASES])
def test_weighted_training_step(shape, precision, train_lm, eps, more):
    """Two consecutive weighted forward_backward + optimizer_step: loss, plain NLL, both g32 arenas, and w32, m, v, w16 after each step.
    The options compose: with GPT-2's train-mode dropout, global-norm clipping and the weight average in the same step (and the fp16
    loss scale in the fp16 case) the chain still repeats bit for bit and stays finite."""
    s = SHAPES[shape]
    drop = DROP if more else None

    def chain(fill):
        eng = _engine(s, precision, train_lm)
        out = {}
        with injected_workspaces(_train_specs(eng, _shape_of(eng, s, dropout=drop), eps, 1.0 if more else None), fill, DEV):
            for i in range(2):
                tokens, embeds = _batch(s, 20 + i)
                eng.zero_grad()
                loss = eng.forward_backward(tokens, embeds, label_smoothing=eps, token_weights=_weights(tokens, 30 + i), dropout=drop)
                _keep(out, f"step {i} loss", loss)
                _keep(out, f"step {i} nll", eng.last_nll)
                _keep_grads(out, eng, f"step {i}")
                if more:
                    eng.optimizer_step(LR, i + 1, max_grad_norm=1.0, ema_decay=0.9)
                    _keep(out, f"step {i} grad norm", eng.last_grad_norm)
                    for name, a in zip(("mapper", "gpt2"), eng.arenas()):
                        _keep(out, f"step {i} {name} ema", a.ema)
                else:
                    eng.optimizer_step(LR, i + 1)
                _keep_arenas(out, eng, f"step {i}")
        return out

    out = _three_runs(chain, f"weighted training step {shape} {precision} {'full' if train_lm else 'frozen'} eps {eps}")
    assert bool(out["step 1 mapper g32"].ne(0).any()) and not torch.equal(out["step 0 loss"], out["step 0 nll"])
