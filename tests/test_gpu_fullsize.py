"""Full BASELINE size (configs[1]: E=512, TransformerMapper 8 layers P=L=10 H=8, GPT-2-small, B=256, 40 tokens) — the CPU oracle is
far too slow here, so parity is checked through size-independent properties of the training step:
  * batch-permutation invariance of the loss and of the (summed) gradients,
  * additivity: the global-batch gradient equals the kept-token-weighted combination of two half-batch gradients,
  * gradient scale linearity through the loss divisor, determinism of the loss, finite values everywhere,
  * decode: KV-cached logits == full re-forward logits at GPT-2-small size."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def big():
    import bench
    c = dict(bench.CONFIGS["2"])
    me, ge, eng = bench.init_engines(c, torch.device("cuda", 0))
    gen = torch.Generator(device="cuda").manual_seed(7)
    embeds = torch.randn(c["B"], c["E"], generator=gen, device="cuda")
    tokens = torch.randint(1, c["V"], (c["B"], c["cap"]), generator=gen, device="cuda")
    tokens[::7, 30:] = -1            # ragged captions
    tokens[3, 5] = 0                 # an explicit id-0 target (ignored, model.py:109)
    return c, me, ge, eng, tokens, embeds


def _grads(eng, tokens, embeds):
    eng.zero_grad()
    loss = eng.forward_backward(tokens, embeds)
    torch.cuda.synchronize()
    return float(loss), eng.mapper.arena.g32.clone(), float(eng.stats[1])


def _rel(a, b):
    return ((a - b).norm() / b.norm()).item()


def test_full_size_step_properties(big):
    c, me, ge, eng, tokens, embeds = big
    l0, g0, n0 = _grads(eng, tokens, embeds)
    assert torch.isfinite(g0).all() and abs(l0) < 20 and n0 == float((tokens > 0).sum())
    # determinism of the loss (no atomics on its path)
    l0b, g0b, _ = _grads(eng, tokens, embeds)
    assert l0b == l0 and torch.equal(g0b, g0)          # gradients too: every cross-block reduction folds its partials in a fixed order
    # permutation invariance
    perm = torch.randperm(c["B"], device="cuda")
    l1, g1, n1 = _grads(eng, tokens[perm], embeds[perm])
    assert n1 == n0 and abs(l1 - l0) <= 2e-5 * abs(l0) and _rel(g1, g0) <= 2e-3
    # additivity over a split of the batch, weighted by kept-target counts
    h = c["B"] // 2
    la, ga, na = _grads(eng, tokens[:h], embeds[:h])
    lb, gb, nb = _grads(eng, tokens[h:], embeds[h:])
    assert na + nb == n0
    assert abs((la * na + lb * nb) / n0 - l0) <= 2e-5 * abs(l0)
    # the halves scale dlogits by 1/na, 1/nb instead of 1/n0 before the bf16 rounding: bf16-level, not fp32-level, agreement
    assert _rel((ga * na + gb * nb) / n0, g0) <= 2e-2


def _reduced_groups(views):
    """the parameters whose gradients come out of the cross-block reductions (ln_bwd dgamma / dbeta / dcol, colsum_bf16*, batch_sum)"""
    return {k: v for k, v in views.items() if k.endswith(".bias") or "norm" in k or "ln_" in k or k in ("prefix_const", "pos_embeddings")}


PERMUTATION_TOL = 1e-5     # measured worst 1.7e-7; a fold that skips its last slice: 0.75
ADDITIVITY_TOL = 1e-1      # measured worst 3.0e-2 (bf16-level, see below); a fold that skips its last slice: 0.53


def test_full_size_per_parameter_permutation_and_additivity(big):
    """Per parameter, for every LN weight and bias, every Linear bias, prefix_const and pos_embeddings (the gradients the cross-block
    reductions fold: at B = 256 ln_bwd folds 256 blocks, colsum_bf16 up to 20 row slices, batch_sum 32 slices of 8 samples).
    permutation: the batch in another order.  M is unchanged, so every per-row value of the backward is bit for bit the same and only
    the rows' assignment to blocks / slices changes: the gradients agree to the fp32 summation order, while a block's partial lost or
    counted twice removes or adds other samples in the two orders (about 1 / sqrt(blocks) >= 6e-2 of a tensor's norm).
    additivity: the mean of two half-batch gradients with equal kept-token counts (the halves' loss divisor is exactly twice the full
    batch's) against the full-batch gradient.  Other row counts change the deep-K lm_head GEMM's K split, so its 16-bit output
    rounds differently here and there: bf16-level noise that the bound has to admit.  A layer's bias gradient sent to another layer in
    every call is linear in the batch and passes both properties; the oracle comparisons (below, and the full-size mapper test) catch it."""
    c, me, ge, eng, tokens, embeds = big
    h = c["B"] // 2
    t = tokens.clone()
    fresh = torch.randint(1, c["V"], (h, c["cap"]), generator=torch.Generator(device="cuda").manual_seed(3), device="cuda")
    t[h:] = torch.where(t[:h] > 0, fresh, t[:h])      # the second half ignores the same positions as the first
    _, g0, n0 = _grads(eng, t, embeds)
    perm = torch.randperm(c["B"], generator=torch.Generator(device="cuda").manual_seed(4), device="cuda")
    _, gp, _ = _grads(eng, t[perm], embeds[perm])
    _, ga, na = _grads(eng, t[:h], embeds[:h])
    _, gb, nb = _grads(eng, t[h:], embeds[h:])
    assert na == nb and na + nb == n0
    v0, vp, vc = me.views(g0), me.views(gp), me.views((ga + gb) / 2)
    groups = _reduced_groups(v0)
    assert len(groups) == 2 + 7 * c["N"] + ("pos_embeddings" in v0)      # linear.bias, prefix_const; per layer 2 LNs and 3 biases
    rp = {k: _rel(vp[k], v0[k]) for k in groups}
    ra = {k: _rel(vc[k], v0[k]) for k in groups}
    for name, r in (("permutation", rp), ("additivity", ra)):
        k = max(r, key=r.get)
        print(f"per-parameter {name} at B = 256: worst relative difference {r[k]:.3e} ({k})")
    assert max(rp.values()) <= PERMUTATION_TOL, rp
    assert max(ra.values()) <= ADDITIVITY_TOL, ra


@pytest.mark.parametrize("precision", ["bf16", 32])
def test_full_finetune_per_parameter_gradients_vs_oracle(precision):
    """One full-finetune step at a small config against the CPU oracle, per parameter, for the parameters the reductions produce: the
    GPT-2 LN weights / biases (ln_f through ln_bwd with the lm_head's row map), every Conv1D / Linear bias, prefix_const,
    pos_embeddings.  B * T = 448 rows: the column sums fold two row slices.  bf16 operands against the oracle's bf16 rounding points;
    split-bf16 operands (--fp-precision 32) against the fp32 oracle.  A window of 2 gives the
    mapper its pos_embeddings (batch_sum over 2 slices of the batch).  A layer's
    bias gradient sent to another layer, or one of two partials lost, is off by O(1)."""
    from clipcap_amd.engine import ClipCapEngine, Gpt2Engine, MapperEngine
    from oracle import clipcap_oracle as O
    torch.manual_seed(21)
    E, D, P, L, H, N, n_head, n_layer, V, npos, B, cap, W = 64, 128, 4, 4, 4, 2, 4, 2, 300, 32, 16, 24, 2
    me = MapperEngine(E, D, L, P, H, N, window=W, use_pos=True, device="cuda")
    ge = Gpt2Engine(D, n_head, n_layer, V, npos, device="cuda")
    sd = {}
    for pre, e in (("transformer_mapper.", me), ("language_model.", ge)):
        for k, v in e.views(e.arena.w32).items():
            if ("norm" in k or "ln_" in k) and k.endswith("weight"):
                t = 1.0 + 0.1 * torch.randn(v.shape)
            elif k.endswith(".bias") or ("norm" in k or "ln_" in k):
                t = 0.05 * torch.randn(v.shape)
            elif k == "prefix_const":
                t = torch.randn(v.shape)
            else:
                t = torch.randn(v.shape) * (0.5 / v.shape[-1] ** 0.5 if "wte" not in k and "wpe" not in k else 0.1)
            sd[pre + k] = t
            v.copy_(t)
    if precision != "bf16":
        me.set_precision(precision)
        ge.set_precision(precision)
    tokens = torch.randint(1, V, (B, cap))
    tokens[::3, 17:] = -1
    embeds = torch.randn(B, W, E)
    eng = ClipCapEngine(me, ge, train_lm=True)
    eng.zero_grad()
    loss = eng.forward_backward(tokens.cuda(), embeds.cuda())
    torch.cuda.synchronize()
    cfg = dict(projection_length=P, prefix_length=L, heads=H, layers=N, n_head=n_head, n_layer=n_layer, window=W)
    sdr = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ref = O.clipcap_loss(sdr, tokens, embeds, cfg=cfg, rb=precision == "bf16")
    ref.backward()
    tol = 2e-2 if precision == "bf16" else 2e-4         # measured worst 5.2e-3 / 1.1e-5
    assert abs(loss.item() - ref.item()) <= tol * abs(ref.item())
    checked, worst = 0, ("", 0.0)
    for pre, e in (("transformer_mapper.", me), ("language_model.", ge)):
        for k, v in _reduced_groups(e.views(e.arena.g32)).items():
            r = _rel(v.cpu(), sdr[pre + k].grad)
            worst = max(worst, (pre + k, r), key=lambda w: w[1])
            assert r <= tol, (pre + k, r)
            checked += 1
    assert checked == (3 + 7 * N) + (8 * n_layer + 2)      # + pos_embeddings; per layer 2 LNs and 3 / 4 biases; + ln_f
    print(f"full finetune ({precision}): worst relative gradient error of the reduced parameters vs oracle {worst[1]:.3e} ({worst[0]})")


def test_full_size_kv_cache_equals_reforward(big):
    from clipcap_amd.engine import DecodeSession
    c, me, ge, eng, tokens, embeds = big
    torch.manual_seed(1)
    x = torch.randn(4, 14, c["D"], device="cuda") * 0.3
    full = ge.logits(x)
    sess = DecodeSession(ge, 4, 32)
    l = sess.forward(x[:, :10]).clone()
    scale = max(1.0, full.abs().max().item())

    def close(a, b):
        # two bf16 evaluation orders of the same 12-layer network (tile shapes / K slices differ between the skinny decode GEMMs and
        # the training-size ones): measured rms 1.0e-3 and max 4.4e-3 .. 5.1e-3 of the logit scale over 200 k logits
        d = (a - b).float()
        return d.abs().max().item() <= 8e-3 * scale and d.pow(2).mean().sqrt().item() <= 2e-3 * scale

    assert close(l, full[:, 9])
    for t in range(10, 14):
        l = sess.forward(x[:, t:t + 1])
        assert close(l, full[:, t]), t


def test_full_size_full_finetune_with_dropout_properties():
    """BASELINE configs[2] size (GPT-2-small unfrozen, B=256) with GPT-2 dropout: same seed -> bitwise the same loss and (up to
    atomic-order rounding) gradients, another seed -> other masks, finite everywhere, and the layer-sliced backward used for
    all-reduce overlap regenerates exactly the masks of the single-call backward."""
    import bench
    c = dict(bench.CONFIGS["3"])
    me, ge, eng = bench.init_engines(c, torch.device("cuda", 0))
    gen = torch.Generator(device="cuda").manual_seed(11)
    embeds = torch.randn(c["B"], c["E"], generator=gen, device="cuda")
    tokens = torch.randint(1, c["V"], (c["B"], c["cap"]), generator=gen, device="cuda")

    def run(seed, sliced=False):
        eng.zero_grad()
        loss = eng.forward_backward(tokens, embeds, dropout=(0.1, 0.1, 0.1, seed), on_grads_ready=(lambda a, lo, hi: None) if sliced else None)
        torch.cuda.synchronize()
        return float(loss), me.arena.g32.clone(), ge.arena.g32.clone()

    l0, gm0, gg0 = run(5)
    l1, gm1, gg1 = run(5)
    l2, gm2, gg2 = run(5, sliced=True)
    l3, _, gg3 = run(6)
    assert torch.isfinite(gm0).all() and torch.isfinite(gg0).all() and abs(l0) < 20
    assert l1 == l0 and _rel(gm1, gm0) <= 1e-5 and _rel(gg1, gg0) <= 1e-5
    assert l2 == l0 and _rel(gm2, gm0) <= 1e-4 and _rel(gg2, gg0) <= 1e-4
    assert l3 != l0 and _rel(gg3, gg0) > 0.05
    eng.zero_grad()
    plain = float(eng.forward_backward(tokens, embeds))
    assert abs(plain - l0) > 1e-4                  # dropout is actually on


@pytest.mark.parametrize("N", [3, 8])
def test_full_size_mapper_gradients_vs_oracle_and_layer_slices(N):
    """The mapper at the FULL config-2 size (B = 256 -> M = 5120 rows; 3 layers = 216 weight-gradient tiles, one round; 8 layers = 576 tiles = two
    full rounds of whole-K tiles + a K-sliced tail added with atomics): at this M the backward takes
    the grouped weight-gradient path that small-shape tests never reach (K >= 1024) — round 5: every layer's weight gradients parked until ONE
    launch at the end of the call.  (1) every gradient tensor against the oracle's autograd with bf16 rounding points; (2) the single-call
    backward against the layer-sliced backward (1, 2 and 3 layers per cc_mapper_bwd_range call): the same kernels on the same operands, so
    equal up to the order of fp32 atomics — a deferred launch that reads an operand a later layer has overwritten shows up in both."""
    from clipcap_amd.engine import MapperEngine
    from oracle import clipcap_oracle as O
    torch.manual_seed(17)
    E, D, P, L, H, B = 512, 768, 10, 10, 8, 256
    eng = MapperEngine(E, D, L, P, H, N, device="cuda")
    views = eng.views(eng.arena.w32)
    sd = {}
    for k, v in views.items():
        if k.endswith("norm1.weight") or k.endswith("norm2.weight"):
            t = 1.0 + 0.1 * torch.randn(v.shape)
        elif k == "prefix_const":
            t = torch.randn(v.shape)
        elif k.endswith(".bias"):
            t = 0.05 * torch.randn(v.shape)
        else:
            t = torch.randn(v.shape) / (v.shape[-1] ** 0.5)
        sd[k] = t
        v.copy_(t)
    eng.arena.mark_dirty() if hasattr(eng.arena, "mark_dirty") else None
    x = torch.randn(B, E)
    out = eng.forward(x.cuda(), save=True)
    dout = (2.0 * out / out.numel())

    def grads(group):
        eng.arena.grads().zero_()
        if group == 0:
            eng.backward(dout)
        else:
            eng.backward(dout, on_layers_done=lambda lo, hi: None, group=group)
        torch.cuda.synchronize()
        return eng.arena.g32.clone()

    g_single = grads(0)
    for group in (1, 2, 3):
        r = _rel(grads(group), g_single)
        assert r <= 1e-5, (group, r)
    sdr = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ref = O.mapper_forward(sdr, x, projection_length=P, num_heads=H, num_layers=N, rb=True)
    ref.square().mean().backward()
    eng.arena.g32.copy_(g_single)
    gv = eng.views(eng.arena.g32)
    worst = ("", 0.0)
    for k in sd:
        r = _rel(gv[k].cpu(), sdr[k].grad)
        if r > worst[1]:
            worst = (k, r)
        assert r <= 3e-2, (k, r)
    print(f"full-size mapper ({N} layers, B = 256): worst relative gradient error vs oracle(bf16 points) {worst[1]:.3e} ({worst[0]})")
