"""Bit reproducibility of a full finetune: the token-indexed scatters into the embedding gradients (the input embedding's wte rows, the tied
lm_head's one-hot term) run through a fixed-order scatter-add (kernels.h scatter_rows) and wpe's gradient through the fixed-order batch
sum, so the whole training step gives the same gradients and weights bit for bit from run to run.

The kernel-level tests pin the documented order exactly: a float32 emulation of it (below) must reproduce cc_embed_tokens_bwd_ws bit for
bit, and the result must lie within 1e-6 of the row scale of a float64 sum."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK = 512                    # kernels.h SCATTER_CHUNK
V, VP = 50257, 50304           # GPT-2's vocabulary and its padded row count


def _emulate(dw0, ids, vals):
    """The order of kernels.h scatter_rows in float32: per id, its rows in ascending row order, cut into chunks of CHUNK rows; each chunk
    summed from its first row in list order; one chunk is added onto the row, several are first added to each other in chunk order."""
    out = dw0.copy()
    order = np.lexsort((np.arange(len(ids)), ids))
    sid = ids[order]
    starts = np.flatnonzero(np.r_[True, sid[1:] != sid[:-1]])
    ends = np.r_[starts[1:], len(sid)]
    for a, b in zip(starts, ends):
        rows = order[a:b]
        sums = []
        for k in range(0, len(rows), CHUNK):
            ch = rows[k:k + CHUNK]
            s = vals[ch[0]].copy()
            for r in ch[1:]:
                s = s + vals[r]
            sums.append(s)
        t = sums[0]
        for x in sums[1:]:
            t = t + x
        out[sid[a]] = out[sid[a]] + t
    return out


def _ids(case, R, rng):
    if case == "one_id":                       # 20 chunks of one list: the multi-chunk fold
        return np.full(R, 7, np.int64)
    if case == "zipf":                         # pads -> id 0 on 20 % of the rows, the rest Zipf-like
        ids = np.minimum(rng.zipf(1.3, R), V - 1).astype(np.int64)
        ids[rng.random(R) < 0.2] = 0
        return ids
    if case == "uniform":
        return rng.integers(0, V, R)
    if case == "chunk_edges":                  # lists of exactly CHUNK, CHUNK + 1, 2 CHUNK and 2 CHUNK + 1 rows
        ids = rng.integers(20, V, R)
        pos = rng.permutation(R)
        o = 0
        for i, n in ((5, CHUNK), (6, CHUNK + 1), (9, 2 * CHUNK), (11, 2 * CHUNK + 1)):
            ids[pos[o:o + n]] = i
            o += n
        return ids
    if case == "edge_ids":                     # the last vocabulary row, the last padded row, and ids clamped into [0, Vp - 1]
        ids = rng.integers(0, V, R)
        ids[:40] = V - 1
        ids[40:70] = VP - 1
        ids[70:80] = -3
        ids[80:90] = VP + 11
        return ids
    raise ValueError(case)


def _cfg(D):
    from clipcap_amd._lib import Gpt2Cfg
    return Gpt2Cfg(D=D, H=1, NL=1, V=V, Vp=VP, NPOS=64, op_dtype=0)


def _scatter(cfg, ids, dout, dw, fill=0xFF):
    """cc_embed_tokens_bwd_ws with a scratch prefilled with garbage and a guard past its end that must stay untouched."""
    from clipcap_amd import _lib
    L = _lib.lib()
    R = ids.numel()
    need = L.cc_embed_tokens_bwd_ws_bytes(C.byref(cfg), R)
    assert need > 0
    ws = torch.full((need + 4096,), fill, dtype=torch.uint8, device="cuda")
    rc = L.cc_embed_tokens_bwd_ws(C.byref(cfg), R, dout.data_ptr(), ids.data_ptr(), dw.data_ptr(), ws.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert bool((ws[need:] == fill).all()), "write past the scratch"


@pytest.mark.parametrize("D", [64, 768, 1024, 1600])
@pytest.mark.parametrize("case", ["one_id", "zipf", "uniform", "chunk_edges", "edge_ids", "one_row"])
def test_embed_tokens_bwd_ws_follows_the_documented_order(case, D):
    rng = np.random.default_rng(D * 7 + len(case))
    R = 1 if case == "one_row" else 10240
    ids = np.array([V - 1]) if case == "one_row" else _ids(case, R, rng)
    cl = np.clip(ids, 0, VP - 1)
    vals = (rng.standard_normal((R, D)) + 0.25).astype(np.float32)        # nonzero mean: the sums grow along the list
    touched = np.unique(cl)
    dw = torch.randn(VP, D, generator=torch.Generator().manual_seed(D)).cuda()    # a nonzero initial gradient
    before = dw.clone()
    dout = torch.from_numpy(vals).cuda()
    ids32 = torch.from_numpy(ids.astype(np.int32)).cuda()
    _scatter(_cfg(D), ids32, dout, dw)
    got = dw[torch.from_numpy(touched).cuda()].cpu().numpy()
    dw0 = before[torch.from_numpy(touched).cuda()].cpu().numpy()
    idx = {int(t): i for i, t in enumerate(touched)}
    emu = _emulate(dw0, np.array([idx[int(t)] for t in cl]), vals)
    bad = np.argwhere(got.view(np.uint32) != emu.view(np.uint32))
    assert len(bad) == 0, f"{len(bad)} elements differ from the documented order, first at row {touched[bad[0][0]]} col {bad[0][1]}"
    # rows without a contribution are untouched
    untouched = torch.ones(VP, dtype=torch.bool, device="cuda")
    untouched[torch.from_numpy(touched).cuda()] = False
    assert torch.equal(dw[untouched], before[untouched])
    # within 1e-6 of the row scale of a float64 sum
    ref = dw0.astype(np.float64)
    scale = np.abs(dw0).astype(np.float64)
    rowi = np.array([idx[int(t)] for t in cl])
    np.add.at(ref, rowi, vals.astype(np.float64))
    np.add.at(scale, rowi, np.abs(vals).astype(np.float64))
    assert (np.abs(got - ref) <= 1e-6 * scale.max(axis=1, keepdims=True)).all()
    # and the same bits again
    dw2 = before.clone()
    _scatter(_cfg(D), ids32, dout, dw2, fill=0x7F)
    assert torch.equal(dw2, dw)


def test_embed_tokens_bwd_ws_rejects_a_missing_scratch():
    from clipcap_amd import _lib
    L = _lib.lib()
    cfg = _cfg(64)
    ids = torch.zeros(8, dtype=torch.int32, device="cuda")
    dout = torch.ones(8, 64, device="cuda")
    dw = torch.zeros(VP, 64, device="cuda")
    assert L.cc_embed_tokens_bwd_ws(C.byref(cfg), 8, dout.data_ptr(), ids.data_ptr(), dw.data_ptr(), None, None) == -4    # CC_ERR_STATE
    torch.cuda.synchronize()
    assert not dw.any()
    assert L.cc_embed_tokens_bwd_ws_bytes(C.byref(cfg), 0) < 0


def _run(cfg_key, precision, steps, seed=99):
    import bench
    c = dict(bench.CONFIGS[cfg_key])
    assert c["train_lm"]
    dev = torch.device("cuda", 0)
    me, ge, eng = bench.init_engines(c, dev)
    if precision != "bf16":
        me.set_precision(precision)
        ge.set_precision(precision)
    gen = torch.Generator(device=dev).manual_seed(seed)
    embeds = torch.randn(c["B"], c["E"], generator=gen, device=dev)
    tokens = torch.randint(1, c["V"], (c["B"], c["cap"]), generator=gen, device=dev)
    tokens[::5, 33:] = -1
    tokens[:, 3] = 13                           # a frequent id: a list longer than one chunk
    losses = []
    for i in range(steps):
        eng.zero_grad()
        losses.append(eng.forward_backward(tokens, embeds, dropout=(0.1, 0.1, 0.1, 1000 + i)).clone())
        eng.optimizer_step(1e-4, i + 1)
    torch.cuda.synchronize()
    out = [torch.stack(losses)] + [t.clone() for t in (me.arena.g32, me.arena.w32, ge.arena.g32, ge.arena.w32)]
    del me, ge, eng
    torch.cuda.empty_cache()
    return out


def _same(a, b):
    assert torch.isfinite(a[0]).all() and torch.isfinite(a[3]).all()
    assert float(a[3].abs().max()) > 0
    for name, x, y in zip(("losses", "mapper gradients", "mapper weights", "GPT-2 gradients", "GPT-2 weights"), a, b):
        assert torch.equal(x, y), f"{name}: max |diff| {(x - y).abs().max().item():.3e}"


@pytest.mark.parametrize("precision", ["bf16", 16, 32])
def test_full_finetune_gpt2_small_is_bit_reproducible(precision):
    """configs[2]: GPT-2-small full finetune, B = 256, cap = 40, dropout 0.1 at all three sites, pads; 3 steps twice."""
    _same(_run("3", precision, 3), _run("3", precision, 3))


def test_full_finetune_gpt2_medium_is_bit_reproducible():
    """configs[3]: GPT-2-medium full finetune, B = 128, bf16; 2 steps twice."""
    _same(_run("4", "bf16", 2), _run("4", "bf16", 2))


def test_module_forward_backward_of_a_full_finetune_is_bit_reproducible():
    """The autograd path (Module.forward, loss.backward()): wte.grad and wpe.grad are the same bits from run to run, and the input
    embedding's gradient equals torch's within 1e-6 of the row scale."""
    from clipcap_amd.encoders import EncoderConfig
    from clipcap_amd.model import ClipCapModel, Config, TrainingConfig
    from clipcap_amd.model.gpt2 import GPT2LM
    torch.manual_seed(0)
    Vs, D, cap, B = 157, 128, 24, 48
    lm = GPT2LM(n_embd=D, n_layer=2, n_head=2, vocab_size=Vs, n_positions=64)
    cfg = Config(language_model="unused", train_language_model=True, prefix_length=3, projection_length=2, transformer_layers=1,
                 transformer_attention_heads=2, encoder_config=EncoderConfig(encoder_embedding_size=16),
                 training_config=TrainingConfig(optimizer_lr=0.0, use_deepspeed_optimisers=False, scheduler_warmup_steps=1, total_steps=4))
    m = ClipCapModel(cfg, language_model=lm).to("cuda").eval()
    g = torch.Generator().manual_seed(3)
    tokens = torch.randint(1, Vs, (B, cap), generator=g)
    tokens[:, :12] = 5                          # 576 rows on one id: two chunks
    tokens[::4, 20:] = -1
    tokens, embeds = tokens.cuda(), torch.randn(B, 16, generator=g).cuda()
    wte = m.language_model.get_input_embeddings().weight
    wpe = m.language_model._arena_params["transformer.wpe.weight"]

    def step():
        for p in (wte, wpe):
            p.grad = None
        logits = m(tokens, embeds).logits
        loss = torch.nn.functional.cross_entropy(logits[:, 2:-1].reshape(-1, Vs), tokens.clamp_min(0).reshape(-1), ignore_index=0)
        loss.backward()
        torch.cuda.synchronize()
        return wte.grad.clone(), wpe.grad.clone()

    a, b = step(), step()
    assert float(a[0].abs().max()) > 0 and float(a[1].abs().max()) > 0
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # the embedding's own gradient against F.embedding's
    emb = m.language_model.get_input_embeddings()
    ids = tokens.clamp_min(0)
    up = torch.randn(B, cap, D, generator=torch.Generator().manual_seed(4)).cuda()
    (gw,) = torch.autograd.grad((emb(ids) * up).sum(), wte)
    w2 = wte.detach().clone().requires_grad_(True)
    (gr,) = torch.autograd.grad((torch.nn.functional.embedding(ids, w2) * up).sum(), w2)
    scale = torch.zeros_like(gr).index_add_(0, ids.reshape(-1), up.abs().reshape(-1, D)).amax(dim=1, keepdim=True)
    assert ((gw - gr).abs() <= 1e-6 * scale).all()
    (gw2,) = torch.autograd.grad((emb(ids) * up).sum(), wte)
    assert torch.equal(gw, gw2)
