"""Global gradient-norm clipping on the device: cc_grad_sqnorm against float64 within the bound its documented summation order gives,
cc_grad_clip_coef against float64, cc_adamw_step_clip bit for bit against cc_adamw_step / cc_adamw_step_cast, and the clipped training
step end to end (bf16 / split-bf16 / fp16 operands, frozen LM and full finetune, two ranks)."""
import ctypes as C
import math
import os
import re
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24          # unit roundoff of fp32, round to nearest


def _lib():
    from clipcap_amd import _lib as L
    return L.lib()


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _grid():
    """(BLOCKS, THREADS, ACC): the grid constants include/clipcap_hip.h states for cc_grad_sqnorm."""
    hdr = open(os.path.join(ROOT, "include", "clipcap_hip.h")).read()
    return tuple(int(re.search(rf"#define CC_GRAD_NORM_{k}\s+(\d+)", hdr).group(1)) for k in ("BLOCKS", "THREADS", "ACC"))


def _depth(n):
    """Roundings on the longest way an input's square takes into sumsq[0], from the order the header documents (every term is
    non-negative, so sum * ((1 + U)^depth - 1) bounds the error; depth * U is that to first order, and three of the counted additions
    are exact — an accumulator's, a fold thread's and sumsq's first addition to 0 — which covers the higher orders many times over)."""
    blocks, threads, acc = _grid()
    n4 = n // 4
    nb = min(-(-n4 // threads), blocks)
    visits = -(-n4 // (nb * threads))
    return (3                               # x*x, then the two levels of (x*x + y*y) + (z*z + w*w)
            + -(-visits // acc)             # the accumulator's chain
            + 2 + 6 + 2                     # (a0 + a1) + (a2 + a3); 64-lane tree; the block's four waves
            + blocks // threads             # the fold thread's run of partials
            + 6 + 2                         # the fold's lane tree and waves
            + 1)                            # sumsq[0] + total


def _scratch():
    n = _lib().cc_grad_norm_scratch_floats()
    assert n == _grid()[0]
    return torch.full((n + 64,), 7.0, device="cuda")      # 64 guard floats behind what the call may use


def _sqnorm(g, sumsq, scratch=None):
    scratch = _scratch() if scratch is None else scratch
    rc = _lib().cc_grad_sqnorm(_p(g), g.numel(), _p(scratch), _p(sumsq), _st())
    torch.cuda.synchronize()
    n = _lib().cc_grad_norm_scratch_floats()
    assert torch.equal(scratch[n:], torch.full((64,), 7.0, device="cuda")), "cc_grad_sqnorm wrote past its scratch"
    return rc


def _sizes():
    blocks, threads, _ = _grid()
    stride = blocks * threads * 4           # floats one full grid stride covers
    return [4, 252, 1024, stride + 4, 2 * stride + 4, 1_000_004]


def _case(n, seed):
    gen = torch.Generator().manual_seed(seed)
    scale = (1e-4, 1.0, 1e3)[int(torch.randint(0, 3, (1,), generator=gen))]
    g = torch.randn(n, generator=gen) * scale
    idx = torch.randint(0, n, (min(n, 5),), generator=gen)
    g[idx] *= 1e3                           # a handful of elements at 1e3 x the rest
    return g.cuda()


@pytest.mark.parametrize("i", range(6))
def test_grad_sqnorm_against_float64_within_the_bound_of_its_order(i):
    n = _sizes()[i]
    g = _case(n, 100 + i)
    ref = float(g.double().square().sum())
    sumsq = torch.zeros(1, device="cuda")
    assert _sqnorm(g, sumsq) == 0
    got = float(sumsq)
    bound = _depth(n) * U
    print(f"n {n}: sumsq {got:.9e} float64 {ref:.9e} relative error {abs(got - ref) / ref:.3e} bound {bound:.3e} (depth {_depth(n)})")
    assert math.isfinite(got) and abs(got - ref) <= bound * ref
    again = torch.zeros(1, device="cuda")
    assert _sqnorm(g, again) == 0
    assert torch.equal(again.view(torch.int32), sumsq.view(torch.int32))          # the same bits from call to call


def test_grad_sqnorm_accumulates_and_rejects_odd_lengths():
    stride = _sizes()[3] - 4
    na, nb = stride + 4, 1_000_004
    a, b = _case(na, 7), _case(nb, 8)
    ra, rb = float(a.double().square().sum()), float(b.double().square().sum())
    ab = torch.cat((a, b))
    s = torch.zeros(1, device="cuda")
    assert _sqnorm(ab, s) == 0
    assert math.isfinite(float(s)) and abs(float(s) - (ra + rb)) <= _depth(na + nb) * U * (ra + rb)
    s = torch.zeros(1, device="cuda")
    assert _sqnorm(a, s) == 0 and _sqnorm(b, s) == 0
    d = max(_depth(na) + 1, _depth(nb))       # a's sum passes through one more addition when b's arrives
    print(f"a then b: {float(s):.9e} float64 {ra + rb:.9e} relative error {abs(float(s) - (ra + rb)) / (ra + rb):.3e} bound {d * U:.3e}")
    assert abs(float(s) - (ra + rb)) <= d * U * (ra + rb)
    before = s.clone()
    for n in (5, 6, 1023):
        assert _lib().cc_grad_sqnorm(_p(a), n, _p(_scratch()), _p(s), _st()) == -2
    assert _lib().cc_grad_sqnorm(_p(a), 0, _p(_scratch()), _p(s), _st()) == 0           # n == 0: a no-op
    assert _lib().cc_grad_sqnorm(None, 4, _p(_scratch()), _p(s), _st()) == -1
    assert _lib().cc_grad_sqnorm(_p(a), 4, None, _p(s), _st()) == -1
    assert _lib().cc_grad_sqnorm(_p(a), 4, _p(_scratch()), None, _st()) == -1
    torch.cuda.synchronize()
    assert torch.equal(s.view(torch.int32), before.view(torch.int32))


def _coef(sumsq, max_norm, grad_scale=1.0, loss_scale=None):
    ss = torch.tensor([sumsq], dtype=torch.float32, device="cuda")
    ls = torch.tensor([loss_scale, 0.0, 0.0], dtype=torch.float32, device="cuda") if loss_scale is not None else None
    clip = torch.full((2,), -5.0, device="cuda")
    assert _lib().cc_grad_clip_coef(_p(ss), max_norm, grad_scale, _p(ls), _p(clip), _st()) == 0
    torch.cuda.synchronize()
    return clip.cpu().numpy()


def _ulps(got, ref):
    return abs(float(got) - ref) / float(np.spacing(np.float32(ref)))


@pytest.mark.parametrize("grad_scale,loss_scale", [(1.0, None), (0.5, 1024.0)])
def test_grad_clip_coef_against_float64(grad_scale, loss_scale):
    """One sqrt, one multiply, one divide, one add and one divide: the build rounds fp32 sqrt and divide correctly (hipcc's default for
    HIP, no fast-math flag in the Makefile), so 4 ulp of fp32 holds the five roundings."""
    for sumsq in (3.7e-3, 41.5, 9.3e7):
        ss = float(np.float32(sumsq))
        norm = math.sqrt(ss) * grad_scale / (loss_scale if loss_scale is not None else 1.0)
        c = _coef(sumsq, float("inf"), grad_scale, loss_scale)
        assert c[0] == np.float32(1.0) and _ulps(c[1], norm) <= 4                 # report only: exactly 1
        c = _coef(sumsq, float(np.float32(norm * 3.0)), grad_scale, loss_scale)
        assert c[0] == np.float32(1.0) and _ulps(c[1], norm) <= 4                 # below max_norm: exactly 1
        mx = float(np.float32(norm * 0.37))
        c = _coef(sumsq, mx, grad_scale, loss_scale)
        want = mx / (norm + float(np.float32(1e-6)))
        print(f"sumsq {ss:.4e}: coefficient {c[0]:.9e} float64 {want:.9e} ({_ulps(c[0], want):.2f} ulp), norm {c[1]:.9e} ({_ulps(c[1], norm):.2f} ulp)")
        assert _ulps(c[0], want) <= 4 and _ulps(c[1], norm) <= 4 and c[0] < 1
    for bad in (float("nan"), float("inf")):
        for mx in (1.0, float("inf")):
            assert math.isnan(_coef(bad, mx, grad_scale, loss_scale)[0])          # a norm that is not finite: NaN coefficient
    assert _lib().cc_grad_clip_coef(None, 1.0, 1.0, None, _p(torch.zeros(2, device="cuda")), _st()) == -1
    assert _lib().cc_grad_clip_coef(_p(torch.zeros(1, device="cuda")), 1.0, 1.0, None, None, _st()) == -1


def _adamw_inputs(n, seed):
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen) * 3.0
    m = torch.randn(n, generator=gen) * 0.1
    v = torch.rand(n, generator=gen) * 0.01
    return [t.cuda() for t in (p, g, m, v)]


def _adamw(n, seed, op, entry, step=3, grad_scale=1.0, state=None, found=None, clip="absent"):
    """One AdamW call on fresh copies of the same inputs; entry "plain" = cc_adamw_step (+ cc_adamw_step_cast when op has a flat cast),
    "clip" = cc_adamw_step_clip.  Returns the bits of (p, m, v, w16)."""
    p, g, m, v = _adamw_inputs(n, seed)
    cast = op != 2                            # split-bf16 operands have no flat cast
    w16 = torch.full((n,), 0x1234, dtype=torch.int16, device="cuda") if cast else None
    hp = (1e-2, 0.9, 0.999, 1e-8, 0.01)
    l = _lib()
    if entry == "plain":
        if cast:
            rc = l.cc_adamw_step_cast(op, _p(p), _p(g), _p(m), _p(v), n, *hp, step, grad_scale, _p(state), _p(found), _p(w16), _st())
        else:
            rc = l.cc_adamw_step(_p(p), _p(g), _p(m), _p(v), n, *hp, step, grad_scale, _p(state), _p(found), _st())
    else:
        rc = l.cc_adamw_step_clip(op, _p(p), _p(g), _p(m), _p(v), n, *hp, step, grad_scale, _p(state), _p(found), _p(clip), _p(w16), _st())
    assert rc == 0
    torch.cuda.synchronize()
    return [t.view(torch.int32).clone() for t in (p, m, v)] + ([w16.clone()] if cast else [])


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("op", [0, 1, 2])
@pytest.mark.parametrize("n", [8, 1024 * 4 + 8, 300_004])
def test_adamw_step_clip_bitwise(n, op):
    seed = n + op
    one = torch.tensor([1.0], device="cuda")
    quarter = torch.tensor([0.25], device="cuda")
    ref = _adamw(n, seed, op, "plain")
    start = [t.view(torch.int32) for t in _adamw_inputs(n, seed)]
    assert not torch.equal(ref[0], start[0])
    assert _same(_adamw(n, seed, op, "clip", clip=None), ref)                           # clip = NULL
    assert _same(_adamw(n, seed, op, "clip", clip=one), ref)                            # clip[0] = 1.0
    assert _same(_adamw(n, seed, op, "clip", clip=quarter), _adamw(n, seed, op, "plain", grad_scale=0.25))
    assert not _same(_adamw(n, seed, op, "clip", clip=quarter), ref)
    # found_inf set: nothing is written
    found = torch.ones(1, device="cuda")
    state = torch.tensor([1024.0, 3.0, 5.0], device="cuda")
    out = _adamw(n, seed, op, "clip", step=0, state=state, found=found, clip=quarter)
    assert torch.equal(out[0], start[0]) and torch.equal(out[1], start[2]) and torch.equal(out[2], start[3])
    if op != 2:
        assert torch.equal(out[3], torch.full((n,), 0x1234, dtype=torch.int16, device="cuda"))
    # step = 0 with a scaler state: the step number and the loss scale come from the device
    clear = torch.zeros(1, device="cuda")
    assert _same(_adamw(n, seed, op, "clip", step=0, state=state, found=clear, clip=one), _adamw(n, seed, op, "plain", step=0, state=state, found=clear))
    assert _same(_adamw(n, seed, op, "clip", step=0, state=state, found=clear, clip=None), _adamw(n, seed, op, "plain", step=0, state=state, found=clear))
    # w16 = NULL: no cast, whatever the operand mode — cc_adamw_step's bits
    p, g, m, v = _adamw_inputs(n, seed)
    assert _lib().cc_adamw_step_clip(op, _p(p), _p(g), _p(m), _p(v), n, 1e-2, 0.9, 0.999, 1e-8, 0.01, 3, 1.0, None, None, _p(one), None, _st()) == 0
    torch.cuda.synchronize()
    assert torch.equal(p.view(torch.int32), ref[0]) and torch.equal(m.view(torch.int32), ref[1]) and torch.equal(v.view(torch.int32), ref[2])
    if op == 2:                               # as cc_adamw_step_cast: no flat cast of split-bf16 operands
        w16 = torch.zeros(n, dtype=torch.int16, device="cuda")
        assert _lib().cc_adamw_step_clip(op, _p(p), _p(g), _p(m), _p(v), n, 1e-2, 0.9, 0.999, 1e-8, 0.01, 3, 1.0, None, None, None, _p(w16), _st()) == -1
    assert _lib().cc_adamw_step_clip(op, _p(p), _p(g), _p(m), _p(v), 6, 1e-2, 0.9, 0.999, 1e-8, 0.01, 3, 1.0, None, None, None, None, _st()) == -2
    assert _lib().cc_adamw_step_clip(op, None, _p(g), _p(m), _p(v), 8, 1e-2, 0.9, 0.999, 1e-8, 0.01, 3, 1.0, None, None, None, None, _st()) == -1


# ---- one training step end to end ---------------------------------------------------------------------------------------------------
def _model(mode, precision):
    from tests.test_gpu_fp16 import _tiny_model
    m, g = _tiny_model(mode, precision)
    m.train()
    return m, (torch.from_numpy(g["in.tokens"]).cuda(), torch.from_numpy(g["in.embeds"]).cuda())


def _state(m):
    out = []
    for a in m.engine.arenas():
        out += [a.w32.view(torch.int32).clone(), a.m.view(torch.int32).clone(), a.v.view(torch.int32).clone()]
    return out


def _norm64(arenas, div=1.0):
    return math.sqrt(sum(float((a.g32.double() / div).square().sum()) for a in arenas))


def _norm_bound(arenas):
    """Relative bound of the squared norm over the arenas in order (an earlier arena's sum passes through one addition per later arena);
    half of it holds after the root (the root's own rounding sits inside the three exact additions _depth counts)."""
    ns = [a.n for a in arenas]
    return max(_depth(n) + (len(ns) - 1 - i) for i, n in enumerate(ns)) * U


@pytest.mark.parametrize("precision", ["bf16", 32])
@pytest.mark.parametrize("mode", ["prefix_only", "full"])
def test_clipped_training_step_end_to_end(mode, precision):
    lr = 1e-3
    plain, batch = _model(mode, precision)
    plain.fused_step((batch[0].clone(), batch[1]), lr)
    assert plain.engine.clipper is None and plain.last_grad_norm is None
    off, _ = _model(mode, precision)
    off.fused_step((batch[0].clone(), batch[1]), lr, max_grad_norm=None)
    assert off.engine.clipper is None and _same(_state(off), _state(plain))             # off: today's step, bit for bit
    rep, _ = _model(mode, precision)
    rep.fused_step((batch[0].clone(), batch[1]), lr, max_grad_norm=float("inf"))
    assert _same(_state(rep), _state(plain))                                            # report only: the same bits, and the norm
    norm = float(rep.last_grad_norm)
    assert float(rep.engine.clipper.coef) == 1.0 and norm > 0
    c = 0.5 * norm
    A, _ = _model(mode, precision)
    A.fused_step((batch[0].clone(), batch[1]), lr, max_grad_norm=c)
    coef = float(A.engine.clipper.coef)
    assert 0.49 < coef < 0.51                                                           # clipping really engages
    B, _ = _model(mode, precision)
    B.engine.zero_grad()
    B.engine.forward_backward(batch[0].clone(), batch[1])
    ref = _norm64(B.engine.arenas())
    B.engine.optimizer_step(lr, 1, weight_decay=B._weight_decay(), grad_scale=coef)
    torch.cuda.synchronize()
    assert _same(_state(A), _state(B))
    assert not _same(_state(A), _state(plain))
    bound = 0.5 * _norm_bound(B.engine.arenas())
    got = float(A.last_grad_norm)
    print(f"{mode} {precision}: last_grad_norm {got:.9e} float64 {ref:.9e} relative error {abs(got - ref) / ref:.3e} bound {bound:.3e}")
    assert abs(got - ref) <= bound * ref and got == norm


@pytest.mark.parametrize("mode", ["prefix_only", "full"])
def test_fp16_norm_is_unscaled_and_an_overflow_still_skips_the_step(mode):
    lr = 1e-3
    A, batch = _model(mode, 16)
    A.fused_step((batch[0].clone(), batch[1]), lr, max_grad_norm=float("inf"))
    B, _ = _model(mode, 16)
    B.engine.zero_grad()
    B.engine.forward_backward(batch[0].clone(), batch[1])
    scale = float(B.engine.scaler.scale)
    assert scale == 65536.0
    ref = _norm64(B.engine.arenas(), scale)
    got = float(A.last_grad_norm)
    bound = 0.5 * _norm_bound(B.engine.arenas())
    print(f"{mode} fp16: last_grad_norm {got:.9e} float64 of g32 / scale {ref:.9e} relative error {abs(got - ref) / ref:.3e} bound {bound:.3e}")
    assert abs(got - ref) <= bound * ref
    # a step whose gradients hold an inf: skipped exactly as without clipping
    eng = A.engine
    before = _state(A)
    applied = float(eng.scaler.state[2])
    eng.zero_grad()
    eng.forward_backward(batch[0].clone(), batch[1])
    eng.arenas()[-1].g32[5] = float("inf")
    eng.optimizer_step(lr, 2, weight_decay=A._weight_decay(), max_grad_norm=1.0)
    torch.cuda.synchronize()
    assert _same(_state(A), before)
    assert float(eng.scaler.scale) == scale / 2 and float(eng.scaler.state[2]) == applied and float(eng.scaler.found_inf) == 0.0
    assert math.isnan(float(eng.clipper.coef))
    A.fused_step((batch[0].clone(), batch[1]), lr, max_grad_norm=1.0)                    # and the next healthy step trains again
    assert not _same(_state(A), before) and all(torch.isfinite(a.w32).all() for a in eng.arenas())
    assert float(eng.scaler.state[2]) == applied + 1


def test_optimizer_object_clips_on_the_configure_optimizers_path():
    """ArenaAdamW(max_grad_norm=c).step() on gradients left in the arenas = the engine's clipped step, bit for bit."""
    lr = 1e-3
    B, batch = _model("full", "bf16")
    B.engine.zero_grad()
    B.engine.forward_backward(batch[0].clone(), batch[1])
    c = 0.5 * _norm64(B.engine.arenas())
    opt = B.configure_optimizers(max_grad_norm=c)["optimizer"]
    assert opt.last_grad_norm is None
    opt.param_groups[0]["lr"] = lr
    opt.step()
    A, _ = _model("full", "bf16")
    A.fused_step((batch[0].clone(), batch[1]), lr, max_grad_norm=c)
    torch.cuda.synchronize()
    assert _same(_state(A), _state(B)) and float(opt.last_grad_norm) == float(A.last_grad_norm) > c
    assert 0.49 < float(A.engine.clipper.coef) < 0.51


# ---- two ranks ------------------------------------------------------------------------------------------------------------------------
def _rank_worker(rank, world, port, c, out, backend, stages):
    """backend "nccl": RCCL, one GPU per rank.  "gloo": both ranks on the one GPU of the box, as tests/test_gpu_ddp.py runs its 2-rank
    steps (gloo moves device tensors for all-reduce and broadcast only, so no reduce-to-owner: stages 0 and 1)."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dev = torch.device("cuda", rank if backend == "nccl" else 0)
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from clipcap_amd.train.ddp import GradReducer, ZeroShard, shard_batch
    from tests.test_gpu_ddp import _build
    res = {}
    for stage in stages:
        eng, tokens, embeds = _build("full")
        for e in (eng.mapper, eng.gpt2):
            e.to(dev)
        arenas = eng.arenas()
        red = GradReducer([a.grads() for a in arenas])
        if stage >= 1:
            owners = ZeroShard(rank, world).apply(arenas)
            if stage >= 2:
                red.set_owners(owners, rank)
        tk, em = shard_batch(tokens, embeds, rank, world)
        red.begin()
        eng.forward_backward(tk.to(dev), em.to(dev), reduce_stats=red.reduce_stats, on_grads_ready=red.on_grads_ready)
        red.finish()
        eng.optimizer_step(1e-3, 1, weight_decay=0.01, sync_flag=red.reduce_flag, max_grad_norm=c,
                           sync_norm=(red.reduce_flag if stage >= 2 else None))
        moments = [a.full_moments() for a in arenas]            # a collective when the state is sharded
        torch.cuda.synchronize()
        res[f"norm{stage}"] = eng.last_grad_norm.cpu().numpy()
        for i, a in enumerate(arenas):
            res[f"w{stage}_{i}"] = a.w32.cpu().numpy()
            res[f"m{stage}_{i}"] = moments[i][0].cpu().numpy()
    np.savez(out.format(rank), **res)
    dist.destroy_process_group()


def _spawn(fn, args, nprocs, limit):
    """One process per rank, each under a time limit: a child still running at the deadline is killed and the test fails."""
    import torch.multiprocessing as mp
    ctx = mp.start_processes(fn, args=args, nprocs=nprocs, join=False, start_method="spawn")
    deadline = time.monotonic() + limit
    while not ctx.join(timeout=1.0):
        if time.monotonic() >= deadline:
            for p in ctx.processes:
                if p.is_alive():
                    p.kill()
            pytest.fail(f"a rank was still running after {limit} s")


def _two_ranks_against_one(tmp_path, backend, stages):
    from tests.test_ddp_gloo import _free_port
    from tests.test_gpu_ddp import _build
    eng, tokens, embeds = _build("full")
    eng.forward_backward(tokens.cuda(), embeds.cuda())
    eng.optimizer_step(1e-3, 1, weight_decay=0.01, max_grad_norm=float("inf"))
    c = 0.5 * float(eng.last_grad_norm)
    eng, tokens, embeds = _build("full")
    eng.forward_backward(tokens.cuda(), embeds.cuda())
    eng.optimizer_step(1e-3, 1, weight_decay=0.01, max_grad_norm=c)
    torch.cuda.synchronize()
    norm1 = float(eng.last_grad_norm)
    assert 0.49 < float(eng.clipper.coef) < 0.51
    out = str(tmp_path / "clip2_rank{}.npz")
    _spawn(_rank_worker, (2, _free_port(), c, out, backend, stages), 2, limit=240)
    ranks = [np.load(out.format(r)) for r in range(2)]
    for stage in stages:
        norms = [float(r[f"norm{stage}"][0]) for r in ranks]
        print(f"{backend} stage {stage}: last_grad_norm per rank {norms}, one rank {norm1}")
        assert all(abs(x - norm1) <= 2e-2 * norm1 for x in norms), (stage, norms, norm1)
        assert norms[0] == norms[1], (stage, norms)               # whole reduced arenas: the same bits alone; stage 2: the same reduced sum
        for i, a in enumerate(eng.arenas()):
            for key, ref in ((f"w{stage}_{i}", a.w32), (f"m{stage}_{i}", a.m)):
                ref = ref.cpu().numpy()
                for r in ranks:
                    rel = np.linalg.norm(r[key] - ref) / np.linalg.norm(ref)
                    assert rel <= 2e-2, (key, rel)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs: RCCL requires one device per rank")
def test_two_rank_clipped_step_equals_single_process(tmp_path):
    """Plain DDP, ZeRO stage 1 and stage 2 (owned slices squared per rank, the 1-float SUM over the ranks) against the 1-rank clipped step
    on the whole batch, at tests/test_gpu_ddp.py's bar for a 2-rank step (per-rank GEMMs see other M tiles: 2e-2 of each tensor's norm);
    with whole reduced arenas every rank computes the norm alone and gets the same bits."""
    _two_ranks_against_one(tmp_path, "nccl", (0, 1, 2))


def test_two_rank_clipped_step_on_one_gpu(tmp_path):
    """The same comparison with both ranks on one GPU (gloo on device tensors): plain DDP and ZeRO stage 1."""
    _two_ranks_against_one(tmp_path, "gloo", (0, 1))


def test_partitioned_gradients_norm_on_a_one_rank_group(tmp_path):
    """The ZeRO stage 2 route (owned slice per arena, sumsq summed over the ranks by GradReducer.reduce_flag) on a 1-rank gloo group: the
    own slice is the whole arena and the step equals the unpartitioned clipped step bit for bit."""
    import torch.distributed as dist
    from tests.test_ddp_gloo import _free_port
    from tests.test_gpu_ddp import _build
    from clipcap_amd.train.ddp import GradReducer, ZeroShard

    def step(partitioned):
        eng, tokens, embeds = _build("full")
        arenas = eng.arenas()
        red = GradReducer([a.grads() for a in arenas])
        if partitioned:
            red.set_owners(ZeroShard(0, 1).apply(arenas), 0)
        eng.forward_backward(tokens.cuda(), embeds.cuda())       # one rank: the gradients are their own sum (gloo has no device reduce)
        eng.optimizer_step(1e-3, 1, weight_decay=0.01, sync_flag=red.reduce_flag, max_grad_norm=0.5,
                           sync_norm=(red.reduce_flag if partitioned else None))
        torch.cuda.synchronize()
        return [a.w32.clone() for a in arenas], eng.clipper.clip.clone()

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        w0, c0 = step(False)
        w1, c1 = step(True)
    finally:
        dist.destroy_process_group()
    assert torch.equal(c0, c1) and 0 < float(c0[0]) < 1 and all(torch.equal(a, b) for a, b in zip(w0, w1))
