#!/usr/bin/env python3
"""Digest the raw output bytes of the kernels of kernels.hip / layernorm.hip / reduce.hip / loss.hip / grads.hip, reached through the
library's existing entry points at small seeded shapes and in every operand type an entry point accepts, to compare two builds of the
library bit for bit.  An entry point that refuses an operand type records its return code.  One library per process, each under its own
time limit, nothing more after a failure:

    CLIPCAP_HIP_LIB=<other libclipcap_hip.so> timeout -k 10 170 tools/kernel_hook_bytes.py a.json && timeout -k 10 170 tools/kernel_hook_bytes.py b.json && cmp a.json b.json
"""
import ctypes as C
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clipcap_amd import _lib as L
from tests import lm_ref as LM
from tests import test_gpu_lm_head as TL
from tests import test_gpu_reductions as TR

l = L.lib()
OPS = (("bf16", 0, torch.bfloat16), ("fp16", 1, torch.float16), ("x3", 2, torch.float32))      # name, op_dtype, stored-activation type
res = {}


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def h(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def record(key, rc, *outs):
    torch.cuda.synchronize()
    assert key not in res, key
    res[key] = [rc] + ([h(t) for t in outs] if rc == 0 else [])


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def randn(g, *shape):
    return torch.randn(*shape, generator=g, device="cuda")


# ---- LayerNorm forward (k_ln_fwd, every NV) and backward (k_ln_bwd, the five variants of test_ln_bwd_variants) ----
for name, op, dt in OPS:
    for rows, D in ((7, 64), (130, 768), (33, 1024), (5, 1600)):
        g = gen(rows * 31 + D)
        x, gamma, beta = randn(g, rows, D) + 0.5, 1.0 + 0.2 * randn(g, D), 0.1 * randn(g, D)
        y = torch.full((rows, D), 3.0, dtype=dt, device="cuda")
        mean, rstd = torch.full((rows,), 7.0, device="cuda"), torch.full((rows,), 7.0, device="cuda")
        record(f"ln_fwd {name} {rows}x{D}", l.cc_layernorm_fwd(op, p(x), p(gamma), p(beta), p(y), p(mean), p(rstd), rows, D, st()), y, mean, rstd)
ws = torch.full((TR.RED_FLOATS + 4096,), float("nan"), device="cuda")
for name in ("bf16", "fp16"):
    for variant in ("plain", "dcol", "dres", "row_map", "row_map_dres"):
        for rows, D in ((7, 64), (2049, 768)):
            code, t = TR._ln_case(name, rows, D, dcol=variant == "dcol", dres="dres" in variant, row_map="row_map" in variant, seed=rows + D + len(variant))
            rc = TR._ln_call(code, t, rows, D, TR._poison(ws))
            record(f"ln_bwd {name} {variant} {rows}x{D}", rc, t["dx32"], t["dx16"], t["dgamma"], t["dbeta"], *([t["dcol"]] if t["dcol"] is not None else []))
dy = torch.ones(8, 64, device="cuda")
record("ln_bwd x3", l.cc_layernorm_bwd(2, p(dy), p(dy), 64, None, p(dy), p(dy), p(dy), None, p(dy), None, None, None, None, 8, 64, None, st()))

# ---- column sums, batch sums (k_colsum_bf16*, k_batch_sum, k_fold_partials): the first two shapes of their tests ----
for name, op, dt in OPS:
    for M, N in TR.CS_SHAPES[:2]:
        X, out0 = TR._colsum_case(dt, M, N, N + 24, M * 13 + N)
        out = out0.clone()
        record(f"colsum {name} {M}x{N}", l.cc_colsum_bf16(op, p(X), N + 24, M, N, p(out), p(TR._poison(ws)), st()), out)
    for M, N in ((5120, 1536), (2049, 72)):
        for n in (1, 3):
            Xs, outs = zip(*[TR._colsum_case(dt, M, N, N + 8, 1000 * i + M + N) for i in range(n)])
            xa = (C.c_void_p * n)(*[x.data_ptr() for x in Xs])
            oa = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
            record(f"colsum_multi {name} n={n} {M}x{N}", l.cc_colsum_multi(op, xa, oa, n, N + 8, M, N, p(TR._poison(ws)), st()), *outs)
for B, length in TR.BS_SHAPES[:2] + [(256, 7680)]:
    g = gen(B * 31 + length)
    src, dst = randn(g, B * (length + 5)) + 0.5, randn(g, length)
    record(f"batch_sum {B}x{length}", l.cc_batch_sum(p(src), length + 5, p(dst), length, B, p(TR._poison(ws)), st()), dst)

# ---- casts and operand images (k_f32_to_bf16, k_x3_split_rows) ----
for name, op, dt in OPS:
    g = gen(11)
    src = randn(g, 8 * 1031)
    dst = torch.zeros(8 * 1031, dtype=torch.int16, device="cuda")
    record(f"cast_op16 {name}", l.cc_cast_op16(op, p(src), p(dst), src.numel(), st()), dst)
    for form in (0, 1):
        rows, width, ld = 37, 72, 76
        src = randn(g, rows, ld)
        dst = torch.zeros(rows, 3 * width, dtype=torch.int16, device="cuda")
        record(f"x3_split_rows {name} form={form}", l.cc_x3_split_rows(op, p(src), ld, rows, width, form, p(dst), st()), dst)

# ---- gradient utilities (grads.hip): wire pack / unpack at an odd length from a misaligned start, non-finite scan, loss scale, norm + clip ----
g = gen(12)
n = 8 * 1031 + 5
src = randn(g, n + 8)
src[17], src[n - 2] = float("nan"), float("inf")
wire = torch.zeros(n + 8, dtype=torch.int16, device="cuda")
record("wire_pack", l.cc_grad_wire_pack(C.c_void_p(src.data_ptr() + 4), C.c_void_p(wire.data_ptr() + 6), n, st()), wire)
back = torch.zeros(n + 8, device="cuda")
record("wire_unpack", l.cc_grad_wire_unpack(C.c_void_p(wire.data_ptr() + 6), C.c_void_p(back.data_ptr() + 12), n, st()), back)
grads = randn(g, 4 * 70001)
found = torch.zeros(1, device="cuda")
record("grad_nonfinite clean", l.cc_grad_nonfinite(p(grads), grads.numel(), p(found), st()), found)
state = torch.tensor([1024.0, 1.0, 5.0], device="cuda")
for i in range(3):      # two good steps (the second grows the scale at interval 3), then an overflow
    if i == 2:
        grads[4 * 70001 - 3] = float("inf")
        record("grad_nonfinite inf", l.cc_grad_nonfinite(p(grads), grads.numel(), p(found), st()), found)
        grads[4 * 70001 - 3] = 0.25
    record(f"loss_scale_update {i}", l.cc_loss_scale_update(p(state), p(found), 2.0, 0.5, 3, st()), state, found)
scratch = torch.full((l.cc_grad_norm_scratch_floats(),), float("nan"), device="cuda")
sumsq, clip = torch.full((1,), 0.5, device="cuda"), torch.zeros(2, device="cuda")
for m in (4, 4 * 70001, 4 * 300000):      # one block, many blocks, the block cap
    gg = randn(g, m)
    record(f"grad_sqnorm {m}", l.cc_grad_sqnorm(p(gg), m, p(scratch), p(sumsq), st()), sumsq)
record("grad_clip_coef", l.cc_grad_clip_coef(p(sumsq), 1.0, 0.5, p(state), p(clip), st()), clip)

# ---- AdamW (k_adamw, host and device step count), with the 16-bit copy and the clip coefficient ----
n = 4 * 4099
for name, op, dt in OPS:
    g = gen(13)
    p0, gr = randn(g, n), randn(g, n)
    for kind in ("step", "cast", "clip", "clip_cast"):
        for step in (3, 0):      # 0: the step number comes from the loss scaler's state
            pp, m, v = p0.clone(), 0.1 * p0, 0.01 * p0 * p0
            w16 = torch.zeros(n, dtype=torch.int16, device="cuda")
            a = (p(pp), p(gr), p(m), p(v), n, 1e-2, 0.9, 0.999, 1e-8, 0.01, step, 0.5, p(state), p(found))
            if kind == "step":
                if op:
                    continue      # no operand type in this entry point
                rc = l.cc_adamw_step(*a, st())
            elif kind == "cast":
                rc = l.cc_adamw_step_cast(op, *a, p(w16), st())
            else:
                rc = l.cc_adamw_step_clip(op, *a, p(clip), p(w16) if kind == "clip_cast" else None, st())
            record(f"adamw {kind} {name} step={step}", rc, pp, m, v, w16)

# ---- dropout mask, token embedding and its fixed-order scatter ----
out = torch.zeros(4099, dtype=torch.uint8, device="cuda")
record("dropout_mask", l.cc_dropout_mask(1234567, 2, 3, 0.1, out.numel(), p(out), st()), out)
cfg = L.Gpt2Cfg(D=64, H=1, NL=1, V=97, Vp=128, NPOS=64, op_dtype=0)
g = gen(14)
R = 1500
w32 = randn(g, l.cc_gpt2_param_count(C.byref(cfg)))
ids = torch.randint(0, 97, (R,), generator=g, device="cuda", dtype=torch.int32)
ids[:700] = 5      # one list of more than one chunk
emb = torch.zeros(R, 64, device="cuda")
record("embed_tokens", l.cc_embed_tokens(C.byref(cfg), R, p(w32), p(ids), p(emb), st()), emb)
dw = randn(g, 128, 64)
sws = torch.full((l.cc_embed_tokens_bwd_ws_bytes(C.byref(cfg), R),), 255, dtype=torch.uint8, device="cuda")
record("embed_tokens_bwd_ws", l.cc_embed_tokens_bwd_ws(C.byref(cfg), R, p(randn(g, R, 64)), p(ids), p(dw), p(sws), st()), dw)

# ---- weight sync / transpose on the tiny configs of tests/test_gpu_kernels.py (casts, k_transpose_bf16_multi, k_x3_split_multi) ----
for name, op, dt in OPS:
    gcfg = L.Gpt2Cfg(64, 4, 2, 97, 128, 16, op)
    mcfg = L.MapperCfg(E=32, D=64, P=3, L=2, H=4, N=2, Hm=128, W=1, use_pos=0, op_dtype=op)
    for what, c, count, sync, transp in (("gpt2", gcfg, l.cc_gpt2_param_count(C.byref(gcfg)), l.cc_gpt2_sync_weights, l.cc_gpt2_transpose_weights),
                                          ("mapper", mcfg, l.cc_mapper_param_count(C.byref(mcfg)), l.cc_mapper_sync_weights, l.cc_mapper_transpose_weights)):
        w = randn(gen(15), count)
        w16 = torch.zeros((6 if op == 2 else 2) * count, dtype=torch.int16, device="cuda")
        record(f"sync_weights {what} {name}", sync(C.byref(c), p(w), p(w16), st()), w16)
        w16[(3 if op == 2 else 1) * count:] = 0
        record(f"transpose_weights {what} {name}", transp(C.byref(c), p(w16), st()), w16)

# ---- lm_head loss rows at the smallest shapes of tests/test_gpu_lm_head.py: D = 64, both training modes and scoring, one deep-K case ----
for name in LM.OPS:
    cs = [c for c in LM.cases(name) if c.D == 64]
    for c in [c for c in cs if c.V == 97] + [next(c for c in cs if LM.deepk_slabs(c, name))]:
        old = l.cc_gemm_tile_mode(c.tile)
        P = TL.Pass(name, c)
        if c.mode == 0:
            lp, ss = P.score()
            outs = [lp, ss, P.get(TL.LSE), P.get(TL.TGT), P.get(TL.HF)]
        else:
            stats = P.fwd()
            outs = [stats, P.get(TL.LSE), P.get(TL.TGT), P.get(TL.ROW_LOSS), P.get(TL.HF)]
            P.bwd(LM.denom_of(c, P.tok.cpu()))
            outs += [P.get(TL.DHF), P.get(TL.DX32), P.g32]
        record(f"lmhead {name} {c.name} {'/'.join(LM.paths(c, name))}", 0, *outs)
        l.cc_gemm_tile_mode(old)

json.dump(res, open(sys.argv[1], "w"), indent=0, sort_keys=True)
print(len(res), "records ->", sys.argv[1])
