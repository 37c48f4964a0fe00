"""The deterministic cross-block reductions of the backward passes (layernorm.hip: ln_bwd's dgamma / dbeta / dcol; reduce.hip:
colsum_bf16, colsum_bf16_multi, batch_sum; all folded by reduce.hip's k_fold_partials), each called on its own through its C-ABI test
hook and compared per column with a float64 reference of the same sum.

What the reference sums is what the kernel sums: 16-bit inputs upcast exactly, dcol = the column sums of the ROUNDED 16-bit dx16 the
kernel wrote.  Every output starts nonzero (the kernels accumulate, on the single-block path and on the fold path alike), every summed
term has a nonzero mean (randn + 0.5, so sum |t| is of the order of |sum t|), and the partial-sum scratch is filled with NaN before
each call (a slot the fold reads but no block wrote this call poisons the result).

Bound, per column: |kernel - ref| <= c * 2^-24 * (|out0| + sum |t|).  A term t reaches the output through at most c fp32 roundings,
so this is the classical bound gamma_c of recursive / tree summation (Higham, Accuracy and Stability of Numerical Algorithms, 4.2),
with c the longest serial chain of the launch as layernorm.hip / reduce.hip compute it (chain_* below mirrors that launch arithmetic):
  * the per-thread serial sum: a wave's rows (ln_bwd), a thread's rows of its slice (colsum: rows_per_slice / 32), a thread's four
    accumulators (batch_sum: ceil(per / 4) + 2);
  * the in-block sum: the NW wave rows of ln_bwd's LDS buffer, the 32 rows of colsum's;
  * the fold (only when there is more than one slice): per chunk of 256 slices a 16-term tree (4 levels), the chunks added serially,
    then the 16 lane sums in lane order;
  * the final += into the output;
  * dgamma only: 3 roundings inside the term d * (x - mu) * rstd.
The chains stay below 200 for every shape here (c * 2^-24 < 1.2e-5), while with terms of one sign one block's partial of a column is
about 1 / (number of partials) >= 1 / 512 of the sum: a partial lost, counted twice or sent to the wrong output is 2 to 3 orders of
magnitude outside the bound.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
RED_FLOATS = 1 << 20           # RED_SCRATCH_FLOATS (kernels.h); test_scratch_size checks the library agrees
WORST = {}                     # reduction -> worst observed |err| / bound (printed at the end of the module)


def _lib():
    from clipcap_amd import _lib
    return _lib.lib()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


OPS = {"bf16": (0, torch.bfloat16), "fp16": (1, torch.float16)}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print(f"\nworst |err| / bound  {k:<14s} {WORST[k]:.3e}")


@pytest.fixture
def ws():
    """the reduction scratch plus a guard tail; NaN everywhere, and the guard must stay NaN"""
    buf = torch.full((RED_FLOATS + 4096,), float("nan"), device="cuda")
    yield buf
    torch.cuda.synchronize()
    assert torch.isnan(buf[RED_FLOATS:]).all(), "a reduction wrote past its scratch"


def _poison(ws):
    ws.fill_(float("nan"))
    return ws


def _check(name, got, ref, abs_sum, chain):
    """per column: |got - ref| <= chain * 2^-24 * abs_sum (ref, abs_sum float64)"""
    torch.cuda.synchronize()
    assert torch.isfinite(got).all(), name
    bound = chain * U * abs_sum
    err = (got.double() - ref).abs()
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    assert ratio <= 1.0, f"{name}: worst |err| / bound {ratio:.3e} (chain {chain})"


def _cdiv(a, b):
    return (a + b - 1) // b


def _fold_chain(S):
    return 0 if S <= 1 else 4 + _cdiv(S, 256) + 16


# ---- launch arithmetic of layernorm.hip / reduce.hip (the grid each wrapper picks), for the chain lengths and to assert which path a shape takes ----
def ln_launch(rows, D, dcol):
    nw = 8 if 16 * D * 4 <= 65536 else 4
    nvec = 3 if dcol else 2
    grid = min(_cdiv(rows, nw), max(1, min(256, RED_FLOATS // (nvec * D))))
    return nw, grid


def colsum_launch(M, N, n=1):
    cb = _cdiv(N, 64)
    slices = max(1, min(_cdiv(M, 256), max(1, 1024 // (cb * n))))
    rps = _cdiv(_cdiv(M, slices), 32) * 32
    return _cdiv(M, rps), rps


def batch_launch(B, length):
    slices = max(1, min(B // 8, 1024 // _cdiv(length, 256)))
    per = _cdiv(B, slices)
    return _cdiv(B, per), per


def chain_ln(rows, D, dcol, dgamma):
    nw, grid = ln_launch(rows, D, dcol)
    return _cdiv(rows, grid * nw) + nw + _fold_chain(max(grid, 2)) + 1 + (3 if dgamma else 0)


def chain_colsum(M, N, n=1):
    slices, rps = colsum_launch(M, N, n)
    return rps // 32 + 32 + _fold_chain(slices) + 1


def chain_batch(B, length):
    slices, per = batch_launch(B, length)
    return _cdiv(per, 4) + 2 + _fold_chain(slices) + 1


# ------------------------------------------------------------------------------------------------------------------------------------
# LayerNorm backward
# ------------------------------------------------------------------------------------------------------------------------------------
def _ln_case(op, rows, D, dcol, dres, row_map, seed):
    code, dt = OPS[op]
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, device="cuda")
    ldx = D + 12 if row_map else D                # row_map: the lm_head's kept rows of a wider row set
    R = rows + 5 if row_map else rows
    rmap = torch.randperm(R, generator=g, device="cuda")[:rows].to(torch.int32).contiguous() if row_map else None
    dy = (rn(rows, D) + 0.5).to(dt)
    x = rn(R, ldx) + 0.5                          # with the given mean / rstd: x_hat has a nonzero mean too
    mean = 0.1 * rn(rows)
    rstd = 0.5 + torch.rand(rows, generator=g, device="cuda")
    gamma = 1.0 + 0.2 * rn(D)
    dres_t = rn(R, ldx) if dres else None
    dx32 = torch.full((R, ldx), 7.0, device="cuda")
    dx16 = torch.full((R, ldx), 3.0, dtype=dt, device="cuda")
    dgamma0, dbeta0, dcol0 = rn(D), rn(D), (rn(D) if dcol else None)
    return code, dict(dy=dy, x=x, ldx=ldx, rmap=rmap, mean=mean, rstd=rstd, gamma=gamma, dres=dres_t, dx32=dx32, dx16=dx16,
                      dgamma=dgamma0.clone(), dbeta=dbeta0.clone(), dcol=dcol0.clone() if dcol else None,
                      dgamma0=dgamma0, dbeta0=dbeta0, dcol0=dcol0)


def _ln_call(code, t, rows, D, ws, with_dg=True):
    return _lib().cc_layernorm_bwd(code, _p(t["dy"]), _p(t["x"]), t["ldx"], _p(t["rmap"]), _p(t["mean"]), _p(t["rstd"]), _p(t["gamma"]),
                                   _p(t["dres"]), _p(t["dx32"]), _p(t["dx16"]), _p(t["dgamma"]) if with_dg else None,
                                   _p(t["dbeta"]) if with_dg else None, _p(t["dcol"]), rows, D, _p(ws), _st())


def _ln_verify(t, rows, D, tag):
    idx = t["rmap"].long() if t["rmap"] is not None else torch.arange(rows, device="cuda")
    dy = t["dy"].double()
    x = t["x"][idx, :D].double()
    mu, rs = t["mean"].double()[:, None], t["rstd"].double()[:, None]
    xh = (x - mu) * rs
    gm = dy * t["gamma"].double()
    m1, m2 = gm.mean(1, keepdim=True), (gm * xh).mean(1, keepdim=True)
    ref = rs * (gm - m1 - xh * m2)
    scale = rs * (gm.abs() + gm.abs().mean(1, keepdim=True) + xh.abs() * (gm * xh).abs().mean(1, keepdim=True))
    if t["dres"] is not None:
        r = t["dres"][idx, :D].double()
        ref, scale = ref + r, scale + r.abs()
    # dx32: a per-row wave reduction over D (4 * NV serial per lane + 6 shuffle levels) and a handful of roundings around it
    nv = min(8, _cdiv(D, 256))
    _check(f"ln dx32{tag}", t["dx32"][idx, :D], ref, scale, 4 * nv + 16)
    # dx16 is exactly the 16-bit rounding of dx32; rows the map does not name and the pad columns are untouched
    dx32, dx16 = t["dx32"], t["dx16"]
    assert torch.equal(dx16[idx, :D], dx32[idx, :D].to(dx16.dtype))
    other = torch.ones(dx32.shape[0], dtype=torch.bool, device="cuda")
    other[idx] = False
    assert (dx32[other] == 7.0).all() and (dx16[other] == 3.0).all()
    assert (dx32[:, D:] == 7.0).all() and (dx16[:, D:] == 3.0).all()
    dcol = t["dcol"] is not None
    tg = dy * xh
    _check(f"ln dgamma{tag}", t["dgamma"], t["dgamma0"].double() + tg.sum(0), t["dgamma0"].double().abs() + tg.abs().sum(0),
           chain_ln(rows, D, dcol, True))
    _check(f"ln dbeta{tag}", t["dbeta"], t["dbeta0"].double() + dy.sum(0), t["dbeta0"].double().abs() + dy.abs().sum(0),
           chain_ln(rows, D, dcol, False))
    if dcol:
        d16 = dx16[idx, :D].double()
        _check(f"ln dcol{tag}", t["dcol"], t["dcol0"].double() + d16.sum(0), t["dcol0"].double().abs() + d16.abs().sum(0),
               chain_ln(rows, D, True, False))


LN_D = [64, 260, 768, 1024, 1280, 1600]
LN_ROWS = [1, 7, 8, 2047, 2049, 7680, 10240]


@pytest.mark.parametrize("D", LN_D)
@pytest.mark.parametrize("rows", LN_ROWS)
def test_ln_bwd_dcol_dres(rows, D, ws):
    """the mapper's form (dres, dx16 and the fused bias column sums) over the shape grid: D <= 1024 runs 8 waves a block and larger D
    4; D = 1600 with dcol clamps the grid to 2^20 / 4800 = 218 blocks; rows from one row to many rows per wave"""
    code, t = _ln_case("bf16", rows, D, dcol=True, dres=True, row_map=False, seed=rows * 7 + D)
    assert _ln_call(code, t, rows, D, _poison(ws)) == 0
    _ln_verify(t, rows, D, "")


def test_ln_bwd_grid_clamp_is_reached():
    assert ln_launch(10240, 1600, True) == (4, 218) and ln_launch(10240, 1600, False) == (4, 256)
    assert ln_launch(10240, 1024, True)[0] == 8 and ln_launch(10240, 1280, True)[0] == 4


@pytest.mark.parametrize("op", ["bf16", "fp16"])
@pytest.mark.parametrize("variant", ["plain", "dcol", "dres", "row_map", "row_map_dres"])
@pytest.mark.parametrize("rows,D", [(7, 64), (2049, 768), (7680, 1600), (10240, 1024)])
def test_ln_bwd_variants(op, variant, rows, D, ws):
    """each optional operand on its own, both operand types; row_map (cc_lmhead_ce_bwd's ln_f: the kept rows of a wider row set)
    with a row stride ldx > D"""
    code, t = _ln_case(op, rows, D, dcol=variant == "dcol", dres="dres" in variant, row_map="row_map" in variant, seed=rows + D + len(variant))
    assert _ln_call(code, t, rows, D, _poison(ws)) == 0
    _ln_verify(t, rows, D, "")


def test_ln_bwd_without_parameter_gradients_needs_no_scratch():
    code, t = _ln_case("bf16", 2049, 768, dcol=False, dres=True, row_map=False, seed=5)
    assert _ln_call(code, t, 2049, 768, None, with_dg=False) == 0
    torch.cuda.synchronize()
    assert torch.equal(t["dgamma"], t["dgamma0"]) and torch.equal(t["dbeta"], t["dbeta0"])
    assert torch.equal(t["dx16"], t["dx32"].to(t["dx16"].dtype))


# ------------------------------------------------------------------------------------------------------------------------------------
# column sums
# ------------------------------------------------------------------------------------------------------------------------------------
def _colsum_case(dt, M, N, ld, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    X = (torch.randn(M, ld, generator=g, device="cuda") + 0.5).to(dt)
    out0 = torch.randn(N, generator=g, device="cuda")
    return X, out0


CS_SHAPES = [(M, N) for N in (8, 72, 776, 768, 3072) for M in (1, 31, 255, 256, 257, 10240)] + [(70001, 8), (70001, 72)]


@pytest.mark.parametrize("op", ["bf16", "fp16"])
@pytest.mark.parametrize("M,N", CS_SHAPES)
def test_colsum(op, M, N, ws):
    code, dt = OPS[op]
    ld = N + 24
    X, out0 = _colsum_case(dt, M, N, ld, M * 13 + N)
    out = out0.clone()
    assert _lib().cc_colsum_bf16(code, _p(X), ld, M, N, _p(out), _p(_poison(ws)), _st()) == 0
    x = X[:, :N].double()
    _check("colsum", out, out0.double() + x.sum(0), out0.double().abs() + x.abs().sum(0), chain_colsum(M, N))


def test_colsum_shapes_reach_the_fold_paths():
    assert colsum_launch(256, 768)[0] == 1 and colsum_launch(257, 768)[0] == 2
    s, rps = colsum_launch(70001, 8)
    assert s > 256 and (s - 1) * rps < 70001 < s * rps          # two chunks of the fold, ragged last slice
    assert colsum_launch(10240, 3072)[0] == 20


@pytest.mark.parametrize("n", [1, 3, 8, 32])
@pytest.mark.parametrize("M,N", [(5120, 1536), (2049, 72), (70001, 8)])
def test_colsum_multi(n, M, N, ws):
    """n matrices with different data: an output routed to the wrong index, or one matrix's partials folded into another, fails"""
    ld = N + 8
    Xs, outs, out0s = [], [], []
    for i in range(n):
        X, out0 = _colsum_case(torch.bfloat16, M, N, ld, 1000 * i + M + N)
        Xs.append(X)
        out0s.append(out0)
        outs.append(out0.clone())
    xa = (C.c_void_p * n)(*[x.data_ptr() for x in Xs])
    oa = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
    assert _lib().cc_colsum_multi(0, xa, oa, n, ld, M, N, _p(_poison(ws)), _st()) == 0
    for i in range(n):
        x = Xs[i][:, :N].double()
        _check("colsum_multi", outs[i], out0s[i].double() + x.sum(0), out0s[i].double().abs() + x.abs().sum(0), chain_colsum(M, N, n))


@pytest.mark.parametrize("op", ["bf16", "fp16"])
@pytest.mark.parametrize("M,N", [(33, 8), (2049, 72), (70001, 8)])
def test_colsum_multi_of_one_is_the_single_form(op, M, N, ws):
    """cc_colsum_multi with n = 1 and cc_colsum_bf16 give the same bits (the single form is a batch of one: the same slices, partial rows
    and fold): one slice with ragged rows; several slices with the fold and a ragged column block; more than 256 slices (two chunks of
    the fold, ragged last slice).  Both outputs start from the same seeded non-zero values, so the += is part of what must agree."""
    code, dt = OPS[op]
    ld = N + 8
    X, out0 = _colsum_case(dt, M, N, ld, 77 * M + N)
    single, multi = out0.clone(), out0.clone()
    assert (out0 != 0).all()
    assert _lib().cc_colsum_bf16(code, _p(X), ld, M, N, _p(single), _p(_poison(ws)), _st()) == 0
    xa, oa = (C.c_void_p * 1)(X.data_ptr()), (C.c_void_p * 1)(multi.data_ptr())
    assert _lib().cc_colsum_multi(code, xa, oa, 1, ld, M, N, _p(_poison(ws)), _st()) == 0
    torch.cuda.synchronize()
    assert torch.equal(single.view(torch.int32), multi.view(torch.int32))
    assert (single != out0).all()


def test_colsum_multi_of_one_shapes_reach_the_paths():
    assert colsum_launch(33, 8) == (1, 64) and colsum_launch(2049, 72)[0] == 9 and colsum_launch(70001, 8)[0] > 256


def test_colsum_multi_shapes_fold():
    assert all(colsum_launch(M, N, n)[0] > 1 for n in (1, 3, 8, 32) for M, N in [(2049, 72), (70001, 8)])


def test_colsum_multi_rejects_more_than_32():
    X = torch.zeros(64, 8, dtype=torch.bfloat16, device="cuda")
    o = torch.ones(8, device="cuda")
    xa = (C.c_void_p * 33)(*([X.data_ptr()] * 33))
    oa = (C.c_void_p * 33)(*([o.data_ptr()] * 33))
    assert _lib().cc_colsum_multi(0, xa, oa, 33, 8, 64, 8, None, _st()) == -1
    torch.cuda.synchronize()
    assert (o == 1).all()


# ------------------------------------------------------------------------------------------------------------------------------------
# batch sums (prefix_const / pos_embeddings gradients: strided rows of the mapper's d x)
# ------------------------------------------------------------------------------------------------------------------------------------
BS_SHAPES = [(B, L) for B in (1, 8, 15, 16, 17, 256, 4096) for L in (4, 255, 7680, 262144) if B * L <= 256 * 262144]


@pytest.mark.parametrize("B,length", BS_SHAPES)
def test_batch_sum(B, length, ws):
    stride = length + 5
    g = torch.Generator(device="cuda").manual_seed(B * 31 + length)
    src = torch.randn(B * stride, generator=g, device="cuda") + 0.5
    dst0 = torch.randn(length, generator=g, device="cuda")
    dst = dst0.clone()
    assert _lib().cc_batch_sum(_p(src), stride, _p(dst), length, B, _p(_poison(ws)), _st()) == 0
    s = src.view(B, stride)[:, :length].double()
    _check("batch_sum", dst, dst0.double() + s.sum(0), dst0.double().abs() + s.abs().sum(0), chain_batch(B, length))


def test_batch_sum_shapes_reach_the_fold_paths():
    assert batch_launch(15, 4)[0] == 1 and batch_launch(16, 4) == (2, 8)
    s, per = batch_launch(17, 4)
    assert s == 2 and per * s > 17                                    # ragged last slice
    assert batch_launch(4096, 4)[0] > 256                             # two chunks of the fold
    s, per = batch_launch(4096, 7680)
    assert s > 1 and per * s > 4096


# ------------------------------------------------------------------------------------------------------------------------------------
# the scratch contract and bit determinism
# ------------------------------------------------------------------------------------------------------------------------------------
def test_scratch_size():
    assert _lib().cc_red_scratch_floats() == RED_FLOATS


def test_missing_scratch_is_an_error_and_writes_nothing():
    l = _lib()
    X, out0 = _colsum_case(torch.bfloat16, 10240, 768, 768, 1)
    out = out0.clone()
    assert l.cc_colsum_bf16(0, _p(X), 768, 10240, 768, _p(out), None, _st()) == -4
    outs = [out0.clone() for _ in range(3)]
    xa = (C.c_void_p * 3)(*([X.data_ptr()] * 3))
    oa = (C.c_void_p * 3)(*[o.data_ptr() for o in outs])
    assert l.cc_colsum_multi(0, xa, oa, 3, 768, 10240, 768, None, _st()) == -4
    src = torch.randn(256 * 7680, device="cuda")
    dst = out0.new_full((7680,), 2.0)
    assert l.cc_batch_sum(_p(src), 7680, _p(dst), 7680, 256, None, _st()) == -4
    code, t = _ln_case("bf16", 2049, 768, dcol=True, dres=True, row_map=False, seed=3)
    assert _ln_call(code, t, 2049, 768, None) == -4
    torch.cuda.synchronize()
    assert torch.equal(out, out0) and all(torch.equal(o, out0) for o in outs) and (dst == 2.0).all()
    assert torch.equal(t["dgamma"], t["dgamma0"]) and torch.equal(t["dbeta"], t["dbeta0"]) and torch.equal(t["dcol"], t["dcol0"])
    assert (t["dx32"] == 7.0).all() and (t["dx16"] == 3.0).all()


def test_single_slice_shapes_need_no_scratch():
    l = _lib()
    X, out0 = _colsum_case(torch.bfloat16, 256, 768, 768, 2)
    out = out0.clone()
    assert colsum_launch(256, 768)[0] == 1 and batch_launch(15, 7680)[0] == 1
    assert l.cc_colsum_bf16(0, _p(X), 768, 256, 768, _p(out), None, _st()) == 0
    src = torch.randn(15 * 7680, device="cuda") + 0.5
    dst0 = torch.randn(7680, device="cuda")
    dst = dst0.clone()
    assert l.cc_batch_sum(_p(src), 7680, _p(dst), 7680, 15, None, _st()) == 0
    x = X.double()
    _check("colsum", out, out0.double() + x.sum(0), out0.double().abs() + x.abs().sum(0), chain_colsum(256, 768))
    s = src.view(15, 7680).double()
    _check("batch_sum", dst, dst0.double() + s.sum(0), dst0.double().abs() + s.abs().sum(0), chain_batch(15, 7680))


def test_reductions_are_bit_deterministic(ws):
    l = _lib()

    def twice(fn):
        a, b = fn(), fn()
        torch.cuda.synchronize()
        for x, y in zip(a, b):
            assert torch.equal(x, y)

    X, out0 = _colsum_case(torch.bfloat16, 70001, 72, 72, 9)

    def colsum():
        out = out0.clone()
        assert l.cc_colsum_bf16(0, _p(X), 72, 70001, 72, _p(out), _p(_poison(ws)), _st()) == 0
        return (out,)

    def multi():
        outs = [out0.clone() for _ in range(8)]
        xa = (C.c_void_p * 8)(*([X.data_ptr()] * 8))
        oa = (C.c_void_p * 8)(*[o.data_ptr() for o in outs])
        assert l.cc_colsum_multi(0, xa, oa, 8, 72, 70001, 72, _p(_poison(ws)), _st()) == 0
        return outs

    src = torch.randn(4096 * 7680, device="cuda") + 0.5

    def bsum():
        dst = torch.ones(7680, device="cuda")
        assert l.cc_batch_sum(_p(src), 7680, _p(dst), 7680, 4096, _p(_poison(ws)), _st()) == 0
        return (dst,)

    code, t = _ln_case("bf16", 10240, 1600, dcol=True, dres=True, row_map=False, seed=4)

    def ln():
        for k in ("dgamma", "dbeta", "dcol"):
            t[k] = t[k + "0"].clone()
        assert _ln_call(code, t, 10240, 1600, _poison(ws)) == 0
        return (t["dgamma"].clone(), t["dbeta"].clone(), t["dcol"].clone(), t["dx32"].clone())

    for fn in (colsum, multi, bsum, ln):
        twice(fn)
