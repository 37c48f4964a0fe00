"""cc_logits_guide (clipcap_amd/csrc/guide.hip) on the device, through the C ABI and engine.guide_logits, against the float64 statement and
the per-element bar of tests/guide_ref.py: every row kind at V in {4, 97, 1001, 4099, 50257} and g in {0, 0.5, 1, 1.5, 3, 7.5}, in three
layouts (ld = V + 13 with NaN padding: the scalar path except where V + 13 is a multiple of 4; ld = V rounded up to 64: 16-byte accesses;
a cond view with row stride 3 * ld), placement (out of place, in place, out == NULL), skip_rows, independence of a row from R, and the
exact cases.

Measured on an MI355X (`-s` prints them; the inputs and the kernel are deterministic, so the figures repeat): the worst |err| / bound
over the six scales and the sixteen row kinds is 0.174 at V = 4, 0.214 at V = 97, 0.338 at V = 1001, 0.135 at V = 4099 and 0.340 at
V = 50257 — and the same figure in all three layouts of a V: what a thread computes does not depend on how the bytes travel.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import guide_ref as G

pytestmark = pytest.mark.gpu

VS = [4, 97, 1001, 4099, 50257]
SCALES = [0.0, 0.5, 1.0, 1.5, 3.0, 7.5]
BATCH = 8                                      # rows per launch: the 16 row kinds go in two launches
SENTINEL = 7.0

_ROWS, _REF = {}, {}


def _rows(V):
    if V not in _ROWS:                         # computed once per V, shared, never modified
        _ROWS[V] = G.random_rows(V, 1000 + V)
    return _ROWS[V]


def _ref(V, g):
    if (V, g) not in _REF:
        _REF[(V, g)] = G.guide_ref(*_rows(V), g)
    return _REF[(V, g)]


def _padded(x, ld, fill=float("nan"), stride_rows=1):
    """fp32 device buffer (R * stride_rows, ld) filled with ``fill``; rows 0, stride_rows, ... hold x in their first V columns."""
    R, V = x.shape
    buf = torch.full((R * stride_rows, ld), fill, dtype=torch.float32)
    buf[::stride_rows, :V] = torch.from_numpy(x)
    return buf.cuda()


def _call(cond, ld_c, uncond, ld_u, R, V, g, out, ld_o, skip=None):
    from clipcap_amd import _lib
    rc = _lib.lib().cc_logits_guide(C.c_void_p(cond.data_ptr()), ld_c, C.c_void_p(uncond.data_ptr()), ld_u, R, V, g,
                                    C.c_void_p(out.data_ptr() if out is not None else 0), ld_o, C.c_void_p(skip.data_ptr() if skip is not None else 0),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def _bits(t):
    return t.contiguous().view(torch.int32)


def _vp(V):
    return (V + 63) // 64 * 64


@pytest.mark.parametrize("layout", ["padded", "aligned", "strided"])
@pytest.mark.parametrize("V", VS)
def test_matches_the_float64_statement_within_the_bar(V, layout):
    from clipcap_amd.engine import guide_logits
    c, u = _rows(V)
    ld = V + 13 if layout == "padded" else _vp(V)
    worst = 0.0
    for lo in range(0, len(G.ROW_KINDS), BATCH):
        cb, ub = c[lo:lo + BATCH], u[lo:lo + BATCH]
        R = cb.shape[0]
        cd = _padded(cb, ld, stride_rows=3 if layout == "strided" else 1)
        ud = _padded(ub, ld)
        c0, u0 = cd.clone(), ud.clone()
        for g in SCALES:
            out = torch.full((R, ld), float("nan"), device="cuda")
            if layout == "strided":                                  # through the engine, on views: cond rows 3 * ld apart
                assert cd[::3, :V].stride(0) == 3 * ld
                got = guide_logits(cd[::3, :V], ud[:, :V], g, out=out[:, :V])
                assert got.data_ptr() == out.data_ptr()
                torch.cuda.synchronize()
            else:
                assert _call(cd, ld, ud, ld, R, V, g, out, ld) == 0
            # out of place: the inputs, their padding included, are bit-unchanged; the padding of out is still NaN
            assert torch.equal(_bits(cd), _bits(c0)) and torch.equal(_bits(ud), _bits(u0))
            assert torch.isnan(out[:, V:]).all()
            ref, bound = _ref(V, g)
            ratio = G.worst_ratio(out[:, :V].cpu().numpy(), ref[lo:lo + BATCH], bound[lo:lo + BATCH])
            assert ratio <= 1.0, (V, layout, g, lo, ratio)
            worst = max(worst, ratio)
    print(f"guide V {V} ld {ld} {layout}: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("V", VS)
def test_in_place_and_null_out_equal_out_of_place_bit_for_bit(V):
    c, u = _rows(V)
    for ld in (V + 13, _vp(V)):
        for g in (0.5, 3.0):
            cd, ud = _padded(c[:BATCH], ld), _padded(u[:BATCH], ld)
            out = torch.full((BATCH, ld), float("nan"), device="cuda")
            assert _call(cd, ld, ud, ld, BATCH, V, g, out, ld) == 0
            inplace = cd.clone()
            assert _call(inplace, ld, ud, ld, BATCH, V, g, inplace, ld) == 0
            null = cd.clone()
            assert _call(null, ld, ud, ld, BATCH, V, g, None, 0) == 0                   # ld_o is ignored with out == NULL
            assert torch.equal(_bits(out[:, :V]), _bits(inplace[:, :V])) and torch.equal(_bits(inplace), _bits(null))
            assert torch.isnan(inplace[:, V:]).all()


@pytest.mark.parametrize("V", [97, 4099, 50257])
def test_skip_rows_and_independence_of_a_row_from_the_others(V):
    from clipcap_amd.engine import guide_logits
    c, u = _rows(V)
    g, ld = 1.5, _vp(V)
    cd, ud = _padded(c[:BATCH], ld), _padded(u[:BATCH], ld)
    full = torch.full((BATCH, ld), SENTINEL, device="cuda")
    assert _call(cd, ld, ud, ld, BATCH, V, g, full, ld) == 0
    skip = torch.tensor([0, 1, 0, 0, 1, 1, 0, 1], dtype=torch.uint8, device="cuda")
    part = torch.full((BATCH, ld), SENTINEL, device="cuda")
    assert _call(cd, ld, ud, ld, BATCH, V, g, part, ld, skip) == 0
    keep = ~skip.bool()
    assert (part[skip.bool()] == SENTINEL).all()                                           # skipped rows keep the sentinel
    assert torch.equal(_bits(part[keep]), _bits(full[keep]))                               # the others do not notice
    via_engine = guide_logits(cd[:, :V], ud[:, :V], g, out=torch.full((BATCH, ld), SENTINEL, device="cuda")[:, :V], skip_rows=skip)
    assert torch.equal(_bits(via_engine), _bits(part[:, :V]))
    for r in (0, 3, BATCH - 1):                                                            # the same row run alone (R = 1) and among 8
        alone = torch.full((1, ld), SENTINEL, device="cuda")
        assert _call(cd[r:r + 1], ld, ud[r:r + 1], ld, 1, V, g, alone, ld) == 0
        assert torch.equal(_bits(alone), _bits(full[r:r + 1])), r
    again = torch.full((BATCH, ld), SENTINEL, device="cuda")                               # and from run to run
    assert _call(cd, ld, ud, ld, BATCH, V, g, again, ld) == 0
    assert torch.equal(_bits(again), _bits(full))


@pytest.mark.parametrize("V", VS)
def test_exact_cases(V):
    """All-equal rows in both streams: -log(V) at every scale; g = 1 with any finite uncond: log_softmax(cond)."""
    ld = V + 13
    rng = np.random.default_rng(V)
    c = np.repeat(rng.standard_normal((BATCH, 1)).astype(np.float32) * 3, V, axis=1)
    u = np.repeat(rng.standard_normal((BATCH, 1)).astype(np.float32) * 3, V, axis=1)
    cd, ud = _padded(c, ld), _padded(u, ld)
    for g in SCALES:
        out = torch.full((BATCH, ld), float("nan"), device="cuda")
        assert _call(cd, ld, ud, ld, BATCH, V, g, out, ld) == 0
        _, bound = G.guide_ref(c, u, g)
        assert G.worst_ratio(out[:, :V].cpu().numpy(), np.full((BATCH, V), -np.log(V)), bound) <= 1.0, g
    c = (rng.standard_normal((BATCH, V)) * 3).astype(np.float32)
    u = (rng.standard_normal((BATCH, V)) * 20).astype(np.float32)
    cd, ud = _padded(c, ld), _padded(u, ld)
    out = torch.full((BATCH, ld), float("nan"), device="cuda")
    assert _call(cd, ld, ud, ld, BATCH, V, 1.0, out, ld) == 0
    want = torch.log_softmax(torch.from_numpy(c).double(), -1).numpy()
    assert G.worst_ratio(out[:, :V].cpu().numpy(), want, G.guide_ref(c, u, 1.0)[1]) <= 1.0


def test_engine_asserts_its_arguments():
    from clipcap_amd.engine import guide_logits
    a, b = torch.zeros(2, 8, device="cuda"), torch.zeros(2, 8, device="cuda")
    for bad in (lambda: guide_logits(a, b[:, :7], 1.5), lambda: guide_logits(a.double(), b, 1.5), lambda: guide_logits(a, b.t().contiguous().t(), 1.5),
                lambda: guide_logits(a, b, 1.5, out=torch.zeros(3, 8, device="cuda")), lambda: guide_logits(a, b.cpu(), 1.5)):
        with pytest.raises(AssertionError):
            bad()
    assert guide_logits(a, b, 1.5) is a                                                    # in place returns cond
