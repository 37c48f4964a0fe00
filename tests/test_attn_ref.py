"""CPU tests of tests/attn_ref.py: the float64 reference agrees with torch.autograd, the input families have the properties they are named
for, the legality edges of the LDS-tile backward are where the kernels' formula puts them, and — the point of the bounds — every emulated
defect leaves the bound around the correct float64 result at every case of tests/test_gpu_attention_ref.py it applies to, in every operand
build.  A bound that lets a defect through at some case says nothing there; the remedy is another input or p for that case, never a
narrower claim."""
import pytest
import torch

from tests import attn_ref as R

OPS = ("bf16", "fp16", "x3")
FWD_DEFECTS = ("mask_transposed", "mask_no_bh", "causal_off_by_one", "ragged_keys", "no_rescale")
BWD_DEFECTS = ("mask_transposed", "mask_no_bh", "dv_no_scale", "delta_no_mask", "causal_off_by_one")


def _keep(c, seed=0):
    """any fixed mask serves the CPU test (the GPU test reads the library's)"""
    if not c.p:
        return None
    g = torch.Generator().manual_seed(c.seed % (2 ** 31) + c.layer + seed)
    return (torch.rand(c.B, c.H, c.S, c.S, generator=g) >= c.p).to(torch.uint8)


def _stored(x, op):
    return x.to(R.DT[op])


@pytest.mark.parametrize("causal,p", [(0, 0.0), (1, 0.0), (1, 0.3)])
def test_reference_matches_autograd(causal, p):
    B, S, H, hd = 2, 37, 3, 16
    qkv, dout = R.make_inputs("flat", B, S, H, hd, 5)
    q, k, v = (t.clone().requires_grad_(True) for t in R.heads(qkv, B, S, H, hd))
    do = R.rows(dout, B, S, H, hd)
    keep = (torch.rand(B, H, S, S, generator=torch.Generator().manual_seed(1)) >= p).to(torch.uint8) if p else None
    ref = R.reference(q.detach(), k.detach(), v.detach(), do, causal, keep, p)
    s = q @ k.transpose(-1, -2) * hd ** -0.5
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(S, S, dtype=torch.bool), 1), float("-inf"))
    a = s.softmax(-1)
    if p:
        a = a * keep.double() * R.keep_scale(p)
    out = a @ v
    out.backward(do)
    assert (ref["lse"] - torch.logsumexp(s, -1)).abs().max() <= 1e-12
    for name, got, want in (("out", ref["out"], out.detach()), ("dq", ref["dq"], q.grad), ("dk", ref["dk"], k.grad), ("dv", ref["dv"], v.grad)):
        assert (got - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item()), name
    assert (ref["delta"].squeeze(-1) - (do * out.detach()).sum(-1)).abs().max() <= 1e-12      # rowsum(A dA) == rowsum(dO out)


def test_lds_edges_are_the_kernels():
    """attn_bwd_lds against 160 KiB: S = 88 is the last legal length at head dim 64, S = 60 at head dim 128"""
    assert R.bwd_lds_edge(64) == 88 and R.bwd_lds_edge(128) == 60
    assert R.paths("x3", 88, 64)[1][0] == "k_attn_bwd" and R.paths("x3", 89, 64)[1][0] == "k_attn_bwd_rows"
    assert R.paths("bf16", 33, 128)[1][0] == "k_attn_bwd_dq+dkv" and R.paths("bf16", 64, 96)[1][0] == "k_attn_bwd_fused<2>"


def test_input_families():
    B, S, H, hd = 2, 200, 2, 64
    for op in OPS:
        qkv, _ = R.make_inputs("rising", B, S, H, hd, 3)
        q, k, _ = R.heads(_stored(qkv, op), B, S, H, hd)
        s = q @ k.transpose(-1, -2) * hd ** -0.5
        bm = torch.nn.functional.pad(s, (0, -S % 32), value=float("-inf")).view(B, H, S, -1, 32).max(-1).values
        assert (bm[..., 1:] > bm[..., :-1] + 1.0).all()          # every block lifts every row's maximum; the last (ragged) block holds it
        qkv, _ = R.make_inputs("offset", B, S, H, hd, 3)
        st = _stored(qkv, op).float().view(B, S, 3, H, hd)
        assert (st[:, :, 0, :, 0] == 40).all() and (st[:, :, 1, :, 0] == 20).all()
    # the offset moves no output of the forward: same out with coordinate 0 of k zeroed
    qkv, dout = R.make_inputs("offset", 2, 40, 2, 64, 3)
    q, k, v = R.heads(qkv, 2, 40, 2, 64)
    do = R.rows(dout, 2, 40, 2, 64)
    k0 = k.clone()
    k0[..., 0] = 0
    a, b = R.reference(q, k, v, do, 1), R.reference(q, k0, v, do, 1)
    assert (a["out"] - b["out"]).abs().max() <= 1e-12 and (a["lse"] - b["lse"] - 100.0).abs().max() <= 1e-10


def _cases(op):
    return R.plain_cases() + R.dropout_cases(op)


@pytest.mark.parametrize("op", OPS)
def test_every_defect_leaves_the_bound(op):
    fails, checked = [], {d: 0 for d in R.DEFECTS}
    for c in _cases(op):
        (_, ffam), (bname, bfam) = R.paths(op, c.S, c.hd, c.mfma_bwd)
        todo = [d for d in R.DEFECTS if R.applicable(d, c.causal, c.p, c.S, c.B, c.H, ffam, c.bwd, c.family)]
        if not todo:
            continue
        qkv, dout = c.inputs()
        q, k, v = R.heads(_stored(qkv, op), c.B, c.S, c.H, c.hd)
        do = R.rows(_stored(dout, op), c.B, c.S, c.H, c.hd)
        keep = _keep(c)
        ref = R.reference(q, k, v, do, c.causal, keep, c.p)
        bf = R.fwd_bounds(ref, op, ffam)
        bb = R.bwd_bounds(ref, op, bfam, "fused" in bname or "dq+dkv" in bname or "rows" in bname, ref["lse"].float(),
                          _stored(ref["out"].float(), op)) if c.bwd else {}
        for d in todo:
            bad = R.reference(q, k, v, do, c.causal, keep, c.p, defect=d)
            if d == "mask_no_bh" and torch.equal(keep[:1, :1].expand_as(keep), keep):
                continue
            checked[d] += 1
            if d in FWD_DEFECTS and not any(((bad[x] - ref[x]).abs() > bf[x]).any() for x in ("out", "lse")):
                fails.append(f"{c.id}: forward {d}")
            if c.bwd and d in BWD_DEFECTS and not any(((bad[x] - ref[x]).abs() > bb[x]).any() for x in ("dq", "dk", "dv")):
                fails.append(f"{c.id}: backward {d}")
    assert all(checked.values()), checked            # every defect met at least one case
    assert not fails, f"{len(fails)} defects inside the bound: " + "; ".join(fails[:20])
