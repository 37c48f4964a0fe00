"""CPU tests of tests/decode_ref.py: the float64 reference agrees with a plain per-row softmax attention over the gathered history, the
mirror of the launch arithmetic puts every case on the kernel, union size and pass count it was written for, the case list reaches what
it claims to reach, and — the point of the bounds — every emulated defect leaves the bound around the correct float64 result by a factor
of at least 2 at every case of tests/test_gpu_decode_attention.py it applies to, in every operand build, while the correct kernel's
arithmetic carried out in fp32 stays inside it.  A bound that lets a defect through at some case says nothing there; the remedy is another
input for that case, never a smaller factor."""
import pytest
import torch

from tests import decode_ref as R

OPS = ("bf16", "fp16", "x3")


def test_reference_matches_plain_attention():
    """the gather + masked softmax against a loop over rows, heads and queries that spells the definition out"""
    for c in (R.Case(16, 6, 1, 9, 12, "beam", group=3, append=1), R.Case(24, 3, 4, 5, 9, "random", append=0), R.Case(8, 2, 3, 0, 3, "null", append=1)):
        S = R.stored(c, "x3")
        ref = R.reference(c, S)["out"]
        qkv = S["qkv"].double().view(c.R, c.Tn, 3, c.H, c.hd)
        kc, vc = S["kc"].double().view(c.R, c.ctx_max, c.H, c.hd), S["vc"].double().view(c.R, c.ctx_max, c.H, c.hd)
        for r in range(c.R):
            for h in range(c.H):
                for t in range(c.Tn):
                    ks, vs = [], []
                    for j in range(c.pos0 + t + 1):
                        if j < c.pos0:
                            src = r if S["rm"] is None else int(S["rm"][r, j])
                            ks.append(kc[src, j, h]), vs.append(vc[src, j, h])
                        else:
                            ks.append(qkv[r, j - c.pos0, 1, h]), vs.append(qkv[r, j - c.pos0, 2, h])
                    k, v = torch.stack(ks), torch.stack(vs)
                    a = torch.softmax(k @ qkv[r, t, 0, h] / c.hd ** 0.5, 0)
                    assert (a @ v - ref[r, t, h * c.hd:(h + 1) * c.hd]).abs().max() <= 1e-13, (c.id, r, h, t)


def test_stored_buffers_and_expected_cache():
    c = R.Case(16, 4, 3, 5, 10, "random", append=0)
    S = R.stored(c, "bf16")
    x = S["qkv"].view(c.R, c.Tn, 3, c.D)
    assert torch.equal(S["kc"][:, 5:8], x[:, :, 1]) and torch.equal(S["vc"][:, 5:8], x[:, :, 2])      # append = 0: the caller has stored them
    k, v = R.expected_cache(c, S)
    assert torch.equal(k, S["kc"]) and torch.equal(v, S["vc"])                                          # ... and the step writes nothing
    assert bool(S["named"][:, 5:8].all()) and not bool(S["named"][:, 8:].any())
    assert bool((S["rm"][:, 5:] == torch.arange(4).view(4, 1)).all())
    for r in range(c.R):
        for j in range(5):
            assert bool(S["named"][int(S["rm"][r, j]), j])
    c = R.Case(16, 4, 3, 5, 10, "random", append=1)
    S = R.stored(c, "fp16")
    x = S["qkv"].view(c.R, c.Tn, 3, c.D)
    assert not torch.equal(S["kc"][:, 5:8], x[:, :, 1]) and not bool(S["named"][:, 5:].any())
    k, v = R.expected_cache(c, S)
    assert torch.equal(k[:, 5:8], x[:, :, 1]) and torch.equal(v[:, 5:8], x[:, :, 2])
    k[:, 5:8], v[:, 5:8] = S["kc"][:, 5:8], S["vc"][:, 5:8]
    assert torch.equal(k, S["kc"]) and torch.equal(v, S["vc"])


def test_launch_arithmetic():
    """the formulas of decode.hip's decode_attn_plan: the LDS edges and the union list on hand-made inputs"""
    assert R.row_lds(1792, 64) == 64 * 1024 and R.row_lds(1793, 64) > 64 * 1024
    assert R.grp_shm(8, 175) <= 64 * 1024 < R.grp_shm(8, 176)
    assert R.path(16, 1, 64, 175, 8, 256) == 1 and R.path(16, 1, 64, 176, 8, 256) == 0
    assert R.path(16, 2, 64, 10, 8, 256) == 0 and R.path(16, 1, 128, 10, 8, 256) == 0 and R.path(18, 1, 64, 10, 9, 256) == 0 and R.path(4, 1, 64, 10, 1, 256) == 0
    assert R.grp_cap(5, 76) == 512 and R.grp_cap(2, 63) == 128 and R.grp_cap(2, 64) == 256
    # union of a hand-made table: G = 3, two positions; position 0 shared by all, position 1: beams 0 and 2 name row 2, beam 1 row 4
    rm = torch.tensor([[0, 2, 0], [0, 4, 1], [0, 2, 2]])
    assert R.union(rm, 3, 3, 2) == [[(0, 0, 0b111), (2, 1, 0b101), (4, 1, 0b010), (0, 2, 1), (1, 2, 2), (2, 2, 4)]]
    assert R.union(None, 2, 2, 1) == [[(0, 0, 1), (1, 0, 2), (0, 1, 1), (1, 1, 2)]]


def test_case_list_reaches_what_it_claims():
    rows, grp = R.row_cases(), R.group_cases()
    assert all(c.path == 0 for c in rows) and all(c.R <= 16 and c.H <= 2 for c in rows + grp)
    assert {c.hd for c in rows} == set(R.ROW_HD)
    for hd in R.ROW_HD:
        counts = set()
        for c in rows:
            if c.hd == hd:
                counts |= set(range(c.pos0 + 1, c.pos0 + c.Tn + 1))
                assert c.pos0 + c.Tn <= c.ctx_max
        assert {1, 2, 31, 32, 33, 63, 64, 65, 77, 127, 128, 129, 200} <= counts, hd
        mine = [c for c in rows if c.hd == hd]
        assert {c.append for c in mine} == {0, 1} and {"null", "random", "beam"} <= {c.table for c in mine}
        assert any(c.ctx_max == c.pos0 + c.Tn for c in mine) and any(c.ctx_max > c.pos0 + c.Tn for c in mine)
    a, b = R.lds_edge_cases()
    assert R.row_lds(a.ctx_max, a.hd) <= R.LDS_LIMIT < R.row_lds(b.ctx_max, b.hd)
    # the group form: every G at every pos0, every table kind, both append modes, the union sizes and the fallback edge
    assert {(c.group, c.pos0) for c in grp} >= {(g, p) for g in range(2, 9) for p in R.GROUP_POS}
    on = [c for c in grp if c.path == 1]
    assert {c.table for c in on} == set(R.GROUP_TABLES) and {c.append for c in on} == {0, 1}
    for g in range(2, 9):
        assert {c.append for c in on if c.group == g} == {0, 1}
    sizes, passes = set(), set()
    for c in on:
        nU = max(len(e) for e in R.union(c.row_map(), c.R, c.group, c.pos0))
        assert nU <= R.grp_cap(c.group, c.pos0)
        if c.want_nU is not None:
            assert nU == c.want_nU, (c.id, nU)
        sizes.add(nU)
        passes.add(-(-nU // R.PASS))
    assert {127, 128, 129, 130, 256, 257, 385} <= sizes and {1, 2, 3, 4} <= passes
    edge = {(c.pos0, c.path) for c in grp if c.group == 8 and c.pos0 >= 175}
    assert edge == {(175, 1), (176, 0)}
    # the union names exactly the keys the row tables name: beam b's entries are its ancestry
    for c in on[::5]:
        rm = c.row_map()
        for s, ent in enumerate(R.union(rm, c.R, c.group, c.pos0)):
            for b in range(c.group):
                r = s * c.group + b
                mine = sorted((j, row) for (row, j, bits) in ent if (bits >> b) & 1)
                assert mine == [(j, int(rm[r, j])) for j in range(c.pos0)] + [(c.pos0, r)], c.id


@pytest.mark.parametrize("op", OPS)
def test_every_defect_leaves_the_bound_and_fp32_stays_inside(op):
    fails, checked, worst32 = [], {d: 0 for d in R.DEFECTS}, 0.0
    for c in R.all_cases():
        S = R.stored(c, op)
        ref = R.reference(c, S)
        b = R.bounds(c, ref, op)
        emu = R.reference(c, S, dtype=torch.float32)["out"].to(R.DT[op]).double()
        r32 = ((emu - ref["out"]).abs() / b).max().item()
        worst32 = max(worst32, r32)
        if not r32 <= 1.0:
            fails.append(f"{c.id}: fp32 emulation of the correct kernel at {r32:.3f} of the bound")
        for d in R.DEFECTS:
            if not R.applicable(d, c, S):
                continue
            checked[d] += 1
            bad = R.reference(c, S, defect=d)["out"]
            ratio = ((bad - ref["out"]).abs() / b)
            ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio).max().item()      # a row left without keys
            if ratio < 2.0:
                fails.append(f"{c.id}: {d} at {ratio:.2f} of the bound")
    print(f"{op}: fp32 emulation worst err / bound {worst32:.3f}; defects checked {checked}")
    assert all(checked.values()), checked            # every defect met at least one case
    assert not fails, f"{len(fails)} failures: " + "; ".join(fails[:20])
