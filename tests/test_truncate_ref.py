"""tests/truncate_ref.py pinned on the CPU: the float64 statement of the truncation rules agrees with the four transformers warpers on the
decided rows; the fp32 emulation of the kernel's passes is accepted on every case; each emulated defect is rejected on at least one; the
case list stays inside its conditions (designed rows decided exactly, random rows with at most MAX_UNDECIDED undecided tokens and a typical
window of at most MAX_WINDOW cuts).  The GPU test (tests/test_gpu_truncate.py) walks the same cases with the same checks."""
import numpy as np
import pytest

from tests import truncate_ref as T


def test_case_list_covers_the_sizes_and_row_kinds():
    cases = T.all_cases()
    assert {c.V for c in cases if c.kind == "random"} == {4, 64, 97, 1000, 4099, 50257}
    assert all(c.R == len(T.SR.ROW_KINDS) for c in cases if c.kind == "random") and all(c.R <= 8 for c in cases)
    for rule in T.RULES:
        assert any(c.P.on[rule] and sum(c.P.on.values()) == 1 for c in cases), f"{rule} never runs alone"
    assert any(all(c.P.on.values()) for c in cases)


def test_conditions_hold_on_the_reference_alone():
    worst_u = worst_w = 0
    for c in T.all_cases():
        for r, ref in enumerate(c.refs()):
            if c.kind == "designed":
                assert ref.decided and ref.window == 1, f"{c.name} row {r}: {ref.n_undecided} undecided tokens, window {ref.window}"
            else:
                assert ref.n_undecided <= T.MAX_UNDECIDED and ref.window <= T.MAX_WINDOW, \
                    f"{c.name} row {r}: {ref.n_undecided} undecided tokens, window {ref.window}: salt the seed (truncate_ref.SALT)"
            worst_u, worst_w = max(worst_u, ref.n_undecided), max(worst_w, ref.window)
            if ref.decided and not ref.dead:                     # decided: the sure sets ARE the definition's kept set
                inter = ref.thr_keep & ref.typ_keep
                assert np.array_equal(ref.sure_in, inter), (c.name, r)
                assert ref.surely_empty == (not inter.any()) and np.array_equal(ref.kept, inter if inter.any() else ref.maxima)
    print(f"most undecided tokens in a row {worst_u}, widest typical window {worst_w}")


def test_designed_rows_keep_what_they_were_designed_to_keep():
    def kept_values(name, r=0):
        c = T.by_name(name)
        return sorted(set(np.round(c.x[r][c.refs()[r].kept].astype(float), 2)))
    for V in (97, 4099):
        c = T.by_name(f"designed-V{V}-tie-group-straddles-cut")
        assert all(int(ref.kept.sum()) == 6 for ref in c.refs()) and kept_values(c.name) == [1.0]
        assert kept_values(f"designed-V{V}-two-groups") == [1.0, 3.0]
        assert kept_values(f"designed-V{V}-typical-and-epsilon-disjoint") == [3.0]
        assert all(ref.surely_empty for ref in T.by_name(f"designed-V{V}-typical-and-epsilon-disjoint").refs())
        assert kept_values(f"designed-V{V}-eta") == [3.0] and kept_values(f"designed-V{V}-eta-small") == [1.0, 3.0]
        one = T.by_name(f"designed-V{V}-one-token")
        assert all(int(ref.kept.sum()) == 1 for ref in one.refs()) and kept_values(one.name) == [1.05]
    c = T.by_name("designed-penalty-crosses-min-p")
    assert np.flatnonzero(c.refs()[0].kept).tolist() == [7, 30] and np.flatnonzero(c.refs()[1].kept).tolist() == [18, 41]
    c = T.by_name("designed-penalty-then-temperature")
    assert np.flatnonzero(c.refs()[0].kept).tolist() == [20, 41] == np.flatnonzero(c.refs()[1].kept).tolist()


def test_emulation_passes_every_case():
    for c in T.all_cases():
        T.check_case(c, T.emulate_case(c))


@pytest.mark.parametrize("defect", T.DEFECTS)
def test_every_defect_is_caught(defect):
    caught = []
    for c in T.all_cases():
        try:
            T.check_case(c, T.emulate_case(c, defect))
        except AssertionError:
            caught.append(c.name)
    assert caught, f"{defect} passes every case"
    print(f"{defect}: caught on {len(caught)} of {len(T.all_cases())} cases, e.g. {caught[0]}")


def test_lds_edge_is_the_edge_and_decided():
    c = T.lds_edge()
    assert T.lds_bytes(c.V) <= T.LDS_LIMIT < T.lds_bytes(c.V + 1)
    assert c.refs()[0].decided and c.refs()[0].window == 1
    T.check_case(c, T.emulate_case(c))


def test_reference_agrees_with_the_transformers_warpers_on_decided_rows():
    """one rule on at a time: what the definition keeps is what the corresponding warper leaves finite, on float64 rows of the values v"""
    torch = pytest.importorskip("torch")
    try:
        from transformers.generation.logits_process import (EpsilonLogitsWarper, EtaLogitsWarper, MinPLogitsWarper, TypicalLogitsWarper)
    except Exception as e:                                       # noqa: BLE001
        pytest.skip(f"transformers' warpers are not importable here: {e}")
    make = dict(min_p=lambda a: MinPLogitsWarper(min_p=a), typical_p=lambda a: TypicalLogitsWarper(mass=a),
                epsilon_cutoff=lambda a: EpsilonLogitsWarper(epsilon=a), eta_cutoff=lambda a: EtaLogitsWarper(epsilon=a, device="cpu"))
    rows = 0
    for c in T.all_cases():
        if c.V > 4099 and c.kind == "random" and rows > 150:
            continue
        for rule in T.RULES:
            if not c.P.on[rule]:
                continue
            P1 = c.P.only(rule)
            a = float(dict(zip(T.RULES, P1.args()))[rule])
            if not 0.0 < a < 1.0:
                continue                                         # the warpers refuse the end points
            for r in range(c.R):
                ref = T.RowRef(c.x[r], P1, c.h(r))
                if ref.dead or not ref.decided or ref.fin.sum() < 2:
                    continue
                scores = torch.from_numpy(ref.v.astype(np.float64))[None]
                got = make[rule](a)(None, scores.clone())[0].numpy() > -np.inf
                assert np.array_equal(got, ref.kept), f"{c.name} row {r} {rule}={a}: {int((got != ref.kept).sum())} tokens differ"
                rows += 1
    assert rows >= 100
    print(f"{rows} decided rows agree with the transformers warpers")
