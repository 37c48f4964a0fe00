"""tests/sample_ref.py on the CPU: the fp32 emulation of the sampler's rule passes the check at every case, every emulated defect is rejected
at a named case, the case list decides what it claims to decide, and the float64 reference agrees with the oracle's restatements of the
reference project's own filters wherever those are not inside their fp32 rounding."""
import numpy as np
import pytest
import torch

from oracle import clipcap_oracle as oracle
from tests import sample_ref as R

KINDS = ("exact", "draw", "zero", "random", "length", "order")


@pytest.mark.parametrize("kind", KINDS)
def test_emulation_passes_every_case(kind):
    cases = [c for c in R.all_cases() if c.kind == kind]
    assert cases
    worst = 0.0
    for c in cases:
        tok, probs = R.emulate_case(c)
        w, exact = R.check_case(c, tok, probs)
        R.check_case(c, tok, None)                   # the token alone, as a call without probs_out is checked
        worst = max(worst, w)
        if kind in ("exact", "draw", "zero", "order"):
            assert exact == c.R, (c.name, exact)
    print(f"{kind}: {len(cases)} cases, worst err / bound of the fp32 emulation {worst:.3f}")


# defect -> the cases that must reject it (each on its own)
CAUGHT_BY = {
    "mode0_strict": ("exact-V4-p0.5-m0", "exact-V50257-p0.75-m0"),
    "mode1_not_strict": ("exact-V4-p0.5-m1", "exact-V4099-p0.25-m1"),
    "mode0_mass_of_topk": ("exact-V4099-k3-p0.5-m0", "singleton-V50257-m0"),
    "mode0_all_topk_ties": ("exact-V4-k3-m0", "exact-V50257-k3-m0"),
    "mode1_exactly_k": ("exact-V4-k3-m1", "singleton-V4099-m1"),
    "ties_reverse_index": ("exact-V4099-p0.5-m0", "exact-V64-k3-m0", "random-V1000-T0.7-k40-p0.5-m1-h0"),
    "topp_ties_all_kept": ("exact-V4-p0.5-m0", "singleton-V4099-m1", "random-V1000-T0.7-k40-p0.5-m0-h6"),
    "penalty_after_temperature": ("penalty-then-temperature-tie",),
    "duplicate_penalised_twice": ("penalty-then-temperature-tie", "random-V4099-T1.0-k0-p0.05-m0-h6", "random-V50257-T1.3-k0-p0.95-m0-h1500"),
    "draw_in_sorted_order": ("singleton-V64-m0", "random-V97-T1.0-k0-p0.8-m0-h0"),
    "u_not_clamped": ("draw-V4099-back-n8-clamp", "draw-V97-spread-n8-clamp"),
    "wave_prefix_dropped": ("exact-V4099-p0.5-m0", "exact-V50257-k3-m0", "draw-V50257-spread-n8-mid", "draw-V97-spread-n64-j56"),
    "ld_taken_as_V": ("exact-V64-p0.5-m0", "random-V50257-T1.0-k0-p0.8-m0-h0"),
    "negative_zero_below_zero": ("zero-V64-m0", "zero-V64-m1", "zero-V4099-m1"),
    "final_maximum_only_raised": ("length-shrink-deep-V97-m0", "length-shrink-deep-V4099-m1"),
}


def test_every_defect_is_named():
    assert set(CAUGHT_BY) == set(R.DEFECTS)


@pytest.mark.parametrize("defect,name", [(d, n) for d in R.DEFECTS for n in CAUGHT_BY[d]])
def test_defect_is_rejected(defect, name):
    c = R.by_name(name)
    tok, probs = R.emulate_case(c, defect)
    with pytest.raises(AssertionError):
        R.check_case(c, tok, probs)


def test_draw_defects_are_rejected_without_probabilities():
    """the token check alone (probs_out == NULL) tells a wrong draw"""
    for defect, name in (("draw_in_sorted_order", "singleton-V64-m0"), ("u_not_clamped", "draw-V4099-back-n8-clamp"),
                         ("wave_prefix_dropped", "draw-V50257-spread-n8-mid")):
        c = R.by_name(name)
        tok, _ = R.emulate_case(c, defect)
        with pytest.raises(AssertionError):
            R.check_case(c, tok, None)


def test_the_case_list_decides_what_it_claims():
    amb = tot = 0
    for c in R.all_cases():
        refs = c.refs()
        if c.kind == "random":
            for kind, ref in zip(R.ROW_KINDS, refs):
                if kind in ("grid", "equal"):
                    assert ref.exact, (c.name, kind, np.flatnonzero(ref.adm))
                if 0 < c.P.top_p < 1 and not ref.dead:
                    tot += 1
                    amb += not ref.exact
        if c.kind in ("exact", "draw", "zero", "order"):
            assert all(ref.exact for ref in refs), c.name
        if c.kind in ("exact", "draw") and not c.name.startswith("singleton") and not c.name.endswith("tiny-p"):
            assert all(ref.T is None or ref.d.max() == 0.0 for ref in refs), c.name          # delta = 0: nothing but exact weights
    print(f"random rows with 0 < top_p < 1 and more than one admissible prefix length: {amb} of {tot}")
    assert tot >= 200 and amb * 20 <= tot


def test_exact_rows_tell_the_two_comparisons_apart():
    """the issue's example: 4 equal tokens, top_p = 0.5: >= keeps two, > keeps three"""
    for mode, want in ((0, 2), (1, 3)):
        ref = R.by_name(f"exact-V4-p0.5-m{mode}").refs()[0]
        assert np.flatnonzero(ref.adm).tolist() == [want]
    ref = R.by_name("exact-V4099-tiny-p").refs()[0]                # the target truncates to 0: the first token and nothing else
    assert np.flatnonzero(ref.adm).tolist() == [1] and ref.T < 1.0
    c = R.by_name("zero-V64-m1")                                    # [3, 2, +0, -0, -1 ...], top_k = 3, every tie of the third value: four
    assert sorted(c.refs()[0].kept(c.refs()[0].K).tolist()) == [0, 1, 2, 3]
    c = R.by_name("zero-V64-m0")                                    # exactly three: the zero with the smaller index, whatever its sign
    assert [sorted(r.kept(r.K).tolist()) for r in c.refs()[::2]] == [[0, 1, 2], [0, 1, 2]]


def test_length_cases_move_the_maximum_as_they_say():
    """raise: the final maximum of every row lies above the row maximum; shrink: below it in at least one row of every case (the rows
    without stop-valued poison: every maximal kept token fires), in every row of the deep cases"""
    seen = {"raise": 0, "shrink": 0}
    for c in R.all_cases():
        if c.kind != "length":
            continue
        what = c.name.split("-")[1]
        below = []
        for ref in c.refs():
            n = int(np.flatnonzero(ref.adm)[0])
            ks = ref.final(n)["ks"]
            f = np.where(ref.bm & (ref.v == np.float32(c.P.stop_tok)), (ref.v * c.P.len_pen).astype(np.float32), ref.v)
            m2 = f[ks].max()
            if what == "raise":
                assert m2 > ref.m, c.name
            else:
                assert m2 <= ref.m, c.name
                below.append(bool(m2 < ref.m) and bool((f[ks & (ref.v == ref.m)] < ref.m).all()))
        if what == "shrink":
            assert all(below) if "deep" in c.name else sum(below) >= 3, (c.name, below)
        seen[what] += 1
    assert seen["raise"] >= 12 and seen["shrink"] >= 10


def test_token_alone_fits_any_admissible_length():
    """A call without probs_out on a row with two admissible lengths (a 0.25 grid, the cut within the bound of a group's member: found by
    tools/fuzz_decode_steps.py): whichever the kernel keeps, its draw passes; a draw for an inadmissible length of the same row does not."""
    V, rng = 14937, np.random.default_rng(1031491901)
    x = rng.standard_normal((7, V)) * 1.2603236464498255
    x = (np.round(x[1] * 4.0) / 4.0).astype(np.float32)
    ref = R.RowRef(x, R.Params(temperature=1.4, top_k=V + 5, top_p=0.477, mode=1), None, 0.6394355)
    lens = np.flatnonzero(ref.adm).tolist()
    assert lens == [2470, 2471]

    def draw(n):
        fin = ref.final(n)
        return int(np.searchsorted(fin["E"][1:], ref.uu * fin["E"][V], side="right"))
    toks = [draw(n) for n in lens]
    assert toks[0] != toks[1]
    for t in toks:
        R.check_row(ref, None, t)
    other = next(t for t in (draw(n) for n in range(2400, 2470)) if t not in toks)
    with pytest.raises(AssertionError):
        R.check_row(ref, None, other)


def test_lds_mirror():
    assert R.lds_bytes(50257) == 16384 + 144 + 8192 + 16 + 128 + 1571 * 4
    c = R.lds_edge()
    assert R.lds_bytes(c.V) == R.LDS_LIMIT and R.lds_bytes(c.V + 1) > R.LDS_LIMIT
    tok, probs = R.emulate_case(c)
    R.check_case(c, tok, probs)


def _oracle_row(c, r):
    """the oracle's distribution of row r of a case (torch fp32, as the reference project computes it), or None where it has no answer"""
    P = c.P
    x = torch.from_numpy(c.x[r].copy())
    T = P.temperature if P.temperature > 0 else 1.0
    hist = None
    if P.hist_len:
        h = c.hist[r, :P.hist_len]
        hist = torch.from_numpy(h[(h >= 0) & (h < c.V)].copy())           # the reference's gather has no answer for the others
    k = min(P.top_k, c.V) if P.top_k > 0 else 0
    if P.mode == 0:
        if P.stop_tok >= 0:
            return None
        if hist is not None and float(P.rep_pen) != 1.0:
            x = oracle.repetition_penalty_apply(x, hist.unique(), float(P.rep_pen))
        return oracle.nucleus_final_p((x / T).unsqueeze(0), top_p=float(P.top_p) if P.top_p > 0 else 1.0, top_k=k or None)[0]
    kw = {}
    if P.stop_tok >= 0:
        kw = dict(stop_token=P.stop_tok, desired_sentence_length=int(hist.numel()), sentence_length_factor=float(P.len_pen))
    return oracle.no_beam_step_distribution(x, hist, top_p=float(P.top_p), top_k=k, temperature=T, repetition_penalty=float(P.rep_pen), **kw)


def test_reference_agrees_with_the_oracle():
    """Rows whose cut is not inside a group of equal values and lies further than 1e-4 of the mass from top_p (the oracle's fp32 cumsum is
    good to ~2e-5), top_p < 1 (at 1 the oracle's cut is wherever its cumsum first rounds to 1): same kept set, probabilities to fp32."""
    compared = {0: 0, 1: 0}
    for c in R.all_cases():
        if c.kind not in ("random", "length") or float(c.P.top_p) >= 1.0 or (c.P.mode == 0 and not c.P.top_p > 0 and c.P.top_k <= 0):
            continue
        if "deep" in c.name:          # thousands of masses each below half an fp32 ulp of the leading one: the oracle's fp32 sum drops part of them
            continue
        for r, ref in enumerate(c.refs()):
            if ref.dead or not ref.exact:
                continue
            n, K, v, o = int(np.flatnonzero(ref.adm)[0]), ref.K, ref.v, ref.order
            if (n < c.V and v[o[n - 1]] == v[o[n]]) or (c.P.mode == 0 and K < c.V and v[o[K - 1]] == v[o[K]]):
                continue                                             # a cut inside equal values: the oracle's sort decides, not a rule
            if ref.T is not None and min(abs(ref.c[n] - ref.T), abs(ref.c[n - 1] - ref.T)) <= 1e-4 * R.S * np.exp(ref.v.astype(np.float64) - float(ref.m)).sum():
                continue
            want = _oracle_row(c, r)
            if want is None:
                continue
            fin = ref.final(n)
            want = want.double().numpy()
            big = fin["p"] > 1e-8                                    # the oracle's fp32 softmax leaves denormals below that
            assert np.array_equal((want > 0) & big, fin["ks"] & big), (c.name, r)
            assert not np.any(want[~fin["ks"]] > 1e-8), (c.name, r)
            assert np.abs(want - fin["p"]).max() <= 2e-6, (c.name, r, np.abs(want - fin["p"]).max())
            compared[c.P.mode] += 1
    print(f"rows compared with the oracle: mode 0 {compared[0]}, mode 1 {compared[1]}")
    assert compared[0] >= 40 and compared[1] >= 40
