"""tests/guide_ref.py on the CPU: the float64 statement of classifier-free guidance is what it claims to be (g = 1 and g = 0, the
product-of-experts form, the -inf rules), the bar accepts an honest fp32 computation of the rule and rejects every named defect, and the
guided CPU beam search reduces to the oracle's beam search at g = 1 and finds the captions the end-to-end GPU tests compare with."""
import numpy as np
import pytest
import torch

from tests import guide_ref as G
from tests.util import load_golden, sd_of

V, LD, R = 97, 110, len(G.ROW_KINDS)
SCALES = (0.0, 0.5, 1.0, 1.5, 3.0, 7.5)


def _rows():
    return G.random_rows(V, 11)


def test_scale_one_and_zero_are_the_log_softmax_of_one_stream():
    c, u = _rows()
    live = np.isfinite(c) & np.isfinite(u)
    for g, x in ((1.0, c), (0.0, u)):
        out, _ = G.guide_ref(c, u, g)
        want = torch.log_softmax(torch.from_numpy(x).double(), -1).numpy()
        assert np.abs(out[live] - want[live]).max() <= 1e-12
        assert np.isneginf(out[~live]).all()


@pytest.mark.parametrize("g", SCALES)
def test_exp_of_the_result_renormalised_is_the_product_of_experts(g):
    """softmax(out) = p_c^g p_u^(1-g) / Z on the support both streams share."""
    c, u = _rows()
    out, _ = G.guide_ref(c, u, g)
    for r, kind in enumerate(G.ROW_KINDS):
        live = np.isfinite(c[r]) & np.isfinite(u[r])
        if not live.any():
            assert np.isneginf(out[r]).all(), kind
            continue
        lpc = torch.log_softmax(torch.from_numpy(c[r]).double(), -1).numpy()[live]        # log p: an element at -1e4 has p = 0 in float64
        lpu = torch.log_softmax(torch.from_numpy(u[r]).double(), -1).numpy()[live]
        lpoe = g * lpc + (1 - g) * lpu
        poe = np.exp(lpoe - lpoe.max())
        got = np.exp(out[r][live] - G.lse64(out[r][live]))
        assert np.allclose(got, poe / poe.sum(), rtol=1e-9, atol=1e-300), kind


def test_minus_inf_rules():
    c, u = _rows()
    for g in SCALES:
        out, bound = G.guide_ref(c, u, g)
        assert not np.isnan(out).any() and not np.isposinf(out).any()
        assert np.array_equal(np.isneginf(out), np.isneginf(c) | np.isneginf(u))             # banned in either stream: banned; nothing else is
        for kind in ("dead_cond", "dead_uncond", "dead_both"):
            assert np.isneginf(out[G.ROW_KINDS.index(kind)]).all()
        assert (bound[np.isfinite(out)] > 0).all() and (bound[np.isneginf(out)] == 0).all()
    k = G.ROW_KINDS.index("one_left_cond")                                                 # one finite element: lse_c is that element
    i = int(np.flatnonzero(np.isfinite(c[k]))[0])
    out, _ = G.guide_ref(c, u, 3.0)
    assert abs(out[k, i] - (1 - 3.0) * (u[k, i] - G.lse64(u[k]))) <= 1e-12
    assert G.worst_ratio(np.full((1, 3), -np.inf), np.full((1, 3), -np.inf), np.zeros((1, 3))) == 0.0
    assert G.worst_ratio(np.array([[0.0, np.nan]]), np.array([[0.0, 1.0]]), np.ones((1, 2))) == float("inf")
    assert G.worst_ratio(np.array([[0.0, -np.inf]]), np.array([[0.0, 1.0]]), np.ones((1, 2))) == float("inf")
    assert G.worst_ratio(np.array([[0.0, 1.0]]), np.array([[0.0, -np.inf]]), np.ones((1, 2))) == float("inf")


def _flat(x, ld, fill):
    buf = np.full(x.shape[0] * ld, fill, dtype=np.float32)
    for r in range(x.shape[0]):
        buf[r * ld:r * ld + x.shape[1]] = x[r]
    return buf


def _emulated(g, defect=None, skip=None):
    c, u = _rows()
    out = np.full(R * LD, 7.0, dtype=np.float32)                                           # 7: the sentinel of rows and columns not written
    G.emulate(_flat(c, LD, 100.0), LD, _flat(u, LD, -100.0), LD, R, V, g, out, LD, skip, defect)
    return out.reshape(R, LD)


def _ratio(got, g, skip=None):
    c, u = _rows()
    ref, bound = G.guide_ref(c, u, g)
    rows = [r for r in range(R) if skip is None or not skip[r]]
    ok = (got[:, V:] == 7.0).all() and all((got[r, :V] == 7.0).all() for r in range(R) if r not in rows)
    return G.worst_ratio(got[rows, :V], ref[rows], bound[rows]) if ok else float("inf")


@pytest.mark.parametrize("g", SCALES)
def test_the_bar_accepts_an_honest_fp32_computation(g):
    skip = np.zeros(R, dtype=np.uint8)
    skip[[1, 6]] = 1
    assert _ratio(_emulated(g), g) <= 1.0
    assert _ratio(_emulated(g, skip=skip), g, skip) <= 1.0


@pytest.mark.parametrize("defect", G.DEFECTS)
def test_the_bar_rejects_every_named_defect(defect):
    skip = np.zeros(R, dtype=np.uint8)
    skip[[1, 6]] = 1
    g = 1.5
    assert _ratio(_emulated(g, defect, skip), g, skip) > 1.0, defect
    if defect == "inf_uncond":                                                             # +inf at g > 1, nan at g = 1 (0 * -inf)
        k = G.ROW_KINDS.index("ban_uncond")
        assert np.isposinf(_emulated(1.5, defect)[k, :V]).any() and np.isnan(_emulated(1.0, defect)[k, :V]).any()
        assert _ratio(_emulated(1.0, defect), 1.0) == float("inf")


# ---- the guided CPU beam search -----------------------------------------------------------------------------------------------------------
STOP, ENTRY = 50, 10
# (scale, beam, case) -> (guided tokens of the best beam, unguided tokens, the margin recorded when the cases were chosen)
CASES = {(3.0, 3, "1"): ([40, 1, 1, 1, 50], [29, 29, 29, 29, 50], 3.4e-2), (3.0, 3, "3"): ([12, 12, 12, 12, 50], [7, 7, 7, 7, 50], 2.9e-2),
         (3.0, 1, "1"): ([40, 1, 1, 1, 50], [40, 40, 40, 40, 50], 1.6e-1), (1.5, 1, "T"): ([29, 29, 29, 29, 50], [50], 5.0e-1)}


def _tiny(case):
    g = load_golden("beam_tiny")
    D, n_layer, n_head, V_, npos = [int(v) for v in g["cfg"]]
    sd = {"language_model." + k: v for k, v in sd_of(g).items()}
    return sd, torch.from_numpy(g[f"beam{case}.prefix"]), dict(n_head=n_head, n_layer=n_layer)


def _best(res):
    toks, scores, lens = res
    b = int(scores.argmax())
    return toks[b, :int(lens[b])].tolist()


@pytest.mark.parametrize("key", sorted(CASES), ids=lambda k: f"g{k[0]}-beam{k[1]}-case{k[2]}")
def test_guided_cpu_search_finds_the_recorded_captions(key):
    scale, beam, case = key
    guided, unguided, margin = CASES[key]
    sd, pref, dims = _tiny(case)
    neg = sd["language_model.transformer.wte.weight"][50].view(1, 1, -1)
    res, m = G.guided_beam_search_ref(sd, pref, neg, scale=scale, beam=beam, entry_length=ENTRY, stop_token=STOP, **dims)
    assert _best(res[0]) == guided
    assert m >= (abs(scale) + abs(1 - scale)) * 2e-3 and abs(m - margin) <= 0.05 * margin + 5e-3, m
    res1, _ = G.guided_beam_search_ref(sd, pref, neg, scale=1.0, beam=beam, entry_length=ENTRY, stop_token=STOP, **dims)
    assert _best(res1[0]) == unguided and unguided != guided


def test_scale_one_is_the_oracle_beam_search():
    from oracle import clipcap_oracle as O
    sd, pref, dims = _tiny("1")
    neg = sd["language_model.transformer.wte.weight"][50].view(1, 1, -1)
    res, _ = G.guided_beam_search_ref(sd, pref, neg, scale=1.0, beam=3, entry_length=ENTRY, stop_token=STOP, rounds=2, **dims)
    want = O.generate_beam_tokens(sd, pref, beam_size=3, entry_length=ENTRY, stop_token=STOP, rounds=2, **dims)
    for (t, s, n), (wt, ws, wn, _) in zip(res, want):
        assert torch.equal(t, wt) and torch.equal(n.float(), wn.float()) and (s - ws.double()).abs().max() <= 1e-5
