"""The reference statement of BLEU and ROUGE-L (tests/bleu_rouge_ref.py) against the values recorded from the reference project's own
scorers (tests/golden/bleu_rouge_ref.npz, tools/gen_metrics_golden.py) and against hand cases whose values follow from the definitions.
Integers match exactly; floats agree to 1e-12 relative: both sides are float64 with the same operations."""
import math

import numpy as np
import pytest

from tests import bleu_rouge_ref as ref
from tests.metrics_cases import golden_cases, lcs_fast

REL = 1e-12


def _close(a, b):
    return abs(a - b) <= REL * abs(b)


def test_recorded_cases_cover_what_they_should():
    cases = golden_cases()
    assert len(cases) == 24
    lengths = {len(w) for case in cases for c, refs in case["images"] for w in [c] + refs}
    assert 0 not in lengths and {1, 2, 3, 4, 5, 9, 17, 40, 63, 64, 65} <= lengths
    vocab = sorted({max(max(w) for c, refs in case["images"] for w in [c] + refs) + 1 for case in cases})
    assert vocab[0] == 2 and 3 <= vocab[1] <= 6 and 30 <= vocab[-1] <= 40
    assert {len(refs) for case in cases for _, refs in case["images"]} == {1, 2, 3, 4, 5}


def test_statement_matches_every_recorded_value():
    n = 0
    for case in golden_cases():
        counts = []
        for (cand, refs), want, bleu, rouge in zip(case["images"], case["counts"], case["bleu"], case["rouge"]):
            got = ref.bleu_counts(cand, refs)
            assert got == want, (cand, refs)
            for a, b in zip(ref.bleu_from_counts(got), bleu):
                assert _close(a, b), (cand, refs, a, b)
            r = ref.rouge_l(cand, refs)
            assert _close(r, rouge) and (rouge != 0.0 or r == 0.0), (cand, refs, r, rouge)
            counts.append(got)
            n += 1
        for a, b in zip(ref.bleu_corpus(counts), case["case_bleu"]):
            assert _close(a, b)
        assert _close(sum(ref.rouge_l(c, r) for c, r in case["images"]) / len(case["images"]), case["case_rouge"])
    assert n == 128


def test_empty_candidate_and_empty_reference():
    assert ref.bleu_counts([], [[1, 2], [3]]) == [0, 1, 0, 0, 0, 0, 0, 0, 0, 0]
    assert ref.bleu_from_counts(ref.bleu_counts([], [[1, 2], [3]])) == [0.0] * 4          # exp(1 - 1e15 (1 + 1e-9)) underflows to 0
    assert ref.rouge_l([], [[1, 2]]) == 0.0
    assert ref.bleu_counts([1, 2], [[]]) == [2, 0, 2, 1, 0, 0, 0, 0, 0, 0]
    assert ref.rouge_l([1, 2], [[]]) == 0.0
    assert ref.rouge_l([1, 2], [[], [2]]) == ref.rouge_l([1, 2], [[2]]) > 0.0                # an empty reference adds 0 to both maxima
    assert ref.bleu_counts([], [[]]) == [0] * 10 and ref.bleu_from_counts([0] * 10) == [0.0] * 4


@pytest.mark.parametrize("L", [1, 2, 3])
def test_short_candidates_have_no_long_ngrams(L):
    cand = [5, 6, 7][:L]
    counts = ref.bleu_counts(cand, [[5, 6, 7]])
    assert counts[:2] == [L, 3] and counts[2:6] == [max(0, L - n) for n in range(4)] and counts[6:] == counts[2:6]
    bleu = ref.bleu_from_counts(counts)
    bp = math.exp(1 - 1 / ((L + 1e-15) / (3 + 1e-9)))                                      # (L = 3: the ratio is still just below 1)
    p = 1.0
    for n in range(4):
        p *= (counts[6 + n] + 1e-15) / (counts[2 + n] + 1e-9)                               # guess = 0: the factor is 1e-15 / 1e-9 = 1e-6
        assert _close(bleu[n], p ** (1.0 / (n + 1)) * bp)
    assert bleu[L - 1] > 0.99 * bp and bleu[3] < 0.04                                   # (1e-6) ** (1 / 4) at most


def test_clipping_and_the_maximum_over_references():
    a, b, c = 1, 2, 3
    assert ref.bleu_counts([a, a, a, a], [[a, a], [a, b, a]])[6:] == [2, 1, 0, 0]            # unigram a: min(4, max(2, 2)) = 2; (a, a): min(3, 1)
    # the maximum is taken per n-gram, over different references: a from the first (3), b from the second (2)
    assert ref.bleu_counts([a, a, a, b, b, b], [[a, a, a, c], [b, b, c, c]])[6:] == [5, 3, 1, 0]


def test_reflen_tie_goes_to_the_shorter_reference():
    assert ref.bleu_counts([1, 2, 3, 4], [[1] * 6, [1] * 2])[1] == 2
    assert ref.bleu_counts([1, 2, 3, 4], [[1] * 2, [1] * 6])[1] == 2
    assert ref.bleu_counts([1, 2, 3, 4], [[1] * 7, [1] * 2, [1] * 5])[1] == 5
    assert ref.bleu_counts([1, 2, 3, 4], [[1] * 7, [1] * 4, [1] * 3])[1] == 4


def test_precision_and_recall_from_different_references():
    cand = [1, 2, 3, 4]
    # reference 0: lcs 4 of 8 words (P = 1, R = 1/2); reference 1: lcs 2 of 2 words (P = 1/2, R = 1)
    refs = [[1, 9, 2, 9, 3, 9, 4, 9], [1, 2]]
    assert ref.lcs(cand, refs[0]) == 4 and ref.lcs(cand, refs[1]) == 2
    b2 = 1.2 ** 2
    assert _close(ref.rouge_l(cand, refs), (1 + b2) * 1.0 * 1.0 / (1.0 + b2 * 1.0)) and _close(ref.rouge_l(cand, refs), 1.0)
    assert _close(ref.rouge_l(cand, refs[:1]), (1 + b2) * 0.5 / (0.5 + b2))
    assert ref.rouge_l(cand, [[7, 8]]) == 0.0


def test_lcs_is_the_textbook_one():
    assert ref.lcs([1, 2, 3, 2, 4, 1, 2], [2, 4, 3, 1, 2, 1]) == 4
    assert ref.lcs([1] * 5, [1] * 3) == 3 and ref.lcs([1, 2, 3], [4, 5]) == 0 and ref.lcs([], [1]) == 0


def test_the_row_at_once_dp_of_the_device_tests_is_the_plain_dp():
    rng = np.random.default_rng(11)
    for case in golden_cases()[::3]:
        for cand, refs in case["images"]:
            for r in refs:
                assert lcs_fast(cand, r) == ref.lcs(cand, r) == ref.lcs(r, cand)
    for V in (1, 2, 3):
        for _ in range(20):
            a, b = rng.integers(0, V, int(rng.integers(0, 70))).tolist(), rng.integers(0, V, int(rng.integers(0, 70))).tolist()
            assert lcs_fast(a, b) == ref.lcs(a, b)
