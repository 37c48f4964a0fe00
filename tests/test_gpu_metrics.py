"""Device tests of BLEU and ROUGE-L: cc_bleu_stats and cc_rouge_l through the C ABI against tests/bleu_rouge_ref.py (float64, dicts and
a plain DP), on the cases recorded from the reference project's scorers and on crafted borders; repeatability; nothing written outside
the outputs; clipcap_amd.eval end to end against the recorded corpus numbers; self_critical_step with MetricReward as its reward.

Integers (the ten BLEU counts, every LCS length) are compared for equality.  Floats: |dev - ref| <= 2^-23 |ref| + 2^-126, and exactly 0
where the reference is exactly 0.  The device computes every sentence BLEU and ROUGE-L score in fp64 from exact integers and rounds it
once to fp32: 2^-24 relative for the rounding, doubled for the fp64 pow / exp (a few fp64 ulps, far below fp32's).  The absolute floor is
fp32's smallest normal: a one-word candidate against a 256-word reference has a brevity penalty of exp(-255), which fp32 cannot hold.
The kernel is given beta as fp32; the statement is evaluated with that fp32 value widened, as the kernel widens it.  Against the numbers
RECORDED with beta = 1.2 in float64 (the end-to-end test) the fp32 beta moves a score by at most
|d ln score / d ln beta^2| * 2 |1.2f / 1.2 - 1| <= 0.59 * 7.95e-8 = 4.7e-8 relative (the derivative is b / (1 + b) - b P / (R + b P),
b = 1.44, P, R in (0, 1]), which with the one rounding (6.0e-8) stays inside 2^-23 = 1.19e-7."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import bleu_rouge_ref as ref
from tests import cider_ref
from tests.cider_cases import pad_refs, pad_rows
from tests.metrics_cases import golden_cases, lcs_fast

pytestmark = pytest.mark.gpu
REL, FLOOR = 2.0 ** -23, 2.0 ** -126
BETA32 = float(np.float32(ref.BETA))
WORST = {"bleu": 0.0, "rouge": 0.0}


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _dev(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


def _launch(kind, cand, cand_len, refs, *, stop=-1, count_stop=0, group=None, ref_count=None, n=None, main=None, extra="alloc"):
    """cc_bleu_stats (main = stats, extra = bleu) or cc_rouge_l (main = out, extra = lcs) on numpy inputs; extra=None passes NULL"""
    from clipcap_amd import _lib
    dc, dr, dg, dn = _dev(cand, np.int64), _dev(refs, np.int32), _dev(group, np.int32), _dev(ref_count, np.int32)
    n = cand.shape[0] if n is None else n
    G, Rmax, Lr = refs.shape
    if kind == "bleu":
        main = torch.full((n, 10), -7, dtype=torch.int32, device="cuda") if main is None else main
        extra = torch.full((n, 4), float("nan"), device="cuda") if isinstance(extra, str) else extra
        rc = _lib.lib().cc_bleu_stats(_ptr(dc), n, cand_len, cand.shape[1], stop, count_stop, _ptr(dg), _ptr(dr), G, Rmax, Lr, _ptr(dn),
                                      _ptr(main), _ptr(extra), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    else:
        main = torch.full((n,), float("nan"), device="cuda") if main is None else main
        extra = torch.full((n, Rmax), -7, dtype=torch.int32, device="cuda") if isinstance(extra, str) else extra
        rc = _lib.lib().cc_rouge_l(_ptr(dc), n, cand_len, cand.shape[1], stop, count_stop, _ptr(dg), _ptr(dr), G, Rmax, Lr, _ptr(dn),
                                   BETA32, _ptr(extra), _ptr(main), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return main, extra


def _words(cand, cand_len, refs, *, stop=-1, count_stop=0, group=None, ref_count=None, **_):
    """per candidate row: (its words, its references' words) as the kernels cut them; None for a group outside [0, G)"""
    G, Rmax, _ = refs.shape
    out = []
    for c, row in enumerate(cand):
        g = c % G if group is None else int(group[c])
        if not 0 <= g < G:
            out.append(None)
            continue
        R = Rmax if ref_count is None else min(max(int(ref_count[g]), 1), Rmax)
        out.append((cider_ref.cut(row[:cand_len], stop if stop >= 0 else None, bool(count_stop)), [cider_ref.cut(r) for r in refs[g][:R]]))
    return out


def _floats_ok(dev, want, what, key):
    worst = 0.0
    for i, (d, w) in enumerate(zip(dev, want)):
        if w == 0.0:
            assert d == 0.0, (what, i, d)
        else:
            assert abs(d - w) <= REL * abs(w) + FLOOR, (what, i, d, w, abs(d - w) / abs(w))
            if abs(w) > 2.0 ** -100:
                worst = max(worst, abs(d - w) / abs(w))
    WORST[key] = max(WORST[key], worst)
    print(f"{what}: {len(want)} {key} floats, {sum(w == 0.0 for w in want)} exactly 0; largest |dev - ref| / |ref| = {worst:.3e} "
          f"(bound {REL:.3e}; largest so far {WORST[key]:.3e})")


def _check_bleu(cand, cand_len, refs, what, **kw):
    stats, bleu = _launch("bleu", cand, cand_len, refs, **kw)
    items = _words(cand, cand_len, refs, **kw)
    want = [[0] * 10 if it is None else ref.bleu_counts(*it) for it in items]
    got = stats.cpu().tolist()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (what, i, g, w, items[i])
    want_f = [v for it, w in zip(items, want) for v in ([0.0] * 4 if it is None else ref.bleu_from_counts(w))]
    _floats_ok(bleu.double().cpu().reshape(-1).tolist(), want_f, what, "bleu")
    return stats, bleu, want


def _check_rouge(cand, cand_len, refs, what, lcs_of=lcs_fast, **kw):
    out, lcs = _launch("rouge", cand, cand_len, refs, **kw)
    items = _words(cand, cand_len, refs, **kw)
    Rmax = refs.shape[1]
    got, want_f = lcs.cpu().tolist(), []
    for i, it in enumerate(items):
        if it is None:
            assert got[i] == [-1] * Rmax, (what, i, got[i])
            want_f.append(0.0)
            continue
        words, rows = it
        want = [lcs_of(words, r) for r in rows] + [-1] * (Rmax - len(rows))
        assert got[i] == want, (what, i, got[i], want, len(words), [len(r) for r in rows])
        want_f.append(ref.rouge_l(words, rows, beta=BETA32))
    _floats_ok(out.double().cpu().tolist(), want_f, what, "rouge")
    return out, lcs


@pytest.fixture(scope="module")
def recorded():
    """every recorded image as one image of ONE launch: (128, 5, 65) references, the unused rows filled with plausible words"""
    images = [im for case in golden_cases() for im in case["images"]]
    docs = [refs for _, refs in images]
    arr, count = pad_refs(docs, 5, 65)
    rng = np.random.default_rng(1)
    for g, rows in enumerate(docs):
        arr[g, len(rows):] = rng.integers(0, 40, (5 - len(rows), 65))
    cand = pad_rows([c for c, _ in images], 65)
    counts = [row for case in golden_cases() for row in case["counts"]]
    bleu = [row for case in golden_cases() for row in case["bleu"]]
    rouge = [v for case in golden_cases() for v in case["rouge"]]
    return dict(cand=cand, arr=arr, count=count, counts=counts, bleu=bleu, rouge=rouge)


def test_recorded_cases(recorded):
    """the ten integers equal the reference scorer's own; the statement's floats (equal to the recorded ones to 1e-12) are met"""
    stats, bleu, want = _check_bleu(recorded["cand"], 65, recorded["arr"], "recorded cases", ref_count=recorded["count"])
    assert want == recorded["counts"] and stats.cpu().tolist() == recorded["counts"]
    _floats_ok(bleu.double().cpu().reshape(-1).tolist(), [v for row in recorded["bleu"] for v in row], "recorded sentence BLEU", "bleu")
    _check_rouge(recorded["cand"], 65, recorded["arr"], "recorded cases", ref_count=recorded["count"])
    assert recorded["count"].min() == 1 and recorded["count"].max() == 5


def _crafted(rng, vocab, lengths, ref_lengths):
    """one image per candidate length: references of ref_lengths over `vocab` words, the candidate = a reference cut or repeated to its
    length with a few substitutions"""
    refs, cands = [], []
    for L in lengths:
        rows = [[int(t) for t in rng.integers(0, vocab, l)] for l in ref_lengths]
        base = rows[len(refs) % len(rows)] or [1]
        c = [base[i % len(base)] for i in range(L)]
        for _ in range(int(rng.integers(0, 4))):
            if c:
                c[int(rng.integers(0, L))] = int(rng.integers(0, vocab))
        refs.append(rows)
        cands.append(c)
    return refs, cands


@pytest.mark.parametrize("vocab", [40, 2])
def test_bleu_candidate_lengths_up_to_256(vocab):
    """candidates of 0, 1, 2, 3, 63, 64, 65, 255 and 256 words (256: no terminator, the caption runs to cand_len) against references of
    0 .. 256 words; with a two-symbol alphabet tf and the clip run to large counts.  A one-word candidate against ONE 256-word reference:
    the brevity penalty exp(-255) is below fp32's range."""
    rng = np.random.default_rng(3 + vocab)
    lengths = [0, 1, 2, 3, 63, 64, 65, 255, 256]
    refs, cands = _crafted(rng, vocab, lengths, [256, 0, 3, 64, 200, 255, 65, 1, 130, 256, 17, 63, 2, 129, 250, 9])
    refs.append([[int(t) for t in rng.integers(0, vocab, 256)]])
    cands.append([refs[-1][0][5]])
    arr, count = pad_refs(refs, 16, 256)
    stats, bleu, want = _check_bleu(pad_rows(cands, 256), 256, arr, f"lengths up to 256, {vocab} words", ref_count=count)
    assert [w[0] for w in want] == lengths + [1] and want[-1][1] == 256 and float(bleu[-1, 0]) < 2.0 ** -126
    if vocab == 2:
        assert want[8][6] > 100 and want[8][7] > 50 and want[8][9] > 5                      # large clipped counts, n = 4 included
    _check_rouge(pad_rows(cands, 256), 256, arr, f"lengths up to 256, {vocab} words", ref_count=count)


def test_ref_count_subsets_never_read_the_other_rows():
    """the rows beyond ref_count hold the candidate itself (and a row of its length): read, they would change every count and reflen"""
    rng = np.random.default_rng(5)
    refs, cands, poison = [], [], []
    for g in range(8):
        rows = [[int(t) for t in rng.integers(0, 6, int(rng.choice([3, 9, 17, 40])))] for _ in range(int(rng.integers(1, 5)))]
        c = [int(t) for t in rng.integers(0, 6, int(rng.choice([5, 12, 30])))]
        refs.append(rows)
        cands.append(c)
    arr, count = pad_refs(refs, 5, 40)
    for g, c in enumerate(cands):
        arr[g, count[g]:, :] = -1
        arr[g, count[g]:, :len(c)] = c
    kw = dict(ref_count=count)
    _, _, want = _check_bleu(pad_rows(cands, 30), 30, arr, "ref_count subsets", **kw)
    _, lcs = _check_rouge(pad_rows(cands, 30), 30, arr, "ref_count subsets", **kw)
    assert all(w[9] < w[5] for w in want)                                                   # no candidate is matched whole
    assert bool((lcs.cpu()[torch.arange(8), torch.from_numpy(count).long()] == -1).all())   # the first row not in use reports -1
    # ref_count NULL: now they count
    stats, _, want_all = _check_bleu(pad_rows(cands, 30), 30, arr, "ref_count NULL")
    assert all(w[9] == w[5] and w[1] == w[0] for w in want_all)
    # counts outside 1..Rmax are clamped
    _check_bleu(pad_rows(cands, 30), 30, arr, "ref_count clamped", ref_count=np.array([0, 9, -3, 5, 1, 2, 7, 1], np.int32))
    _check_rouge(pad_rows(cands, 30), 30, arr, "ref_count clamped", ref_count=np.array([0, 9, -3, 5, 1, 2, 7, 1], np.int32))


def test_cand_group_stop_token_leading_dimension_and_large_ids():
    rng = np.random.default_rng(6)
    stop = 38
    refs = [[[4, 5, 6, 7, 8, 9], [4, 5, 6, stop]], [[10, 11, 12, stop], [10, 11, 12, 13, 14, stop]], [[4, 5, 10, 11], [stop]]]
    arr, count = pad_refs(refs, 2, 7)
    rows = pad_rows([[stop, 4, 5, 6], [10, 11, stop, 12, 13], [4, 5, 6, 7, 8, 9, 4, 5], [10, 11, 12, 13, 14, stop, stop, 3],
                     [4, 5, -1, 6, stop, 7], [10, 11, 12, stop], [4, 5, 6, 7], [10, 11, 12, 13]], 12)
    rows[:, 8:] = [4, 5, 6, 7]                                                             # beyond cand_len = 8: matching words, never read
    group = [0, 1, 0, 1, 2, 1, -1, 3]                                                      # the last two: outside [0, 3)
    for count_stop in (0, 1):
        kw = dict(stop=stop, count_stop=count_stop, group=group, ref_count=count)
        stats, bleu, want = _check_bleu(rows, 8, arr, f"group, stop token, count_stop {count_stop}", **kw)
        assert want[0][0] == count_stop and want[2][0] == 8 and want[5][0] == 3 + count_stop
        assert stats.cpu()[6:].abs().sum() == 0 and float(bleu[6:].abs().sum()) == 0.0       # an all-zero row
        out, _ = _check_rouge(rows, 8, arr, f"group, stop token, count_stop {count_stop}", **kw)
        assert float(out[6]) == 0.0 and float(out[7]) == 0.0
    _check_bleu(rows[:6], 8, arr, "no stop token, modulo rule", ref_count=count)
    _check_rouge(rows[:6], 8, arr, "no stop token, modulo rule", ref_count=count)
    # ids at and beyond 65535 are words like any other; a candidate id >= 2^31 matches no reference word
    big, top = (1 << 40) + 5, (1 << 31) - 1
    refs = [[[0, 65535, 70000, 0, top], [65534, 65534]], [[5, 70000, 6, 70000, 5], [top, top, 5]]]
    arr, count = pad_refs(refs, 2, 5)
    rows = pad_rows([[0, 65535, 70000, 0, top], [5, 70000, 6, 70000], [65534, 1 << 31, 0, (1 << 32) + 65534], [big, 5, big, top, top, 5],
                     [(1 << 32) + 0], [70000, 5, 70000, 5]], 6)
    _, _, want = _check_bleu(rows, 6, arr, "large ids", ref_count=count)
    assert want[0][6:] == [5, 4, 3, 2] and want[1][6:] == [4, 3, 2, 1] and want[2][6:] == [2, 0, 0, 0] and want[4][6] == 0
    _, lcs = _check_rouge(rows, 6, arr, "large ids", ref_count=count, lcs_of=ref.lcs)
    assert lcs.cpu().tolist()[0] == [5, 0] and lcs.cpu().tolist()[4] == [0, 0] and lcs.cpu().tolist()[3] == [2, 3]


LCS_LENGTHS = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256]


@pytest.mark.parametrize("pattern", ["equal", "disjoint", "two_symbols", "subsequence"])
def test_lcs_at_every_word_boundary(pattern):
    """candidate and reference lengths from LCS_LENGTHS in both orders, 100 images of one launch.  Row 0 is the pattern's reference, row 1
    a two-symbol reference of another length, row 2 is in use for every third image only (else it reports -1)."""
    rng = np.random.default_rng(7)
    cands, refs = [], []
    for Lc in LCS_LENGTHS:
        for Lr in LCS_LENGTHS:
            if pattern == "equal":
                c, r = [3] * Lc, [3] * Lr
            elif pattern == "disjoint":
                c, r = rng.integers(0, 20, Lc).tolist(), rng.integers(20, 40, Lr).tolist()
            elif pattern == "two_symbols":                                                  # long runs of matches: carries cross the 64-bit words
                c, r = rng.integers(0, 2, Lc).tolist(), rng.integers(0, 2, Lr).tolist()
            else:                                                                           # the shorter is a subsequence of the longer
                long_ = rng.integers(0, 5, max(Lc, Lr)).tolist()
                short = [long_[i] for i in sorted(rng.choice(max(Lc, Lr), min(Lc, Lr), replace=False).tolist())]
                c, r = (short, long_) if Lc <= Lr else (long_, short)
            other = rng.integers(0, 2, int(rng.choice(LCS_LENGTHS))).tolist()
            rows = [r, other] + ([rng.integers(0, 3, 70).tolist()] if len(cands) % 3 == 0 else [])
            cands.append(c)
            refs.append(rows)
    arr, count = pad_refs(refs, 3, 256)
    arr[np.arange(100)[count == 2], 2, :] = 1                                               # not in use: would match if read
    out, lcs = _check_rouge(pad_rows(cands, 256), 256, arr, f"LCS, {pattern}", ref_count=count)
    first = lcs.cpu()[:, 0].tolist()
    lens = [(Lc, Lr) for Lc in LCS_LENGTHS for Lr in LCS_LENGTHS]
    if pattern in ("equal", "subsequence"):
        assert first == [min(a, b) for a, b in lens]
    elif pattern == "disjoint":
        assert first == [0] * 100
    else:
        assert all(l >= min(a, b) // 2 for l, (a, b) in zip(first, lens)) and len(set(first)) > 15
    assert int((lcs.cpu()[:, 2] == -1).sum()) == int((count == 2).sum()) > 0


def test_repeatable_nothing_else_written_and_null_outputs(recorded):
    cand, arr, count = recorded["cand"], recorded["arr"], recorded["count"]
    C_, n, border = cand.shape[0], cand.shape[0] - 3, 64
    group = np.arange(C_, dtype=np.int32)                                                   # n < C: not a multiple of G, so the map is given
    runs = []
    for canary_i, canary_f in ((-123456, -123.25), (77, 7.5)):
        stats = torch.full((border + C_ * 10 + border,), canary_i, dtype=torch.int32, device="cuda")
        bleu = torch.full((border + C_ * 4 + border,), canary_f, device="cuda")
        out = torch.full((border + C_ + border,), canary_f, device="cuda")
        lcs = torch.full((border + C_ * 5 + border,), canary_i, dtype=torch.int32, device="cuda")
        _launch("bleu", cand, 65, arr, ref_count=count, group=group, n=n, main=stats[border:], extra=bleu[border:])
        _launch("rouge", cand, 65, arr, ref_count=count, group=group, n=n, main=out[border:], extra=lcs[border:])
        got = []
        for buf, width, canary in ((stats, 10, canary_i), (bleu, 4, canary_f), (out, 1, canary_f), (lcs, 5, canary_i)):
            host = buf.cpu()
            assert bool((host[:border] == canary).all()) and bool((host[border + n * width:] == canary).all())   # beyond [C] rows, both borders
            got.append(host[border:border + n * width].clone())
        runs.append(got)
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))                        # the same bits on every run
    assert int((runs[0][2] != 0).sum()) > n // 2
    # NULL bleu / lcs: accepted, the other output is what it was
    stats, none = _launch("bleu", cand, 65, arr, ref_count=count, group=group, n=n, extra=None)
    assert none is None and torch.equal(stats.cpu().reshape(-1), runs[0][0])
    out, none = _launch("rouge", cand, 65, arr, ref_count=count, group=group, n=n, extra=None)
    assert none is None and torch.equal(out.cpu().view(torch.int32), runs[0][2].view(torch.int32))


def test_engine_wrappers_and_corpus_bleu(recorded):
    from clipcap_amd import engine
    cand, arr, count = (torch.from_numpy(recorded[k]).cuda() for k in ("cand", "arr", "count"))
    wide = torch.full((cand.shape[0], 80), 3, dtype=torch.int64, device="cuda")             # a view with a row stride
    wide[:, :65] = cand
    stats, bleu = engine.bleu_stats(wide[:, :65], arr, stop_token=-1, ref_count=count)
    assert stats.cpu().tolist() == recorded["counts"]
    score, lcs = engine.rouge_l(wide[:, :65], arr, stop_token=-1, ref_count=count)
    assert lcs.shape == (cand.shape[0], 5) and score.shape == (cand.shape[0],)
    lo = 0
    for case in golden_cases():
        hi = lo + len(case["images"])
        got = engine.bleu_corpus(stats[lo:hi])
        assert all(abs(a - b) <= 1e-12 * abs(b) for a, b in zip(got, case["case_bleu"]))
        lo = hi


def test_evaluate_metrics_from_lists_on_the_recorded_cases():
    from clipcap_amd.eval.metrics import evaluate_metrics_from_lists
    for case in golden_cases():
        preds = [" ".join(f"w{t}" for t in c) for c, _ in case["images"]]
        truths = [[" ".join(f"w{t}" for t in r) for r in refs] for _, refs in case["images"]]
        total, per = evaluate_metrics_from_lists(preds, truths)
        for n in range(4):
            assert abs(total[f"Bleu_{n + 1}"] - case["case_bleu"][n]) <= 1e-12 * case["case_bleu"][n]
        assert abs(total["ROUGE_L"] - case["case_rouge"]) <= REL * case["case_rouge"]
        assert abs(total["CIDEr"] - case["case_cider"]) <= 2e-5 * case["case_cider"]
        assert len(per) == len(preds) and all(abs(per[i]["ROUGE_L"] - v) <= REL * v for i, v in enumerate(case["rouge"]))


def test_self_critical_step_with_a_mix_of_metrics():
    """MetricReward(cider + bleu4 + rouge_l).for_batch as the reward of self_critical_step on the tiny model of tests/test_gpu_cider.py:
    the loss is finite, and the rewards are the weighted sum of the three metrics launched separately on the ids the step decoded."""
    from clipcap_amd import engine
    from clipcap_amd.inference.base import sample_tokens
    from clipcap_amd.train import CiderReward, MetricReward, self_critical_step
    from tests.test_gpu_token_weights import _scst_model
    model, embeds, eos, V, entry = _scst_model()
    B = embeds.shape[0]
    gen = torch.Generator(device="cuda").manual_seed(7)
    with torch.no_grad():
        prefix = model.engine.mapper.forward(embeds, save=False)
        sampled0, _ = sample_tokens(model, prefix, entry_length=entry, stop_token=eos, mode=0, top_p=1.0, generator=gen, suppress_tokens=[0])
        greedy0, _ = sample_tokens(model, prefix, entry_length=entry, stop_token=eos, mode=0, top_p=1.0, top_k=1, suppress_tokens=[0])
    rng = np.random.default_rng(6)
    docs = []
    for g_row, s_row in zip(greedy0.cpu().tolist(), sampled0.cpu().tolist()):
        words = cider_ref.cut(s_row, eos) or [1]
        edited = list(words)
        edited[int(rng.integers(0, len(edited)))] = int(rng.integers(1, V))
        docs.append([cider_ref.cut(g_row, eos) or [1], edited, words[1:] or [2]][:int(rng.integers(2, 4))])
    arr, count = pad_refs(docs, 3, entry + 2)
    refs, count = torch.from_numpy(arr).cuda(), torch.from_numpy(count).cuda()
    weights = {"cider": 1.0, "bleu4": 0.5, "rouge_l": 0.25}
    cider = CiderReward.from_corpus(docs, stop_token=eos)
    inner = MetricReward(weights, cider=cider, stop_token=eos).for_batch(refs, count)
    seen = {}

    def reward_fn(sampled, greedy):
        r_s, r_g = inner(sampled, greedy)
        seen.update(sampled=sampled.clone(), greedy=greedy.clone(), r_s=r_s.clone(), r_g=r_g.clone())
        return r_s, r_g

    gen = torch.Generator(device="cuda").manual_seed(7)
    loss, m_s, m_g = self_critical_step(model, embeds, reward_fn, 0.0, entry_length=entry, stop_token=eos, generator=gen)
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and torch.equal(seen["sampled"], sampled0) and torch.equal(seen["greedy"], greedy0)
    for ids, r, mean in ((seen["sampled"], seen["r_s"], m_s), (seen["greedy"], seen["r_g"], m_g)):
        ids = ids.contiguous()
        kw = dict(stop_token=eos, count_stop=False, ref_count=count)
        c = engine.cider_score(ids, refs, cider.tab_keys, cider.tab_idf, cider.log_ndocs, sigma=cider.sigma, **kw)
        b = engine.bleu_stats(ids, refs, **kw)[1][:, 3]
        l = engine.rouge_l(ids, refs, **kw)[0]
        assert torch.equal(r, c * 1.0 + b * 0.5 + l * 0.25)                                 # the order of MetricReward.score
        assert float(mean) == float(r.mean())
        rows = [cider_ref.cut(row, eos) for row in ids.cpu().tolist()]
        _floats_ok(b.double().cpu().tolist(), [ref.bleu_from_counts(ref.bleu_counts(w, d))[3] for w, d in zip(rows, docs)], "step BLEU-4", "bleu")
        _floats_ok(l.double().cpu().tolist(), [ref.rouge_l(w, d, beta=BETA32) for w, d in zip(rows, docs)], "step ROUGE-L", "rouge")
    assert float(seen["r_s"].max()) > 0 and bool((seen["r_s"] != seen["r_g"]).any()) and B == seen["r_s"].shape[0]
