"""Device tests of the CIDEr-D reward: cc_cider_score through the C ABI against tests/cider_ref.py (float64) evaluated with the table's own
fp32 idf values, its repeatability and its borders, CiderReward end to end against the scores recorded from the reference project's
scorer, and self_critical_step with CiderReward.for_batch as its reward.

The bound of the kernel: every term is a product of small exact integers and fp32 idf values and none is negative, so nothing cancels;
the relative error is at most about (L + 16) 2^-24 <= 1.6e-5 at L = 256.  Asserted: |dev - ref| <= 2e-5 ref, and exactly 0 where the
reference is exactly 0."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import cider_ref
from tests.cider_cases import MASK64, MUL, golden_cases, pack, pad_refs, pad_rows, shared_inputs, table_find

pytestmark = pytest.mark.gpu
TOL = 2e-5
WORST = {"ratio": 0.0}


def _ptr(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _table(keys, idf, cap=None):
    from clipcap_amd.train.cider import build_table
    tk, ti = build_table(np.asarray(keys, np.uint64), np.asarray(idf, np.float32), cap)
    return dict(tk=tk, ti=ti, dk=torch.from_numpy(tk.view(np.int64)).cuda(), di=torch.from_numpy(ti).cuda())


def _corpus_table(docs, cap=None):
    from clipcap_amd.train.cider import corpus_idf
    keys, idf, N = corpus_idf(docs)
    return _table(keys, idf, cap), float(np.float32(math.log(N)))


def _idf_of(tab, miss):
    def idf(g):
        if any(t < 0 or t >= 65535 for t in g):
            return miss                                        # cannot be packed: misses the table
        return table_find(tab["tk"], tab["ti"], pack(g), miss)
    return idf


def _launch(cand, cand_len, refs, tab, log_n, *, stop=-1, count_stop=0, group=None, ref_count=None, sigma=6.0, out=None, n=None):
    from clipcap_amd import _lib
    dc, dr = torch.from_numpy(np.ascontiguousarray(cand)).cuda(), torch.from_numpy(np.ascontiguousarray(refs)).cuda()
    dg = None if group is None else torch.from_numpy(np.asarray(group, np.int32)).cuda()
    dn = None if ref_count is None else torch.from_numpy(np.asarray(ref_count, np.int32)).cuda()
    n = cand.shape[0] if n is None else n
    out = torch.full((n,), float("nan"), device="cuda") if out is None else out
    G, Rmax, Lr = refs.shape
    rc = _lib.lib().cc_cider_score(_ptr(dc), n, cand_len, cand.shape[1], stop, count_stop, _ptr(dg), _ptr(dr), G, Rmax, Lr, _ptr(dn),
                                   _ptr(tab["dk"]), _ptr(tab["di"]), len(tab["tk"]), log_n, sigma, _ptr(out),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out


def _reference(cand, cand_len, refs, tab, log_n, *, stop=-1, count_stop=0, group=None, ref_count=None, sigma=6.0):
    idf = _idf_of(tab, log_n)
    G, Rmax, _ = refs.shape
    want = []
    for c, row in enumerate(cand):
        g = c % G if group is None else int(group[c])
        words = cider_ref.cut(row[:cand_len], stop if stop >= 0 else None, bool(count_stop))
        rows = [cider_ref.cut(r) for r in refs[g][:Rmax if ref_count is None else int(ref_count[g])]]
        want.append(cider_ref.cider_d(words, rows, idf, sigma))
    return want


def _compare(dev, want, what):
    dev = dev.double().cpu().tolist()
    worst = 0.0
    for i, (d, w) in enumerate(zip(dev, want)):
        if w == 0.0:
            assert d == 0.0, (what, i, d)
        else:
            worst = max(worst, abs(d - w) / w)
    WORST["ratio"] = max(WORST["ratio"], worst)
    print(f"{what}: {len(want)} candidates, {sum(w == 0.0 for w in want)} score 0, max {max(want):.4f}; "
          f"largest |dev - ref| / ref = {worst:.3e} (bound {TOL:.0e}; largest so far {WORST['ratio']:.3e})")
    assert worst <= TOL, (what, worst)


def _check(cand, cand_len, refs, tab, log_n, what, **kw):
    dev = _launch(cand, cand_len, refs, tab, log_n, **kw)
    _compare(dev, _reference(cand, cand_len, refs, tab, log_n, **kw), what)
    return dev


@pytest.fixture(scope="module")
def shared():
    """G = 8 images; references padded to (8, 5, 65) with the unused rows filled with plausible tokens; the corpus table of the references"""
    refs, cands = shared_inputs(seed=5)
    arr, count = pad_refs(refs, 5, 65)
    rng = np.random.default_rng(1)
    for g, rows in enumerate(refs):
        arr[g, len(rows):] = rng.integers(0, 40, (5 - len(rows), 65))
    tab, log_n = _corpus_table(refs)
    return dict(refs=refs, cands=cands, arr=arr, count=count, tab=tab, log_n=log_n)


def test_shared_inputs_lengths_layout_and_groups(shared):
    """The shared candidates plus candidates of 0, 1, 2, 3, 4, 63, 64 and 65 words; cand_ld > cand_len with garbage in the gap; ref_count
    below Rmax; cand_group given — and the modulo rule on a reordering of the same candidates gives the same bits."""
    refs, cands = shared["refs"], list(shared["cands"])
    want_shared = _reference(pad_rows([c for _, c in cands], 65), 65, shared["arr"], shared["tab"], shared["log_n"],
                             group=[g for g, _ in cands], ref_count=shared["count"])
    assert sum(w == 0.0 for w in want_shared) <= 0.10 * len(want_shared)                    # the recipe: few cases score 0
    for k, L in enumerate([0, 1, 2, 3, 4, 63, 64, 65]):
        g = k % len(refs)
        base = max(refs[g], key=len) or [3]
        cands.append((g, [base[i % len(base)] for i in range(L)]))
    rows = pad_rows([c for _, c in cands], 72)
    rows[:, 65:] = np.random.default_rng(2).integers(0, 40, (len(cands), 7))               # beyond cand_len = 65: never read
    group = [g for g, _ in cands]
    dev = _check(rows, 65, shared["arr"], shared["tab"], shared["log_n"], "shared inputs", group=group, ref_count=shared["count"])
    assert shared["count"].min() < 5
    # the modulo rule: two candidates per image, image-major order undone
    by_image = {g: [i for i, gg in enumerate(group) if gg == g][:2] for g in range(8)}
    order = [by_image[g][j] for j in range(2) for g in range(8)]
    dev2 = _check(rows[order], 65, shared["arr"], shared["tab"], shared["log_n"], "modulo rule", ref_count=shared["count"])
    assert torch.equal(dev2.view(torch.int32).cpu(), dev.view(torch.int32).cpu()[order])    # a score does not depend on its neighbours
    # all Rmax rows in use (ref_count NULL): the filler rows now count
    _check(rows, 65, shared["arr"], shared["tab"], shared["log_n"], "ref_count NULL", group=group)


def test_longest_shapes():
    """Rmax * Lr = 4096 with Lr = 256, candidates of 256 words (no terminator: they run to cand_len), 255 and 250 words"""
    rng = np.random.default_rng(3)
    refs = [[[int(t) for t in rng.integers(0, 40, L)] for L in [256, 256, 255, 250, 241, 256, 199, 256, 256, 230, 256, 256, 254, 256, 253, 256]]
            for _ in range(2)]
    arr, _ = pad_refs(refs, 16, 256)
    tab, log_n = _corpus_table(refs)
    cands = []
    for g in range(2):
        for L, sub in ((256, 3), (256, 40), (255, 0), (250, 10)):
            c = list(refs[g][len(cands) % 16][:L])
            c += [int(t) for t in rng.integers(0, 40, L - len(c))]
            for _ in range(sub):
                c[int(rng.integers(0, L))] = int(rng.integers(0, 40))
            cands.append((g, c))
    _check(pad_rows([c for _, c in cands], 256), 256, arr, tab, log_n, "Rmax * Lr = 4096, L = 256", group=[g for g, _ in cands])


def test_repeats_stop_tokens_and_token_ids():
    # one token 9 times against a reference repeating it 3 times (and a second reference): tf > 1, first occurrence, the clip
    refs = [[[7, 7, 7], [7, 2, 7, 7, 7, 7, 1]], [[1, 2, 3, 4, 5], [7]]]
    arr, count = pad_refs(refs, 2, 8)
    tab, log_n = _corpus_table(refs + [[[9, 9]]])
    rows = pad_rows([[7] * 9, [7] * 9, [7, 7, 7], [1, 2, 3, 1, 2, 3, 1, 2, 3]], 9)
    dev = _check(rows, 9, arr, tab, log_n, "repeated tokens", group=[0, 1, 0, 1], ref_count=count)
    assert float(dev[0]) > 0 and float(dev[2]) > float(dev[0])
    # the stop token at position 0, in the middle and absent, a negative id before it; count_stop 0 and 1
    stop = 38
    refs = [[[4, 5, 6, 7, 8, 9], [4, 5, 6, stop]], [[10, 11, 12, stop], [10, 11, 12, 13, 14, stop]]]
    arr, count = pad_refs(refs, 2, 7)
    tab, log_n = _corpus_table(refs + [[[1, 2]]])
    rows = pad_rows([[stop, 4, 5, 6], [10, 11, stop, 12, 13], [4, 5, 6, 7, 8, 9, 4, 5], [10, 11, 12, 13, 14, stop, stop, 3],
                     [4, 5, -1, 6, stop, 7], [10, 11, 12, stop]], 8)
    a = _check(rows, 8, arr, tab, log_n, "stop token, not counted", stop=stop, count_stop=0)
    b = _check(rows, 8, arr, tab, log_n, "stop token, counted", stop=stop, count_stop=1)
    assert float(a[0]) == 0.0 and float(b[0]) > 0.0 and float(a[2]) == float(b[2])          # (stop) alone matches reference 2 of image 0
    _check(rows, 8, arr, tab, log_n, "no stop token", stop=-1)
    # token ids 0 and 65534 (packed), 65535 / 70000 / 2^40 + 5 (not packed: they miss the table and still match exactly)
    big = (1 << 40) + 5
    refs = [[[0, 65534, 0, 0, 65534], [65534, 65534]], [[5, 70000, 6, 70000, 5], [65535, 5]]]
    arr, count = pad_refs(refs, 2, 5)
    tab, log_n = _corpus_table([[[0, 65534, 0, 0, 65534], [65534, 65534]], [[5, 6, 5], [5]], [[0, 1]]])
    rows = pad_rows([[0, 65534, 0, 65534], [5, 70000, 6, 70000], [65534, 0, 0], [big, 5, big, 5, 65535, 5], [0], [70000, 5, 70000, 5]], 6)
    dev = _check(rows, 6, arr, tab, log_n, "token ids", ref_count=count)
    assert all(float(v) > 0 for v in dev)


def _colliding_tokens(cap, slot, n):
    lg = cap.bit_length() - 1
    return [t for t in range(65535) if ((pack((t,)) * MUL) & MASK64) >> (64 - lg) == slot][:n]


def test_table_at_load_one_half_and_forced_probe_chains(shared):
    from clipcap_amd.train.cider import corpus_idf
    # load exactly 0.5: the shared corpus's keys filled up to a power of two with keys no caption holds
    keys, idf, N = corpus_idf(shared["refs"])
    n = 1 << (len(keys) - 1).bit_length()
    extra = np.array([pack((60000 + i % 5000, 60001 + i // 5000)) for i in range(n - len(keys))], np.uint64)
    tab = _table(np.concatenate((keys, extra)), np.concatenate((idf, np.full(len(extra), 9.0, np.float32))), cap=2 * n)
    assert int((tab["tk"] != MASK64).sum()) * 2 == len(tab["tk"])
    cands = shared["cands"]
    dev = _check(pad_rows([c for _, c in cands], 65), 65, shared["arr"], tab, shared["log_n"], "load 0.5", group=[g for g, _ in cands],
                 ref_count=shared["count"])
    assert float(dev.max()) > 1.0
    # forced chains: 12 unigrams that hash into the second-last of 64 slots, so the chain wraps round the end; arbitrary idf values
    toks = _colliding_tokens(64, 62, 13)
    absent, toks = toks[12], toks[:12]
    rng = np.random.default_rng(4)
    grams = [(t,) for t in toks] + [(toks[i], toks[i + 1]) for i in range(8)] + [(toks[0], toks[1], toks[2]), (toks[0], toks[1], toks[2], toks[3])]
    tab = _table([pack(g) for g in grams], rng.uniform(0.1, 3.0, len(grams)).astype(np.float32), cap=64)
    slots = [int(np.nonzero(tab["tk"] == np.uint64(pack((t,))))[0][0]) for t in toks]
    assert slots[:4] == [62, 63, 0, 1] and max(slots) >= 9                                  # the chain is real and wraps
    refs = [[toks[:6], [toks[5], toks[0], toks[1], toks[11], absent]], [list(reversed(toks)), [toks[3]] * 4]]
    arr, count = pad_refs(refs, 2, 12)
    rows = pad_rows([toks[:5] + [absent], list(reversed(toks))[2:9], [toks[0], toks[1], toks[2], toks[3], toks[0], toks[1]], [toks[3]] * 3 + [absent] * 2], 7)
    dev = _check(rows, 7, arr, tab, 1.25, "forced probe chains", ref_count=count)
    assert all(float(v) > 0 for v in dev)


def test_repeatable_and_nothing_else_written(shared):
    cands = shared["cands"]
    rows, group = pad_rows([c for _, c in cands], 65), [g for g, _ in cands]
    n, border = len(cands) - 3, 64
    bufs = []
    for canary in (-123.25, 7.5):
        buf = torch.full((border + len(cands) + border,), canary, device="cuda")
        _launch(rows, 65, shared["arr"], shared["tab"], shared["log_n"], group=group, ref_count=shared["count"], out=buf[border:], n=n)
        got = buf.cpu()
        assert bool((got[:border] == canary).all()) and bool((got[border + n:] == canary).all())       # out beyond C and both borders
        assert bool((got[border:border + n] >= 0).all())
        bufs.append(got[border:border + n].view(torch.int32).clone())
    assert torch.equal(bufs[0], bufs[1])                                                    # the same bits on every run
    assert int((bufs[0] != 0).sum()) > n // 2


def test_end_to_end_against_the_recorded_reference_scores():
    """CiderReward.from_corpus(...).score on the recorded cases against the reference scorer's own scores: the kernel's 2e-5 plus what
    rounding the idf to fp32 moves — that term bounded here in float64 (the statement with the float64 idf against the statement with the
    table's fp32 idf), never taken from the device."""
    from clipcap_amd.train import CiderReward
    worst, n = 0.0, 0
    for case in golden_cases():
        images = case["images"]
        docs = [refs for _, refs in images]
        rw = CiderReward.from_corpus(docs)
        arr, count = pad_refs(docs, max(len(d) for d in docs), max(1, max(len(r) for d in docs for r in d)))
        cand = pad_rows([c for c, _ in images], max(1, max(len(c) for c, _ in images)))
        dev = rw.score(torch.from_numpy(cand).cuda(), torch.from_numpy(arr).cuda(), torch.from_numpy(count).cuda()).double().cpu().tolist()
        tab = dict(tk=rw.tab_keys.cpu().numpy().view(np.uint64), ti=rw.tab_idf.cpu().numpy())
        idf64 = cider_ref.idf_from_df(case["df"], len(images))
        idf32 = _idf_of(tab, float(np.float32(math.log(len(images)))))
        for (c, refs), want, d in zip(images, case["score"], dev):
            rounding = abs(cider_ref.cider_d(c, refs, idf64) - cider_ref.cider_d(c, refs, idf32))
            assert abs(d - want) <= TOL * want + rounding, (c, refs, d, want, rounding)
            if want > 0:
                worst = max(worst, abs(d - want) / want)
            n += 1
    print(f"{n} recorded candidates: largest |dev - recorded| / recorded = {worst:.3e}")


def test_self_critical_step_with_the_device_reward():
    """for_batch as the reward of self_critical_step on the suite's tiny model: the rewards it returned are cider_ref's on the ids it
    was given, the step's mean rewards are their means, and the loss is fused_step's with the weights built from those rewards."""
    from clipcap_amd.inference.base import sample_tokens
    from clipcap_amd.train import CiderReward, scst_tokens_and_weights, self_critical_step
    from tests.test_gpu_token_weights import _scst_model
    model, embeds, eos, V, entry = _scst_model()
    B = embeds.shape[0]
    # references near what the model says: lr = 0 and the same seed give the step the captions decoded here.  Per image: the greedy
    # caption (the tiny model says much the same for every image: idf near 0), the sampled one with a substitution, and with a deletion
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
        k = int(rng.integers(0, len(words)))
        docs.append([cider_ref.cut(g_row, eos) or [1], edited, words[:k] + words[k + 1:]][:int(rng.integers(2, 4))])
    arr, count = pad_refs(docs, 3, entry + 2)
    rw = CiderReward.from_corpus(docs, stop_token=eos)
    inner = rw.for_batch(torch.from_numpy(arr).cuda(), torch.from_numpy(count).cuda())
    seen = {}

    def reward_fn(sampled, greedy):
        r_s, r_g = inner(sampled, greedy)
        seen.update(sampled=sampled.clone(), greedy=greedy.clone(), r_s=r_s.clone(), r_g=r_g.clone())
        return r_s, r_g

    gen = torch.Generator(device="cuda").manual_seed(7)
    loss, m_s, m_g = self_critical_step(model, embeds, reward_fn, 0.0, entry_length=entry, stop_token=eos, generator=gen)
    torch.cuda.synchronize()
    tab = dict(tk=rw.tab_keys.cpu().numpy().view(np.uint64), ti=rw.tab_idf.cpu().numpy())
    idf = _idf_of(tab, float(np.float32(rw.log_ndocs)))
    for ids, r, what in ((seen["sampled"], seen["r_s"], "sampled"), (seen["greedy"], seen["r_g"], "greedy")):
        want = [cider_ref.cider_d(cider_ref.cut(row, eos), docs[b], idf) for b, row in enumerate(ids.cpu().tolist())]
        _compare(r, want, f"self-critical step, {what} captions")
    assert torch.equal(seen["sampled"], sampled0) and torch.equal(seen["greedy"], greedy0)
    assert float(seen["r_s"].max()) > 0 and bool((seen["r_s"] != seen["r_g"]).any())
    assert float(m_s) == float(seen["r_s"].mean()) and float(m_g) == float(seen["r_g"].mean())
    tokens, weights = scst_tokens_and_weights(seen["sampled"], seen["r_s"] - seen["r_g"], eos)
    by_hand = model.fused_step((tokens, embeds), 0.0, token_weights=weights)
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and float(by_hand) == float(loss)
    assert B == seen["r_s"].shape[0]
