"""CPU side of the CIDEr-D reward: cc_cider_score and its host-only table builder are declared, bound and exported under ABI version 3;
the argument checks need no device; CiderReward.from_corpus counts document frequencies as a dict count does and builds a table every
key is found in; for_batch pads and groups as documented (the launch stubbed out).  The kernel is tested on the device in
tests/test_gpu_cider.py."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import cider_ref
from tests.cider_cases import MASK64, golden_cases, pack, table_find

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = {
    "cc_cider_score": ["const int64_t* cand", "int32_t C", "int32_t cand_len", "int64_t cand_ld", "int32_t stop_token", "int32_t count_stop",
                       "const int32_t* cand_group", "const int32_t* refs", "int32_t G", "int32_t Rmax", "int32_t Lr", "const int32_t* ref_count",
                       "const uint64_t* tab_keys", "const float* tab_idf", "int64_t cap", "float log_ndocs", "float sigma", "float* out",
                       "void* stream"],
    "cc_cider_table_build": ["const uint64_t* keys", "const float* idf", "int64_t n", "uint64_t* tab_keys", "float* tab_idf", "int64_t cap"],
}


@pytest.mark.parametrize("name", sorted(ENTRY))
def test_header_binding_and_library_carry_the_entry_point(name):
    from clipcap_amd import _lib
    raw = open(os.path.join(ROOT, "include", "clipcap_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr, flags=re.M)
    assert m, f"{name} is not declared in include/clipcap_hip.h"
    params = [p.strip() for p in " ".join(m.group(1).split()).split(",")]
    assert params == ENTRY[name]
    res, args = _lib.SIGNATURES[name]
    assert res is _lib._I and len(args) == len(params)
    for p, a in zip(params, args):
        want = _lib._P if "*" in p else _lib._L if p.startswith("int64_t") else _lib._F if p.startswith("float") else _lib._I
        assert a is want, (p, a)
    l = _lib.lib()
    assert hasattr(l, name) and l.cc_abi_version() == 3 and _lib.ABI_VERSION == 3
    added = raw[raw.index("ADDED since (still 3"):raw.index("#define CC_ABI_VERSION")]
    assert name in added                                                                   # the list of entry points added without a bump


def test_generated_abi_files_are_current_and_name_it():
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_abi.py"), "--check"]).returncode == 0
    csrc = os.path.join(ROOT, "clipcap_amd", "csrc")
    for f in ("abi_dispatch.cpp", "exports.map", "exports_lab.map"):
        text = open(os.path.join(csrc, f)).read()
        assert all(name in text for name in ENTRY), f
    mk = open(os.path.join(csrc, "Makefile")).read()
    once = next(line for line in mk.splitlines() if line.startswith("SRCS_ONCE"))
    assert "cider.hip" in once                                                             # fp32 / integer work: built once
    assert "cider_table.h" in next(line for line in mk.splitlines() if line.startswith("HDRS"))
    hdr = open(os.path.join(ROOT, "include", "clipcap_hip.h")).read()
    assert "cand_len <= 256, Lr <= 256, Rmax * Lr <= 4096, stop_token < 65535" in hdr       # the limits are written down


def test_argument_errors_need_no_device():
    """Every return code is decided before anything touches the device: the pointers given here are never followed."""
    from clipcap_amd import _lib
    f = _lib.lib().cc_cider_score
    p = [C.c_void_p(4096 * (i + 1)) for i in range(7)]
    nan, inf = float("nan"), float("inf")

    def call(cand=p[0], C_=6, cand_len=20, cand_ld=24, stop=50256, count_stop=0, group=p[1], refs=p[2], G=3, Rmax=5, Lr=30, ref_count=p[3],
             keys=p[4], idf=p[5], cap=1024, log_n=3.0, sigma=6.0, out=p[6]):
        return f(cand, C_, cand_len, cand_ld, stop, count_stop, group, refs, G, Rmax, Lr, ref_count, keys, idf, cap, log_n, sigma, out, None)

    # nothing to score: 0, nothing launched, whatever the pointers and the limits
    assert call(C_=0) == 0 and call(C_=0, cand=None, refs=None, keys=None, idf=None, out=None, group=None, ref_count=None) == 0
    assert call(C_=0, cand_len=300, cand_ld=300) == 0 and call(C_=0, Rmax=100, Lr=100) == 0
    # -1: bad arguments
    for bad in (dict(cand=None), dict(refs=None), dict(keys=None), dict(idf=None), dict(out=None)):
        assert call(**bad) == -1, bad
    assert call(sigma=0.0) == -1 and call(sigma=-6.0) == -1 and call(sigma=nan) == -1 and call(sigma=inf) == -1
    assert call(log_n=nan) == -1 and call(log_n=inf) == -1
    assert call(cap=0) == -1 and call(cap=1000) == -1 and call(cap=-1024) == -1 and call(cap=3) == -1
    assert call(cand_ld=19) == -1 and call(cand_len=-1) == -1 and call(C_=-1) == -1
    assert call(G=0) == -1 and call(Rmax=0) == -1 and call(Lr=0) == -1
    assert call(group=None, C_=7) == -1 and call(group=None, C_=2) == -1                   # no map: C must be a multiple of G
    assert call(C_=0, sigma=nan) == -1 and call(C_=0, cap=12) == -1 and call(C_=0, cand_ld=3) == -1      # a bad argument is one whatever C is
    # -2: beyond the limits
    assert call(cand_len=257, cand_ld=257) == -2 and call(Lr=257, Rmax=1) == -2
    assert call(Rmax=17, Lr=256) == -2 and call(Rmax=4097, Lr=1) == -2 and call(Rmax=65, Lr=64) == -2
    assert call(stop=65535) == -2 and call(stop=70000) == -2
    # the table builder's refusals through the library
    b = _lib.lib().cc_cider_table_build
    keys, idf = np.array([5, 6, 7, 5], np.uint64), np.ones(4, np.float32)
    tk, ti = np.empty(8, np.uint64), np.empty(8, np.float32)
    ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    assert b(ptr(keys), ptr(idf), 3, ptr(tk), ptr(ti), 8) == 0 and sorted(tk[tk != MASK64].tolist()) == [5, 6, 7]
    assert b(ptr(keys), ptr(idf), 4, ptr(tk), ptr(ti), 8) == -1                             # a duplicate
    assert b(ptr(keys), ptr(idf), 3, ptr(tk), ptr(ti), 4) == -1 and b(ptr(keys), ptr(idf), 3, ptr(tk), ptr(ti), 6) == -1
    keys[1] = MASK64
    assert b(ptr(keys), ptr(idf), 3, ptr(tk), ptr(ti), 8) == -1                             # the empty key


def _check_against_dict_count(docs, rw):
    df = cider_ref.doc_freq(docs)
    tk, ti = rw.tab_keys.numpy().view(np.uint64), rw.tab_idf.numpy()
    cap = len(tk)
    assert cap & (cap - 1) == 0 and cap >= 2 * len(df) and (cap == 2 or cap < 4 * len(df))
    assert int((tk != MASK64).sum()) == len(df)                                            # nothing but the corpus's n-grams
    N = len(docs)
    assert rw.n_docs == N and rw.log_ndocs == math.log(N)
    for g, n in df.items():
        want = np.float32(math.log(N) - math.log(max(1.0, float(n))))                      # float64, rounded once
        assert table_find(tk, ti, pack(g), None) == float(want), (g, n)
    return df, tk, ti


def test_from_corpus_counts_as_a_dict_count_does():
    from clipcap_amd.train import CiderReward
    docs = [[[1, 2, 3, 1, 2, 3, 1, 2], [1, 2, 9]],             # repeated n-grams inside one caption and across one document's captions
            [[1, 2, 4], [], [7]],                              # an empty caption; (1, 2) is in every document: idf 0
            [[0, 65534, 1, 2, 65534, 0]],                      # the smallest and the largest token
            [[1, 2], [1, 2], [5, 5, 5, 5, 5, 5]]]
    rw = CiderReward.from_corpus(docs, device="cpu")
    df, tk, ti = _check_against_dict_count(docs, rw)
    assert df[(1, 2)] == 4 and table_find(tk, ti, pack((1, 2)), None) == 0.0 and table_find(tk, ti, pack((1,)), None) == 0.0
    assert df[(1, 2, 3)] == 1 and df[(5, 5)] == 1 and df[(5, 5, 5, 5)] == 1                  # counted once per document, not per occurrence
    assert table_find(tk, ti, pack((3, 3)), "miss") == "miss" and table_find(tk, ti, pack((2, 1, 2)), "miss") == "miss"
    assert rw.sigma == 6.0 and rw.count_stop is False and rw.stop_token == 50256
    # the recorded cases: the reference scorer's own document frequencies
    for case in golden_cases()[:6]:
        docs = [refs for _, refs in case["images"]]
        assert _check_against_dict_count(docs, CiderReward.from_corpus(docs, device="cpu"))[0] == case["df"]
    # count_stop: the stop token is a word of every corpus caption
    rw = CiderReward.from_corpus([[[1, 2]], [[3]]], count_stop=True, stop_token=9, device="cpu")
    _check_against_dict_count([[[1, 2, 9]], [[3, 9]]], rw)


def test_from_corpus_refuses_what_cannot_be_packed():
    from clipcap_amd.train import CiderReward
    for bad in ([[[1, 65535]]], [[[1, 2]], [[70000]]], [[[3, -1]]]):
        with pytest.raises(ValueError, match="65535"):
            CiderReward.from_corpus(bad, device="cpu")
    with pytest.raises(ValueError):
        CiderReward.from_corpus([], device="cpu")
    with pytest.raises(ValueError, match="stop_token"):
        CiderReward.from_corpus([[[1]]], stop_token=65535, device="cpu")
    with pytest.raises(ValueError, match="sigma"):
        CiderReward.from_corpus([[[1]]], sigma=0.0, device="cpu")


def test_engine_cider_score_validates_before_it_touches_a_device():
    from clipcap_amd import engine
    from clipcap_amd.train import CiderReward
    rw = CiderReward.from_corpus([[[1, 2, 3]], [[2, 3, 4]]], device="cpu")
    cand, refs = torch.zeros(4, 10, dtype=torch.int64), torch.zeros(2, 3, 12, dtype=torch.int32)
    score = lambda c=cand, r=refs, **kw: engine.cider_score(c, r, rw.tab_keys, rw.tab_idf, rw.log_ndocs, **kw)  # noqa: E731
    assert score(cand[:0]).shape == (0,)                                                    # nothing to score: no device is needed
    for bad in (lambda: score(cand.int()), lambda: score(cand[0]), lambda: score(r=refs.long()), lambda: score(r=refs[0]),
                lambda: score(torch.zeros(4, 257, dtype=torch.int64)), lambda: score(r=torch.zeros(2, 1, 257, dtype=torch.int32)),
                lambda: score(r=torch.zeros(2, 17, 256, dtype=torch.int32)), lambda: score(stop_token=65535), lambda: score(sigma=0.0),
                lambda: score(sigma=float("nan")), lambda: score(cand[:3]), lambda: score(cand_group=torch.zeros(4, dtype=torch.int64)),
                lambda: score(cand_group=torch.zeros(3, dtype=torch.int32)), lambda: score(ref_count=torch.ones(3, dtype=torch.int32)),
                lambda: score(out=torch.zeros(5)), lambda: score(cand.t()),
                lambda: engine.cider_score(cand, refs, rw.tab_keys[:3], rw.tab_idf[:3], rw.log_ndocs)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError, match="MI355X"):                                       # valid arguments: only then the device matters
        score()


def test_for_batch_pads_and_groups(monkeypatch):
    from clipcap_amd import engine
    from clipcap_amd.train import CiderReward
    seen = {}

    def launch(cand, refs, tab_keys, tab_idf, log_ndocs, **kw):
        seen.update(cand=cand.clone(), refs=refs.clone(), log_ndocs=log_ndocs, **kw)
        return torch.arange(cand.shape[0], dtype=torch.float32)

    monkeypatch.setattr(engine, "cider_score", launch)
    B = 3
    refs = torch.tensor([[[4, 5, 6, -1], [7, -1, -1, -1]], [[1, 2, 3, 4], [-1, -1, -1, -1]], [[9, 9, -1, 3], [2, 2, 2, -1]]], dtype=torch.int32)
    count = torch.tensor([2, 1, 2], dtype=torch.int32)
    sampled = torch.tensor([[5, 6, 8, 0, 0], [1, 8, 3, 3, 3], [2, 2, 2, 2, 8]])
    greedy = torch.tensor([[5, 8], [8, 1], [4, 4]])
    rw = CiderReward.from_corpus([[[4, 5, 6], [7]], [[1, 2, 3, 4]]], stop_token=8, device="cpu")
    r_s, r_g = rw.for_batch(refs, count)(sampled, greedy)
    assert seen["cand"].dtype == torch.int64 and seen["cand"].shape == (2 * B, 5)
    assert torch.equal(seen["cand"][:B], sampled)                                           # candidate c belongs to image c % B
    assert torch.equal(seen["cand"][B:, :2], greedy) and bool((seen["cand"][B:, 2:] == -1).all())
    assert seen["cand_group"] is None and seen["ref_count"] is count and torch.equal(seen["refs"], refs)
    assert seen["stop_token"] == 8 and seen["count_stop"] is False and seen["sigma"] == 6.0 and seen["log_ndocs"] == math.log(2)
    assert torch.equal(r_s, torch.tensor([0.0, 1.0, 2.0])) and torch.equal(r_g, torch.tensor([3.0, 4.0, 5.0]))
    # the wider tensor may be the greedy one
    rw.for_batch(refs)(greedy, sampled)
    assert torch.equal(seen["cand"][B:], sampled) and torch.equal(seen["cand"][:B, :2], greedy) and bool((seen["cand"][:B, 2:] == -1).all())
    assert seen["ref_count"] is None
    # count_stop: the stop token is appended to every reference here (a row ends at its first negative id), not in the kernel
    rw = CiderReward.from_corpus([[[4, 5, 6], [7]], [[1, 2, 3, 4]]], stop_token=8, count_stop=True, device="cpu")
    rw.for_batch(refs, count)(sampled, greedy)
    want = torch.tensor([[[4, 5, 6, 8, -1], [7, 8, -1, -1, -1]], [[1, 2, 3, 4, 8], [8, -1, -1, -1, -1]], [[9, 9, 8, -1, -1], [2, 2, 2, 8, -1]]],
                        dtype=torch.int32)
    assert torch.equal(seen["refs"], want) and seen["count_stop"] is True and seen["refs"].is_contiguous()
    with pytest.raises(ValueError):
        rw.for_batch(refs)(sampled[:2], greedy)
    with pytest.raises(ValueError):
        rw.for_batch(refs.long())
