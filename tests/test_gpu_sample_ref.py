"""cc_sample_step_lp / cc_sample_step (clipcap_amd/csrc/sample.hip: k_sample_rows) through the C ABI against float64 (tests/sample_ref.py):
the kept set at its admissible cuts (exactly one wherever the case list says so: rows of equal candidates, the +-0 rows, grid rows),
every probability within its derived bound, the drawn token inside its float64 CDF interval.

Every call runs on buffers a stray access shows in: the logits have ld = V + 13 with NaN in the padding, the history hist_ld = hist_len + 3
with the row's next-largest tokens beyond hist_len (a read of them would penalise them visibly), probs_out and next_token lie between
guard bands that must come back bit for bit.  Every case is launched twice (bit-identical results: the kernel claims determinism), once
more without probs_out (same tokens, the buffer untouched), — without the sentence-length penalty — through cc_sample_step (the same
bits) and — where the case has no history — with a non-NULL history of the row's largest tokens, hist_len = 0 and a penalty of 1.2
(the same bits: nothing of it may be read).  The poison beyond hist_len can show a stray read only where the history does not already
cover the vocabulary: at hist_len = 1500 with V = 4, 64 or 97 nearly every id is in it, and the larger V carry that check.  The bounds are derived in tests/sample_ref.py, none tuned; tests/test_sample_ref.py shows on the CPU that they reject every
emulated defect at these very cases.  The rows of equal candidates also assert what their exactness rests on: __expf(0) == 1 gives them
probability 1 / n to the few roundings of the normalisation, __expf(-inf) == 0 gives every other token exactly 0."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import sample_ref as R

pytestmark = pytest.mark.gpu

ERR_SHAPE = -2
GUARD = 256
TOKEN_POISON = 0x5A5A5A5A


def _lib():
    from clipcap_amd import _lib
    return _lib.lib()


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.uint8)


class Guarded:
    """a device buffer between two guard bands, all of it poison until written"""

    def __init__(self, n, dt, poison):
        self.poison = poison
        self.flat = torch.full((n + 2 * GUARD,), poison, dtype=dt, device="cuda")
        self.t = self.flat[GUARD:GUARD + n]
        self.ptr = C.c_void_p(self.t.data_ptr())
        self.fresh = self.flat.clone()

    def reset(self):
        self.flat.copy_(self.fresh)

    def guards_intact(self):
        return torch.equal(_bits(self.flat[:GUARD]), _bits(self.fresh[:GUARD])) and torch.equal(_bits(self.flat[-GUARD:]), _bits(self.fresh[-GUARD:]))

    def untouched(self):
        return torch.equal(_bits(self.flat), _bits(self.fresh))


class Call:
    def __init__(self, c):
        self.c = c
        self.logits = torch.from_numpy(c.padded()).cuda()
        self.hist = None if c.hist is None else torch.from_numpy(c.hist).cuda()
        self.u = torch.from_numpy(c.u).cuda()
        self.probs = Guarded(c.R * c.V, torch.float32, float("nan"))
        self.tok = Guarded(c.R, torch.int32, TOKEN_POISON)

    def run(self, probs=True, lp=True, empty_hist=False):
        """-> (rc, tokens [R] numpy, probs [R][V] numpy or None).  empty_hist (a case without history): a history buffer of the rows' largest
        tokens with hist_len = 0 and a repetition penalty of 1.2"""
        c, P = self.c, self.c.P
        self.probs.reset()
        self.tok.reset()
        hist, rep = self.hist, float(P.rep_pen)
        if empty_hist:
            assert self.hist is None and P.hist_len == 0
            top = np.argsort(-c.x, axis=1, kind="stable")[:, :c.hist_ld]
            hist, rep = torch.from_numpy(np.ascontiguousarray(np.resize(top, (c.R, c.hist_ld)), dtype=np.int64)).cuda(), 1.2
        head = (C.c_void_p(self.logits.data_ptr()), c.R, c.V, c.ld, P.temperature, P.top_k, float(P.top_p), P.mode,
                None if hist is None else C.c_void_p(hist.data_ptr()), P.hist_len, c.hist_ld, rep)
        tail = (C.c_void_p(self.u.data_ptr()), self.tok.ptr, self.probs.ptr if probs else None, _st())
        if lp:
            rc = _lib().cc_sample_step_lp(*head, P.stop_tok, float(P.len_pen), *tail)
        else:
            rc = _lib().cc_sample_step(*head, *tail)
        torch.cuda.synchronize()
        assert self.probs.guards_intact() and self.tok.guards_intact(), f"{c.name}: a guard band changed"
        return rc, self.tok.t.cpu().numpy().copy(), (self.probs.t.view(c.R, c.V).cpu().numpy().copy() if probs else None)


def walk(c):
    """one case through every form of the call -> (worst err / bound, rows decided exactly)"""
    x = Call(c)
    rc, tok, probs = x.run()
    assert rc == 0, (c.name, rc)
    worst, exact = R.check_case(c, tok, probs)
    rc, tok2, probs2 = x.run()
    assert rc == 0 and np.array_equal(tok, tok2) and np.array_equal(probs.view(np.uint32), probs2.view(np.uint32)), f"{c.name}: two launches differ"
    rc, tok3, _ = x.run(probs=False)
    assert rc == 0 and np.array_equal(tok, tok3), f"{c.name}: tokens without probs_out {tok3}, with {tok}"
    assert x.probs.untouched(), f"{c.name}: probs_out written though NULL was passed"
    R.check_case(c, tok3, None)
    if c.P.stop_tok < 0:
        rc, tok4, probs4 = x.run(lp=False)
        assert rc == 0 and np.array_equal(tok, tok4) and np.array_equal(probs.view(np.uint32), probs4.view(np.uint32)), f"{c.name}: cc_sample_step differs"
    if c.hist is None:
        rc, tok5, probs5 = x.run(empty_hist=True)
        assert rc == 0 and np.array_equal(tok, tok5) and np.array_equal(probs.view(np.uint32), probs5.view(np.uint32)), f"{c.name}: a history of length 0 was read"
    return worst, exact


GROUPS = ("exact-m0", "exact-m1", "draw", "zero", "random-m0", "random-m1", "length", "order")


def _group(c):
    return f"{c.kind}-m{c.P.mode}" if c.kind in ("exact", "random") else c.kind


def test_every_case_belongs_to_a_group_that_runs():
    assert {_group(c) for c in R.all_cases()} == set(GROUPS)


@pytest.mark.parametrize("group", GROUPS)
def test_sampling_step_against_float64(group):
    cases = [c for c in R.all_cases() if _group(c) == group]
    assert cases
    worst, exact, rows = 0.0, 0, 0
    for c in cases:
        w, e = walk(c)
        if c.kind in ("exact", "draw", "zero", "order"):
            assert e == c.R, c.name
        worst, exact, rows = max(worst, w), exact + e, rows + c.R
    print(f"{group}: {len(cases)} launches x 4 or 5, {rows} rows, {exact} decided exactly; worst probs_out err / bound {worst:.6f}")


def test_equal_candidates_get_exactly_equal_probabilities():
    """what delta = 0 rests on, asserted and not assumed: n tokens at the row maximum, everything else -inf: each weight is S exactly
    (__expf(0) == 1), every other weight 0 (__expf(-inf) == 0); p = fl(S * fl(1 / fl(n S))), within 7 roundings of 1 / n"""
    c = R.by_name("exact-V4099-k3-m1")                           # mode 1 keeps every tie of the third value: all n
    _, _, probs = Call(c).run()
    worst = 0.0
    for r, ref in enumerate(c.refs()):
        n = int(np.isfinite(c.x[r]).sum())
        kept = probs[r][np.isfinite(c.x[r])]
        bound = 7 * R.U32 * 1.02 / n
        assert np.all(kept == kept[0]) and abs(float(kept[0]) - 1.0 / n) <= bound, (r, n, kept[0])
        assert not np.any(probs[r][~np.isfinite(c.x[r])])
        worst = max(worst, abs(float(kept[0]) - 1.0 / n) / bound)
    print(f"{c.name}: {c.R} rows, {sum(ref.exact for ref in c.refs())} decided exactly; worst |p - 1 / n| / bound {worst:.4f}")


def test_lds_edge_runs_and_one_more_token_is_refused():
    c = R.lds_edge()
    assert R.lds_bytes(c.V) <= R.LDS_LIMIT < R.lds_bytes(c.V + 1)
    w, e = walk(c)
    assert e == 1
    print(f"{c.name}: {R.lds_bytes(c.V)} bytes of LDS, {e} row decided exactly; worst probs_out err / bound {w:.4f}")
    V = c.V + 1
    big = R.Case("lds-refused", "exact", np.concatenate([c.x, np.full((1, 1), 1.5, dtype=np.float32)], axis=1), c.P, c.u)
    assert big.V == V
    x = Call(big)
    rc, _, _ = x.run()
    assert rc == ERR_SHAPE, rc
    assert x.probs.untouched() and x.tok.untouched()
