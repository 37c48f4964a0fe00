#!/usr/bin/env python
"""Randomised sweep of the device-side decode bookkeeping against the oracle: cc_beam_step (beam widths 1..10, vocabularies 50..60000,
padded leading dimensions, stop tokens, frozen beams) and cc_sample_step / cc_sample_step_lp (nucleus / top-k / temperature, both filter
conventions, repetition and sentence-length penalties) —
the assertions of tests/test_gpu_beam.py, tests/test_gpu_sample_ref.py (the float64 reference of tests/sample_ref.py: every row is
compared, a cut inside a group of equal values is held to the index-order rule) and tests/test_gpu_sampling.py (the sentence-length
penalty against the oracle) on random parameters.  Not part of the test suite:
    python tools/fuzz_decode_steps.py [seconds] [seed]"""
import os
import random
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import test_gpu_beam as TB


def beam_case(beam, V, ld):
    """tests/test_gpu_beam.py::test_beam_step_matches_oracle, except that a step whose kept candidates are the oracle's in another ORDER
    is accepted when the candidates' average scores agree to 3e-5 (the device's expf / logf differ from the host's by an ulp and the
    reference's fp32 softmax().log() is itself good to ~1e-5; two candidates tied that closely sort either way) — the run stops there, the states having diverged."""
    import torch
    from clipcap_amd.engine import beam_step
    torch.manual_seed(beam * 1000 + V)
    S, temp, stop = 6, 0.9, 17
    R = S * beam
    scores = torch.zeros(R, device="cuda"); seql = torch.ones(R, device="cuda"); stopped = torch.zeros(R, dtype=torch.uint8, device="cuda")
    o_scores, o_seql, o_stopped = torch.zeros(R), torch.ones(R), torch.zeros(R, dtype=torch.bool)
    for step in range(5):
        buf = torch.randn(R, ld, device="cuda") * 3.0
        if step >= 1:
            buf[::3, stop] += 25.0
        lg = buf[:, :V]
        nt, sr = beam_step(lg, S, beam, temp, step == 0, stop, scores, seql, stopped)
        ont, osr = TB._oracle_step(lg.cpu().float(), step == 0, S, beam, temp, stop, o_scores, o_seql, o_stopped)
        torch.cuda.synchronize()
        if torch.equal(nt.cpu().long(), ont) and (step == 0 or torch.equal(sr.cpu().long(), osr)):
            assert torch.allclose(scores.cpu(), o_scores, rtol=1e-5, atol=3e-5), step
            continue
        for s in range(S):
            sl = slice(s * beam, (s + 1) * beam)
            a = sorted(zip(nt[sl].tolist(), (sr[sl].tolist() if step else [0] * beam), (scores[sl] / seql[sl]).tolist()))
            b = sorted(zip(ont[sl].tolist(), (osr[sl].tolist() if step else [0] * beam), (o_scores[sl] / o_seql[sl]).tolist()))
            assert [x[:2] for x in a] == [x[:2] for x in b], (step, s, "different candidates")
            assert all(abs(x[2] - y[2]) <= 3e-5 for x, y in zip(a, b)), (step, s)      # the oracle's fp32 softmax().log() is good to ~1e-5
        return "tie"
    return "exact"


def sample_ref_case(V, scale, top_p, top_k, temperature, mode, hist_len, seed):
    """One launch of 7 random rows (Gaussian at `scale`, one of them on a 0.25 grid, one with a handful of -inf) through every form of the
    call tests/test_gpu_sample_ref.py walks, held to tests/sample_ref.py's check: the kept set at an admissible cut (no row is left out;
    a row with more than one admissible prefix length is counted, not skipped), every probability within its bound, the drawn token in
    its CDF interval.  Returns (rows, rows with more than one admissible length, worst err / bound)."""
    import numpy as np
    from tests import sample_ref as SR
    from tests import test_gpu_sample_ref as TR
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((7, V)) * scale
    x[1] = np.round(x[1] * 4.0) / 4.0
    x[2, rng.choice(V, size=min(5, V - 1), replace=False)] = -np.inf
    hist = None
    if hist_len:
        hist = rng.integers(-1, V + 1, size=(7, hist_len + SR.HIST_PAD)).astype(np.int64)
        hist[:, 1] = hist[:, 0]
    P = SR.Params(temperature=temperature, top_k=top_k, top_p=top_p, mode=mode, rep_pen=1.2 if hist_len else 1.0, hist_len=hist_len)
    c = SR.Case(f"fuzz-V{V}-s{scale:.3f}-p{top_p}-k{top_k}-T{temperature}-m{mode}-h{hist_len}-seed{seed}", "random", x, P, rng.random(7), hist)
    worst, exact = TR.walk(c)
    return c.R, c.R - exact, worst


def length_penalty_case(V, stop, temp, rep, top_p, top_k, want_len, factor, hl, seed):
    """The no_beam step with the sentence-length penalty (cc_sample_step_lp) on rows whose logits sit on a 0.25 grid, so that history tokens
    hit float(stop) exactly now and then (the reference's value comparison, utils.py:40-51), against the oracle's restatement of
    no_beam.py:45-63 (pinned by tests/golden/length_penalty.npz)."""
    import numpy as np
    import torch
    from clipcap_amd.engine import sample_step
    from oracle import clipcap_oracle as O
    gen = torch.Generator().manual_seed(seed)
    lg = (torch.randn(V, generator=gen) * 3.0 + stop * 0.6).mul(4).round().div(4) * temp     # grid values; / temp restores them exactly for temp = 2^k
    hist = torch.randint(0, V, (hl,), generator=gen)
    for t in hist[: max(1, hl // 3)].tolist():
        lg[t] = float(stop) * temp
    pen = (hl / want_len) * factor
    _, probs = sample_step(lg.cuda().unsqueeze(0), torch.tensor([0.5], device="cuda"), temperature=temp, top_k=top_k, top_p=top_p, mode=1,
                           history=hist.cuda().unsqueeze(0), hist_len=hl, repetition_penalty=rep, return_probs=True, length_penalty_stop=stop,
                           length_penalty=pen)
    ref = O.no_beam_step_distribution(lg, hist, top_p=top_p, top_k=top_k, temperature=temp, repetition_penalty=rep, stop_token=stop,
                                      desired_sentence_length=want_len, sentence_length_factor=factor).numpy()
    got = probs[0].cpu().numpy()
    fired = int(((lg[hist] / temp) == stop).sum())
    if np.array_equal(got > 1e-8, ref > 1e-8):
        assert np.abs(got - ref).max() <= 3e-6, np.abs(got - ref).max()
        return fired, "exact"
    # The rows sit on a grid, so the top-k / top-p cut often falls INSIDE a group of equal values: the reference keeps whichever members its
    # sort put first, the device the first in index order.  Then: the kept sets before the penalty must hold the same VALUES,
    # and the device's distribution must be the penalty + softmax applied to ITS kept set.
    _, p0 = sample_step(lg.cuda().unsqueeze(0), torch.tensor([0.5], device="cuda"), temperature=temp, top_k=top_k, top_p=top_p, mode=1,
                        history=hist.cuda().unsqueeze(0), hist_len=hl, repetition_penalty=rep, return_probs=True)
    r0 = O.no_beam_step_distribution(lg, hist, top_p=top_p, top_k=top_k, temperature=temp, repetition_penalty=rep).numpy()
    x = O.repetition_penalty_apply(lg.clone(), hist, rep) if rep != 1.0 else lg.clone()
    x = (x / temp).numpy()
    kd, kr = p0[0].cpu().numpy() > 0, r0 > 0
    big = x >= x.max() - 18.0                                    # 2^-32 fixed point: compare the members that can carry weight
    if not np.array_equal(np.sort(x[kd & big]), np.sort(x[kr & big])):
        # the cumulative mass at the cut is within fp32 rounding of top_p: one side keeps the boundary value's group (or one more member
        # of it), the other does not — every token the two sets disagree on must sit at the cut, i.e. at or below the smallest value both keep
        both = kd & kr & big
        diff = (kd ^ kr) & big
        assert both.any() and x[diff].max() <= x[both].min() + 1e-6 and np.unique(x[diff]).size <= 2, "kept sets differ away from the cut"
    inh = np.zeros(V, dtype=bool)
    inh[hist.numpy()] = True
    y = np.where(kd, np.where(inh & (x == np.float32(stop)), x * np.float32(pen), x), -np.inf).astype(np.float64)
    e = np.exp(y - y.max())
    assert np.abs(got - e / e.sum()).max() <= 3e-6
    return fired, "cut"


def main():
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
    rng = random.Random(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
    t0, n, fails, ties, lp_fired, lp_cut, sr_rows, sr_several, sr_worst = time.time(), 0, [], 0, 0, 0, 0, 0, 0.0
    while time.time() - t0 < budget:
        kind = rng.choice(["beam", "nucleus", "filter", "length"])
        V = rng.choice([rng.randint(50, 400), rng.randint(400, 6000), rng.randint(6000, 60000)])
        try:
            if kind == "beam":
                args = (rng.randint(1, 10), V, V + rng.choice([0, 0, 3, 8, 47]))
                if beam_case(*args) == "tie":
                    ties += 1
            elif kind == "length":
                stop = rng.choice([5, 13, min(V - 1, 40)])
                args = (V, stop, rng.choice([1.0, 0.5, 2.0]), rng.choice([1.0, 1.0, 1.25, 2.0]), rng.choice([0.95, 0.9, 0.7, 0.0]), rng.choice([0, 0, 8, 40]),
                        rng.choice([5, 10, 50]), rng.choice([0.0, 0.5, 1.0, 3.0]), rng.randint(1, 40), rng.randint(0, 1 << 30))
                if args[4] == 0.0 and args[5] == 0:
                    continue                                  # no filter at all: see the 2^-32 note below
                f, how = length_penalty_case(*args)
                lp_fired += f > 0
                lp_cut += how == "cut"
            else:
                k = rng.choice([0, 0, 1, rng.randint(2, 500), V - 1, V, V + 5])
                top_p = rng.choice([0.0, 1.0, round(rng.uniform(0.02, 0.999), 3), round(rng.uniform(0.02, 0.999), 3)])
                args = (V, rng.uniform(1.0, 7.0), top_p, k, round(rng.uniform(0.5, 1.5), 2), 0 if kind == "nucleus" else 1, rng.choice([0, 0, 6, 1500]),
                        rng.randint(0, 1 << 30))
                rows, several, worst = sample_ref_case(*args)
                sr_rows += rows
                sr_several += several
                sr_worst = max(sr_worst, worst)
        except Exception as e:
            fails.append((kind, args))
            print("FAIL", kind, args, repr(e)[:300], flush=True)
        n += 1
    print(f"{n} cases in {time.time() - t0:.0f} s, {len(fails)} failures, {ties} beam steps with a tie below the reference's own rounding sorted the other way; "
          f"sampling: {sr_rows} rows against float64, {sr_several} with more than one admissible prefix length, worst probs_out err / bound {sr_worst:.3f}; "
          f"sentence-length penalty: fired in {lp_fired} rows, {lp_cut} rows compared by mass (top_p cut inside a tie)")
    sys.exit(1 if fails else 0)


if __name__ == "__main__":
    main()
