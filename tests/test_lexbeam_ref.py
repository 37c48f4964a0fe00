"""The float64 statement of lexically constrained beam search (tests/lexbeam_ref.py) on the CPU: the transition on hand-written cases, one
allocation worked by hand, no phrases = the plain beam update, the consequences of the rule on random decodes, best_constrained_beams on a
stub, and clipcap_amd/csrc/lex_state.h on its own — tests/lex_state_check.cpp includes only that header and is compiled with the host
compiler and no HIP include path, plainly and with -fsanitize=address,undefined, and run directly on values this statement printed."""
import itertools
import math
import os
import shutil
import subprocess

import pytest
import torch

from oracle import clipcap_oracle as O
from tests.beam_group_ref import beam_group_step_ref
from tests.lexbeam_ref import clean, full_mask, lex_next, lex_step_ref, pack, phrase_table, tokens_met, unpack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
STOP = 9
NONE = -1


# ---- the transition ------------------------------------------------------------------------------------------------------------------------
def test_packing():
    assert pack(0, NONE, 0) == 0 and pack(0b101, 2, 3) == 0b101 | 3 << 8 | 3 << 12 and unpack(pack(0xFF, 7, 7)) == (0xFF, 7, 7)
    assert unpack(0) == (0, NONE, 0)


def test_progress_completion_and_a_drop():
    ph = [[4, 5, 6]]
    s1 = lex_next(0, 4, ph)
    s2 = lex_next(s1, 5, ph)
    s3 = lex_next(s2, 6, ph)
    assert unpack(s1) == (0, 0, 1) and unpack(s2) == (0, 0, 2) and unpack(s3) == (1, NONE, 0)
    assert [tokens_met(s, ph) for s in (0, s1, s2, s3)] == [0, 1, 2, 3]
    assert lex_next(s2, 7, ph) == 0 and tokens_met(lex_next(s2, 7, ph), ph) == 0          # the progress is dropped
    assert lex_next(s3, 4, ph) == s3                                                      # a met phrase does not start again
    assert unpack(lex_next(s2, 4, ph)) == (0, 0, 1)                                       # a drop whose token is the phrase's own first token
    assert lex_next(s2, 5, ph) == 0                                                       # no fallback to a shorter partial match


def test_a_drop_whose_token_restarts_another_phrase():
    ph = [[4, 5, 6], [7, 8]]
    s = lex_next(lex_next(0, 4, ph), 5, ph)
    assert unpack(lex_next(s, 7, ph)) == (0, 1, 1)
    assert unpack(lex_next(lex_next(s, 7, ph), 8, ph)) == (0b10, NONE, 0)


def test_two_phrases_with_one_first_token_the_lowest_index_wins():
    ph = [[4, 5], [4, 6]]
    assert unpack(lex_next(0, 4, ph)) == (0, 0, 1)
    assert lex_next(lex_next(0, 4, ph), 6, ph) == 0                                        # phrase 1 was not tracked: dropped
    met0 = lex_next(lex_next(0, 4, ph), 5, ph)
    assert unpack(met0) == (0b01, NONE, 0) and unpack(lex_next(met0, 4, ph)) == (0b01, 1, 1)   # phrase 0 met: now 4 starts phrase 1
    assert unpack(lex_next(lex_next(met0, 4, ph), 6, ph)) == (0b11, NONE, 0)


def test_a_one_token_phrase_and_a_phrase_that_does_not_exist():
    ph = [[3], [], [-1, 2], [5, 6]]
    assert clean(ph) == [[3], [], [], [5, 6]] and full_mask(ph) == 0b1001
    assert unpack(lex_next(0, 3, ph)) == (0b0001, NONE, 0) and tokens_met(lex_next(0, 3, ph), ph) == 1
    assert lex_next(0, 2, ph) == 0
    mid = lex_next(0, 5, ph)
    assert unpack(lex_next(mid, 3, ph)) == (0b0001, NONE, 0)                               # a one-token phrase met while another one drops


def test_a_phrase_needed_twice_because_a_shorter_phrase_shares_its_token():
    """[4] and [4, 5]: the first 4 meets phrase 0; only a second 4 can begin phrase 1."""
    ph = [[4], [4, 5]]
    a = lex_next(0, 4, ph)
    assert unpack(a) == (0b01, NONE, 0) and unpack(lex_next(a, 5, ph)) == (0b01, NONE, 0)
    b = lex_next(a, 4, ph)
    assert unpack(b) == (0b01, 1, 1) and unpack(lex_next(b, 5, ph)) == (0b11, NONE, 0)
    assert tokens_met(lex_next(b, 5, ph), ph) == 3


# ---- one allocation by hand ----------------------------------------------------------------------------------------------------------------
def test_allocation_by_hand_three_banks_beam_4():
    """V = 10, phrases [1, 2] and [3].  Parents: row 0 nothing met; row 1 has met [3] (bank 1); row 2 is one token into [1, 2] (bank 1);
    row 3 has stopped with both met (bank 3).  Equal lengths and scores, so a candidate's value orders as its log-probability."""
    ph = [[1, 2], [3]]
    V, beam = 10, 4
    lg = torch.full((beam, V), -4.0)
    lg[0, 5], lg[0, 6] = 3.0, 2.5              # row 0: its two best tokens advance nothing (bank 0); 1 and 3 are poor (-4)
    lg[1, 7] = 3.0                             # row 1: best 7 (bank 1), first token 1 of its unmet phrase poor
    lg[2, 2], lg[2, 8] = 0.0, 3.0              # row 2: 2 completes [1, 2] (bank 2), its best 8 drops the progress (bank 0)
    scores = torch.tensor([-2.0, -2.0, -2.0, -0.3])
    seql = torch.tensor([2.0, 2.0, 2.0, 3.0])
    stopped = torch.tensor([False, False, False, True])
    states = [0, pack(0b10, NONE, 0), pack(0, 0, 1), pack(0b11, NONE, 0)]
    r = lex_step_ref(lg, scores, seql, stopped, states, beam=beam, phrases=ph, stop_token=STOP)
    # T = (3, 0), (1, 7), (2, 8), (0, 5); every row's best is among them.  The banks of K, best first:
    #   3: (3, 0) | 2: (2, 2), (1, 1) | 1: (1, 7), (2, 1), (2, 3), (0, 1), (0, 3) | 0: (2, 8), (0, 5)
    # round 1: banks 3, 2, 1, 0 give (3, 0), (2, 2), (1, 7), (2, 8); (0, 6), row 0's second best, is in no set
    assert list(zip(r.src.tolist(), r.tokens.tolist())) == [(3, 0), (2, 2), (1, 7), (2, 8)]
    assert [unpack(int(s)) for s in r.states] == [(0b11, NONE, 0), (0b01, NONE, 0), (0b10, NONE, 0), (0, NONE, 0)]
    assert [tokens_met(int(s), ph) for s in r.states] == [3, 2, 1, 0]
    assert r.stopped.tolist() == [True, False, False, False] and r.lengths.tolist() == [3.0, 3.0, 3.0, 3.0]
    assert math.isclose(float(r.scores[0]), float(scores[3]), abs_tol=1e-12)               # (score / 3) * 3
    lp = torch.log_softmax(lg.double(), -1)
    assert math.isclose(float(r.scores[1]), -2.0 + float(lp[2, 2]), abs_tol=1e-12)
    # with beam 6 the second round goes on: bank 2 gives (1, 1); bank 1 gives (2, 1), which ties with (2, 3) and has the lower flat index
    pad = lambda t, fill: torch.cat((t, torch.full((2,), fill, dtype=t.dtype)))  # noqa: E731
    lg6 = torch.cat((lg, torch.full((2, V), float("-inf"))))
    r6 = lex_step_ref(lg6, pad(scores, float("-inf")), pad(seql, 1.0), pad(stopped, True), states + [0, 0], beam=6, phrases=ph, stop_token=STOP)
    assert list(zip(r6.src.tolist(), r6.tokens.tolist())) == [(3, 0), (2, 2), (1, 7), (2, 8), (1, 1), (2, 1)]
    assert tokens_met(int(r6.states[4]), ph) == 2 and tokens_met(int(r6.states[5]), ph) == 1


def test_the_stop_token_waits_for_every_phrase_and_the_softmax_keeps_it():
    ph = [[1]]
    lg = torch.zeros(2, 6)
    lg[:, 5] = 9.0                                                                          # the stop token dominates
    r = lex_step_ref(lg, None, None, None, None, beam=2, phrases=ph, first=True, stop_token=5)
    assert 5 not in r.tokens.tolist() and int(r.tokens[0]) == 1 and tokens_met(int(r.states[0]), ph) == 1
    lp = torch.log_softmax(lg[0].double(), -1)
    assert math.isclose(float(r.scores[0]), float(lp[1]), abs_tol=1e-12) and float(lp[1]) < -9.0   # the denominator holds exp(9)
    r2 = lex_step_ref(lg, r.scores, r.lengths, r.stopped, r.states, beam=2, phrases=ph, stop_token=5)
    assert (int(r2.src[0]), int(r2.tokens[0])) == (0, 5) and bool(r2.stopped[0])            # row 0 has met it and may stop now
    assert all(unpack(int(s))[0] == 1 for s, st in zip(r2.states, r2.stopped) if st)


def test_an_empty_slot_is_defined_and_stays_empty():
    lg = torch.full((3, 8), float("-inf"))
    lg[0, 2] = 1.0
    r = lex_step_ref(lg, None, None, None, None, beam=3, phrases=[[2, 3]], first=True, stop_token=7)
    assert r.tokens.tolist() == [2, 0, 0] and r.src.tolist() == [0, 0, 0] and r.scores.tolist()[1:] == [-math.inf] * 2
    assert r.stopped.tolist() == [False, True, True] and r.states.tolist() == [pack(0, 0, 1), 0, 0] and r.lengths.tolist() == [1.0] * 3
    lg2 = torch.zeros(3, 8)
    r2 = lex_step_ref(lg2, r.scores, r.lengths, r.stopped, r.states, beam=3, phrases=[[2, 3]], stop_token=7)
    assert int(r2.tokens[0]) == 3 and r2.scores.tolist()[1:] != [-math.inf] * 2            # row 0's other continuations fill the slots
    assert all(int(s) == 0 for s in r2.src)


# ---- no phrases: the plain beam update -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beam,V", [(5, 211), (4, 4099), (1, 97)])
@pytest.mark.parametrize("phrases", [[], [[], [-1, 3]]], ids=["none", "table-of-minus-one"])
def test_no_phrases_is_the_plain_beam_update(beam, V, phrases):
    """Against the float64 statement of the plain update (beam_group_step_ref with one beam group, which tests/test_beam_group_ref.py pins to
    the oracle's beam_update) and against the oracle's beam_update itself."""
    torch.manual_seed(beam * 1000 + V)
    lg = torch.randn(beam, V) * 3.0
    r = lex_step_ref(lg, None, None, None, None, beam=beam, phrases=phrases, temperature=0.9, first=True, stop_token=STOP)
    w = beam_group_step_ref(lg, None, None, None, beam=beam, groups=1, temperature=0.9, first=True, stop_token=STOP)
    assert torch.equal(r.tokens, w.tokens) and torch.equal(r.src, w.src) and torch.equal(r.scores, w.scores)
    assert torch.equal(r.lengths, w.lengths) and torch.equal(r.stopped, w.stopped) and not r.states.any()
    g = torch.Generator().manual_seed(beam + V)
    scores = -torch.rand(beam, generator=g) * 6.0 - 0.5
    seql = torch.randint(1, 4, (beam,), generator=g).float()
    stopped = torch.zeros(beam, dtype=torch.bool)
    stopped[1::3] = True
    lg[0, STOP] += 25.0
    r = lex_step_ref(lg, scores, seql, stopped, [0] * beam, beam=beam, phrases=phrases, temperature=0.9, stop_token=STOP)
    w = beam_group_step_ref(lg, scores, seql, stopped, beam=beam, groups=1, temperature=0.9, stop_token=STOP)
    assert torch.equal(r.tokens, w.tokens) and torch.equal(r.src, w.src) and torch.equal(r.scores, w.scores)
    assert torch.equal(r.lengths, w.lengths) and torch.equal(r.stopped, w.stopped) and not r.states.any()
    assert math.isclose(r.margin, w.margins[0], rel_tol=0, abs_tol=0) and r.margin > 0
    nt, src, sc, ln, hs = O.beam_update(lg.clone(), scores.clone(), seql.clone(), stopped.clone(), beam_size=beam, temperature=0.9, stop_token=STOP)
    assert torch.equal(r.tokens, nt) and torch.equal(r.src, src) and torch.equal(r.stopped, hs) and torch.equal(r.lengths.float(), ln)
    assert torch.allclose(r.scores.float(), sc, rtol=1e-5, atol=3e-5)


# ---- the consequences of the rule on random decodes ------------------------------------------------------------------------------------------
def _random_phrases(g, n, V, stop):
    out = []
    while len(out) < n:
        p = [int(t) for t in torch.randint(0, V, (int(torch.randint(1, 5, (1,), generator=g)),), generator=g)]
        if stop not in p and p not in out:
            out.append(p)
    return out


@pytest.mark.parametrize("seed", range(40))
def test_consequences_on_random_decodes(seed):
    g = torch.Generator().manual_seed(seed)
    V = int(torch.randint(12, 41, (1,), generator=g))
    beam = int(torch.randint(1, 7, (1,), generator=g))
    n_phr = int(torch.randint(0, 5, (1,), generator=g))
    stop = int(torch.randint(0, V, (1,), generator=g))
    ph = _random_phrases(g, n_phr, V, stop)
    total, full = sum(len(p) for p in ph), full_mask(ph)
    scores = seql = stopped = states = None
    for i in range(total + 6):
        lg = torch.randn(beam, V, generator=g) * 2.0
        if i >= 2:
            lg[::2, stop] += 5.0
        r = lex_step_ref(lg, scores, seql, stopped, states, beam=beam, phrases=ph, first=i == 0, stop_token=stop)
        live = r.scores > float("-inf")
        met = [tokens_met(int(s), ph) for s in r.states]
        assert met[0] == max(m for m, ok in zip(met, live) if ok)                            # slot 0 has the most
        assert met[0] >= min(i + 1, total), (i, met, ph)                                    # one more constraint token every step
        for k in range(beam):
            if live[k] and r.stopped[k]:
                assert unpack(int(r.states[k]))[0] == full                                  # stopped only with every phrase produced
            if not live[k]:
                assert int(r.tokens[k]) == 0 and int(r.src[k]) == 0 and int(r.states[k]) == 0 and bool(r.stopped[k])
        if n_phr == 0:                                                                      # one bank: the plain update
            w = beam_group_step_ref(lg, scores, seql, stopped, beam=beam, groups=1, first=i == 0, stop_token=stop)
            assert torch.equal(r.tokens, w.tokens) and torch.equal(r.src, w.src) and torch.equal(r.scores, w.scores)
        scores, seql, stopped, states = r.scores, r.lengths, r.stopped, r.states


# ---- the order of the returned beams --------------------------------------------------------------------------------------------------------
def test_best_constrained_beams_on_a_stub():
    from clipcap_amd.inference.lexical import best_constrained_beams
    scores = torch.tensor([[-1.0, -0.5, -0.5, -3.0], [-2.0, -2.0, -2.0, -2.0], [-4.0, -3.0, -2.0, -1.0]])
    met = torch.tensor([[3, 1, 3, 3], [0, 2, 2, 1], [1, 1, 1, 1]], dtype=torch.int32)
    assert best_constrained_beams(scores, met, 1).tolist() == [[2], [1], [3]]
    assert best_constrained_beams(scores, met, 4).tolist() == [[2, 0, 3, 1], [1, 2, 3, 0], [3, 2, 1, 0]]
    assert best_constrained_beams(scores, met, 2).tolist() == [[2, 0], [1, 2], [3, 2]]


# ---- lex_state.h alone -----------------------------------------------------------------------------------------------------------------------
def _cases_file(path):
    """Every state of a small phrase table (every met mask; no phrase in progress, or any unmet existing phrase at any position inside it)
    with every token of the vocabulary and one id on either side of it: the transition and tokens_met as the Python statement gives them."""
    ph = [[4, 5, 6], [4], [], [7, 4, 5, 2, 1, 0, 3, 8], [5, 4]]
    V, n_phr, phr_len = 10, len(ph), 8
    lines = []
    for met in range(1 << n_phr):
        if met & ~full_mask(ph):
            continue
        states = [pack(met, NONE, 0)] + [pack(met, c, pos) for c, p in enumerate(ph) if p and not met >> c & 1 for pos in range(1, len(p))]
        for s, v in itertools.product(states, range(-1, V + 1)):
            lines.append(f"{s} {v} {lex_next(s, v, ph)} {tokens_met(s, ph)}")
    table = phrase_table(ph, n_phr, phr_len).view(-1).tolist()
    with open(path, "w") as f:
        f.write(f"{n_phr} {phr_len} {V}\n{' '.join(map(str, table))}\n{len(lines)}\n" + "\n".join(lines) + f"\n{full_mask(ph)}\n")
    return len(lines)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_state_header_alone(tmp_path, sanitize):
    assert CXX, "no host C++ compiler"
    exe, cases = str(tmp_path / "lex_state_check"), str(tmp_path / "cases.txt")
    n = _cases_file(cases)
    assert n >= 1000                                                                        # 96 states x 12 ids
    flags = ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-g", "-I", os.path.join(ROOT, "clipcap_amd", "csrc")]
    # (the sanitizer runtimes linked statically: the program does not depend on the order in which shared libraries are loaded)
    static = ["-static-libasan", "-static-libubsan"] if "g++" in os.path.basename(CXX) and "clang" not in os.path.basename(CXX) else ["-static-libsan"]
    flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static] if sanitize else []
    subprocess.run([CXX, *flags, os.path.join(ROOT, "tests", "lex_state_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe, cases], capture_output=True, text=True)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1].startswith(f"ok: {n} transitions")
