"""The float64 statement of the diverse-beam-search update (tests/beam_group_ref.py) on the CPU: with one beam group it is the oracle's
beam_update; with a penalty of 0 every beam group is beam_update at the group's width on its own rows; hand cases for the penalty, for a
stopped beam's padding token and for a token picked twice."""
import math

import pytest
import torch

from oracle import clipcap_oracle as O
from tests.beam_group_ref import beam_group_step_ref

STOP = 17


def _state(beam, seed):
    g = torch.Generator().manual_seed(seed)
    scores = -torch.rand(beam, generator=g) * 6.0 - 0.5
    seql = torch.randint(1, 4, (beam,), generator=g).float()
    stopped = torch.zeros(beam, dtype=torch.bool)
    stopped[1::3] = True
    return scores, seql, stopped


@pytest.mark.parametrize("beam,V", [(5, 211), (4, 50257), (1, 97)])
def test_one_beam_group_is_the_oracles_beam_update(beam, V):
    torch.manual_seed(beam * 1000 + V)
    lg = torch.randn(beam, V) * 3.0
    # first step
    r = beam_group_step_ref(lg, None, None, None, beam=beam, groups=1, temperature=0.9, penalty=0.7, first=True, stop_token=STOP)
    nt, _, sc, ln, hs = O.beam_update(lg[:1].clone(), None, torch.ones(beam), torch.zeros(beam, dtype=torch.bool), beam_size=beam, temperature=0.9,
                                      stop_token=STOP)
    assert torch.equal(r.tokens, nt) and torch.equal(r.src, torch.zeros(beam, dtype=torch.int64))
    assert torch.allclose(r.scores.float(), sc, rtol=1e-5, atol=3e-5)            # the tolerance tests/test_gpu_beam.py holds the kernel to
    assert torch.equal(r.lengths.float(), ln) and torch.equal(r.stopped, hs)
    # a later step, with stopped beams
    scores, seql, stopped = _state(beam, beam + V)
    lg[0, STOP] += 25.0
    r = beam_group_step_ref(lg, scores, seql, stopped, beam=beam, groups=1, temperature=0.9, penalty=0.7, stop_token=STOP)
    nt, src, sc, ln, hs = O.beam_update(lg.clone(), scores.clone(), seql.clone(), stopped.clone(), beam_size=beam, temperature=0.9, stop_token=STOP)
    assert torch.equal(r.tokens, nt) and torch.equal(r.src, src)
    assert torch.allclose(r.scores.float(), sc, rtol=1e-5, atol=3e-5)
    assert torch.equal(r.lengths.float(), ln) and torch.equal(r.stopped, hs)
    assert r.stopped.any() and len(r.margins) == 1 and r.margins[0] > 0


@pytest.mark.parametrize("beam,groups,V", [(6, 3, 211), (4, 2, 4099), (4, 4, 130)])
def test_penalty_zero_is_beam_update_per_beam_group(beam, groups, V):
    torch.manual_seed(beam * 100 + groups + V)
    W = beam // groups
    lg = torch.randn(beam, V) * 3.0
    lg[::2, STOP] += 25.0
    scores, seql, stopped = _state(beam, V)
    r = beam_group_step_ref(lg, scores, seql, stopped, beam=beam, groups=groups, temperature=0.9, penalty=0.0, stop_token=STOP)
    for g in range(groups):
        sl = slice(g * W, (g + 1) * W)
        nt, src, sc, ln, hs = O.beam_update(lg[sl].clone(), scores[sl].clone(), seql[sl].clone(), stopped[sl].clone(), beam_size=W, temperature=0.9,
                                            stop_token=STOP)
        assert torch.equal(r.tokens[sl], nt) and torch.equal(r.src[sl], src + g * W), g
        assert torch.allclose(r.scores[sl].float(), sc, rtol=1e-5, atol=3e-5), g
        assert torch.equal(r.lengths[sl].float(), ln) and torch.equal(r.stopped[sl], hs), g
    # first step: every beam group reads row 0 and, without a penalty, finds the same
    f = beam_group_step_ref(lg, None, None, None, beam=beam, groups=groups, temperature=0.9, penalty=0.0, first=True, stop_token=STOP)
    nt, _, sc, _, _ = O.beam_update(lg[:1].clone(), None, torch.ones(W), torch.zeros(W, dtype=torch.bool), beam_size=W, temperature=0.9, stop_token=STOP)
    for g in range(groups):
        assert torch.equal(f.tokens[g * W:(g + 1) * W], nt) and torch.equal(f.scores[g * W:(g + 1) * W], f.scores[:W])
    assert torch.equal(f.src, torch.zeros(beam, dtype=torch.int64)) and torch.allclose(f.scores[:W].float(), sc, rtol=1e-5, atol=3e-5)


def _logp(p):
    return torch.tensor(p, dtype=torch.float64).log().float()      # logits whose softmax is p


def test_hand_case_the_penalty_moves_beam_group_1_off_beam_group_0s_token():
    """V = 6, beam 4 in 2 beam groups whose first rows are alike (the second rows are far behind in score): both beam groups would take
    tokens 2 and 4; with a penalty of 2 beam group 1 loses them (0.40 e^-2 = 0.054, 0.25 e^-2 = 0.034) to tokens 1 (0.15) and 0 (0.10)."""
    p = [0.10, 0.15, 0.40, 0.05, 0.25, 0.05]
    lg = _logp([p, [1 / 6] * 6, p, [1 / 6] * 6])
    scores = torch.tensor([-1.0, -9.0, -1.0, -9.0])
    seql = torch.ones(4)
    stopped = torch.zeros(4, dtype=torch.bool)
    free = beam_group_step_ref(lg, scores, seql, stopped, beam=4, groups=2, penalty=0.0, stop_token=5)
    assert free.tokens.tolist() == [2, 4, 2, 4] and free.src.tolist() == [0, 0, 2, 2]
    r = beam_group_step_ref(lg, scores, seql, stopped, beam=4, groups=2, penalty=2.0, stop_token=5)
    assert r.tokens.tolist() == [2, 4, 1, 0] and r.src.tolist() == [0, 0, 2, 2]
    want = [-1.0 + math.log(q) for q in (0.40, 0.25, 0.15, 0.10)]                # average (-1 + log q) / 2, times the length 2
    assert torch.allclose(r.scores, torch.tensor(want, dtype=torch.float64), atol=1e-6)
    assert r.lengths.tolist() == [2.0] * 4 and not r.stopped.any()
    # decision margins, in halves of log ratios (length 2): beam group 0 keeps 0.40, 0.25 over 0.15; beam group 1 keeps 0.15, 0.10 over 0.054
    assert abs(r.margins[0] - 0.5 * math.log(0.40 / 0.25)) < 1e-6
    assert abs(r.margins[1] - 0.5 * math.log(0.15 / 0.10)) < 1e-6
    # a penalised token that still wins keeps the penalised value in its score: 0.40 e^-0.5 = 0.243 and 0.25 e^-0.5 = 0.1516 > 0.15
    r2 = beam_group_step_ref(lg, scores, seql, stopped, beam=4, groups=2, penalty=0.5, stop_token=5)
    assert r2.tokens.tolist() == [2, 4, 2, 4]
    assert abs(float(r2.scores[2]) - (-1.0 + math.log(0.40) - 0.5)) < 1e-6 and abs(float(r2.scores[3]) - (-1.0 + math.log(0.25) - 0.5)) < 1e-6


def test_a_stopped_beams_padding_token_is_not_counted():
    """Beam group 0 holds a stopped beam, whose continuation is token 0 (padding), and a live beam that picks token 3.  Beam group 1's best
    token is 0: it is penalised only if the padding were counted."""
    V = 5
    lg = torch.zeros(4, V)
    lg[1] = _logp([0.05, 0.05, 0.1, 0.7, 0.1])
    lg[2] = _logp([0.5, 0.1, 0.1, 0.28, 0.02])
    lg[3] = lg[2]
    scores = torch.tensor([-0.1, -1.0, -1.0, -1.0])
    seql = torch.tensor([2.0, 1.0, 1.0, 1.0])
    stopped = torch.tensor([True, False, False, False])
    r = beam_group_step_ref(lg, scores, seql, stopped, beam=4, groups=2, penalty=5.0, stop_token=4)
    assert r.tokens[:2].tolist() == [0, 3] and r.src[:2].tolist() == [0, 1]              # the stopped beam's average -0.05 leads
    assert r.stopped[:2].tolist() == [True, False] and r.lengths[:2].tolist() == [2.0, 2.0]
    assert abs(float(r.scores[0]) - float(scores[0])) < 1e-12                            # the state came in as fp32
    # beam group 1: token 0 (0.5) unpenalised, token 3 (0.28) penalised once -> tokens 0 of both rows win
    assert r.tokens[2:].tolist() == [0, 0] and r.src[2:].tolist() == [2, 3]
    assert abs(float(r.scores[2]) - (-1.0 + math.log(0.5))) < 1e-6


def test_a_token_picked_twice_is_penalised_twice():
    """Beam 3 in 3 beam groups of one: beam groups 0 and 1 both take token 1 (a penalty of 0.2 does not move group 1 off it), and beam
    group 2 sees c(1) = 2: log 0.5 - 0.4 < log 0.35, while one penalty (log 0.5 - 0.2 > log 0.35) would have kept token 1."""
    lg = _logp([[0.1, 0.5, 0.35, 0.05]] * 3)
    scores = torch.tensor([-1.0, -1.0, -1.0])
    seql = torch.ones(3)
    stopped = torch.zeros(3, dtype=torch.bool)
    r = beam_group_step_ref(lg, scores, seql, stopped, beam=3, groups=3, penalty=0.2, stop_token=3)
    assert r.tokens.tolist() == [1, 1, 2] and r.src.tolist() == [0, 1, 2]
    assert abs(float(r.scores[1]) - (-1.0 + math.log(0.5) - 0.2)) < 1e-6
    assert abs(float(r.scores[2]) - (-1.0 + math.log(0.35))) < 1e-6
    # the margin of beam group 2 is the gap token 2 keeps over the twice-penalised token 1, per unit of length 2
    assert abs(r.margins[2] - 0.5 * (math.log(0.35) - (math.log(0.5) - 0.4))) < 1e-6
    # first step: the same from row 0
    f = beam_group_step_ref(lg, None, None, None, beam=3, groups=3, penalty=0.2, first=True, stop_token=3)
    assert f.tokens.tolist() == [1, 1, 2] and f.src.tolist() == [0, 0, 0] and f.lengths.tolist() == [1.0] * 3
