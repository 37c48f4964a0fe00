"""cc_beam_step (the device-side beam update of generate_beam, reference inference/base.py:82-119) against the oracle's beam_update
at GPT-2's vocabulary size: first step, later steps with stopped beams, compile-time (1-5, 8) and run-time beam widths, a padded
leading dimension, and the all-ties case (lowest flat index wins; also the overflow path of the candidate list)."""
import pytest
import torch

from clipcap_amd.engine import beam_step
from oracle import clipcap_oracle as O

pytestmark = pytest.mark.gpu


def _oracle_step(lg, first, S, beam, temp, stop, scores, seql, stopped):
    V = lg.shape[1]
    nts, srcs = [], []
    for s in range(S):
        sl = slice(s * beam, (s + 1) * beam)
        if first:
            nt, src, sc, ln, hs = O.beam_update(lg[s * beam:s * beam + 1].clone(), None, seql[sl].clone(), stopped[sl].clone(), beam_size=beam,
                                                temperature=temp, stop_token=stop)
            src = torch.zeros(beam, dtype=torch.int64)
        else:
            nt, src, sc, ln, hs = O.beam_update(lg[sl].clone(), scores[sl].clone(), seql[sl].clone(), stopped[sl].clone(), beam_size=beam,
                                                temperature=temp, stop_token=stop)
        scores[sl], seql[sl], stopped[sl] = sc, ln, hs
        nts.append(nt)
        srcs.append(src)
    return torch.cat(nts), torch.cat(srcs)


@pytest.mark.parametrize("beam,V,ld", [(5, 50257, 50304), (3, 50257, 50257), (7, 4099, 4104), (8, 1001, 1001), (1, 50257, 50304)])
def test_beam_step_matches_oracle(beam, V, ld):
    torch.manual_seed(beam * 1000 + V)
    S, temp, stop = 6, 0.9, 17
    R = S * beam
    scores = torch.zeros(R, device="cuda")
    seql = torch.ones(R, device="cuda")
    stopped = torch.zeros(R, dtype=torch.uint8, device="cuda")
    o_scores, o_seql, o_stopped = torch.zeros(R), torch.ones(R), torch.zeros(R, dtype=torch.bool)
    for step in range(5):
        buf = torch.randn(R, ld, device="cuda") * 3.0
        if step >= 1:
            buf[::3, stop] += 25.0                     # some beams pick the stop token and freeze
        lg = buf[:, :V]
        nt, sr = beam_step(lg, S, beam, temp, step == 0, stop, scores, seql, stopped)
        ont, osr = _oracle_step(lg.cpu().float(), step == 0, S, beam, temp, stop, o_scores, o_seql, o_stopped)
        torch.cuda.synchronize()
        assert torch.equal(nt.cpu().long(), ont), step
        if step > 0:
            assert torch.equal(sr.cpu().long(), osr), step
        # the oracle follows the reference's fp32 `softmax(-1).log()`, which is itself only good to ~1e-5 (a random sweep found a 1.2e-5
        # row); the kernel's first-step scores are checked against fp64 below
        assert torch.allclose(scores.cpu(), o_scores, rtol=1e-5, atol=3e-5), step
        if step == 0:
            exact = torch.log_softmax(lg.double().cpu()[::beam] / temp, -1).topk(beam, -1).values.reshape(-1)
            assert (scores.cpu().double() - exact).abs().max().item() <= 2e-6
        assert torch.equal(seql.cpu(), o_seql) and torch.equal(stopped.cpu().bool(), o_stopped), step
    assert o_stopped.any()


@pytest.mark.parametrize("beam", [5, 6])
def test_beam_step_all_ties_lowest_flat_index(beam):
    S, V = 3, 50257
    R = S * beam
    scores = torch.zeros(R, device="cuda")
    seql = torch.ones(R, device="cuda")
    stopped = torch.zeros(R, dtype=torch.uint8, device="cuda")
    lg = torch.zeros(R, V, device="cuda")
    nt, sr = beam_step(lg, S, beam, 1.0, True, 50256, scores, seql, stopped)
    assert nt.view(S, beam).cpu().tolist() == [list(range(beam))] * S
    nt, sr = beam_step(lg, S, beam, 1.0, False, 50256, scores, seql, stopped)
    assert nt.view(S, beam).cpu().tolist() == [list(range(beam))] * S and sr.view(S, beam).cpu().tolist() == [[0] * beam] * S


def test_beam_advance_matches_indexing():
    """cc_beam_advance = tokens[src] ++ next, wte[next], ancestry rows gathered (base.py:104-117), against plain tensor indexing."""
    from clipcap_amd.engine import DecodeSession
    from clipcap_amd.model.gpt2 import GPT2LM
    torch.manual_seed(3)
    lm = GPT2LM(n_embd=64, n_layer=1, n_head=4, vocab_size=211, n_positions=32).to("cuda")
    wte = lm.get_input_embeddings().weight.detach()
    S, beam, n = 3, 4, 9
    R = S * beam
    sess = DecodeSession(lm.engine, R, 20)
    sess.forward(torch.randn(R, 6, 64, device="cuda"))
    sess.row_map[:, :6] = torch.randint(0, R, (R, 6), dtype=torch.int32, device="cuda")
    before = sess.row_map.clone()
    tin = torch.randint(0, 211, (R, n), dtype=torch.int32, device="cuda")
    tout = torch.full((R, n), -7, dtype=torch.int32, device="cuda")
    nxt = torch.randint(0, 211, (R,), dtype=torch.int32, device="cuda")
    src = torch.randint(0, beam, (R,), dtype=torch.int32, device="cuda")
    x = torch.empty(R, 1, 64, device="cuda")
    sess.beam_advance(beam, nxt, src, wte, 5, tin, tout, x)
    g = ((torch.arange(R, device="cuda") // beam) * beam + src).long()
    assert torch.equal(tout[:, :5], tin[g, :5]) and torch.equal(tout[:, 5], nxt) and (tout[:, 6:] == -7).all()
    assert torch.equal(x.view(R, 64), wte[nxt.long()])
    assert torch.equal(sess.row_map[:, :6], before[g, :6])
    assert torch.equal(sess.row_map[:, 6:], torch.arange(R, dtype=torch.int32, device="cuda").view(R, 1).expand(R, 14))


def _partials(lg, V):
    """what the decode lm_head epilogue writes (gemm.hip.h EpiLogits): per (row, 64-column block) max and sum of exp(x - max)"""
    R = lg.shape[0]
    npart = (V + 63) // 64
    pad = torch.full((R, npart * 64), float("-inf"), device=lg.device)
    pad[:, :V] = lg[:, :V]
    blk = pad.view(R, npart, 64)
    pmax = blk.max(dim=2).values
    psum = torch.exp(blk - pmax[:, :, None]).sum(dim=2)
    return (torch.cat((pmax.reshape(-1), psum.reshape(-1))).contiguous(), npart)


@pytest.mark.parametrize("beam,V,ld", [(5, 50257, 50304), (3, 50257, 50257), (8, 1001, 1001), (1, 50257, 50304), (4, 130, 136)])
def test_beam_step_from_partials_matches_oracle(beam, V, ld):
    """cc_beam_step_p: the one-launch update driven by the lm_head epilogue's partials (temperature 1) — same tokens, source rows,
    scores, lengths and stop flags as the oracle, through stopped beams."""
    torch.manual_seed(beam * 77 + V)
    S, stop = 6, 17
    R = S * beam
    scores = torch.zeros(R, device="cuda")
    seql = torch.ones(R, device="cuda")
    stopped = torch.zeros(R, dtype=torch.uint8, device="cuda")
    o_scores, o_seql, o_stopped = torch.zeros(R), torch.ones(R), torch.zeros(R, dtype=torch.bool)
    for step in range(5):
        buf = torch.randn(R, ld, device="cuda") * 3.0
        if step >= 1:
            buf[::3, stop] += 25.0
        lg = buf[:, :V]
        nt, sr = beam_step(lg, S, beam, 1.0, step == 0, stop, scores, seql, stopped, None, _partials(lg, V))
        ont, osr = _oracle_step(lg.cpu().float(), step == 0, S, beam, 1.0, stop, o_scores, o_seql, o_stopped)
        torch.cuda.synchronize()
        assert torch.equal(nt.cpu().long(), ont), step
        if step > 0:
            assert torch.equal(sr.cpu().long(), osr), step
        assert torch.allclose(scores.cpu(), o_scores, rtol=1e-5, atol=3e-5), step
        assert torch.equal(seql.cpu(), o_seql) and torch.equal(stopped.cpu().bool(), o_stopped), step
    assert o_stopped.any()


def test_beam_step_from_partials_all_ties_takes_the_exact_overflow_path():
    S, V, beam = 3, 50257, 5
    R = S * beam
    scores = torch.zeros(R, device="cuda")
    seql = torch.ones(R, device="cuda")
    stopped = torch.zeros(R, dtype=torch.uint8, device="cuda")
    lg = torch.zeros(R, V, device="cuda")
    part = _partials(lg, V)
    nt, sr = beam_step(lg, S, beam, 1.0, True, 50256, scores, seql, stopped, None, part)
    assert nt.view(S, beam).cpu().tolist() == [list(range(beam))] * S
    nt, sr = beam_step(lg, S, beam, 1.0, False, 50256, scores, seql, stopped, None, part)
    assert nt.view(S, beam).cpu().tolist() == [list(range(beam))] * S and sr.view(S, beam).cpu().tolist() == [[0] * beam] * S


# ---- plateau logits: the overflow paths of the candidate lists (clipcap_amd/csrc/beam.hip) at the smallest shape that reaches them ----
# V = 4099, beam 5: a later step has 5 * 4099 candidates = 1 281 per chunk of k_beam_partial (> its list of 1 024, so the per-thread
# sorted lists take over) and 5 * 65 = 325 (row, 64-column block) bounds in k_beam_fused (<= its 512 survivors, while the candidates of
# the surviving blocks overflow its list of 1 024: the full-scan path).  On a first step a chunk holds 257 candidates: only k_beam_fused
# overflows there.
PL_S, PL_BEAM, PL_V, PL_LD, PL_STOP = 2, 5, 4099, 4104, 777


def _plateau_case(first):
    """-> logits (R, ld) fp32 CPU and the hand-set state (scores, seq_lengths, stopped).  Every row is constant but for at most one raised
    column; three rows of ten are raised, so winners also come from the plateaus.  Later step: unequal scores, lengths 1, 2 and 3, per
    sample one stopped beam whose token 0 wins and one whose token 0 loses; beams 0 and 1 of sample 1 are identical (tie across rows)."""
    R = PL_S * PL_BEAM
    buf = torch.zeros(R, PL_LD)
    const = [0.0, 0.5, -1.25, 0.0, 0.5, 0.5, 0.5, 0.0, -1.25, 0.0]
    for r, c in enumerate(const):
        buf[r] = c
    for r, col, bump in ((1, PL_STOP, 3.0), (4, PL_V - 1, 2.0), (8, 64, 3.0)):      # the stop token, the last column, a block boundary
        buf[r, col] += bump
    if first:                                       # row 0 of a sample is all a first step reads: sample 0 gets a raised row, sample 1 a flat one
        buf = buf.roll(-1, 0)
        return buf, torch.zeros(R), torch.ones(R), torch.zeros(R, dtype=torch.bool)
    scores = torch.tensor([-1.0, -2.0, -3.0, -15.0, -0.5, -1.5, -1.5, -2.0, -6.0, -9.0])
    seql = torch.tensor([1.0, 2.0, 3.0, 3.0, 2.0, 2.0, 2.0, 1.0, 3.0, 2.0])
    stopped = torch.tensor([0, 0, 1, 1, 0, 0, 0, 1, 0, 1], dtype=torch.bool)
    return buf, scores, seql, stopped


def _expect64(lg, first, temp, scores, seql, stopped):
    """The update of base.py:84-119 in float64 with the documented order: value descending, flat index b * V + v ascending.
    -> tokens, source rows, scores, lengths, stop flags, and per sample the best beam + 1 (value, flat index) pairs."""
    import numpy as np
    V = PL_V
    lp = torch.log_softmax(lg[:, :V].double() / temp, -1)
    nt, sr, ns, nl, nh, top = [], [], [], [], [], []
    for s in range(PL_S):
        rows = range(s * PL_BEAM, s * PL_BEAM + (1 if first else PL_BEAM))
        vals = []
        for r in rows:
            if first:
                vals.append(lp[r])
            elif stopped[r]:
                v = torch.full((V,), float("-inf"), dtype=torch.float64)
                v[0] = scores[r].double() / seql[r].double()
                vals.append(v)
            else:
                vals.append((scores[r].double() + lp[r]) / (seql[r].double() + 1.0))
        vals = torch.cat(vals).numpy()
        order = np.lexsort((np.arange(vals.size), -vals))[:PL_BEAM + 1]
        top.append([(float(vals[i]), int(i)) for i in order])
        for i in order[:PL_BEAM]:
            b, v = int(i) // V, int(i) % V
            r = s * PL_BEAM + b
            ln = 1.0 if first else float(seql[r]) + (0.0 if stopped[r] else 1.0)
            nt.append(v); sr.append(b); nl.append(ln); ns.append(float(vals[i]) * ln)
            nh.append((False if first else bool(stopped[r])) or v == PL_STOP)
    return (torch.tensor(nt), torch.tensor(sr), torch.tensor(ns, dtype=torch.float64), torch.tensor(nl), torch.tensor(nh)), top


def _assert_order_is_decided(lg, first, scores, seql, stopped, top):
    """Any two of a sample's best beam + 1 candidates are tied by construction (same row and logit, or rows with identical logits and
    state) or differ by more than 1e-4, so fp32 rounding cannot decide the order."""
    for s, best in enumerate(top):
        for (va, ia), (vb, ib) in zip(best, best[1:]):
            ra, rb = s * PL_BEAM + ia // PL_V, s * PL_BEAM + ib // PL_V
            if va == vb:
                same_rows = ra == rb or (torch.equal(lg[ra], lg[rb]) and scores[ra] == scores[rb] and seql[ra] == seql[rb] and
                                         stopped[ra] == stopped[rb])
                assert same_rows and lg[ra, ia % PL_V] == lg[rb, ib % PL_V], (s, ia, ib)
            else:
                assert va - vb > 1e-4, (s, va, vb)
        if not first:
            assert len({i // PL_V for _, i in best[:PL_BEAM]}) >= 2


@pytest.mark.parametrize("path", ["three_kernels", "partials"])
@pytest.mark.parametrize("first", [True, False])
def test_beam_step_plateau_overflow_matches_float64(path, first):
    """Plateau logits at V = 4099, beam 5: the list-overflow paths of k_beam_partial (temperature 0.9, three kernels) and k_beam_fused
    (cc_beam_step_p with partials, temperature 1) against the float64 expectation, exact in tokens, source rows, lengths and stop flags."""
    temp = 0.9 if path == "three_kernels" else 1.0
    buf, scores, seql, stopped = _plateau_case(first)
    want, top = _expect64(buf, first, temp, scores, seql, stopped)
    _assert_order_is_decided(buf, first, scores, seql, stopped, top)
    if not first:
        won = {s * PL_BEAM + i // PL_V for s, best in enumerate(top) for _, i in best[:PL_BEAM]}
        assert {2, 7} <= won and not ({3, 9} & won)           # stopped beams: token 0 of rows 2 and 7 wins, of rows 3 and 9 loses
    lg = buf.cuda()[:, :PL_V]
    d_scores, d_seql, d_stopped = scores.cuda(), seql.cuda(), stopped.to(torch.uint8).cuda()
    nt, sr = beam_step(lg, PL_S, PL_BEAM, temp, first, PL_STOP, d_scores, d_seql, d_stopped, None, _partials(lg, PL_V) if path == "partials" else None)
    torch.cuda.synchronize()
    assert torch.equal(nt.cpu().long(), want[0]) and torch.equal(sr.cpu().long(), want[1])
    assert torch.allclose(d_scores.cpu().double(), want[2], rtol=1e-5, atol=3e-5)
    assert torch.equal(d_seql.cpu(), want[3]) and torch.equal(d_stopped.cpu().bool(), want[4])
    assert want[4].any() and not want[4].all()


def _seeded_outputs(partials):
    """five steps with stopping beams (beam 5, V = 4099, padded rows), every output array of every step as raw bits"""
    beam, V, ld, S, stop = 5, 4099, 4104, 6, 17
    temp = 1.0 if partials else 0.9
    R = S * beam
    g = torch.Generator().manual_seed(5 * 1000 + V)
    scores = torch.zeros(R, device="cuda")
    seql = torch.ones(R, device="cuda")
    stopped = torch.zeros(R, dtype=torch.uint8, device="cuda")
    out = []
    for step in range(5):
        buf = (torch.randn(R, ld, generator=g) * 3.0).cuda()
        if step >= 1:
            buf[::3, stop] += 25.0
        lg = buf[:, :V]
        nt, sr = beam_step(lg, S, beam, temp, step == 0, stop, scores, seql, stopped, None, _partials(lg, V) if partials else None)
        out += [nt.cpu(), sr.cpu(), scores.cpu().view(torch.int32), seql.cpu().view(torch.int32), stopped.cpu()]
    assert stopped.any()
    return out


@pytest.mark.parametrize("partials", [False, True])
def test_beam_step_is_bit_identical_from_run_to_run(partials):
    a, b = _seeded_outputs(partials), _seeded_outputs(partials)
    assert len(a) == len(b) == 25 and all(torch.equal(x, y) for x, y in zip(a, b))
