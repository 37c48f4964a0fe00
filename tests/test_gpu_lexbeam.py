"""cc_beam_lex_step (lexically constrained beam search with dynamic beam allocation, clipcap_amd/csrc/lexbeam.hip) on the device: the step
against the float64 statement of its semantics (tests/lexbeam_ref.py) with the state carried and the consequences of the rule on every
step's outputs, bit for bit against cc_beam_step without phrases (three ways to say so), with a phrase's next token banned, with fewer
candidates than slots, from run to run and on a poisoned workspace, and end to end through generate_constrained_beam_tokens on the
beam_tiny golden model against a CPU search built from the oracle's full re-forward and the float64 step.

The inputs' decision margins in the float64 statement (computed on the CPU; MIN_MARGIN = 1e-4 is asserted on them), per shape of SHAPES:
  8.2e-4, 4.8e-3, 3.8e-4, 3.0e-2, 9.8e-4, 6.7e-3; stopped rows occur in all of them.  The banned-token inputs: 1.2e-4.
Measured on an MI355X (the print statements below; inputs and kernels are deterministic, so the figures repeat):
  scores          largest |score - score64| per shape: 5.373e-6, 4.721e-6, 1.132e-5, 7.706e-6, 8.526e-6, 7.041e-6, at most 0.54 of the per-element
                  bound below (SCORE_TOL scaled with the float64 score's magnitude; the scores reach -77); banned-token inputs 4.121e-6 (0.55)
  cost            (tools/lexbeam_bench.py; alternating under device events, median of 5 blocks of 100 calls) S = 64, beam 5, V = 50257, ld =
                  50304: cc_beam_lex_step 112.2 / 117.9 / 139.7 us with 0 / 2 / 8 phrases against 60.5 us for the three-kernel cc_beam_step on
                  the same logits.  Both read the 64.3 MB of logits in the row statistics; this step reads them once more (k_lex_rows), the
                  plain step's two-pass selection scans them twice.  A whole generate_constrained_beam_tokens (2 phrases) at the decode
                  benchmark's shape (GPT-2-medium geometry, 64 prefixes of 10 rows, beam 5, 67 tokens): 0.1033 s against 0.0935 s for
                  generate_beam_tokens, 1.542 against 1.395 ms per position (0.905 of its tokens/s); the update is a tenth of a position"""
import ctypes as C

import pytest
import torch

from clipcap_amd import _lib
from clipcap_amd.engine import beam_buffers, beam_lex_buffers, beam_lex_step, beam_step
from tests.lexbeam_ref import full_mask, lex_search_ref, lex_step_ref, phrase_table, tokens_met, unpack
from tests.util import load_golden, sd_of
from tests.ws_poison import FILL_NAN, FILL_ZERO, Framed

pytestmark = pytest.mark.gpu

# (beam, V, row stride), those of tests/test_gpu_gumbel.py: compile-time widths 5, 3, 1, 8, the list of 16 at its own width and at the run-time
# width 6; padded, unpadded and unaligned rows (4099: a row stride that is no multiple of 4 -> scalar loads); V no multiple of 4
SHAPES = [(5, 50257, 50304), (3, 130, 136), (16, 4099, 4104), (1, 1001, 1001), (8, 257, 260), (6, 4099, 4099)]
S, STEPS, TEMP, STOP = 3, 5, 0.9, 17
# sample 0: no phrase; sample 1: a one-token and a three-token phrase; sample 2: eight phrases, one of length 8, two that share a first token
PHRASES = [[], [[23], [40, 41, 42]], [[1, 2, 3, 4, 5, 6, 7, 8], [30, 31], [30, 32, 33], [50], [60, 61], [70, 71, 72, 73], [80], [90, 91]]]
N_PHR, PHR_LEN = 8, 8
MIN_MARGIN = 1e-4
# Scores.  SCORE_TOL = 5.25e-6 is the bound tests/test_gpu_beam_group.py derives for the same value arithmetic (beam_val) summed over the same five
# steps.  It is an absolute bound for that test's scores, whose magnitude in the float64 statement is at most SCORE_MAG = 13.771 (computed
# on the CPU from that test's inputs).  Here the hypotheses that are kept are the ones that hold forced, improbable tokens: in the float64
# statement their scores reach -77.3 (shape 5x50257x50304, sample 2), where one fp32 ulp is 7.6e-6 and 5.25e-6 is less than one rounding.  An
# fp32 rounding error is proportional to the magnitude of what is rounded (the running score is rounded three times per step: the sum, the
# division by the length and the product with it), so the bound is carried over in proportion: |score - score64| <= SCORE_TOL *
# max(1, |score64| / SCORE_MAG) per element, from the float64 statement's own magnitudes.  Where scores are as small as in that test (sample
# 0, no phrase) it is 5.25e-6 unchanged.
SCORE_TOL = 5.25e-6
SCORE_MAG = 13.771


def _score_excess(got, want):
    """(largest |got - want|, largest |got - want| / bound) over the finite elements of the float64 scores ``want``; the -inf ones must agree."""
    finite = want > float("-inf")
    assert torch.equal(got > float("-inf"), finite)
    err = (got.double() - want)[finite].abs()
    bound = SCORE_TOL * torch.clamp(want[finite].abs() / SCORE_MAG, min=1.0)
    return err.max().item(), (err / bound).max().item()

# generator seeds of the inputs, chosen on the CPU so that the float64 statement's margin is >= MIN_MARGIN and stopped rows occur
SEEDS = {shape: shape[0] * 1000 + shape[1] for shape in SHAPES}
SEEDS[(16, 4099, 4104)] += 2                  # 20099 and 20100 give margins of 2.7e-5 and 9.8e-5
SEEDS[(1, 1001, 1001)] += 1                    # 2001: no row stops


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _table(phrases=PHRASES, n_phr=N_PHR, phr_len=PHR_LEN):
    return torch.stack([phrase_table(p, n_phr, phr_len) for p in phrases])


def _inputs(shape, steps=STEPS, samples=S, seed=None):
    """The steps' logits (R, ld) fp32, generated on the CPU: randn * 3, from step 1 on +8 on the stop logit of every third row."""
    beam, V, ld = shape
    g = torch.Generator().manual_seed(SEEDS[shape] if seed is None else seed)
    out = []
    for step in range(steps):
        buf = torch.randn(samples * beam, ld, generator=g) * 3.0
        if step >= 1:
            buf[::3, STOP] += 8.0
        out.append(buf)
    return out


def _reference(bufs, beam, V, phrases=PHRASES):
    """The float64 statement, sample by sample with its own float64 state -> per step (tokens, src, scores, lengths, stopped, states), and the
    smallest decision margin of any sample at any step."""
    samples = len(phrases)
    state = [(None, None, None, None)] * samples
    steps, margin = [], float("inf")
    for i, buf in enumerate(bufs):
        rs = []
        for s in range(samples):
            r = lex_step_ref(buf[s * beam:(s + 1) * beam, :V], *state[s], beam=beam, phrases=phrases[s], temperature=TEMP, first=i == 0,
                             stop_token=STOP)
            state[s] = (r.scores, r.lengths, r.stopped, r.states)
            margin = min(margin, r.margin)
            rs.append(r)
        steps.append(tuple(torch.cat([getattr(r, f) for r in rs]) for f in ("tokens", "src", "scores", "lengths", "stopped", "states")))
    return steps, margin


_REF = {}


def _shared_reference(shape):
    if shape not in _REF:                      # computed once per shape, shared by the tests that need it, never modified
        bufs = _inputs(shape)
        _REF[shape] = (bufs, _reference(bufs, shape[0], shape[1]))
    return _REF[shape]


def _state(R):
    return (torch.zeros(R, device="cuda"), torch.ones(R, device="cuda"), torch.zeros(R, dtype=torch.uint8, device="cuda"),
            torch.zeros(R, dtype=torch.int32, device="cuda"))


def _check_consequences(beam, phrases, step, nt, sr, scores, stopped, states, bound=True):
    """The consequences of the rule on one step's device outputs: slot 0 has the largest tokens_met of its sample, at least min(step + 1,
    the summed phrase lengths) (``bound``: no phrase token is banned); a non-empty slot is stopped only with every phrase produced; an empty
    slot is the defined one; every index is in bounds."""
    samples = len(phrases)
    nt, sr, scores, stopped, states = (t.cpu().view(samples, beam) for t in (nt, sr, scores, stopped, states))
    assert int(sr.min()) >= 0 and int(sr.max()) < (1 if step == 0 else beam) and int(nt.min()) >= 0
    for s, ph in enumerate(phrases):
        live = scores[s] > float("-inf")
        met = [tokens_met(int(x), ph) for x in states[s]]
        assert live[0] and met[0] == max(m for m, ok in zip(met, live) if ok), (s, met)
        if bound:
            assert met[0] >= min(step + 1, sum(len(p) for p in ph)), (s, step, met)
        for k in range(beam):
            if live[k] and stopped[s, k]:
                assert unpack(int(states[s, k]))[0] == full_mask(ph), (s, k)
            if not live[k]:
                assert (int(nt[s, k]), int(sr[s, k]), int(states[s, k]), int(stopped[s, k])) == (0, 0, 0, 1), (s, k)
        if not ph:
            assert not states[s].any()


def _run_against(bufs, ref, margin, beam, V, phrases, table, label, bound=True):
    """Every step against the float64 statement with the state carried on the device: tokens, sources, stop flags, lengths and lex_state
    exact, scores within the bound above; -> the largest score error."""
    samples = len(phrases)
    assert margin >= MIN_MARGIN, margin             # a condition on the inputs, met by the float64 statement alone
    scores, seql, stopped, states = _state(samples * beam)
    ws = beam_lex_buffers("cuda", samples, beam, table.shape[1], V)
    tab = table.cuda()
    worst, worst_ratio = 0.0, 0.0
    for i, buf in enumerate(bufs):
        nt, sr = beam_lex_step(buf.cuda()[:, :V], samples, beam, TEMP, i == 0, STOP, scores, seql, stopped, states, tab, ws)
        want = ref[i]
        err, ratio = _score_excess(scores.cpu(), want[2])
        worst, worst_ratio = max(worst, err), max(worst_ratio, ratio)
        print(f"{label} step {i}: margin {margin:.2e} score error {err:.3e}, {ratio:.3f} of its bound")
        assert torch.equal(nt.cpu().long(), want[0]), (i, nt.tolist(), want[0].tolist())
        assert torch.equal(sr.cpu().long(), want[1]), i
        assert torch.equal(seql.cpu().double(), want[3]) and torch.equal(stopped.cpu().bool(), want[4]), i
        assert torch.equal(states.cpu().long(), want[5]), i
        _check_consequences(beam, phrases, i, nt, sr, scores, stopped, states, bound)
    print(f"{label}: largest score error {worst:.3e}, at most {worst_ratio:.3f} of the bound")
    assert worst_ratio <= 1.0, (worst, worst_ratio)
    return worst


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_step_matches_the_float64_statement(shape):
    beam, V, ld = shape
    bufs, (ref, margin) = _shared_reference(shape)
    assert ref[-1][4].any()                         # stopped rows occur
    assert any(int(x) for x in ref[-1][5])          # and phrases are in progress or met
    _run_against(bufs, ref, margin, beam, V, PHRASES, _table(), f"shape {shape}")


# ---- no phrases: cc_beam_step bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_no_phrases_three_ways_are_bit_identical_to_beam_step(shape):
    """n_phr == 0 (with a table pointer that is not followed), a NULL table, and a table of -1: outputs and state torch.equal to
    cc_beam_step's three-kernel path on the same inputs over the five steps, the bits of ``scores`` included; the row state stays 0."""
    beam, V, ld = shape
    bufs = _inputs(shape)
    R = S * beam
    plain = _state(R)[:3]
    pb = beam_buffers("cuda", S, beam, V)
    ways = {"n_phr == 0": (_state(R), 0), "NULL table": (_state(R), None), "table of -1": (_state(R), torch.full((S, N_PHR, PHR_LEN), -1, dtype=torch.int32).cuda())}
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")                      # n_phr == 0: a pointer that must not be followed as [S][0][..]
    for i, buf in enumerate(bufs):
        lg = buf.cuda()[:, :V]
        nt0, sr0 = beam_step(lg, S, beam, TEMP, i == 0, STOP, *plain, pb)
        for name, (st, tab) in ways.items():
            if isinstance(tab, int):                                               # the raw entry point: the wrapper passes NULL when n_phr == 0
                nt, sr, ws = beam_lex_buffers("cuda", S, beam, 0, V)
                p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
                rc = _lib.lib().cc_beam_lex_step(S, beam, V, p(lg), lg.stride(0), TEMP, int(i == 0), STOP, p(bad), 0, 1, p(st[0]), p(st[1]), p(st[2]),
                                                 p(st[3]), p(nt), p(sr), p(ws), C.c_void_p(torch.cuda.current_stream().cuda_stream))
                assert rc == 0
            else:
                nt, sr = beam_lex_step(lg, S, beam, TEMP, i == 0, STOP, *st, tab)
            assert torch.equal(nt, nt0) and torch.equal(sr, sr0), (name, i)
            assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(st[:3], plain)), (name, i)
            assert not st[3].any(), (name, i)
    assert plain[2].any()


# ---- a phrase's next token banned ----------------------------------------------------------------------------------------------------------
def test_a_banned_phrase_token_matches_the_statement():
    """-inf on the second token of sample 1's three-token phrase and of sample 2's eight-token phrase on the odd rows, on sample 1's
    one-token phrase everywhere at step 0, and on a whole 64-column block: the device follows the float64 statement; the bound on slot 0's
    tokens_met does not hold here and is not asserted."""
    shape = (8, 257, 260)
    beam, V, ld = shape
    bufs = [b.clone() for b in _inputs(shape, seed=4242)]
    for i, b in enumerate(bufs):
        b[1::2, 41] = float("-inf")
        b[1::2, 2] = float("-inf")
        b[:, 128:192] = float("-inf")
        if i == 0:
            b[:, 23] = float("-inf")
    ref, margin = _reference(bufs, beam, V)
    _run_against(bufs, ref, margin, beam, V, PHRASES, _table(), "banned phrase tokens", bound=False)
    for i, want in enumerate(ref):                                                  # no banned token was picked
        rows = (torch.arange(S * beam) // beam) * beam + want[1]
        live = want[2] > float("-inf")
        was = ref[i - 1][4][rows] if i else torch.zeros(S * beam, dtype=torch.bool)
        assert torch.isfinite(bufs[i][rows, want[0]][live & ~was]).all()


# ---- fewer candidates than slots ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beam", [16, 4], ids=["list-of-16", "compile-time-width"])
def test_fewer_candidates_than_slots_leave_defined_empty_slots(beam):
    """A sample with only 2 finite tokens, on the first step and on a later step, one of them a phrase token: the two candidates come
    first, the one that advances the phrase in slot 0; the empty slots hold token 0, source row 0, score -inf, the stop flag, state 0 and row
    0's length; they stay empty; every index is in bounds."""
    samples, V, ld = 2, 130, 136
    phrases = [[[41, 7]], [[41, 7]]]
    table = _table(phrases, 1, 2).cuda()
    R, ninf = samples * beam, float("-inf")
    lg0 = torch.full((R, ld), ninf)
    for s in range(samples):
        lg0[s * beam, 41], lg0[s * beam, 99] = 1.0, 2.0
    lg1 = torch.full((R, ld), ninf)
    for s in range(samples):
        lg1[s * beam, 7], lg1[s * beam, 40] = 0.0, 0.5                          # row 0 of the sample: two finite tokens; row 1: none
        lg1[s * beam + 2:(s + 1) * beam, :] = 1.0                               # rows that hold empty slots: finite logits that must not be read
    lg2 = lg1.clone()
    for s in range(samples):
        lg2[s * beam + 1, 41], lg2[s * beam + 1, 60] = 0.3, 0.1                  # a later step: row 1 has two finite tokens too
    scores, seql, stopped, states = _state(R)
    state = [(None, None, None, None)] * samples
    for i, lg in enumerate((lg0, lg1, lg2)):
        nt, sr = beam_lex_step(lg.cuda()[:, :V], samples, beam, TEMP, i == 0, STOP, scores, seql, stopped, states, table)
        assert int(nt.min()) >= 0 and int(nt.max()) < V and int(sr.min()) >= 0 and int(sr.max()) < beam
        for s in range(samples):
            sl = slice(s * beam, (s + 1) * beam)
            r = lex_step_ref(lg[sl, :V], *state[s], beam=beam, phrases=phrases[s], temperature=TEMP, first=i == 0, stop_token=STOP)
            state[s] = (r.scores, r.lengths, r.stopped, r.states)
            assert nt[sl].tolist() == r.tokens.tolist() and sr[sl].tolist() == r.src.tolist(), (i, s)
            assert states[sl].tolist() == r.states.tolist() and stopped[sl].bool().tolist() == r.stopped.tolist(), (i, s)
            assert torch.equal(seql[sl].cpu().double(), r.lengths), (i, s)
            live = r.scores > ninf
            assert _score_excess(scores[sl].cpu(), r.scores)[1] <= 1.0
            if i == 0:
                assert nt[sl].tolist() == [41, 99] + [0] * (beam - 2) and int(live.sum()) == 2
                assert seql[sl].tolist() == [1.0] * beam and stopped[sl].tolist() == [0, 0] + [1] * (beam - 2)
            elif i == 1:
                assert nt[sl].tolist() == [7, 40] + [0] * (beam - 2) and sr[sl].tolist() == [0] * beam and int(live.sum()) == 2
                assert seql[sl].tolist() == [2.0, 2.0] + [1.0] * (beam - 2) and tokens_met(int(states[s * beam]), phrases[s]) == 2
            else:
                assert int(live.sum()) == 4 and not live[4:].any()                    # two parents with two finite tokens each; the rest stays empty


# ---- determinism and the workspace -------------------------------------------------------------------------------------------------------
def _seeded_run(fill=None, shape=(6, 4099, 4104)):
    beam, V, ld = shape
    scores, seql, stopped, states = _state(S * beam)
    table = _table().cuda()
    nt, sr, ws = beam_lex_buffers("cuda", S, beam, N_PHR, V)
    frame = None
    if fill is not None:
        frame = Framed(ws.numel(), fill, "cuda")
        ws = frame.body
    out = []
    for i, buf in enumerate(_inputs(shape, seed=607)):
        if frame is not None:
            frame.refill()
        beam_lex_step(buf.cuda()[:, :V], S, beam, TEMP, i == 0, STOP, scores, seql, stopped, states, table, (nt, sr, ws))
        out += [nt.cpu(), sr.cpu(), _bits(scores.cpu()), _bits(seql.cpu()), stopped.cpu(), states.cpu()]
    if frame is not None:
        torch.cuda.synchronize()
        frame.check_guards()                                                     # nothing written outside cc_beam_lex_ws_bytes
        assert frame.touched()
    assert stopped.any() and states.any()
    return out


def test_step_is_bit_identical_from_run_to_run_and_on_a_poisoned_workspace():
    a, b = _seeded_run(), _seeded_run()
    assert len(a) == 6 * STEPS and all(torch.equal(x, y) for x, y in zip(a, b))
    for fill in (FILL_ZERO, FILL_NAN):                                           # 0xFF: NaN as fp32, -1 as a token
        c = _seeded_run(fill)
        assert all(torch.equal(x, y) for x, y in zip(a, c)), fill


# ---- end to end: generate_constrained_beam_tokens on the beam_tiny golden model (split-bf16 operands) against a CPU search ------------------
# Chosen on the CPU (golden cases 1 and 2, stop token 50, 12 tokens, beam 4): the phrases are ids that no beam of the unconstrained search of
# that prefix holds, and the CPU search's smallest decision margin clears the decode path's logit error by the factor the other beam_tiny
# end-to-end tests use: 1e-3 (tests/test_gpu_beam_group.py), under guidance (|g| + |1 - g|) * 2e-3 (tests/test_gpu_guide_decode.py).
#   plain:  case 1 [[53], [44, 45]] 1.2e-2, case 2 [[91], [67, 2]] 3.2e-3      bans: case 2 [[91], [67, 2]] 1.5e-3, case 2 [[78], [26, 72]] 1.2e-3
#   guided: case 1 [[53], [44, 45]] 7.5e-3, case 2 [[91], [67, 2]] 1.2e-2 (needed 4e-3)
E2E_BEAM, E2E_GUIDANCE = 4, 1.5
E2E = {"plain": ({}, [("1", [[53], [44, 45]]), ("2", [[91], [67, 2]])]),
       "bans": (dict(no_repeat_ngram_size=2, min_length=3), [("2", [[91], [67, 2]]), ("2", [[78], [26, 72]])]),
       "guided": (dict(guidance_scale=E2E_GUIDANCE), [("1", [[53], [44, 45]]), ("2", [[91], [67, 2]])])}


def _holds(seq, phrase):
    return any(seq[i:i + len(phrase)] == phrase for i in range(len(seq) - len(phrase) + 1))


@pytest.mark.parametrize("config", sorted(E2E))
def test_constrained_beam_search_equals_the_cpu_search(config):
    from types import SimpleNamespace
    from clipcap_amd.inference import generate_beam_tokens, generate_constrained_beam_tokens
    from clipcap_amd.inference.lexical import best_constrained_beams
    from clipcap_amd.model.gpt2 import GPT2LM
    opts, cases = E2E[config]
    g = load_golden("beam_tiny")
    D, n_layer, n_head, V, npos = [int(v) for v in g["cfg"]]
    lm = GPT2LM(n_embd=D, n_layer=n_layer, n_head=n_head, vocab_size=V, n_positions=npos, precision=32)
    lm.load_state_dict(sd_of(g), strict=False)
    model = SimpleNamespace(language_model=lm.to("cuda"))
    sd = {"language_model." + k: v for k, v in sd_of(g).items()}
    dims = dict(n_head=n_head, n_layer=n_layer)
    metas = {tuple(int(v) for v in g[f"beam{c}.meta"][:2]) for c, _ in cases}
    assert len(metas) == 1
    stop, entry = metas.pop()
    pref = torch.cat([torch.from_numpy(g[f"beam{c}.prefix"]) for c, _ in cases])
    phrases = [ph for _, ph in cases]
    kw, ref_kw, need = dict(opts), dict(opts), 1e-3
    if "guidance_scale" in opts:
        neg = sd["language_model.transformer.wte.weight"][50].view(1, 1, -1).clone()
        kw["negative_embeds"] = neg.cuda()
        ref_kw = dict(negative=neg, scale=opts["guidance_scale"])
        need = (abs(E2E_GUIDANCE) + abs(1 - E2E_GUIDANCE)) * 2e-3
    free = generate_beam_tokens(model, pref.cuda(), E2E_BEAM, entry, 1.0, stop)[0].cpu()
    r = generate_constrained_beam_tokens(model, pref.cuda(), phrases, E2E_BEAM, entry, 1.0, stop, **kw)
    again = generate_constrained_beam_tokens(model, pref.cuda(), phrases, E2E_BEAM, entry, 1.0, stop, **kw)
    assert all(torch.equal(a, b) for a, b in zip(r, again))
    toks, scores, lens, met, done = (t.cpu() for t in r)
    best = best_constrained_beams(scores, met, 1)
    for s, ph in enumerate(phrases):
        assert not set(free[s].view(-1).tolist()) & {t for p in ph for t in p}, (s, "the unconstrained beams hold a phrase token")
        ot, osc, ol, ost, margin = lex_search_ref(sd, pref[s:s + 1], ph, beam=E2E_BEAM, entry_length=entry, stop_token=stop, **dims, **ref_kw)
        print(f"{config} prefix {s}: CPU-search margin {margin:.2e} (needed {need:.1e})")
        assert margin >= need, (s, margin)          # a condition on the case, met by the reference alone: every case is compared
        assert torch.equal(lens[s].double(), ol), s
        for b in range(E2E_BEAM):
            n = int(ol[b])
            assert toks[s, b, :n].tolist() == ot[b, :n].tolist(), (s, b)
            assert abs(float(scores[s, b]) - float(osc[b])) <= need, (s, b)
            assert int(met[s, b]) == tokens_met(int(ost[b]), ph) and bool(done[s, b]) == (unpack(int(ost[b]))[0] == full_mask(ph)), (s, b)
        b = int(best[s, 0])
        seq = toks[s, b, :int(lens[s, b])].tolist()
        assert bool(done[s, b]) and int(met[s, b]) == sum(len(p) for p in ph)
        assert all(_holds(seq, p) for p in ph) and seq[-1] == stop and stop not in seq[:-1], (s, seq)
        if "min_length" in opts:
            assert len(seq) > 3 and len({tuple(seq[i:i + 2]) for i in range(len(seq) - 1)}) == len(seq) - 1, seq
