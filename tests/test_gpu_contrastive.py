"""Contrastive search on the device (clipcap_amd/csrc/contrastive.hip, cc_decode_hidden_unit in decode.hip, inference/contrastive.py):
the top-k and the selection kernels against the float64 statement (tests/contrastive_ref.py), the hidden states against the oracle's
gpt2_hidden, and the decoders end to end on the beam_tiny golden model against a CPU search built from the oracle's full re-forward.

Measured on an MI355X (the inputs and the kernels are deterministic, so the figures repeat; `measure_*` below print them):
  top-k: largest |log p_dev - log p_ref| over the four shapes, k in {1, 3, 4, 8}, both row selections: 2.096e-7 (V 50257, k 3; bar 1.05e-5)
  select: largest |sel_score - float64| over the seven shapes: 8.8e-8, at most 0.022 of the bound (D + 16) * 2^-24 (shape 3x4x32x0x1)
  hidden states, split-bf16 operands: eps_h 2.283e-6 (largest L2 deviation of a unit vector), eps_p 2.699e-6 (largest softmax deviation):
      (1 - alpha) eps_p + 2 alpha eps_h = 3.6e-6 at alpha = 0.5, against the asserted 1e-3
  hidden states, bf16 operands (recorded, not asserted beyond eps_h < 0.1): eps_h 1.073e-3, eps_p 5.761e-4
"""
import pytest
import torch

from tests.contrastive_ref import contrastive_search_ref, contrastive_select_ref, contrastive_topk_ref
from tests.util import load_golden, sd_of

pytestmark = pytest.mark.gpu

S = 3
# 4 x the 2.626e-6 tests/test_gpu_beam_group.py records for cc_beam_step's softmax (the same arithmetic with one reduction fewer)
LOGP_TOL = 4 * 2.626e-6
TOPK_SHAPES = [(50257, 50304), (4099, 4104), (1001, 1001), (97, 104)]
TOPK_KS = [1, 3, 4, 8]


# ---- top-k ----------------------------------------------------------------------------------------------------------------------------------
_TOPK = {}


def _topk_case(V, ld, k, rows_per):
    """Logits (S * rows_per, ld) randn * 3, the row selection and the float64 statement of the selected rows; computed once, never modified."""
    key = (V, ld, k, rows_per)
    if key not in _TOPK:
        g = torch.Generator().manual_seed(V * 10 + k + rows_per)
        lg = torch.randn(S * rows_per, ld, generator=g) * 3.0
        sel = None if rows_per == 1 else torch.tensor([(2 * s + 1) % rows_per for s in range(S)], dtype=torch.int32)
        ref = [contrastive_topk_ref(lg[s * rows_per + (0 if sel is None else int(sel[s])), :V], k) for s in range(S)]
        _TOPK[key] = (lg, sel, ref)
    return _TOPK[key]


def _run_topk(lg, V, k, rows_per, sel, stopped=None):
    from clipcap_amd.engine import contrastive_topk
    n = lg.shape[0] // rows_per
    tok = torch.full((n * k,), -7, dtype=torch.int32, device="cuda")
    prob = torch.full((n * k,), -7.0, device="cuda")
    contrastive_topk(lg.cuda()[:, :V], n, rows_per, sel.cuda() if sel is not None else None, k, stopped.cuda() if stopped is not None else None, tok, prob)
    return tok.cpu().view(n, k), prob.cpu().view(n, k)


def measure_topk(V, ld, k, rows_per):
    """-> (ids equal, largest |log p_dev - log p_ref|)."""
    lg, sel, ref = _topk_case(V, ld, k, rows_per)
    tok, prob = _run_topk(lg, V, k, rows_per, sel)
    same = all(tok[s].tolist() == ref[s][0].tolist() for s in range(S))
    err = max((prob[s].double().log() - ref[s][1].log()).abs().max().item() for s in range(S))
    return same, err


@pytest.mark.parametrize("k", TOPK_KS)
@pytest.mark.parametrize("shape", TOPK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_topk_matches_the_float64_statement(shape, k):
    """Ids exactly (comparisons of the fp32 inputs); log-probabilities within LOGP_TOL; the first row of every caption (rows_per = 1, no
    sel) and a selected row among k (a sel that is not all zeros)."""
    V, ld = shape
    for rows_per in sorted({1, max(k, 2)}):
        same, err = measure_topk(V, ld, k, rows_per)
        print(f"top-k V {V} ld {ld} k {k} rows_per {rows_per}: log p error {err:.3e}")
        assert same, rows_per
        assert err <= LOGP_TOL, (rows_per, err)
    if k > 1:
        assert _topk_case(V, ld, k, k)[1].any()


def test_topk_all_logits_equal():
    V, k = 50257, 8
    tok, prob = _run_topk(torch.zeros(2, V), V, k, 1, None)
    assert tok.tolist() == [list(range(k))] * 2
    assert torch.allclose(prob.double(), torch.full((2, k), 1.0 / V, dtype=torch.float64), rtol=2.0 ** -23, atol=0)    # exp(0) = 1, V ones add exactly: one division


def test_topk_with_banned_entries_and_a_stopped_caption():
    V, ld, k = 1001, 1001, 4
    g = torch.Generator().manual_seed(5)
    lg = torch.randn(4, ld, generator=g) * 3.0
    lg[0][torch.rand(ld, generator=g) < 0.4] = float("-inf")
    lg[0, lg[0].argmax()] = float("-inf")                                                      # what an unconstrained step would have picked
    lg[1] = float("-inf")
    lg[1, 700], lg[1, 3] = 0.25, -1.0                                                          # only 2 finite logits
    lg[2] = float("nan")                                                                       # the stopped caption's row: never read
    lg[3, :4] = float("-inf")                                                                  # a whole first float4 banned
    stopped = torch.tensor([0, 0, 1, 0], dtype=torch.uint8)
    tok, prob = _run_topk(lg, V, k, 1, None, stopped)
    for s in (0, 1, 3):
        t, p, _ = contrastive_topk_ref(lg[s, :V], k)
        assert tok[s].tolist() == t.tolist(), s
        ok = p >= 0
        assert torch.equal(prob[s][~ok], torch.full((int((~ok).sum()),), -1.0)), s
        assert (prob[s][ok].double().log() - p[ok].log()).abs().max().item() <= LOGP_TOL, s
    assert tok[1].tolist() == [700, 3, 0, 0] and prob[1, 2:].tolist() == [-1.0, -1.0]
    assert tok[2].tolist() == [0] * k and prob[2].tolist() == [-1.0] * k


# ---- select ---------------------------------------------------------------------------------------------------------------------------------
# (captions, k, D, hist_lo, hist_n); the last: the largest candidate buffer the kernel accepts (64 KB of LDS)
SELECT_SHAPES = [(3, 4, 32, 0, 1), (2, 8, 1600, 0, 77), (3, 3, 768, 10, 40), (2, 1, 64, 0, 5), (2, 5, 1024, 7, 7), (2, 4, 2048, 0, 130),
                 (3, 8, 2048, 1, 6)]
STOP, CAP_LD, STEP = 17, 6, 2
SELECT_SEED = 0         # seeds were tried from 0 up on the CPU until the float64 statement's smallest margin was >= 10 x the score bound at every shape: the first does


def _score_bound(D):
    return (D + 16) * 2.0 ** -24          # an fp32 dot product of unit vectors in any summation order, plus the two multiplies


def _select_inputs(shape, seed=SELECT_SEED):
    """Random unit vectors (the last history row of a non-empty range: slot 0's vector plus noise, a cosine of about 0.96), probabilities =
    the k largest of softmax(randn * 3) in descending order; caption 0 had already stopped; the last caption's slot 1 (slot 0 when k == 1) holds the stop token with a probability that wins clearly; one slot of caption 1 (of caption 0's
    neighbour when there are two captions) is invalid when k > 1."""
    n, k, D, lo, hn = shape
    g = torch.Generator().manual_seed(1000 * seed + D + k)
    unit = lambda *s: torch.nn.functional.normalize(torch.randn(*s, generator=g), dim=-1)  # noqa: E731
    hist_ld = hn + 3
    cand_h, hist = unit(n * k, D), unit(n, hist_ld, D)
    if hn > lo:                                                                               # the context already holds (nearly) the most probable candidate
        hist[:, hn - 1] = torch.nn.functional.normalize(cand_h[::k] + 0.3 * unit(n, D), dim=-1)
    prob = torch.softmax(torch.randn(n, 64, generator=g) * 3, -1).topk(k, dim=1).values.contiguous()
    tok = torch.randint(20, 90, (n, k), generator=g, dtype=torch.int32)
    stopped = torch.zeros(n, dtype=torch.uint8)
    stopped[0] = 1
    c = min(1, k - 1)
    tok[n - 1, c] = STOP
    prob[n - 1, c] = 3.0                                                                      # beyond any penalty: a clear winner
    if k > 1:
        prob[1, k - 1] = -1.0
    lengths = torch.arange(n, dtype=torch.int32) + 2
    return cand_h, prob.view(-1), tok.view(-1), hist, stopped, lengths


def _select_reference(shape, seed=SELECT_SEED, alpha=0.5):
    n, k, D, lo, hn = shape
    cand_h, prob, tok, hist, stopped, lengths = _select_inputs(shape, seed)
    refs = [None if stopped[s] else contrastive_select_ref(cand_h[s * k:(s + 1) * k], prob[s * k:(s + 1) * k], tok[s * k:(s + 1) * k], hist[s], lo, hn,
                                                           alpha, STOP) for s in range(n)]
    return refs, min(r.margin for r in refs if r is not None)


_SELECT = {}


def _select_case(shape):
    if shape not in _SELECT:                  # computed once per shape, shared, never modified
        _SELECT[shape] = (SELECT_SEED, _select_inputs(shape), _select_reference(shape))
    return _SELECT[shape]


def _run_select(shape, inputs, alpha=0.5):
    from types import SimpleNamespace
    from clipcap_amd.engine import contrastive_select
    n, k, D, lo, hn = shape
    cand_h, prob, tok, hist, stopped, lengths = inputs
    dev = lambda t: t.clone().cuda()  # noqa: E731
    b = SimpleNamespace(cand_h=dev(cand_h), cand_prob=dev(prob), cand_tok=dev(tok), hist=dev(hist), stopped=dev(stopped), lengths=dev(lengths),
                        sel=torch.full((n,), -7, dtype=torch.int32, device="cuda"), src_rows=torch.full((n * k,), -7, dtype=torch.int32, device="cuda"),
                        skip_rows=torch.full((n * k,), 7, dtype=torch.uint8, device="cuda"),
                        captions=torch.full((n, CAP_LD), -7, dtype=torch.int32, device="cuda"), scores=torch.full((CAP_LD, n), -7.0, device="cuda"))
    contrastive_select(b, k, lo, hn, alpha, STOP, STEP)
    torch.cuda.synchronize()
    return SimpleNamespace(**{f: getattr(b, f).cpu() for f in vars(b)})


def measure_select(shape):
    """-> largest |sel_score - float64| of the captions that took part, as a fraction of the bound."""
    n, k, D, lo, hn = shape
    seed, inputs, (refs, margin) = _select_case(shape)
    out = _run_select(shape, inputs)
    return max(abs(float(out.scores[STEP, s]) - refs[s].score) for s in range(n) if refs[s] is not None) / _score_bound(D)


@pytest.mark.parametrize("shape", SELECT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_select_matches_the_float64_statement(shape):
    n, k, D, lo, hn = shape
    seed, inputs, (refs, margin) = _select_case(shape)
    cand_h, prob, tok, hist, stopped, lengths = inputs
    bound = _score_bound(D)
    assert margin >= 10 * bound, (seed, margin)
    out = _run_select(shape, inputs)
    print(f"select {shape}: seed {seed} margin {margin:.3e} bound {bound:.3e}")
    for s in range(n):
        rows = slice(s * k, (s + 1) * k)
        r = refs[s]
        if r is None:                                                                          # had stopped: padding, state untouched
            assert int(out.sel[s]) == 0 and int(out.captions[s, STEP]) == 0 and out.skip_rows[rows].tolist() == [1] * k
            assert out.src_rows[rows].tolist() == [0] * k and float(out.scores[STEP, s]) == 0.0
            assert int(out.lengths[s]) == int(lengths[s]) and int(out.stopped[s]) == 1
            assert torch.equal(out.hist[s], hist[s])
            continue
        assert int(out.sel[s]) == r.sel and int(out.captions[s, STEP]) == r.token, s
        assert out.src_rows[rows].tolist() == [r.sel] * k, s
        stop = r.token == STOP
        assert int(out.stopped[s]) == int(stop) and int(out.lengths[s]) == int(lengths[s]) + 1, s
        assert out.skip_rows[rows].tolist() == [1 if (c != r.sel or stop) else 0 for c in range(k)], s
        err = abs(float(out.scores[STEP, s]) - r.score)
        print(f"  caption {s}: score error {err:.3e} = {err / bound:.3f} of the bound")
        assert err <= bound, (s, err)
        assert torch.equal(out.hist[s, hn].view(torch.int32), cand_h[s * k + r.sel].view(torch.int32)), s     # the appended row: a copy
        keep = torch.arange(hist.shape[1]) != hn
        assert torch.equal(out.hist[s][keep], hist[s][keep]), s                                # nothing else of the history is written
    assert refs[n - 1].token == STOP and out.captions[:, [c for c in range(CAP_LD) if c != STEP]].eq(-7).all()
    assert torch.equal(out.cand_h, cand_h) and torch.equal(out.cand_prob, prob)


def test_select_without_a_valid_slot_stops_the_caption():
    shape = (2, 3, 64, 0, 4)
    cand_h, prob, tok, hist, stopped, lengths = _select_inputs(shape, 0)
    stopped[:] = 0
    prob[:3] = -1.0
    out = _run_select(shape, (cand_h, prob, tok, hist, stopped, lengths))
    assert int(out.captions[0, STEP]) == STOP and int(out.stopped[0]) == 1 and int(out.lengths[0]) == int(lengths[0]) + 1
    assert out.skip_rows[:3].tolist() == [1, 1, 1] and out.src_rows[:3].tolist() == [0, 0, 0] and int(out.sel[0]) == 0
    assert torch.equal(out.hist[0], hist[0]) and float(out.scores[STEP, 0]) == 0.0


def test_select_alpha_bounds():
    """alpha = 0: the largest probability wins whatever the history holds; alpha = 1: the least similar candidate wins."""
    shape = (2, 4, 128, 0, 9)
    inputs = _select_inputs(shape, 3)
    inputs[4][:] = 0
    for alpha in (0.0, 1.0):
        out = _run_select(shape, inputs, alpha)
        for s in range(2):
            r = contrastive_select_ref(inputs[0][s * 4:(s + 1) * 4], inputs[1][s * 4:(s + 1) * 4], inputs[2][s * 4:(s + 1) * 4], inputs[3][s], 0, 9, alpha, STOP)
            assert r.margin > 1e-4 and int(out.sel[s]) == r.sel, (alpha, s)


# ---- hidden states --------------------------------------------------------------------------------------------------------------------------
E2E_CASES = ("1", "3")


def _tiny(precision=32, cases=E2E_CASES):
    from types import SimpleNamespace
    from clipcap_amd.model.gpt2 import GPT2LM
    g = load_golden("beam_tiny")
    D, n_layer, n_head, V, npos = [int(v) for v in g["cfg"]]
    lm = GPT2LM(n_embd=D, n_layer=n_layer, n_head=n_head, vocab_size=V, n_positions=npos, precision=precision)
    lm.load_state_dict(sd_of(g), strict=False)
    sd = {"language_model." + k: v for k, v in sd_of(g).items()}
    pref = torch.cat([torch.from_numpy(g[f"beam{c}.prefix"]) for c in cases])
    return SimpleNamespace(language_model=lm.to("cuda")), sd, pref, dict(n_head=n_head, n_layer=n_layer), V


def measure_hidden(precision):
    """Prefill of the two prefixes (Tnew = 4), then one step at R = S * 3 after expand -> (eps_h: the largest L2 deviation of a unit vector
    from the oracle's normalised gpt2_hidden over every position of both forwards, eps_p: the largest softmax deviation of the rows whose
    logits the forwards return)."""
    from clipcap_amd.engine import DecodeSession
    from oracle import clipcap_oracle as O
    model, sd, pref, dims, V = _tiny(precision)
    lm = model.language_model
    g = lm.engine
    n, L0, D = pref.shape
    k = 3
    unit = lambda h: torch.nn.functional.normalize(h.double(), dim=-1)  # noqa: E731
    wte = sd["language_model.transformer.wte.weight"]
    sess = DecodeSession(g, n, L0 + 2)
    lg0 = sess.forward(pref.cuda()).cpu()
    out0 = torch.full((n, L0 + 2, D), 9.0, device="cuda")
    sess.hidden_unit(out0, out0.stride(0), D)
    h0, _ = O.gpt2_hidden(sd, pref, pre="language_model.transformer.", **dims)
    eps_h = (out0.cpu()[:, :L0].double() - unit(h0)).norm(dim=-1).max().item()
    assert (out0[:, L0:] == 9.0).all()                                                         # nothing past the Tnew positions is written
    eps_p = (torch.softmax(lg0.double(), -1) - torch.softmax((h0[:, -1] @ wte.t()).double(), -1)).abs().max().item()
    sess = sess.expand(torch.arange(n, dtype=torch.int32, device="cuda").repeat_interleave(k), n * k)
    nxt = wte[torch.tensor([40, 29, 1, 7, 14, 50])].view(n * k, 1, D)
    lg1 = sess.forward(nxt.cuda(), group=k).cpu()
    out1 = torch.empty(n * k, D, device="cuda")
    sess.hidden_unit(out1, D, D)
    h1, _ = O.gpt2_hidden(sd, torch.cat((pref.repeat_interleave(k, 0), nxt), 1), pre="language_model.transformer.", **dims)
    eps_h = max(eps_h, (out1.cpu().double() - unit(h1[:, -1])).norm(dim=-1).max().item())
    eps_p = max(eps_p, (torch.softmax(lg1.double(), -1) - torch.softmax((h1[:, -1] @ wte.t()).double(), -1)).abs().max().item())
    norm_err = max((out0.cpu()[:, :L0].double().norm(dim=-1) - 1).abs().max().item(), (out1.cpu().double().norm(dim=-1) - 1).abs().max().item())
    return eps_h, eps_p, norm_err


def test_hidden_unit_matches_the_oracle_in_split_bf16_operands():
    """(1 - alpha) eps_p + 2 alpha eps_h <= 1e-3 at alpha = 0.5: half of the 2e-3 score margin the end-to-end tests assert on the reference
    (|d(u . v)| <= |du| + |dv| for unit vectors), i.e. the condition under which that margin decides them."""
    eps_h, eps_p, norm_err = measure_hidden(32)
    print(f"hidden states, split-bf16 operands: eps_h {eps_h:.3e} eps_p {eps_p:.3e} | |u| - 1 | {norm_err:.3e}")
    assert norm_err <= 1e-6
    assert 0.5 * eps_p + 2 * 0.5 * eps_h <= 1e-3, (eps_h, eps_p)


def test_hidden_unit_in_bf16_operands_is_recorded():
    eps_h, eps_p, norm_err = measure_hidden("bf16")
    print(f"hidden states, bf16 operands: eps_h {eps_h:.3e} eps_p {eps_p:.3e} | |u| - 1 | {norm_err:.3e}")
    assert norm_err <= 1e-6 and eps_h < 0.1


def test_hidden_unit_needs_a_forward_first():
    from clipcap_amd.engine import DecodeSession
    model, _, pref, _, _ = _tiny(32)
    sess = DecodeSession(model.language_model.engine, 2, 8)
    with pytest.raises(RuntimeError, match="forward"):
        sess.hidden_unit(torch.empty(2, 32, device="cuda"), 32, 32)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
STOP_E2E, ENTRY = 50, 10
BANS = dict(no_repeat_ngram_size=2, min_length=3)
MARGIN = 2e-3


def _check_against_cpu(model, sd, pref, dims, out, *, top_k, penalty_alpha, stop_token, **kw):
    toks, lens, scores = (t.cpu() for t in out)
    moved = []
    for s in range(pref.shape[0]):
        rt, rs, smargin, setmargin, slot0 = contrastive_search_ref(sd, pref[s:s + 1], top_k=top_k, penalty_alpha=penalty_alpha, entry_length=ENTRY,
                                                                   stop_token=stop_token, **dims, **kw)
        print(f"caption {s}: {rt.tolist()} score margin {smargin:.3e} set margin {setmargin:.3e}")
        assert smargin >= MARGIN and setmargin >= MARGIN, (s, smargin, setmargin)
        n = rt.numel()
        assert int(lens[s]) == n and toks[s, :n].tolist() == rt.tolist(), (s, toks[s].tolist(), rt.tolist())
        assert (toks[s, n:] == 0).all() and (scores[s, n:] == 0).all()
        assert (scores[s, :n].double() - rs).abs().max().item() <= 1e-3, s
        greedy = contrastive_search_ref(sd, pref[s:s + 1], top_k=top_k, penalty_alpha=0.0, entry_length=ENTRY, stop_token=stop_token, **dims, **kw)[0]
        moved.append(greedy.tolist() != rt.tolist() and slot0 < n)
    return moved


@pytest.mark.parametrize("bans", [{}, BANS], ids=["free", "bans"])
def test_contrastive_search_equals_the_cpu_search(bans):
    from clipcap_amd.inference import generate_contrastive_tokens
    model, sd, pref, dims, _ = _tiny(32)
    out = generate_contrastive_tokens(model, pref.cuda(), 3, 0.5, ENTRY, STOP_E2E, **bans)
    moved = _check_against_cpu(model, sd, pref, dims, out, top_k=3, penalty_alpha=0.5, stop_token=STOP_E2E, **bans)
    assert all(moved)                                                                          # the penalty moved every caption off greedy
    if bans:
        for s in range(pref.shape[0]):
            seq = out[0][s, :int(out[1][s])].tolist()
            assert STOP_E2E not in seq[:3] and len({tuple(seq[i:i + 2]) for i in range(len(seq) - 1)}) == len(seq) - 1, seq


def test_contrastive_search_four_candidates_and_without_the_prefix():
    """Case 1 at top_k = 4, alpha = 0.6, with the prefix positions in the penalty and without: both equal the CPU search, and they differ
    (without the prefix the first token is greedy's 40)."""
    from clipcap_amd.inference import generate_contrastive_tokens
    model, sd, pref, dims, _ = _tiny(32, cases=("1",))
    a = generate_contrastive_tokens(model, pref.cuda(), 4, 0.6, ENTRY, STOP_E2E)
    assert all(_check_against_cpu(model, sd, pref, dims, a, top_k=4, penalty_alpha=0.6, stop_token=STOP_E2E))
    b = generate_contrastive_tokens(model, pref.cuda(), 4, 0.6, ENTRY, STOP_E2E, include_prefix=False)
    _check_against_cpu(model, sd, pref, dims, b, top_k=4, penalty_alpha=0.6, stop_token=STOP_E2E, include_prefix=False)
    assert a[0][0].tolist() != b[0][0].tolist() and int(b[0][0, 0]) == 40 and int(a[0][0, 0]) == 29


def test_contrastive_search_that_never_stops_runs_to_entry_length():
    from clipcap_amd.inference import generate_contrastive_tokens
    model, sd, pref, dims, _ = _tiny(32, cases=("T",))
    out = generate_contrastive_tokens(model, pref.cuda(), 3, 0.5, ENTRY, 5, **BANS)
    _check_against_cpu(model, sd, pref, dims, out, top_k=3, penalty_alpha=0.5, stop_token=5, **BANS)
    assert out[0].shape == (1, ENTRY) and int(out[1][0]) == ENTRY and 5 not in out[0][0].tolist()


def test_alpha_zero_is_the_existing_greedy_decoder():
    from clipcap_amd.inference import generate_beam_tokens, generate_contrastive_tokens
    model, sd, pref, dims, _ = _tiny(32)
    toks, lens, _ = (t.cpu() for t in generate_contrastive_tokens(model, pref.cuda(), 3, 0.0, ENTRY, STOP_E2E))
    bt, _, bl = (t.cpu() for t in generate_beam_tokens(model, pref.cuda(), 1, ENTRY, 1.0, STOP_E2E))
    for s in range(pref.shape[0]):
        n = int(lens[s])
        assert n == int(bl[s, 0]) and toks[s, :n].tolist() == bt[s, 0, :n].tolist(), s
        r = contrastive_search_ref(sd, pref[s:s + 1], top_k=3, penalty_alpha=0.0, entry_length=ENTRY, stop_token=STOP_E2E, **dims)
        assert r[2] >= MARGIN and r[0].tolist() == toks[s, :n].tolist()
    one = generate_contrastive_tokens(model, pref.cuda(), 1, 0.5, ENTRY, STOP_E2E)                # one candidate: greedy too
    assert torch.equal(one[0].cpu()[:, :toks.shape[1]], toks) and torch.equal(one[1].cpu(), lens)


def _run_with_history(precision, **kw):
    """generate_contrastive_tokens with the decode's buffers kept: (tokens, lengths, scores, history)."""
    from clipcap_amd import engine
    from clipcap_amd.inference import contrastive
    model, _, pref, _, V = _tiny(precision)
    kept = []
    make = engine.contrastive_buffers

    def keep(*a):
        kept.append(make(*a))
        return kept[-1]

    contrastive.contrastive_buffers = keep
    try:
        out = contrastive.generate_contrastive_tokens(model, pref.cuda(), 3, 0.5, ENTRY, STOP_E2E, **kw)
    finally:
        contrastive.contrastive_buffers = make
    return [t.cpu() for t in out] + [kept[0].hist.cpu()], V


def test_contrastive_search_is_bit_identical_from_run_to_run():
    a, _ = _run_with_history(32, **BANS)
    b, _ = _run_with_history(32, **BANS)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32)) and torch.equal(a[3].view(torch.int32), b[3].view(torch.int32))
    assert a[3].abs().sum() > 0


def test_contrastive_search_in_bf16_operands_is_well_formed():
    """bf16 operands: structure only — ids inside the vocabulary, nothing but padding behind a stop token, consistent lengths, and the
    same result from run to run."""
    (toks, lens, scores, hist), V = _run_with_history("bf16")
    again, _ = _run_with_history("bf16")
    assert torch.equal(toks, again[0]) and torch.equal(lens, again[1]) and torch.equal(scores.view(torch.int32), again[2].view(torch.int32))
    assert toks.min() >= 0 and toks.max() < V
    for s in range(toks.shape[0]):
        n = int(lens[s])
        seq = toks[s].tolist()
        assert 1 <= n <= ENTRY and STOP_E2E not in seq[:n - 1]
        assert seq[n - 1] == STOP_E2E or n == toks.shape[1] == ENTRY
        assert all(t == 0 for t in seq[n:]) and (scores[s, n:] == 0).all()


def test_generate_contrastive_returns_the_text_with_its_stop_token():
    from tests.test_api_surface import FakeTokenizer
    from clipcap_amd.inference import generate_contrastive, generate_contrastive_tokens
    model, _, pref, _, V = _tiny(32)
    tk = FakeTokenizer(V, STOP_E2E)
    toks, lens, _ = (t.cpu() for t in generate_contrastive_tokens(model, pref.cuda(), 3, 0.5, ENTRY, STOP_E2E))
    texts = generate_contrastive(model, tk, pref.cuda(), top_k=3, penalty_alpha=0.5, entry_length=ENTRY)
    assert texts == [tk.decode(toks[s, :int(lens[s])].numpy()) for s in range(pref.shape[0])]
    assert all(int(toks[s, int(lens[s]) - 1]) == STOP_E2E for s in range(pref.shape[0]))
