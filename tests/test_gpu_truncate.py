"""cc_logits_truncate (clipcap_amd/csrc/truncate.hip) through the C ABI against the float64 statement (tests/truncate_ref.py), and the
sampling decoder with the rules on, end to end.

Every call runs on buffers a stray access shows in: the logits have ld = V + 13 with NaN in the padding (it must come back bit for bit),
the history hist_ld = hist_len + 3 with the row's next-largest tokens beyond hist_len (a read of them would penalise them visibly).  The
kept set is held to the reference's report: surely-kept tokens kept, surely-removed ones -inf, undecided ones either way, the typical cut
anywhere in its window with groups of equal value whole; kept logits bit-identical to the input.  Every case is launched twice (same bits)
and every row once more alone (same bits as among the others).  The bounds are derived in tests/truncate_ref.py, none tuned;
tests/test_truncate_ref.py shows on the CPU that they reject every emulated defect at these very cases."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import seeded
from tests import truncate_ref as T

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_SHAPE = -1, -2


def _lib():
    from clipcap_amd import _lib
    return _lib.lib()


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _call(c, buf, hist, rows=None, P=None):
    """the case's call on device buffers, all rows or the one row ``rows``"""
    P = c.P if P is None else P
    r0, n = (0, c.R) if rows is None else (rows, 1)
    return _lib().cc_logits_truncate(C.c_void_p(buf.data_ptr() + 4 * r0 * c.ld), n, c.V, c.ld, P.temperature,
                                     None if hist is None else C.c_void_p(hist.data_ptr() + 8 * r0 * c.hist_ld), P.hist_len, c.hist_ld,
                                     float(P.rep_pen), *P.args(), _st())


def walk(c):
    fresh = torch.from_numpy(c.padded()).cuda()
    hist = None if c.hist is None else torch.from_numpy(c.hist).cuda()
    buf = fresh.clone()
    assert _call(c, buf, hist) == 0, c.name
    torch.cuda.synchronize()
    T.check_case(c, buf.cpu().numpy())
    again = fresh.clone()
    assert _call(c, again, hist) == 0 and torch.equal(_bits(buf), _bits(again)), f"{c.name}: two launches differ"
    alone = fresh.clone()
    for r in range(c.R):
        assert _call(c, alone, hist, rows=r) == 0
    assert torch.equal(_bits(buf), _bits(alone)), f"{c.name}: a row alone differs from the row among the others"
    if c.hist is None:                                           # a history of length 0 is not read, whatever the penalty
        top = np.argsort(-c.x, axis=1, kind="stable")[:, :c.hist_ld]
        h0 = torch.from_numpy(np.ascontiguousarray(np.resize(top, (c.R, c.hist_ld)), dtype=np.int64)).cuda()
        P = T.Params(c.P.temperature, 1.2, 0, *c.P.args())
        empty = fresh.clone()
        assert _call(c, empty, h0, P=P) == 0 and torch.equal(_bits(buf), _bits(empty)), f"{c.name}: a history of length 0 was read"
    return sum(ref.n_undecided for ref in c.refs()), max(ref.window for ref in c.refs())


GROUPS = ("designed", "random-small", "random-50257")


def _group(c):
    return c.kind if c.kind == "designed" else ("random-50257" if c.V == 50257 else "random-small")


@pytest.mark.parametrize("group", GROUPS)
def test_truncation_against_float64(group):
    cases = [c for c in T.all_cases() if _group(c) == group]
    assert cases
    und = win = rows = 0
    for c in cases:
        u, w = walk(c)
        und, win, rows = und + u, max(win, w), rows + c.R
    print(f"{group}: {len(cases)} cases, {rows} rows, {und} undecided tokens in all, widest typical window {win}")


def test_each_rule_alone_on_the_all_rules_cases():
    """the cases with all four rules on, once more with each rule alone: only the rules that are on act"""
    n = 0
    for c in T.all_cases():
        if not all(c.P.on.values()) or c.V > 4099:
            continue
        for rule in T.RULES:
            walk(T.Case(f"{c.name}-only-{rule}", c.kind, c.x, c.P.only(rule), c.hist))
            n += 1
    assert n >= 8


def test_off_call_and_no_rows_launch_nothing():
    c = T.by_name("designed-V97-eta")
    fresh = torch.from_numpy(c.padded()).cuda()
    buf = fresh.clone()
    off = T.Params(temperature=0.7)
    assert _call(c, buf, None, P=off) == 0
    assert _lib().cc_logits_truncate(C.c_void_p(buf.data_ptr()), 0, c.V, c.ld, 1.0, None, 0, 0, 1.0, *c.P.args(), _st()) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf), _bits(fresh))


def test_error_codes_leave_the_buffer_alone():
    c = T.by_name("designed-penalty-crosses-min-p")
    fresh = torch.from_numpy(c.padded()).cuda()
    hist = torch.from_numpy(c.hist).cuda()
    buf = fresh.clone()
    f, x, h = _lib().cc_logits_truncate, C.c_void_p(buf.data_ptr()), C.c_void_p(hist.data_ptr())
    nan = float("nan")

    def call(logits=x, R=c.R, V=c.V, ldl=c.ld, hist=h, hl=c.P.hist_len, hld=c.hist_ld, min_p=0.3, typ=1.0, eps=0.0, eta=0.0):
        return f(logits, R, V, ldl, 1.0, hist, hl, hld, 2.0, min_p, typ, eps, eta, _st())

    for bad in (dict(R=-1), dict(V=0), dict(ldl=c.V - 1), dict(min_p=1.5), dict(min_p=nan), dict(typ=0.0), dict(typ=nan), dict(eps=1.0),
                dict(eps=nan), dict(eta=-0.1), dict(eta=nan), dict(hist=None), dict(hld=c.P.hist_len - 1), dict(logits=None)):
        assert call(**bad) == ERR_ARG, bad
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf), _bits(fresh))
    assert call() == 0
    torch.cuda.synchronize()
    T.check_case(c, buf.cpu().numpy())


def test_lds_edge_runs_and_one_more_token_is_refused():
    c = T.lds_edge()
    assert T.lds_bytes(c.V) <= T.LDS_LIMIT < T.lds_bytes(c.V + 1)
    walk(c)
    V = c.V + 1
    big = torch.zeros(1, V + T.PAD, device="cuda")
    rc = _lib().cc_logits_truncate(C.c_void_p(big.data_ptr()), 1, V, V + T.PAD, 1.0, None, 0, 0, 1.0, *c.P.args(), _st())
    torch.cuda.synchronize()
    assert rc == ERR_SHAPE and not big.any()
    print(f"{c.name}: {T.lds_bytes(c.V)} bytes of LDS")


# ---- end to end: the sampling decoder on a small seeded GPT-2 -------------------------------------------------------------------------------
D, NL, NH, V2, NPOS, ROWS, L0, ENTRY, STOP, SEED = 64, 2, 2, 331, 32, 4, 3, 8, 330, 5100
TEMP, REP = 0.8, 1.2
_MODEL = []


def _model():
    from types import SimpleNamespace
    from clipcap_amd.model.gpt2 import GPT2LM
    if not _MODEL:
        gsd = seeded.state_dict(seeded.gpt2_shapes(D, NL, V2, NPOS), SEED)
        gsd["transformer.wte.weight"] = gsd["transformer.wte.weight"] * 4.0          # the last token leads by a few units, the rest stays spread
        lm = GPT2LM(n_embd=D, n_layer=NL, n_head=NH, vocab_size=V2, n_positions=NPOS, precision=32)
        lm.load_state_dict({k: torch.from_numpy(v) for k, v in gsd.items()}, strict=False)
        pref = torch.randn(ROWS, L0, D, generator=torch.Generator().manual_seed(SEED)) * 0.5
        _MODEL.append((SimpleNamespace(language_model=lm.to("cuda")), pref.cuda()))
    return _MODEL[0]


def _by_hand(model, pref, P, top_p, seed):
    """sample_tokens's loop from the entry points that were there before, the truncation as the float64 kept set applied from outside.
    -> (tokens (R, n), n = the steps up to and including the first one whose reference is not decided, tokens removed per step)"""
    from clipcap_amd.engine import DecodeSession, embed_tokens, sample_step
    g = model.language_model.engine
    sess = DecodeSession(g, ROWS, L0 + ENTRY)
    gen = torch.Generator(device="cuda").manual_seed(seed)
    hist = torch.zeros(ROWS, ENTRY, dtype=torch.int64, device="cuda")
    xbuf = torch.empty(ROWS, 1, D, dtype=torch.float32, device="cuda")
    x, removed, valid = pref, [], ENTRY
    for step in range(ENTRY):
        logits = sess.forward(x)
        lg, hs = logits.cpu().numpy(), hist.cpu().numpy()
        Ps = T.Params(P.temperature, float(P.rep_pen), step, *P.args())
        refs = [T.RowRef(lg[r], Ps, hs[r]) for r in range(ROWS)]
        if not all(ref.decided for ref in refs):
            valid = step
            break
        drop = torch.from_numpy(np.stack([~ref.kept & ref.fin for ref in refs])).cuda()
        removed.append(int(drop.sum()))
        logits.masked_fill_(drop, float("-inf"))
        u = torch.rand(ROWS, device="cuda", generator=gen)
        nxt = sample_step(logits, u, temperature=P.temperature, top_p=top_p, mode=0, history=hist, hist_len=step, repetition_penalty=float(P.rep_pen))
        hist[:, step] = nxt
        x = embed_tokens(g, nxt, xbuf)
    return hist[:, :valid].cpu(), valid, removed


RULE_VALUES = dict(min_p=0.2, typical_p=0.6, epsilon_cutoff=4e-3, eta_cutoff=2e-2)


@pytest.mark.parametrize("rule", T.RULES + ("all",))
def test_sample_tokens_equals_the_loop_with_the_float64_kept_set(rule):
    from clipcap_amd.inference.base import sample_tokens
    model, pref = _model()
    opts = dict(RULE_VALUES) if rule == "all" else {rule: RULE_VALUES[rule]}
    P = T.Params(TEMP, REP, 0, **opts)
    want, valid, removed = _by_hand(model, pref, P, 0.9, SEED)
    assert valid >= 4 and all(n > 0 for n in removed), (valid, removed)             # the rule cut something at every compared step
    got, _ = sample_tokens(model, pref, ENTRY, STOP, mode=0, top_p=0.9, temperature=TEMP, repetition_penalty=REP,
                           generator=torch.Generator(device="cuda").manual_seed(SEED), **opts)
    n = min(valid, got.shape[1])
    assert n >= 4 and torch.equal(got[:, :n].cpu(), want[:, :n]), (got.cpu().tolist(), want.tolist())
    print(f"{rule}: {n} steps compared, tokens removed per step {removed[:n]}")


def test_sample_tokens_with_every_rule_off_is_the_decoder_as_it_was(monkeypatch):
    from clipcap_amd import engine
    from clipcap_amd.inference.base import sample_tokens
    model, pref = _model()
    want, valid, _ = _by_hand(model, pref, T.Params(TEMP, REP, 0), 0.9, SEED)         # no rule on: nothing removed, the plain loop
    assert valid == ENTRY
    calls = []
    real = engine.truncate_logits
    monkeypatch.setattr(engine, "truncate_logits", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    got, _ = sample_tokens(model, pref, ENTRY, STOP, mode=0, top_p=0.9, temperature=TEMP, repetition_penalty=REP,
                           generator=torch.Generator(device="cuda").manual_seed(SEED))
    assert not calls                                                                 # no launch is made
    n = got.shape[1]
    assert torch.equal(got.cpu(), want[:, :n])
    on, _ = sample_tokens(model, pref, ENTRY, STOP, mode=0, top_p=0.9, temperature=TEMP, repetition_penalty=REP,
                          generator=torch.Generator(device="cuda").manual_seed(SEED), min_p=0.2)
    assert calls and not torch.equal(on[:, :min(n, on.shape[1])].cpu(), want[:, :min(n, on.shape[1])])      # and the option does act
