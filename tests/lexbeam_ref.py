"""Float64 statement of lexically constrained beam search's device step (cc_beam_lex_step, include/clipcap_hip.h; dynamic beam allocation,
Post & Vilar 2018) for ONE sample, and of a whole search for one prefix.  Written literally over all beam * V candidates: the values are
the plain beam update's, a candidate's validity, the candidate set K = T + B + P, the transition, the banks and the round-robin as the header
states them, without the kernels' row lists.  The GPU tests compare the kernels with this; tests/test_lexbeam_ref.py pins it on the CPU.

A sample's phrases are a list of token-id lists (an empty list or one that begins with a negative id: the phrase does not exist; ids after
the first negative one are ignored), which is the device table row by row."""
from collections import namedtuple

import torch

LexStep = namedtuple("LexStep", "tokens src scores lengths stopped states margin")
INF = float("inf")


# ---- the row state ----------------------------------------------------------------------------------------------------------------------
def pack(met: int, cur: int, pos: int) -> int:
    """bits 0-7 met | bits 8-11 cur + 1 (cur = -1: none) | bits 12-15 pos"""
    return (met & 0xFF) | (((cur + 1) & 0xF) << 8) | ((pos & 0xF) << 12)


def unpack(state: int):
    return state & 0xFF, ((state >> 8) & 0xF) - 1, (state >> 12) & 0xF


def clean(phrases):
    """every phrase cut at its first negative id"""
    out = []
    for p in phrases:
        q = []
        for t in p:
            if int(t) < 0:
                break
            q.append(int(t))
        out.append(q)
    return out


def full_mask(phrases) -> int:
    return sum(1 << c for c, p in enumerate(clean(phrases)) if p)


def tokens_met(state: int, phrases) -> int:
    met, cur, pos = unpack(state)
    return sum(len(p) for c, p in enumerate(clean(phrases)) if met >> c & 1) + (pos if cur >= 0 else 0)


def lex_next(state: int, v: int, phrases) -> int:
    """the state after token v from a parent that has not stopped"""
    ph = clean(phrases)
    met, cur, pos = unpack(state)
    if cur >= 0 and pos < len(ph[cur]) and ph[cur][pos] == v:
        return pack(met | 1 << cur, -1, 0) if pos + 1 == len(ph[cur]) else pack(met, cur, pos + 1)
    for c, p in enumerate(ph):
        if p and not met >> c & 1 and p[0] == v:
            return pack(met | 1 << c, -1, 0) if len(p) == 1 else pack(met, c, 1)
    return pack(met, -1, 0)


def phrase_table(phrases, n_phr: int, phr_len: int) -> torch.Tensor:
    """int32 (n_phr, phr_len), -1 padded: one sample's slice of the device table"""
    t = torch.full((n_phr, phr_len), -1, dtype=torch.int32)
    for c, p in enumerate(clean(phrases)):
        t[c, :len(p)] = torch.tensor(p, dtype=torch.int32)
    return t


# ---- one step ---------------------------------------------------------------------------------------------------------------------------
def _gap(a: float, b: float) -> float:
    return 0.0 if a == b else a - b


def lex_step_ref(logits, scores, seq_lengths, has_stopped, states, *, beam, phrases, temperature=1.0, first=False, stop_token=50256) -> LexStep:
    """logits (beam, V) (first: only row 0 is read); scores, seq_lengths (beam,), has_stopped (beam,) bool and states (beam,) ints are the
    state BEFORE the step (ignored when ``first``).  Returns the new state in float64: tokens, src (source row inside the sample; 0 on the
    first step), scores (= average * length), lengths, stop flags, row states, and the step's decision margin: the smallest gap between a
    picked candidate and the best not yet picked member of K in its bank, between the last member and the first non-member of T, and, for
    a picked candidate that is in K only as its row's best, to the row's second best."""
    V = logits.shape[1]
    ph = clean(phrases)
    full = full_mask(ph)
    nrows = 1 if first else beam
    T = temperature if temperature > 0 else 1.0
    st = [False] * nrows if first else [bool(x) for x in has_stopped]
    state = [0] * nrows if first else [int(x) for x in states]
    vals = torch.full((nrows, V), -INF, dtype=torch.float64)
    for b in range(nrows):
        if st[b]:                                                        # only token 0 continues a stopped beam, at its own average
            vals[b, 0] = float(scores[b]) / float(seq_lengths[b])
        else:
            lp = torch.log_softmax(logits[b].double() / T, -1)
            vals[b] = lp if first else (float(scores[b]) + lp) / (float(seq_lengths[b]) + 1.0)
            if unpack(state[b])[0] != full:
                vals[b, stop_token] = -INF                               # the candidate is banned, the softmax above kept the token
    vals[torch.isnan(vals)] = -INF
    flat = vals.view(-1)
    key = lambda i: (-float(flat[i]), i)  # noqa: E731
    valid = torch.nonzero(flat > -INF).flatten().tolist()
    margin = INF
    # T: the beam best valid candidates
    k1 = min(beam + 1, len(valid))
    order = []
    if k1:
        thr = torch.topk(flat, k1).values[-1]
        order = sorted(torch.nonzero(flat >= thr).flatten().tolist(), key=key)[:k1]
    if len(order) > beam:
        margin = min(margin, _gap(float(flat[order[beam - 1]]), float(flat[order[beam]])))
    in_t = set(order[:beam])
    K = set(in_t)
    # B: every row's best valid candidate
    second = {}
    for b in range(nrows):
        row = vals[b]
        if float(row.max()) > -INF:
            top = torch.topk(row, min(2, V))
            best = sorted(torch.nonzero(row >= top.values[0]).flatten().tolist())[0]
            K.add(b * V + best)
            rest = row.clone()
            rest[best] = -INF
            second[b * V + best] = float(rest.max())
    only_b = {i for i in K if i not in in_t}
    # P: what advances a phrase of a parent that has not stopped
    for b in range(nrows):
        if st[b]:
            continue
        met, cur, pos = unpack(state[b])
        want = [ph[cur][pos]] if cur >= 0 else []
        want += [p[0] for c, p in enumerate(ph) if p and not met >> c & 1]
        for v in want:
            if 0 <= v < V and float(vals[b, v]) > -INF:
                K.add(b * V + v)
                only_b.discard(b * V + v)
    new = {i: (state[i // V] if st[i // V] else lex_next(state[i // V], i % V, ph)) for i in K}
    banks = {}
    for i in K:
        banks.setdefault(tokens_met(new[i], ph), []).append(i)
    for k in banks:
        banks[k].sort(key=key)
    picked = []
    while len(picked) < beam and any(banks.values()):
        for k in sorted(banks, reverse=True):
            if banks[k] and len(picked) < beam:
                i = banks[k].pop(0)
                if banks[k]:
                    margin = min(margin, _gap(float(flat[i]), float(flat[banks[k][0]])))
                if i in only_b:
                    margin = min(margin, _gap(float(flat[i]), second[i]))
                picked.append(i)
    tokens, src, nsc, nlen, nstop, nstate = [], [], [], [], [], []
    for k in range(beam):
        if k < len(picked):
            i = picked[k]
            b, v = i // V, i % V
            ln = 1.0 if first else float(seq_lengths[b]) + (0.0 if st[b] else 1.0)
            tokens.append(v); src.append(b); nlen.append(ln); nsc.append(float(flat[i]) * ln)
            nstop.append(st[b] or v == stop_token); nstate.append(new[i])
        else:                                                            # an empty slot
            tokens.append(0); src.append(0); nsc.append(-INF); nstop.append(True); nstate.append(0)
            nlen.append(1.0 if first else float(seq_lengths[0]))
    return LexStep(torch.tensor(tokens), torch.tensor(src), torch.tensor(nsc, dtype=torch.float64), torch.tensor(nlen, dtype=torch.float64),
                   torch.tensor(nstop), torch.tensor(nstate, dtype=torch.int64), margin)


# ---- a whole search for one prefix ------------------------------------------------------------------------------------------------------
def lex_search_ref(sd, embeds, phrases, *, n_head, n_layer, beam, entry_length, stop_token, temperature=1.0, no_repeat_ngram_size=0, min_length=0,
                   negative=None, scale=1.0, pre="language_model."):
    """Constrained beam search for ONE prefix (1, L, D) on the CPU: the oracle's full re-forward per step (oracle.gpt2_logits, fp32; with
    ``negative`` (1, Ln, D) both streams, combined in float64 by guide_ref), the bans of the constrained decoders masked into the logits of
    every beam that has not stopped, and lex_step_ref for the update.
    -> (tokens (beam, n) int64, length-normalised scores, seq_lengths, row states, the smallest decision margin at any step)."""
    from clipcap_amd.inference.utils import banned_tokens
    from oracle import clipcap_oracle as O
    from tests.guide_ref import guide_ref
    wte = sd[pre + "transformer.wte.weight"]
    tokens, scores, seql, stopped, states = None, None, None, None, None
    margin = INF
    for step in range(entry_length):
        logits = O.gpt2_logits(sd, embeds, n_head, n_layer, pre=pre)[:, -1, :].clone()
        if negative is not None:
            lu = O.gpt2_logits(sd, negative, n_head, n_layer, pre=pre)[:, -1, :]
            logits = torch.from_numpy(guide_ref(logits.numpy(), lu.numpy(), scale)[0])
        for r in range(logits.shape[0]):
            if tokens is not None and bool(stopped[r]):
                continue
            ban = (banned_tokens(tokens[r], no_repeat_ngram_size) if tokens is not None else set()) | ({stop_token} if step < min_length else set())
            if ban:
                logits[r, sorted(ban)] = -INF
        first = tokens is None
        r = lex_step_ref(logits.expand(beam, -1) if first else logits, scores, seql, stopped, states, beam=beam, phrases=phrases,
                         temperature=temperature, first=first, stop_token=stop_token)
        margin = min(margin, r.margin)
        scores, seql, stopped, states = r.scores, r.lengths, r.stopped, r.states
        if first:
            embeds = embeds.expand(beam, *embeds.shape[1:])
            tokens = r.tokens.unsqueeze(1)
            if negative is not None:
                negative = negative.expand(beam, *negative.shape[1:])
        else:
            tokens = torch.cat((tokens[r.src], r.tokens.unsqueeze(1)), dim=1)
            embeds = embeds[r.src]
            if negative is not None:
                negative = negative[r.src]
        nxt = wte[r.tokens].view(beam, 1, -1)
        embeds = torch.cat((embeds, nxt), dim=1)
        if negative is not None:
            negative = torch.cat((negative, nxt), dim=1)
        if bool(stopped.all()):
            break
    return tokens, scores / seql, seql, states, margin
