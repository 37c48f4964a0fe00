"""Float64 statement of one diverse-beam-search update (cc_beam_group_step, include/clipcap_hip.h) for ONE sample: the beam rows are
``groups`` beam groups of W = beam / groups consecutive rows, advanced in order; beam group g takes the reference's beam update
(inference/base.py:84-119) on its own rows, and the log-probability of a non-stopped row's token v loses penalty * c(v), c(v) = the
picks of v made at this step by beam groups 0 .. g - 1 from rows that had not stopped.  Candidates are ordered by value descending, then
flat index b_local * V + v ascending.  The GPU tests compare the kernels with this; tests/test_beam_group_ref.py pins it on the CPU."""
from collections import namedtuple

import torch

GroupStep = namedtuple("GroupStep", "tokens src scores lengths stopped margins")


def _best(vals: torch.Tensor, k: int):
    """Flat indices of the k + 1 best entries of a 1-D float64 tensor (value descending, index ascending), fewer if it is shorter."""
    k1 = min(k + 1, vals.numel())
    thr = torch.topk(vals, k1).values[-1]
    idx = torch.nonzero(vals >= thr).flatten()                        # everything that can rank among the first k + 1, ties included
    order = sorted(idx.tolist(), key=lambda i: (-float(vals[i]), i))
    return order[:k1]


def _gap(a: float, b: float) -> float:
    return 0.0 if a == b else a - b                                   # (-inf, -inf): tied, not nan


def beam_group_step_ref(logits, scores, seq_lengths, has_stopped, *, beam, groups, temperature=1.0, penalty=0.0, first=False,
                        stop_token=50256) -> GroupStep:
    """logits (beam, V) (first: only row 0 is read); scores, seq_lengths (beam,) and has_stopped (beam,) bool are the state BEFORE the
    step (ignored when ``first``).  Returns the new state in float64: tokens, src (source row inside the sample; 0 on the first step),
    scores (= average * length, base.py:114), lengths, stop flags, and per beam group the decision margin: the smallest gap between
    consecutive kept values and between the last kept and the first rejected candidate."""
    assert beam % groups == 0
    W = beam // groups
    V = logits.shape[1]
    lp_all = torch.log_softmax(logits.double() / (temperature if temperature > 0 else 1.0), -1)
    scores = None if first else scores.double()
    seq_lengths = None if first else seq_lengths.double()
    counts = {}                                                        # token -> picks by the earlier beam groups at this step
    tokens, src, nscores, nlen, nstop, margins = [], [], [], [], [], []
    for g in range(groups):
        rows = [0] if first else list(range(g * W, (g + 1) * W))
        vals = []
        for r in rows:
            if not first and bool(has_stopped[r]):                    # base.py:96-101: only token 0 continues a stopped beam, at its average
                v = torch.full((V,), float("-inf"), dtype=torch.float64)
                v[0] = scores[r] / seq_lengths[r]
            else:
                lp = lp_all[r].clone()
                for t, c in counts.items():
                    lp[t] -= penalty * c
                v = lp if first else (scores[r] + lp) / (seq_lengths[r] + 1.0)
            vals.append(v)
        vals = torch.cat(vals)
        order = _best(vals, W)
        kept = order[:W]
        assert len(kept) == W
        margins.append(min(_gap(float(vals[a]), float(vals[b])) for a, b in zip(order, order[1:])) if len(order) > 1 else float("inf"))
        picked = []
        for i in kept:
            b, v = rows[i // V], i % V
            st = False if first else bool(has_stopped[b])
            ln = 1.0 if first else float(seq_lengths[b]) + (0.0 if st else 1.0)
            tokens.append(v); src.append(b); nlen.append(ln); nscores.append(float(vals[i]) * ln)
            nstop.append(st or v == stop_token)
            if not st:
                picked.append(v)
        for v in picked:                                               # visible to the beam groups after this one only
            counts[v] = counts.get(v, 0) + 1
    return GroupStep(torch.tensor(tokens), torch.tensor(src), torch.tensor(nscores, dtype=torch.float64),
                     torch.tensor(nlen, dtype=torch.float64), torch.tensor(nstop), margins)


def beam_group_search_ref(sd, embeds, *, n_head, n_layer, beam, groups, penalty, entry_length, stop_token, temperature=1.0,
                          no_repeat_ngram_size=0, min_length=0, pre="language_model."):
    """Diverse beam search for ONE prefix (1, L, D) on the CPU: the oracle's full re-forward per step (oracle.gpt2_logits, fp32), the bans of
    the constrained decoders masked into the logits of every beam that has not stopped, and beam_group_step_ref for the update.
    -> (tokens (beam, n) int64, length-normalised scores, seq_lengths, the smallest decision margin of any beam group at any step)."""
    from clipcap_amd.inference.utils import banned_tokens
    from oracle import clipcap_oracle as O
    wte = sd[pre + "transformer.wte.weight"]
    tokens, scores, seql, stopped = None, None, None, None
    margin = float("inf")
    for step in range(entry_length):
        logits = O.gpt2_logits(sd, embeds, n_head, n_layer, pre=pre)[:, -1, :].clone()
        for r in range(logits.shape[0]):
            if tokens is not None and bool(stopped[r]):
                continue
            ban = (banned_tokens(tokens[r], no_repeat_ngram_size) if tokens is not None else set()) | ({stop_token} if step < min_length else set())
            if ban:
                logits[r, sorted(ban)] = float("-inf")
        first = tokens is None
        r = beam_group_step_ref(logits.expand(beam, -1) if first else logits, scores, seql, stopped, beam=beam, groups=groups,
                                temperature=temperature, penalty=penalty, first=first, stop_token=stop_token)
        margin = min(margin, min(r.margins))
        scores, seql, stopped = r.scores, r.lengths, r.stopped
        if first:
            embeds = embeds.expand(beam, *embeds.shape[1:])
            tokens = r.tokens.unsqueeze(1)
        else:
            tokens = torch.cat((tokens[r.src], r.tokens.unsqueeze(1)), dim=1)
            embeds = embeds[r.src]
        embeds = torch.cat((embeds, wte[r.tokens].view(beam, 1, -1)), dim=1)
        if bool(stopped.all()):
            break
    return tokens, scores / seql, seql, margin
