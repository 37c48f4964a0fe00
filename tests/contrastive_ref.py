"""Float64 statement of contrastive search (cc_contrastive_topk / cc_contrastive_select, include/clipcap_hip.h; Su et al., 2022) for ONE
caption: the candidates of a logits row, one selection step, and the whole search on the CPU from the oracle's full re-forward.  The GPU
tests compare the kernels and the decoders with this; tests/test_contrastive_ref.py pins it on the CPU."""
from collections import namedtuple

import torch

Select = namedtuple("Select", "sel token score deg scores margin valid")


def contrastive_topk_ref(row: torch.Tensor, k: int):
    """row (V,) logits -> (tokens (k,) int64, probs (k,) float64, set margin).  The ids of the k largest logits, largest first, ties to the
    lower id; their softmax probabilities over the whole row in float64 (-inf entries contribute nothing); a slot without a finite logit
    holds token 0 and probability -1.  Set margin: the gap between the k-th and the (k+1)-th logit (inf when fewer than k + 1 are finite)."""
    x = row.double()
    kk = min(k + 1, x.numel())
    thr = torch.topk(x, kk).values[-1]
    idx = torch.nonzero(x >= thr).flatten().tolist()                    # everything that can rank among the first k + 1, ties included
    order = sorted(idx, key=lambda v: (-float(x[v]), v))[:kk]
    p = torch.softmax(x, -1)
    toks, probs = [], []
    for c in range(k):
        ok = c < len(order) and float(x[order[c]]) > float("-inf")
        toks.append(order[c] if ok else 0)
        probs.append(float(p[order[c]]) if ok else -1.0)
    margin = float("inf")
    if len(order) > k and float(x[order[k]]) > float("-inf"):
        margin = float(x[order[k - 1]] - x[order[k]])
    return torch.tensor(toks), torch.tensor(probs, dtype=torch.float64), margin


def contrastive_select_ref(cand_h, cand_prob, cand_tok, hist, hist_lo: int, hist_n: int, alpha: float, stop_token: int) -> Select:
    """One selection step for one caption that has not stopped: cand_h (k, D) and hist (>= hist_n, D) unit vectors, cand_prob (k,) with -1
    = invalid.  deg(c) = max_j in [hist_lo, hist_n) of dot(cand_h[c], hist[j]) (empty: 0); score(c) = (1 - alpha) p(c) - alpha deg(c) over
    the valid slots; the winner is the largest score, ties to the lowest slot.  No valid slot: the caption stops with stop_token (slot 0,
    score 0, valid False).  margin: best score minus second-best score (inf with fewer than two valid slots)."""
    ch, hs, p = cand_h.double(), hist.double(), cand_prob.double()
    k = ch.shape[0]
    deg = (ch @ hs[hist_lo:hist_n].t()).max(dim=1).values if hist_n > hist_lo else torch.zeros(k, dtype=torch.float64)
    scores = (1.0 - alpha) * p - alpha * deg
    valid = [c for c in range(k) if float(p[c]) >= 0.0]
    if not valid:
        return Select(0, int(stop_token), 0.0, deg, scores, float("inf"), False)
    ranked = sorted(valid, key=lambda c: (-float(scores[c]), c))
    w = ranked[0]
    margin = float(scores[w] - scores[ranked[1]]) if len(ranked) > 1 else float("inf")
    return Select(w, int(cand_tok[w]), float(scores[w]), deg, scores, margin, True)


def _unit(h: torch.Tensor) -> torch.Tensor:
    h = h.double()
    n = h.norm(dim=-1, keepdim=True)
    return torch.where(n > 0, h / n.clamp_min(1e-300), torch.zeros_like(h))


def contrastive_search_ref(sd, embeds, *, n_head, n_layer, top_k, penalty_alpha, entry_length, stop_token, include_prefix=True,
                           no_repeat_ngram_size=0, min_length=0, pre="language_model."):
    """Contrastive search for ONE prefix (1, L, D) on the CPU: the oracle's full re-forward of the k candidate sequences per step
    (oracle.gpt2_hidden, fp32; logits = hidden @ wte^T), the bans of the constrained decoders (inference.utils.banned_tokens, the stop
    token while fewer than min_length tokens are generated) masked into the winner's logits, contrastive_topk_ref and
    contrastive_select_ref.  -> (tokens (n,) int64 with the stop token if it stopped, scores (n,) float64, the smallest score margin, the
    smallest candidate-set margin, greedy_steps: at how many steps the winner was slot 0)."""
    from clipcap_amd.inference.utils import banned_tokens
    from oracle import clipcap_oracle as O
    wte = sd[pre + "transformer.wte.weight"]
    L0 = embeds.shape[1]
    hid, _ = O.gpt2_hidden(sd, embeds, n_head, n_layer, pre=pre + "transformer.")
    hist = _unit(hid[0])                                                # (L0, D): the prefix positions
    hist_lo = 0 if include_prefix else L0
    tokens, scores = [], []
    smargin, setmargin, slot0 = float("inf"), float("inf"), 0

    def candidates(h_last):
        nonlocal setmargin
        logits = (h_last @ wte.t()).clone()
        ban = banned_tokens(tokens, no_repeat_ngram_size) | ({stop_token} if len(tokens) < min_length else set())
        if ban:
            logits[sorted(ban)] = float("-inf")
        t, p, m = contrastive_topk_ref(logits, top_k)
        setmargin = min(setmargin, m)
        return t, p

    cand_tok, cand_prob = candidates(hid[0, -1])
    for i in range(entry_length):
        rows = torch.cat((embeds.expand(top_k, -1, -1), wte[cand_tok].view(top_k, 1, -1)), dim=1)
        hid, _ = O.gpt2_hidden(sd, rows, n_head, n_layer, pre=pre + "transformer.")
        r = contrastive_select_ref(_unit(hid[:, -1]), cand_prob, cand_tok, hist, hist_lo, L0 + i, penalty_alpha, stop_token)
        smargin = min(smargin, r.margin)
        slot0 += int(r.sel == 0)
        tokens.append(r.token)
        scores.append(r.score)
        if r.token == stop_token or i + 1 == entry_length:
            break
        hist = torch.cat((hist, _unit(hid[r.sel, -1]).view(1, -1)))
        embeds = rows[r.sel:r.sel + 1]
        cand_tok, cand_prob = candidates(hid[r.sel, -1])
    return torch.tensor(tokens), torch.tensor(scores, dtype=torch.float64), smargin, setmargin, slot0
