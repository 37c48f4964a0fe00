"""Contrastive search on the HIP path (not in the reference: Su et al., 2022, "A Contrastive Framework for Neural Text Generation" — the
decoder of the same authors' MAGIC captioner; ``penalty_alpha`` / ``top_k`` of the transformers library): a deterministic decoder that
needs no sampling seed and no beam bookkeeping, and that prevents the repetition greedy and beam search fall into ("a man a man a man")
instead of banning it after the fact.

At every step the model's ``top_k`` most probable tokens are run through the model, and the one kept is the candidate c with the largest

    (1 - penalty_alpha) * p(c) - penalty_alpha * max_j cos(h_c, h_j)

h_c = the candidate's final hidden state (after ln_f), h_j = the final hidden states of the context so far (the prefix positions and the
tokens already kept; ``include_prefix=False`` leaves the prefix positions, which are mapped image embeddings and not text, out).

On the device the k candidates of a caption are the k rows of one decode group (the rows of a beam: they share one KV ancestry), so a step
is the width-k beam step's forward plus four small launches:
  forward(group=k) -> hidden_unit (cc_decode_hidden_unit: ln_f of the fp32 residual, L2-normalised) -> contrastive_select (similarities,
  maxima, scores, winner, commit) -> [cc_logits_constrain on the winner's row] -> contrastive_topk on the winner's logits ->
  cc_beam_advance (every row of the caption continues the winner with one of the new candidates).
With ``penalty_alpha == 0`` or ``top_k == 1`` the same code path is greedy decoding.  The keyword-only constraints are those of the other
decoders (inference/base.py); a banned token cannot become a candidate.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Tuple

import torch

from clipcap_amd.engine import DecodeSession, contrastive_buffers, contrastive_select, contrastive_topk
from clipcap_amd.inference.base import _bans, _persistent_decode_on, _stop_id, _with_text_prefix
from clipcap_amd.inference.utils import validate_contrastive


@torch.no_grad()
def generate_contrastive_tokens(model, embeds: torch.Tensor, top_k: int = 4, penalty_alpha: float = 0.6, entry_length: int = 67,
                                stop_token: int = 50256, *, include_prefix: bool = True, no_repeat_ngram_size: int = 0, min_length: int = 0,
                                suppress_tokens=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Contrastive search for a batch of prefixes, embeds fp32 (S, L, D); every step on the device, no host sync except an
    all-captions-stopped poll every 4th step.  Returns (tokens int64 (S, n), lengths int64 (S,), scores fp32 (S, n)): row s holds
    lengths[s] generated tokens, its stop token included if it stopped, then padding (token 0, score 0); scores[s, i] is the winning
    (1 - alpha) p - alpha max-cos of step i."""
    lm = model.language_model
    g = lm.engine
    dev = g.arena.device
    validate_contrastive(top_k, penalty_alpha)
    k, alpha = int(top_k), float(penalty_alpha)
    V = g.dims["V"]
    bans = _bans(V, stop_token, no_repeat_ngram_size, min_length, suppress_tokens, dev)
    if entry_length < 1:
        raise ValueError(f"entry_length must be >= 1, got {entry_length}")
    if _persistent_decode_on():
        raise RuntimeError("contrastive search does not support the persistent decode engines (cc_decode_mode bits 1 and 2)")
    embeds = embeds.to(dev, torch.float32)
    S, L0, D = embeds.shape
    R = S * k
    total = min(int(entry_length), g.dims["NPOS"] - L0)
    if total < 1:
        raise RuntimeError(f"a {L0}-position prefix leaves no room to generate (n_positions = {g.dims['NPOS']})")
    wte = lm.get_input_embeddings().weight.detach()
    b = contrastive_buffers(dev, S, k, D, L0 + total, total)
    hist_lo = 0 if include_prefix else L0
    # prefill: one row per caption; the prefix positions' hidden states go straight into the history
    sess = DecodeSession(g, S, L0 + total)
    logits = sess.forward(embeds)                                               # (S, V)
    sess.hidden_unit(b.hist, b.hist.stride(0), D)
    if bans is not None:
        bans.apply(logits, 0)                                                   # no history yet
    contrastive_topk(logits, S, 1, None, k, None, b.cand_tok, b.cand_prob)
    base = torch.arange(S, device=dev, dtype=torch.int32).repeat_interleave(k)
    sess = sess.expand(base, R)
    # token histories (int32, ping-pong), the next input embedding and the cache ancestry: one launch per step, as in beam search
    tok = [torch.zeros(R, total, dtype=torch.int32, device=dev) for _ in range(2)]
    x = torch.empty(R, 1, D, dtype=torch.float32, device=dev)
    sess.beam_advance(k, b.cand_tok, None, wte, 0, tok[1], tok[0], x)
    n = 0                                                                       # tokens decided so far
    for i in range(total):
        # steps taken after every caption has stopped only append padding: polling the flags every 4th step cannot change the result
        if i % 4 == 1 and bool(b.stopped.all()):
            break
        logits = sess.forward(x, group=k)                                       # the k candidates of every caption: (R, V)
        sess.hidden_unit(b.cand_h, D, D)
        contrastive_select(b, k, hist_lo, L0 + i, alpha, stop_token, i)         # token i of every caption
        n = i + 1
        if n == total:
            break                                                               # the last token needs no further candidates
        if bans is not None:                                                    # only the winner's row of a caption that goes on is read below
            bans.apply(logits, n, tok[i & 1], n, None, b.skip_rows)
        contrastive_topk(logits, S, k, b.sel, k, b.stopped, b.cand_tok, b.cand_prob)
        sess.beam_advance(k, b.cand_tok, b.src_rows, wte, n, tok[i & 1], tok[n & 1], x)
    if n == total and total < int(entry_length) and not bool(b.stopped.all()):
        raise RuntimeError(f"generation reached n_positions = {g.dims['NPOS']} ({L0}-position prefix + {n} tokens)")
    return b.captions[:, :n].to(torch.int64), b.lengths.to(torch.int64), b.scores[:n].t().contiguous()


def generate_contrastive(model, tokenizer: Callable, embeds: torch.Tensor, text_prefix_tokens: Optional[torch.Tensor] = None, top_k: int = 4,
                         penalty_alpha: float = 0.6, entry_length: int = 67, *, include_prefix: bool = True, no_repeat_ngram_size: int = 0,
                         min_length: int = 0, suppress_tokens=None) -> List[str]:
    """One caption per prefix row of ``embeds`` (S, L, D) by contrastive search (module docstring).  ``text_prefix_tokens`` enter as
    embeddings behind the prefix, as in generate_beam, and count as prefix positions.  The text of a row includes its stop token, as
    generate_beam's does."""
    validate_contrastive(top_k, penalty_alpha)
    stop = _stop_id(tokenizer)
    embeds = _with_text_prefix(model, embeds, text_prefix_tokens)
    tokens, lengths, _ = generate_contrastive_tokens(model, embeds, top_k, penalty_alpha, entry_length, stop, include_prefix=include_prefix,
                                                     no_repeat_ngram_size=no_repeat_ngram_size, min_length=min_length,
                                                     suppress_tokens=suppress_tokens)
    tokens, lengths = tokens.cpu(), lengths.cpu()
    return [tokenizer.decode(tokens[s, :int(lengths[s])].numpy()) for s in range(tokens.shape[0])]
