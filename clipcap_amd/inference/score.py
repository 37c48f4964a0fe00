"""Caption likelihoods under the captioner: ``log p(caption | prefix)`` per token and per sample, and reranking by it.

The reference has no likelihood entry point (its demo reranks with CLAP, an encoder); this is the language-model side of the same
job: rerank the ``number_to_generate`` captions of generate_nucleus_sampling, held-out loss / perplexity (clipcap_amd.train.evaluate),
likelihood-based retrieval.  One forward-only pass per call whose lm_head keeps no logits (ClipCapEngine.score, cc_lmhead_score).
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import torch

from clipcap_amd.inference.base import _with_text_prefix


class CaptionScores(NamedTuple):
    token_logprobs: torch.Tensor    # (B, cap) fp32: log p(token | prefix, earlier tokens) at kept positions, 0 elsewhere
    logprob: torch.Tensor           # (B,) fp32: their sum per sample
    num_tokens: torch.Tensor        # (B,) fp32: kept positions per sample


@torch.no_grad()
def score_captions(model, embeds: torch.Tensor, tokens: torch.Tensor, *, text_prefix_tokens: Optional[torch.Tensor] = None,
                   ignore_zero: bool = False, from_prefix: bool = False) -> CaptionScores:
    """Teacher-forced log-likelihood of ``tokens`` int64 (B, cap), padded with -1, given each row's prefix.

    ``embeds``: encoder embeddings (B, E) / (B, W, E) — or, with ``from_prefix``, an already mapped prefix (B, L, D), the form the
    generate_* functions take.  ``text_prefix_tokens``: token ids whose embeddings follow the mapped prefix of every row, as in the
    generate_* functions (inference/base.py:75-77); they condition the caption and are not scored themselves.
    Kept positions are tokens >= 0; ``ignore_zero`` also drops token 0, the training loss's ignore_index (model.py:108-109)."""
    eng = model.engine
    if not from_prefix and text_prefix_tokens is None:
        out = eng.score(tokens, embeds, ignore_zero=ignore_zero)
    else:
        dev = eng.gpt2.arena.device
        prefix = embeds.to(dev, torch.float32) if from_prefix else eng.mapper.forward(embeds, save=False)
        out = eng.score(tokens, prefix=_with_text_prefix(model, prefix, text_prefix_tokens), ignore_zero=ignore_zero)
    return CaptionScores(*out)


@torch.no_grad()
def rerank_captions(model, prefix: torch.Tensor, candidates: torch.Tensor, *, length_normalise: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """Order N candidate captions per prefix row by their likelihood under the model.

    ``prefix`` fp32 (B, L, D) (mapped, text prefix included if any); ``candidates`` int64 (B, N, n) padded with -1 — e.g. sample_tokens
    output cut after each row's stop token.  Returns (order int64 (B, N), best first; scores fp32 (B, N) in candidate order):
    scores = logprob / num_tokens when ``length_normalise`` — the rule generate_beam ranks its beams by (base.py:123) — else logprob.
    Ties keep candidate order."""
    if candidates.dim() != 3 or candidates.shape[0] != prefix.shape[0]:
        raise ValueError(f"candidates must be (B, N, n) with B = {prefix.shape[0]}, got {tuple(candidates.shape)}")
    B, N, n = candidates.shape
    rows = prefix.repeat_interleave(N, dim=0) if N > 1 else prefix
    s = score_captions(model, rows, candidates.reshape(B * N, n), from_prefix=True)
    scores = (s.logprob / s.num_tokens.clamp_min(1.0) if length_normalise else s.logprob).view(B, N)
    order = torch.argsort(scores, dim=1, descending=True, stable=True)
    return order, scores
