"""A weighted mix of caption metrics as a reward that never leaves the device: the ``reward_fn`` of ``self_critical_step``.

Self-critical training is commonly run on CIDEr plus BLEU-4, sometimes plus ROUGE-L.  ``MetricReward`` adds cc_bleu_stats and cc_rouge_l
(``engine.bleu_stats`` / ``engine.rouge_l``) to ``CiderReward``'s cc_cider_score: one launch per metric with a non-zero weight, both
decodes of the step in the same launch, no value read back.  As with ``CiderReward`` the words are TOKEN IDS: a training signal, not the
published word-level metrics (``clipcap_amd.eval`` computes those).  DESIGN.md states the metrics exactly.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, Optional

import torch

from clipcap_amd import engine
from clipcap_amd.train.cider import CiderReward

METRICS = ("cider", "bleu1", "bleu2", "bleu3", "bleu4", "rouge_l")              # the order the weighted sum is taken in


class MetricReward:
    """sum_m weights[m] * metric_m(candidate, references) over token ids, on the device.  ``weights``: any of "cider", "bleu1" .. "bleu4"
    (the sentence scores of cc_bleu_stats), "rouge_l"; a metric whose weight is 0 (or absent) is not launched.  A non-zero "cider" weight
    needs ``cider``, a ``CiderReward`` (it holds the corpus's idf table) built with the same ``stop_token`` and ``count_stop``."""

    def __init__(self, weights: Optional[Dict[str, float]] = None, cider: Optional[CiderReward] = None, stop_token: int = 50256,
                 count_stop: bool = False):
        weights = {"cider": 1.0, "bleu4": 0.5, "rouge_l": 0.0} if weights is None else dict(weights)
        unknown = sorted(set(weights) - set(METRICS))
        if unknown:
            raise ValueError(f"unknown metrics {unknown}: the weights may name {list(METRICS)}")
        self.weights = {m: float(weights[m]) for m in METRICS if m in weights and float(weights[m]) != 0.0}
        if not all(math.isfinite(w) for w in self.weights.values()):
            raise ValueError(f"the weights must be finite, got {weights}")
        if not self.weights:
            raise ValueError("every weight is 0: there is nothing to score")
        self.stop_token, self.count_stop = int(stop_token), bool(count_stop)
        if "cider" in self.weights:
            if cider is None:
                raise ValueError("a non-zero \"cider\" weight needs cider=CiderReward.from_corpus(...): CIDEr-D takes its idf from a corpus")
            if cider.stop_token != self.stop_token or cider.count_stop != self.count_stop:
                raise ValueError(f"the CiderReward was built with stop_token = {cider.stop_token}, count_stop = {cider.count_stop}; "
                                 f"this reward with {self.stop_token}, {self.count_stop}")
        self.cider = cider

    def score(self, cand: torch.Tensor, refs: torch.Tensor, ref_count: Optional[torch.Tensor] = None,
              cand_group: Optional[torch.Tensor] = None) -> torch.Tensor:
        """fp32 (C,) on the device: the weighted sum for ``cand`` int64 (C, n) against ``refs`` int32 (G, Rmax, Lr), arguments as
        ``CiderReward.score``.  The terms weight * metric are fp32 and are added in the order of ``METRICS``.  The references are taken
        as they are (``for_batch`` appends the stop token under ``count_stop``)."""
        kw = dict(stop_token=self.stop_token, count_stop=self.count_stop, ref_count=ref_count, cand_group=cand_group)
        bleu, total = None, None
        for m, w in self.weights.items():
            if m == "cider":
                value = self.cider.score(cand, refs, ref_count, cand_group)
            elif m == "rouge_l":
                value = engine.rouge_l(cand, refs, **kw)[0]
            else:
                if bleu is None:
                    bleu = engine.bleu_stats(cand, refs, **kw)[1]
                value = bleu[:, int(m[-1]) - 1]
            total = value * w if total is None else total + value * w
        return total

    def for_batch(self, refs: torch.Tensor, ref_count: Optional[torch.Tensor] = None) -> Callable:
        """The ``reward_fn`` of ``self_critical_step``, as ``CiderReward.for_batch``: row b of the batch has the references ``refs[b]``
        (int32 (B, Rmax, Lr), -1 after each row's last word; ``ref_count`` int32 (B,) rows in use, None = all).  The sampled and the
        greedy ids are padded with -1 into one (2B, n) buffer, candidate c against image c % B, and every metric scores both halves in
        one launch.  No value is read back."""
        if refs.dim() != 3 or refs.dtype != torch.int32:
            raise ValueError(f"refs must be int32 (B, Rmax, Lr), got {refs.dtype} {tuple(refs.shape)}")
        refs = CiderReward.with_stop(self, refs) if self.count_stop else refs.contiguous()     # (with_stop reads self.stop_token only)
        B = refs.shape[0]

        def reward_fn(sampled: torch.Tensor, greedy: torch.Tensor):
            if sampled.dim() != 2 or greedy.dim() != 2 or sampled.shape[0] != B or greedy.shape[0] != B:
                raise ValueError(f"sampled and greedy must be (B = {B}, n), got {tuple(sampled.shape)} and {tuple(greedy.shape)}")
            n = max(sampled.shape[1], greedy.shape[1], 1)
            cand = torch.full((2 * B, n), -1, dtype=torch.int64, device=refs.device)
            cand[:B, :sampled.shape[1]] = sampled
            cand[B:, :greedy.shape[1]] = greedy
            r = self.score(cand, refs, ref_count)
            return r[:B], r[B:]

        return reward_fn
