"""Self-critical sequence training (Rennie et al., 2017, "Self-critical Sequence Training for Image Captioning") as one fused step.

The REINFORCE term with the model's own greedy caption as the baseline is a cross-entropy over the SAMPLED caption in which every token
carries the weight ``reward(sample) - reward(greedy)``: exactly the weighted loss of ``ClipCapModel.fused_step(token_weights=...)``.
This module adds no device code; it decodes twice with ``sample_tokens``, asks the caller for the rewards and takes the weighted step.
``reward_fn`` gets token ids and may be any metric of the caller's; ``clipcap_amd.train.cider.CiderReward(...).for_batch(refs)`` is one
that never leaves the device: CIDEr-D over token ids against token-id references, one launch for both decodes (cc_cider_score);
``clipcap_amd.train.metrics.MetricReward`` mixes it with BLEU and ROUGE-L (cc_bleu_stats, cc_rouge_l), one launch per metric.
"""
from typing import Callable, Optional, Tuple

import torch

from clipcap_amd.inference.base import sample_tokens


def scst_tokens_and_weights(sampled: torch.Tensor, advantage: torch.Tensor, stop_token: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The loss's tokens and weights of a self-critical step from the sampled ids (B, n) and the advantage (B,).

    tokens int64 (B, n): the sampled caption up to AND INCLUDING its first stop token (the model has to learn to stop), -1 after it
    (the loss's padding); a row that never stopped is kept whole.  weights fp32 (B, n): the row's advantage at every position (the
    weight of a position the loss ignores is never used, so nothing has to be masked).  Host-free: no value is read back."""
    if sampled.dim() != 2 or advantage.shape != (sampled.shape[0],):
        raise ValueError(f"sampled must be (B, n) and advantage (B,), got {tuple(sampled.shape)} and {tuple(advantage.shape)}")
    B, n = sampled.shape
    after_stop = (sampled == stop_token).to(torch.int64).cumsum(dim=1) - (sampled == stop_token).to(torch.int64) > 0
    tokens = torch.where(after_stop, torch.full_like(sampled, -1), sampled).to(torch.int64)
    weights = advantage.to(torch.float32).reshape(B, 1).expand(B, n).contiguous()
    return tokens, weights


def self_critical_step(model, batch_embeds: torch.Tensor, reward_fn: Callable, lr: float, *, temperature: float = 1.0,
                       top_k: Optional[int] = None, top_p: float = 1.0, entry_length: int = 67, stop_token: int = 50256,
                       generator: Optional[torch.Generator] = None, min_p: float = 0.0, typical_p: float = 1.0, epsilon_cutoff: float = 0.0,
                       eta_cutoff: float = 0.0, **fused_step_kw) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """One self-critical optimizer step on ``batch_embeds`` (the encoder embeddings ``fused_step`` takes).

    1. prefix = mapper(batch_embeds);  2. one SAMPLED caption per row (``sample_tokens`` with ``temperature`` / ``top_k`` / ``top_p`` /
    ``generator``, and the truncation rules ``min_p`` / ``typical_p`` / ``epsilon_cutoff`` / ``eta_cutoff`` of ``sample_tokens``, off by
    default: they cut the tail whose advantage is noise and go to the SAMPLED decode only);  3. one GREEDY caption per row (the same function at its deterministic setting, top_k = 1);
    4. ``reward_fn(sampled, greedy)`` -> two (B,) tensors, the rewards of the sampled and of the greedy captions.  It gets token ids,
    int64 (B, n_s) and (B, n_g), each row valid up to and including its first ``stop_token``;  5. advantage A = r_sample - r_greedy;
    6. the loss's tokens = the sampled caption up to and including its stop token, -1 after it;  7. ``fused_step`` with the advantage
    as the weight of every kept position (``scst_tokens_and_weights``).  The divisor is the number of kept tokens, as in every step.

    Token id 0 is ``ignore_index`` of this model's loss: a sampled 0 would silently drop out of the loss.  Both decodes therefore run
    with ``suppress_tokens=[0]``, so id 0 is never generated.

    ``**fused_step_kw`` goes to ``fused_step`` (reducer, max_grad_norm, label_smoothing, ema_decay, sample_weights).
    Returns (loss, mean reward of the samples, mean reward of the greedy captions), device scalars."""
    if "token_weights" in fused_step_kw:
        raise ValueError("self_critical_step builds token_weights from the advantage; pass sample_weights to re-weight captions")
    eng = model.engine
    with torch.no_grad():
        prefix = eng.mapper.forward(batch_embeds, save=False)
        common = dict(entry_length=entry_length, stop_token=stop_token, suppress_tokens=[0])
        sampled, _ = sample_tokens(model, prefix, mode=0, top_p=top_p, top_k=top_k, temperature=temperature, generator=generator,
                                   min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff, **common)
        greedy, _ = sample_tokens(model, prefix, mode=0, top_p=1.0, top_k=1, temperature=1.0, **common)
        r_sample, r_greedy = reward_fn(sampled, greedy)
        r_sample = torch.as_tensor(r_sample, dtype=torch.float32, device=sampled.device)
        r_greedy = torch.as_tensor(r_greedy, dtype=torch.float32, device=sampled.device)
        tokens, weights = scst_tokens_and_weights(sampled, r_sample - r_greedy, stop_token)
    loss = model.fused_step((tokens, batch_embeds), lr, token_weights=weights, **fused_step_kw)
    return loss, r_sample.mean(), r_greedy.mean()
