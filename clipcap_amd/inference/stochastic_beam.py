"""Stochastic beam search (Kool, van Hoof, Welling, ICML 2019: "Stochastic Beams and Where to Find Them"; not in the reference): k DISTINCT
captions per prefix that are exact samples without replacement from the model, in sampling order, at the cost of one beam decode.

It is the decoder between the beam decoders (deterministic, k near-duplicates) and the sampling decoders (k independent decodes that may
all be the same caption).  Every candidate's log-probability is perturbed with Gumbel noise, a child's perturbed value is conditioned on its
parent's, and a top-k over the beam * V children of a step gives the k sequences (cc_beam_gumbel_step: two launches; the noise comes from a
counter-based generator inside the kernel, a pure function of (seed, step, row, token)).  The rest of a step is the beam decoders': the
KV-cached forward, cc_logits_guide, cc_logits_constrain, cc_beam_advance.

The constraints and the guidance change the distribution that is sampled from: a ban removes tokens before the softmax and guidance replaces
the logits, so the k captions are samples without replacement from the renormalised constrained / guided model, and ``logprobs`` are
log-probabilities under THAT distribution.  With all of them off they are the model's own log p(caption | prefix).
"""
from __future__ import annotations

from typing import Callable, List, NamedTuple, Optional

import torch

from clipcap_amd import engine
from clipcap_amd.engine import DecodeSession, beam_gumbel_buffers, beam_gumbel_step
from clipcap_amd.inference.base import (_bans, _negative_context, _negative_rows, _persistent_decode_on, _stop_id, _with_text_prefix)
from clipcap_amd.inference.utils import validate_stochastic_beam


class StochasticBeams(NamedTuple):
    """tokens int64 (S, k, n); logprobs (S, k) = the summed token log-probabilities phi; gumbels (S, k) = the perturbed log-probabilities,
    descending along k (slot order is sampling order); seq_lengths (S, k).  An empty slot (fewer than k sequences exist under extreme
    bans) has logprobs = gumbels = -inf."""
    tokens: torch.Tensor
    logprobs: torch.Tensor
    gumbels: torch.Tensor
    seq_lengths: torch.Tensor


def _draw_seed(generator: Optional[torch.Generator]) -> int:
    """one 62-bit integer from ``generator`` or torch's CPU generator (torch.manual_seed reproduces a decode), as ClipCapModel._dropout
    draws its seed"""
    return int(torch.randint(0, 2 ** 62, (1,), generator=generator).item())


@torch.no_grad()
def generate_stochastic_beam_tokens(model, embeds: torch.Tensor, beam_size: int = 5, entry_length: int = 67, temperature: float = 1.0,
                                    stop_token: int = 50256, *, seed: Optional[int] = None, generator: Optional[torch.Generator] = None,
                                    no_repeat_ngram_size: int = 0, min_length: int = 0, suppress_tokens=None, guidance_scale: float = 1.0,
                                    negative_embeds: Optional[torch.Tensor] = None) -> StochasticBeams:
    """Token-level stochastic beam search for a batch of prefixes, embeds fp32 (S, L, D): for every prefix ``beam_size`` distinct
    sequences sampled without replacement from the model at ``temperature``, best perturbed log-probability first (sampling order).
    ``seed``: an int in [0, 2^64) that fixes every draw of the decode (the noise of a token is a function of seed, position, row and token
    id); None: one 62-bit integer from ``generator``, or from torch's CPU generator, so torch.manual_seed reproduces a decode.
    The loop is generate_beam_rounds' single round with this update reading the plain logits: prefill one row per prefix, the first update,
    the fan-out, then per position the forward(s), the guidance, the bans (stopped beams skipped), the update and cc_beam_advance (both
    sessions when guided), with the all-stopped poll every 4th step.
    ``no_repeat_ngram_size`` / ``min_length`` / ``suppress_tokens`` / ``guidance_scale`` with ``negative_embeds`` (needed here when the
    scale is not 1; inference/base.py's docstring): the sample is then drawn from the renormalised constrained / guided distribution, and
    ``logprobs`` are log-probabilities under it (module docstring).
    Returns StochasticBeams(tokens int64 (S, k, n), logprobs (S, k), gumbels (S, k), seq_lengths (S, k))."""
    validate_stochastic_beam(beam_size, None, seed)
    lm = model.language_model
    g = lm.engine
    V = g.dims["V"]
    dev = g.arena.device
    embeds = embeds.to(dev, torch.float32)
    S, L0, D = embeds.shape
    R = S * beam_size
    gs, neg = _negative_rows(negative_embeds, guidance_scale, S, D, dev, "generate_stochastic_beam_tokens")
    guided = neg is not None
    bans = _bans(V, stop_token, no_repeat_ngram_size, min_length, suppress_tokens, dev)
    if seed is None:
        seed = _draw_seed(generator)
    total = min(entry_length, g.dims["NPOS"] - L0)
    if total < 1:
        raise RuntimeError(f"a {L0}-position prefix leaves no room to generate (n_positions = {g.dims['NPOS']})")
    wte = lm.get_input_embeddings().weight.detach()
    scores = torch.zeros(R, dtype=torch.float32, device=dev)
    gumbels = torch.zeros(R, dtype=torch.float32, device=dev)
    seq_lengths = torch.ones(R, dtype=torch.float32, device=dev)
    has_stopped = torch.zeros(R, dtype=torch.uint8, device=dev)
    fan = torch.arange(S, device=dev, dtype=torch.int32).repeat_interleave(beam_size)
    sess = DecodeSession(g, S, L0 + total)
    logits0 = sess.forward(embeds)                                              # (S, V)
    lg = torch.empty(R, V, dtype=torch.float32, device=dev)
    if guided:                                                                  # the unconditional stream: its own positions, from 0
        usess = DecodeSession(g, S, neg.shape[1] + total)
        engine.guide_logits(logits0, usess.forward(neg), gs, out=lg[::beam_size])
    else:
        lg[::beam_size] = logits0                                               # row 0 of every beam set, under the row index the noise uses
    bufs = beam_gumbel_buffers(dev, S, beam_size, V)

    def update(logits, first, step):
        return beam_gumbel_step(logits, S, beam_size, temperature, first, stop_token, seed, step, scores, gumbels, seq_lengths, has_stopped, bufs)

    if bans is not None:
        bans.apply(lg[::beam_size], 0)
    next_tok, src = update(lg, True, 0)
    sess = sess.expand(fan, R)
    if guided:
        usess = usess.expand(fan, R)
    tok = [torch.zeros(R, total, dtype=torch.int32, device=dev) for _ in range(2)]
    x = torch.empty(R, 1, D, dtype=torch.float32, device=dev)
    sess.beam_advance(beam_size, next_tok, None, wte, 0, tok[1], tok[0], x)
    n = 1                                                                       # token columns written so far = the next position index
    for i in range(1, entry_length):
        # a step after every beam has stopped only appends token 0: scores, gumbels, lengths and the slot order pass through bit for bit
        if i % 4 == 1 and bool(has_stopped.all()):
            break
        if n >= total:
            raise RuntimeError(f"generation reached n_positions = {g.dims['NPOS']} ({L0}-position prefix + {n} tokens)")
        logits = sess.forward(x, group=beam_size)
        if guided:
            engine.guide_logits(logits, usess.forward(x, group=beam_size), gs, skip_rows=has_stopped)
        if bans is not None:
            bans.apply(logits, n, tok[(n - 1) & 1], n, None, has_stopped)
        next_tok, src = update(logits, False, n)
        sess.beam_advance(beam_size, next_tok, src, wte, n, tok[(n - 1) & 1], tok[n & 1], x)
        if guided:
            usess.beam_advance(beam_size, next_tok, src, wte, n, tok[(n - 1) & 1], tok[n & 1], x)
        n += 1
    if _persistent_decode_on():
        sess.check()
    return StochasticBeams(tok[(n - 1) & 1][:, :n].to(torch.int64).view(S, beam_size, -1), scores.view(S, beam_size).clone(),
                           gumbels.view(S, beam_size).clone(), seq_lengths.view(S, beam_size).clone())


def generate_stochastic_beam(model, tokenizer: Callable, embeds: torch.Tensor, text_prefix_tokens: Optional[torch.Tensor] = None,
                             beam_size: int = 5, entry_length: int = 67, temperature: float = 1.0, *,
                             num_return_sequences: Optional[int] = None, seed: Optional[int] = None,
                             generator: Optional[torch.Generator] = None, no_repeat_ngram_size: int = 0, min_length: int = 0,
                             suppress_tokens=None, guidance_scale: float = 1.0, negative_embeds: Optional[torch.Tensor] = None) -> List[str]:
    """Texts of generate_stochastic_beam_tokens: for every prefix row its first ``num_return_sequences`` (None: all ``beam_size``) captions in
    sampling order, next to each other; empty slots are skipped.  The captions of a prefix are pairwise distinct token sequences.
    ``guidance_scale`` != 1: ``negative_embeds`` None = the embedding of tokenizer.bos_token, the text prefix after it, as generate_beam
    builds it.  Bans and guidance change the distribution that is sampled from (module docstring)."""
    validate_stochastic_beam(beam_size, num_return_sequences, seed)
    stop = _stop_id(tokenizer)
    negative_embeds = _negative_context(model, tokenizer, negative_embeds, text_prefix_tokens, guidance_scale)
    embeds = _with_text_prefix(model, embeds, text_prefix_tokens)
    r = generate_stochastic_beam_tokens(model, embeds, beam_size, entry_length, temperature, stop, seed=seed, generator=generator,
                                        no_repeat_ngram_size=no_repeat_ngram_size, min_length=min_length, suppress_tokens=suppress_tokens,
                                        guidance_scale=guidance_scale, negative_embeds=negative_embeds)
    tokens, logprobs, lengths = r.tokens.cpu(), r.logprobs.cpu(), r.seq_lengths.cpu()
    k = beam_size if num_return_sequences is None else int(num_return_sequences)
    out = []
    for s in range(tokens.shape[0]):
        for b in range(k):
            if logprobs[s, b] > float("-inf"):
                out.append(tokenizer.decode(tokens[s, b, :int(lengths[s, b])].numpy()))
    return out


def sbs_importance_weights(logprobs: torch.Tensor, gumbels: torch.Tensor, normalise: bool = True) -> torch.Tensor:
    """Importance weights of a stochastic-beam sample for estimating expectations under the model (Kool et al., 2019, eq. 21 / 23).
    logprobs, gumbels (S, k) as StochasticBeams holds them.  The threshold kappa is the smallest perturbed log-probability of the k slots;
    each of the other k - 1 slots gets w = exp(phi) / q with q = P(Gumbel(phi) > kappa) = -expm1(-exp(phi - kappa)); ``normalise``: divided by
    their sum per row (the normalised estimator: biased, lower variance).  Returns (S, k - 1) in the slots' order without the threshold's
    slot.  ValueError for k < 2.  Pure torch."""
    if logprobs.dim() != 2 or gumbels.shape != logprobs.shape or logprobs.shape[1] < 2:
        raise ValueError(f"sbs_importance_weights needs logprobs and gumbels of one shape (S, k) with k >= 2, got {tuple(logprobs.shape)} and "
                         f"{tuple(gumbels.shape)}")
    kappa, at = gumbels.min(dim=1, keepdim=True)
    keep = torch.ones_like(gumbels, dtype=torch.bool).scatter_(1, at, False)
    k = logprobs.shape[1]
    phi = logprobs[keep].view(-1, k - 1)
    q = -torch.expm1(-torch.exp(phi - kappa))
    w = torch.exp(phi) / q
    return w / w.sum(dim=1, keepdim=True) if normalise else w
