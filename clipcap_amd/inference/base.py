"""Caption decoding with a KV cache on the HIP path — same entry points as the reference's clipcap/inference/base.py
(generate_beam :55-132, generate_nucleus_sampling :135-201, generate_no_beam :204-279) with the same arguments.

Differences that do not change results: GPT-2 runs incrementally (cc_decode_fwd) instead of re-forwarding the growing
sequence every step (base.py:81), the beam update runs in one device kernel (cc_beam_step), and ``embeds`` may carry a
batch of prefixes (B, L, D): the reference is batch-1 only, and B == 1 reproduces its outputs.

Not in the reference: every decoder takes three keyword-only constraints, all off by default —
  * ``no_repeat_ngram_size`` = g: no n-gram of g tokens occurs twice in a caption's generated tokens (sampling: in head_tokens ++ generated);
  * ``min_length`` = m: the stop token is banned until m tokens have been generated;
  * ``suppress_tokens``: ids that are never generated.
A ban sets the logit to -inf before the softmax, temperature, penalties and filters (cc_logits_constrain, one launch per step, which also
repairs the lm_head partials the fused beam update reads); with all three off a decoder launches exactly what it launched without them.

Not in the reference either: diverse beam search (Vijayakumar et al., 2016) on the beam decoders, keyword-only and off by default —
  * ``num_beam_groups`` = G > 1: the beam_size beams are G beam groups of beam_size / G beams, advanced one after the other inside a step;
  * ``diversity_penalty`` > 0: what a token's log-probability loses in a beam group per earlier beam group pick of that token at this step
    (cc_beam_group_step; the two come together);
  * ``num_return_sequences`` = n (generate_beam): the n best beams of every prefix instead of the best one.
With G == 1 the beam decoders launch exactly what they launched without these options.

Not in the reference either: classifier-free guidance at decode time (Kornblith et al., ICCV 2023; Sanchez et al., 2023) on the beam and
sampling decoders, keyword-only and off by default —
  * ``guidance_scale`` = g != 1: the language model runs a second time on the same generated tokens behind ``negative_embeds`` instead of
    the prefix, in a second DecodeSession that follows the first one's ancestry, and every step scores
    log_softmax(uncond) + g * (log_softmax(cond) - log_softmax(uncond)) (cc_logits_guide, one launch) in place of the logits: g > 1 rewards
    a token for what the prefix adds to its probability.  The order within a step is forward x 2, guidance, bans, then the step with its
    temperature, penalties and filters; the step's own softmax renormalises the guided scores.  The beam decoders then read the logits,
    not the lm_head partials, as diverse beam search does;
  * ``negative_embeds``: the unconditional context, fp32 (S, Ln, D) or (1, Ln, D) for all prefixes, Ln >= 1.  None: the functions that
    have a tokenizer take one position, the input embedding of ``tokenizer.bos_token``, and append a text prefix to it as they do to the
    prefix; the token-level functions need it whenever g != 1.
With g == 1 a decoder launches exactly what it launched without these options and allocates nothing more.

Contrastive search (Su et al., 2022), the deterministic decoder with a degeneration penalty, lives in inference/contrastive.py
(generate_contrastive, generate_contrastive_tokens); it takes the same three constraints.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Tuple, Union

import torch

from clipcap_amd import engine
from clipcap_amd.engine import (DecodeSession, beam_buffers, beam_group_buffers, beam_group_step, beam_step, constrain_logits, embed_tokens,
                                sample_step)
from clipcap_amd.inference.utils import (nucleus_distribution, repetition_penalty_apply, sentence_length_penalty_apply,  # noqa: F401
                                         top_k_top_p_filtering, truncation_is_on, validate_beam_groups, validate_constraints,
                                         validate_guidance, validate_truncation)


def _persistent_decode_on() -> bool:
    from clipcap_amd import _lib
    return bool(_lib.lib().cc_decode_mode(-1) & 6)          # bit 1: persistent layer launch, bit 2: XCD-team engine (include/clipcap_hip.h)


def _stop_id(tokenizer) -> int:
    return tokenizer.encode(tokenizer.eos_token)[0]          # base.py:66


def _with_text_prefix(model, embeds, text_prefix_tokens):
    if text_prefix_tokens is None:
        return embeds
    emb = model.language_model.get_input_embeddings()(text_prefix_tokens.to(embeds.device))
    return torch.cat((embeds, emb.expand(embeds.shape[0], -1, -1)), dim=1)   # base.py:75-77


class _Bans:
    """The decoding constraints of one decode (module docstring): validated once, the suppress list uploaded once; ``apply`` is the one
    extra launch per step.  _bans() returns None when all three are off, and the decoders then make no call and allocate nothing."""

    def __init__(self, ngram: int, min_length: int, stop_token: int, suppress: Optional[torch.Tensor]):
        self.ngram, self.min_length, self.stop_token, self.suppress = ngram, min_length, stop_token, suppress

    def apply(self, logits: torch.Tensor, generated: int, history: Optional[torch.Tensor] = None, hist_len: int = 0, lpart=None,
              skip_rows: Optional[torch.Tensor] = None) -> None:
        """Bans on the logits of the step that follows ``generated`` generated tokens; ``history[:, :hist_len]``: the rows' tokens so far."""
        constrain_logits(logits, lpart=lpart, history=history if self.ngram else None, hist_len=hist_len if self.ngram else 0,
                         no_repeat_ngram=self.ngram, ban_token=self.stop_token if generated < self.min_length else -1, suppress=self.suppress,
                         skip_rows=skip_rows)


def _bans(V: int, stop_token: int, no_repeat_ngram_size: int, min_length: int, suppress_tokens, dev) -> Optional[_Bans]:
    ids = validate_constraints(V, stop_token, no_repeat_ngram_size, min_length, suppress_tokens)
    if not (no_repeat_ngram_size or min_length or ids):
        return None
    return _Bans(int(no_repeat_ngram_size), int(min_length), int(stop_token), torch.tensor(ids, dtype=torch.int32, device=dev) if ids else None)


def _negative_rows(negative_embeds: Optional[torch.Tensor], guidance_scale: float, rows: int, D: int, dev, who: str):
    """(scale, the unconditional context as fp32 (rows, Ln, D) on ``dev``) of a token-level decoder; (1.0, None) when guidance is off.
    Validated once, before anything touches the device."""
    gs = validate_guidance(guidance_scale)
    if gs == 1.0:
        return gs, None
    if negative_embeds is None:
        raise ValueError(f"{who}: guidance_scale = {gs} needs negative_embeds, the unconditional context (fp32 ({rows}, Ln, {D}) or (1, Ln, {D}))")
    if negative_embeds.dim() != 3 or negative_embeds.shape[0] not in (1, rows) or negative_embeds.shape[1] < 1 or negative_embeds.shape[2] != D:
        raise ValueError(f"{who}: negative_embeds must be ({rows}, Ln, {D}) or (1, Ln, {D}) with Ln >= 1, got {tuple(negative_embeds.shape)}")
    return gs, negative_embeds.to(dev, torch.float32).expand(rows, -1, -1)


def _negative_context(model, tokenizer, negative_embeds: Optional[torch.Tensor], text_prefix_tokens, guidance_scale: float):
    """The unconditional context of a decoder that has a tokenizer: ``negative_embeds``, or one position holding the input embedding of
    tokenizer.bos_token, with the text prefix appended exactly as it is to the prefix.  None (and nothing computed) when guidance is off."""
    if validate_guidance(guidance_scale) == 1.0:
        return None
    emb = model.language_model.get_input_embeddings()
    if negative_embeds is None:
        bos = tokenizer.encode(tokenizer.bos_token)[0]
        negative_embeds = emb.weight.detach()[int(bos)].view(1, 1, -1)
    return _with_text_prefix(model, negative_embeds.to(emb.weight.device, torch.float32), text_prefix_tokens)


@torch.no_grad()
def generate_beam_rounds(model, embeds: torch.Tensor, beam_size: int = 5, entry_length: int = 67, temperature: float = 1.0,
                         stop_token: int = 50256, rounds: int = 1, *, no_repeat_ngram_size: int = 0, min_length: int = 0,
                         suppress_tokens=None, num_beam_groups: int = 1, diversity_penalty: float = 0.0, guidance_scale: float = 1.0,
                         negative_embeds: Optional[torch.Tensor] = None) -> List[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]:
    """Token-level beam search for a batch of prefixes, embeds fp32 (S, L, D), as ``rounds`` consecutive generations with LIVE state —
    the reference's ``for _ in range(number_to_generate)`` around its entry_length loop (base.py:79-130): a later round continues the beams
    of the one before (token histories, has_stopped, seq_lengths, the KV cache), its running ``scores`` are the previous round's scores
    already divided by seq_lengths (base.py:123 rebinds the name), beams that never stopped keep generating for another entry_length
    tokens, and a round that starts with every beam stopped still takes one step (base.py:80-121) before it breaks.
    The constraints (module docstring) see a beam row's own generated tokens after the reorder; histories and the min_length count carry
    on across rounds like the rest of the state.  Text-prefix tokens are not part of the history: they enter as embeddings.
    ``num_beam_groups`` > 1 with ``diversity_penalty`` > 0 (module docstring): beam rows g * W .. (g + 1) * W - 1, W = beam_size /
    num_beam_groups, of every prefix are beam group g; a step is then the plain decode forward, the bans and cc_beam_group_step.
    ``guidance_scale`` != 1 with ``negative_embeds`` (module docstring; needed here, there is no tokenizer to build a default from): a second
    session of the same rows, prefilled with the negative context and fed the same token embeddings, is fanned out and advanced with the
    first; a step is then the plain decode forward of both, cc_logits_guide (stopped beams skipped), the bans and the update on the logits.
    Returns one (tokens int64 (S, beam, n_r), scores (S, beam) length-normalised, seq_lengths (S, beam)) per round."""
    lm = model.language_model
    g = lm.engine
    dev = g.arena.device
    embeds = embeds.to(dev, torch.float32)
    S, L0, D = embeds.shape
    R = S * beam_size
    V = g.dims["V"]
    rounds = max(1, int(rounds))
    validate_beam_groups(beam_size, num_beam_groups, diversity_penalty)
    G = int(num_beam_groups)
    gs, neg = _negative_rows(negative_embeds, guidance_scale, S, D, dev, "generate_beam_rounds")
    guided = neg is not None
    bans = _bans(V, stop_token, no_repeat_ngram_size, min_length, suppress_tokens, dev)
    # positions are allocated up to n_positions; like the reference (base.py:79-130), a large number_to_generate only fails if generation
    # actually REACHES the position limit — beams normally stop far earlier
    total = min(rounds * entry_length, g.dims["NPOS"] - L0)
    if total < 1:
        raise RuntimeError(f"a {L0}-position prefix leaves no room to generate (n_positions = {g.dims['NPOS']})")
    wte = lm.get_input_embeddings().weight.detach()
    scores = torch.zeros(R, dtype=torch.float32, device=dev)
    seq_lengths = torch.ones(R, dtype=torch.float32, device=dev)
    has_stopped = torch.zeros(R, dtype=torch.uint8, device=dev)
    base = (torch.arange(S, device=dev, dtype=torch.int32) * beam_size).repeat_interleave(beam_size)
    # step 0: one row per sample (base.py:86-94), then fan the cache out to beam rows
    sess = DecodeSession(g, S, L0 + total)
    logits0 = sess.forward(embeds)                                              # (S, V)
    lg = torch.empty(R, V, dtype=torch.float32, device=dev)
    if guided:                                                                  # the unconditional stream: its own positions, from 0
        usess = DecodeSession(g, S, neg.shape[1] + total)
        engine.guide_logits(logits0, usess.forward(neg), gs, out=lg[::beam_size])   # the S prefill rows, written where the first update reads
    else:
        lg[::beam_size] = logits0                                               # row 0 of every beam set
    bufs = beam_buffers(dev, S, beam_size, V) if G == 1 else beam_group_buffers(dev, S, beam_size, G, V)   # this decode's own step outputs + scratch

    def update(logits, first, lpart=None):                                      # the step's update -> (next tokens, source rows); state in place
        if G == 1:
            return beam_step(logits, S, beam_size, temperature, first, stop_token, scores, seq_lengths, has_stopped, bufs, lpart)
        return beam_group_step(logits, S, beam_size, G, temperature, diversity_penalty, first, stop_token, scores, seq_lengths, has_stopped, bufs)

    if bans is not None:
        bans.apply(lg[::beam_size], 0)                                          # the rows the first update reads; no history yet
    next_tok, src = update(lg, True)
    sess = sess.expand((base // beam_size).to(torch.int32), R)
    if guided:
        usess = usess.expand((base // beam_size).to(torch.int32), R)
    # token histories (int32, ping-pong), the next input embedding and the cache ancestry are advanced by one launch per step
    tok = [torch.zeros(R, total, dtype=torch.int32, device=dev) for _ in range(2)]
    x = torch.empty(R, 1, D, dtype=torch.float32, device=dev)
    sess.beam_advance(beam_size, next_tok, None, wte, 0, tok[1], tok[0], x)     # step 0: tokens = next_tokens (base.py:94)
    plain = G > 1 or guided                                                     # the update reads the logits, not the lm_head partials
    n = 1                                                                       # token columns written so far
    out = []
    for r in range(rounds):
        for i in range(1 if r == 0 else 0, entry_length):
            # base.py:120-121 breaks as soon as every beam has stopped.  Steps taken after that point only append token 0 to frozen
            # beams (lengths and the truncated outputs are unchanged; scores are re-sorted and change by ulps at most), so polling the flag every 4th step — one host sync
            # instead of four — cannot change the result.  (i == 0 of a later round is never skipped: the reference takes that step.)
            if i % 4 == 1 and bool(has_stopped.all()):
                break
            if n >= total:
                raise RuntimeError(f"generation reached n_positions = {g.dims['NPOS']} ({L0}-position prefix + {n} tokens; round {r + 1} of {rounds})")
            if not plain:
                logits = sess.forward(x, partials=True, group=beam_size)        # x = wte[next_tokens] (base.py:117)
                if bans is not None:                                            # a stopped beam's logits are ignored by the update: skipped
                    bans.apply(logits, n, tok[(n - 1) & 1], n, sess.lpart, has_stopped)
                next_tok, src = update(logits, False, sess.lpart)
            else:                                                               # beam groups, guidance: the update reads the logits, not the partials
                logits = sess.forward(x, group=beam_size)
                if guided:                                                      # the same tokens without the prefix; a stopped beam's logits are ignored
                    engine.guide_logits(logits, usess.forward(x, group=beam_size), gs, skip_rows=has_stopped)
                if bans is not None:
                    bans.apply(logits, n, tok[(n - 1) & 1], n, None, has_stopped)
                next_tok, src = update(logits, False)
            sess.beam_advance(beam_size, next_tok, src, wte, n, tok[(n - 1) & 1], tok[n & 1], x)   # base.py:104-117
            if guided:                                                          # the same ancestry for the second cache; rewrites the same tokens and x
                usess.beam_advance(beam_size, next_tok, src, wte, n, tok[(n - 1) & 1], tok[n & 1], x)
            n += 1
        final = scores / seq_lengths                                            # base.py:123
        out.append((tok[(n - 1) & 1][:, :n].to(torch.int64).view(S, beam_size, -1), final.view(S, beam_size).clone(),
                    seq_lengths.view(S, beam_size).clone()))
        scores.copy_(final)                                                     # the next round starts from the normalised scores (base.py:123)
    if _persistent_decode_on():
        sess.check()                                                            # a persistent decode launch that gave up must not go unnoticed (the flag is sticky)
    return out


def generate_beam_tokens(model, embeds: torch.Tensor, beam_size: int = 5, entry_length: int = 67, temperature: float = 1.0,
                         stop_token: int = 50256, *, no_repeat_ngram_size: int = 0, min_length: int = 0,
                         suppress_tokens=None, num_beam_groups: int = 1, diversity_penalty: float = 0.0, guidance_scale: float = 1.0,
                         negative_embeds: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """One generation (the reference's number_to_generate = 1): (tokens int64 (S, beam, n), scores (S, beam) length-normalised,
    seq_lengths (S, beam))."""
    return generate_beam_rounds(model, embeds, beam_size, entry_length, temperature, stop_token, 1, no_repeat_ngram_size=no_repeat_ngram_size,
                                min_length=min_length, suppress_tokens=suppress_tokens, num_beam_groups=num_beam_groups,
                                diversity_penalty=diversity_penalty, guidance_scale=guidance_scale, negative_embeds=negative_embeds)[0]


def best_beams(scores: torch.Tensor, n: int = 1) -> torch.Tensor:
    """Indices (S, n) of the n best beams of every row of final ``scores`` (S, beam), best first; ties go to the lower beam index."""
    if n == 1:
        return scores.argmax(dim=1, keepdim=True)     # == argsort(descending)[0]; ties resolve to the first beam like a stable sort
    return torch.sort(scores, dim=1, descending=True, stable=True).indices[:, :n]


def generate_beam(model, tokenizer: Callable, embeds: torch.Tensor, number_to_generate: int = 1,
                  text_prefix_tokens: Optional[torch.Tensor] = None, beam_size: int = 5, entry_length: int = 67,
                  temperature: float = 1.0, *, no_repeat_ngram_size: int = 0, min_length: int = 0, suppress_tokens=None,
                  num_beam_groups: int = 1, diversity_penalty: float = 0.0, num_return_sequences: int = 1, guidance_scale: float = 1.0,
                  negative_embeds: Optional[torch.Tensor] = None) -> List[str]:
    """Reference signature (base.py:55-64) plus the keyword-only constraints and diverse-beam-search options (module docstring).  For the reference's batch-1 input: ``number_to_generate`` texts, the best beam after each of
    the consecutive generations (base.py:79-130, see generate_beam_rounds).  A batch of prefixes (S > 1, an extension — the reference is
    batch-1) returns the best caption of every prefix row, round-major when number_to_generate > 1.
    ``num_return_sequences`` = n > 1: for every prefix row (and round) its n best beams by final score, best first, next to each other.
    ``guidance_scale`` != 1 (module docstring): ``negative_embeds`` None = the embedding of tokenizer.bos_token; the text prefix follows it."""
    stop = _stop_id(tokenizer)
    negative_embeds = _negative_context(model, tokenizer, negative_embeds, text_prefix_tokens, guidance_scale)
    embeds = _with_text_prefix(model, embeds, text_prefix_tokens)
    validate_beam_groups(beam_size, num_beam_groups, diversity_penalty, num_return_sequences)
    out = []
    for tokens, scores, lengths in generate_beam_rounds(model, embeds, beam_size, entry_length, temperature, stop, number_to_generate,
                                                        no_repeat_ngram_size=no_repeat_ngram_size, min_length=min_length,
                                                        suppress_tokens=suppress_tokens, num_beam_groups=num_beam_groups,
                                                        diversity_penalty=diversity_penalty, guidance_scale=guidance_scale,
                                                        negative_embeds=negative_embeds):
        best = best_beams(scores, int(num_return_sequences)).cpu()
        for s in range(tokens.shape[0]):
            for b in best[s].tolist():
                n = int(lengths[s, b])
                out.append(tokenizer.decode(tokens[s, b, :n].cpu().numpy()))
    return out


@torch.no_grad()
def sample_tokens(model, embeds: torch.Tensor, entry_length: int = 67, stop_token: int = 50256, *, mode: int = 0, top_p: float = 0.8,
                  top_k: Optional[int] = None, temperature: float = 1.0, repetition_penalty: float = 1.0,
                  generator: Optional[torch.Generator] = None, head_tokens: Optional[torch.Tensor] = None,
                  desired_sentence_length: Optional[int] = None, sentence_length_factor: float = 1.0, no_repeat_ngram_size: int = 0,
                  min_length: int = 0, suppress_tokens=None, min_p: float = 0.0, typical_p: float = 1.0, epsilon_cutoff: float = 0.0,
                  eta_cutoff: float = 0.0, guidance_scale: float = 1.0,
                  negative_embeds: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """KV-cached sampling for a batch of prefixes, every step on the device (cc_decode_fwd + cc_sample_step, no host sync except
    an all-rows-stopped poll every 4th step).  embeds fp32 (R, L, D).  mode 0 = the nucleus rule of generate_nucleus_sampling
    (base.py:165-181), mode 1 = top_k_top_p_filtering + softmax (base.py:245-262).
    ``head_tokens`` int64 (R, H0) or (1, H0): tokens that precede the generated ones in the repetition-penalty history (the
    reference penalises ``tokens`` = text_prefix_tokens ++ generated, no_beam.py:32,45-48).
    ``desired_sentence_length`` not None: the sentence-length penalty of no_beam.py:55-60 — with a non-empty history, history tokens
    whose filtered logit equals float(stop_token) are scaled by (len(history) / desired_sentence_length) * sentence_length_factor
    (utils.py:40-51) before the softmax, inside cc_sample_step_lp.
    The constraints (module docstring) are applied to the logits before all of that; their history is head_tokens ++ generated, the one
    the repetition penalty uses, and head tokens do not count towards ``min_length``.
    ``guidance_scale`` != 1 with ``negative_embeds`` (R, Ln, D) or (1, Ln, D) (module docstring; needed here): a second session of R rows is
    prefilled with the negative context and fed the same token embeddings; every step's logits are replaced by the guided scores
    (cc_logits_guide) before the bans and the sampling step.
    ``min_p`` / ``typical_p`` / ``epsilon_cutoff`` / ``eta_cutoff`` (off at 0 / 1 / 0 / 0; engine.truncate_logits, cc_logits_truncate): the
    truncation rules, applied after the guidance and the bans and immediately before the sampling step, on the values it draws from (same
    temperature, history and repetition penalty).  The kept set is the intersection of the rules that are on, all taken against the same
    incoming distribution (transformers renormalises between several rules, this does not); the sampling step's own top_k / top_p then
    act on the truncated row, so the mode-0 ``top_p`` mass is relative to it.  With all four off no launch is made.
    Returns (tokens int64 (R, n), stop_pos int64 (R,)): stop_pos[r] = index of the first stop token of row r (n if none)."""
    trunc = validate_truncation(min_p, typical_p, epsilon_cutoff, eta_cutoff)
    trunc_on = truncation_is_on(trunc)
    lm = model.language_model
    g = lm.engine
    dev = g.arena.device
    embeds = embeds.to(dev, torch.float32)
    R, L0, D = embeds.shape
    gs, neg = _negative_rows(negative_embeds, guidance_scale, R, D, dev, "sample_tokens")
    bans = _bans(g.dims["V"], stop_token, no_repeat_ngram_size, min_length, suppress_tokens, dev)
    sess = DecodeSession(g, R, L0 + entry_length)
    usess = DecodeSession(g, R, neg.shape[1] + entry_length) if neg is not None else None
    H0 = 0 if head_tokens is None else int(head_tokens.shape[-1])
    hist = torch.zeros(R, H0 + entry_length, dtype=torch.int64, device=dev)          # [head | generated]: the penalty's history
    if H0:
        hist[:, :H0] = head_tokens.to(dev, torch.int64).reshape(-1, H0).expand(R, H0)
    toks = hist[:, H0:]
    xbuf = torch.empty(R, 1, D, dtype=torch.float32, device=dev)
    x = embeds
    n = 0
    for step in range(entry_length):
        logits = sess.forward(x)                                                     # (R, V) fp32
        if usess is not None:                                                        # the same tokens behind the negative context
            engine.guide_logits(logits, usess.forward(neg if step == 0 else x), gs)
        if bans is not None:
            bans.apply(logits, step, hist, H0 + step)
        if trunc_on:                                                                 # on the values sample_step draws from
            engine.truncate_logits(logits, temperature=temperature, history=hist, hist_len=H0 + step, repetition_penalty=repetition_penalty,
                                   **trunc)
        u = torch.rand(R, device=dev, generator=generator)
        nxt = sample_step(logits, u, temperature=temperature, top_k=top_k or 0, top_p=top_p, mode=mode, history=hist, hist_len=H0 + step,
                          repetition_penalty=repetition_penalty,
                          length_penalty_stop=stop_token if desired_sentence_length is not None else -1,
                          length_penalty=((H0 + step) / desired_sentence_length) * sentence_length_factor if desired_sentence_length else 1.0)  # int32 (R,)
        toks[:, step] = nxt
        n = step + 1
        # every row has produced its stop token: polled every 4th step (one host sync instead of four; the extra tokens are cut below)
        if step % 4 == 3 and bool((toks[:, :n] == stop_token).any(dim=1).all()):
            break
        x = embed_tokens(g, nxt, xbuf)                                               # wte[next] (base.py:184), one launch
    toks = toks[:, :n]
    hit = toks == stop_token
    stop_pos = torch.where(hit.any(dim=1), hit.to(torch.int32).argmax(dim=1), torch.full((R,), n, dtype=torch.int64, device=dev))
    return toks, stop_pos


def _rows_for(embeds: torch.Tensor, number_to_generate: int) -> torch.Tensor:
    return embeds.repeat_interleave(max(1, number_to_generate), dim=0) if number_to_generate > 1 else embeds


def _negative_rows_for(negative_embeds: Optional[torch.Tensor], number_to_generate: int) -> Optional[torch.Tensor]:
    """_rows_for for the unconditional context: a context per prefix row is repeated like the prefix rows, a shared one (or None) stays."""
    return negative_embeds if negative_embeds is None or negative_embeds.shape[0] == 1 else _rows_for(negative_embeds, number_to_generate)


def generate_nucleus_sampling(model, tokenizer: Callable, embeds: torch.Tensor, number_to_generate: int = 1,
                              text_prefix_tokens: Optional[torch.Tensor] = None, entry_length: int = 67, top_p: float = 0.8, top_k=None,
                              temperature: float = 1.0, generator: Optional[torch.Generator] = None, rerank: bool = False, *,
                              no_repeat_ngram_size: int = 0, min_length: int = 0, suppress_tokens=None, min_p: float = 0.0,
                              typical_p: float = 1.0, epsilon_cutoff: float = 0.0, eta_cutoff: float = 0.0, guidance_scale: float = 1.0,
                              negative_embeds: Optional[torch.Tensor] = None) -> List[str]:
    """base.py:135-201 with a KV cache and the sampling step on the device.  The reference is batch-1 and loops number_to_generate
    times; here every (prefix row, repetition) is one row of a single batched decode.  The returned text of a row includes its
    stop token, as the reference's does (it appends before breaking, base.py:186-195).
    ``rerank`` (not in the reference; off by default): the ``number_to_generate`` texts of every prefix row come back ordered by their
    length-normalised likelihood under the model, best first (inference/score.py rerank_captions), instead of in sampling order.
    ``guidance_scale`` != 1 (module docstring): ``negative_embeds`` None = the embedding of tokenizer.bos_token; the text prefix follows it.
    Guidance shapes what is sampled; ``rerank`` keeps ranking by the UNGUIDED likelihood, the model's own p(caption | prefix).
    ``min_p`` / ``typical_p`` / ``epsilon_cutoff`` / ``eta_cutoff``: the truncation rules of sample_tokens (off by default); ``top_p`` is
    then a mass of the truncated row."""
    stop = _stop_id(tokenizer)
    negative_embeds = _negative_context(model, tokenizer, negative_embeds, text_prefix_tokens, guidance_scale)
    embeds = _with_text_prefix(model, embeds, text_prefix_tokens)
    toks, stop_pos = sample_tokens(model, _rows_for(embeds, number_to_generate), entry_length, stop, mode=0, top_p=top_p, top_k=top_k,
                                   temperature=temperature, generator=generator, no_repeat_ngram_size=no_repeat_ngram_size,
                                   min_length=min_length, suppress_tokens=suppress_tokens, min_p=min_p, typical_p=typical_p,
                                   epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff, guidance_scale=guidance_scale,
                                   negative_embeds=_negative_rows_for(negative_embeds, number_to_generate))
    rows = list(range(toks.shape[0]))
    if rerank and number_to_generate > 1:
        rows = _likelihood_order(model, embeds, toks, stop_pos, number_to_generate)
    head = [] if text_prefix_tokens is None else [int(t) for t in text_prefix_tokens.flatten()]
    toks, stop_pos = toks.cpu(), stop_pos.cpu()
    return [tokenizer.decode(head + toks[r, :min(int(stop_pos[r]) + 1, toks.shape[1])].tolist()) for r in rows]


def _likelihood_order(model, embeds: torch.Tensor, toks: torch.Tensor, stop_pos: torch.Tensor, n_gen: int) -> List[int]:
    """Row indices of a sample_tokens result of ``n_gen`` repetitions per prefix row, each prefix row's repetitions best first:
    every text as it is returned (up to and including its stop token) scored by rerank_captions."""
    from clipcap_amd.inference.score import rerank_captions
    keep = torch.arange(toks.shape[1], device=toks.device).view(1, -1) <= stop_pos.view(-1, 1)
    cand = torch.where(keep, toks, torch.full_like(toks, -1)).view(embeds.shape[0], n_gen, -1)
    order, _ = rerank_captions(model, embeds, cand)
    base = torch.arange(embeds.shape[0], device=order.device).view(-1, 1) * n_gen
    return (base + order).flatten().tolist()


def generate_no_beam(model, tokenizer: Callable, embeds: torch.Tensor, text_prefix_tokens: Optional[torch.Tensor] = None,
                     top_p: float = 0.9, top_k: float = 0.0, entry_length: int = 67, temperature: float = 1.0,
                     repetition_penalty: float = 1.2, desired_sentence_length: int = 50, sentence_length_factor: float = 1.0,
                     sweep: bool = True, generator: Optional[torch.Generator] = None, *, no_repeat_ngram_size: int = 0, min_length: int = 0,
                     suppress_tokens=None, min_p: float = 0.0, typical_p: float = 1.0, epsilon_cutoff: float = 0.0, eta_cutoff: float = 0.0,
                     guidance_scale: float = 1.0, negative_embeds: Optional[torch.Tensor] = None) -> List[str]:
    """base.py:204-279: the reference's debugging sweep over top_p x temperature (sweep=True reproduces it; sweep=False samples
    once with the given top_p / temperature).  Like the reference, ``repetition_penalty`` is accepted but not applied (its call is
    commented out, base.py:236-239).  The sentence-length penalty (base.py:248-254) is applied as the reference applies it: after the
    filter, history tokens whose VALUE equals the stop token id (utils.py:45 compares values, not ids) are scaled — on the device,
    inside the sampling step.  The text of a row excludes its stop token (the reference breaks before appending, base.py:261-262).
    ``guidance_scale`` != 1 (module docstring): ``negative_embeds`` None = the embedding of tokenizer.bos_token; the text prefix follows it.
    ``min_p`` / ``typical_p`` / ``epsilon_cutoff`` / ``eta_cutoff``: the truncation rules of sample_tokens (off by default), like the
    sampling step here without a repetition penalty; the filter's top_k / top_p then act on the truncated row."""
    stop = _stop_id(tokenizer)
    negative_embeds = _negative_context(model, tokenizer, negative_embeds, text_prefix_tokens, guidance_scale)
    embeds = _with_text_prefix(model, embeds, text_prefix_tokens)
    grid = [(p, t) for p in (0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95, 1.0) for t in (0.9, 0.95, 1.0)] if sweep \
        else [(top_p, temperature)]
    head = [] if text_prefix_tokens is None else [int(v) for v in text_prefix_tokens.flatten()]
    gens = []
    for p, t in grid:
        toks, stop_pos = sample_tokens(model, embeds, entry_length, stop, mode=1, top_p=p, top_k=int(top_k), temperature=t, generator=generator,
                                       head_tokens=text_prefix_tokens, desired_sentence_length=desired_sentence_length,
                                       sentence_length_factor=sentence_length_factor, no_repeat_ngram_size=no_repeat_ngram_size,
                                       min_length=min_length, suppress_tokens=suppress_tokens, min_p=min_p, typical_p=typical_p,
                                       epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff, guidance_scale=guidance_scale,
                                       negative_embeds=negative_embeds)
        toks, stop_pos = toks.cpu(), stop_pos.cpu()
        gens.extend(tokenizer.decode(head + toks[r, :int(stop_pos[r])].tolist()) for r in range(toks.shape[0]))
    return gens
