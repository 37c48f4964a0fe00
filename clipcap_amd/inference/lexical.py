"""Lexically constrained beam search (not in the reference): captions that contain required phrases — a product name, a detected class label,
a keyword.  Constrained beam search was introduced for image captioning (Anderson et al., EMNLP 2017, "Guided Open Vocabulary Image
Captioning with Constrained Beam Search"); the variant here is dynamic beam allocation (Post & Vilar, NAACL 2018, "Fast Lexically Constrained
Decoding with Dynamic Beam Allocation for Neural Machine Translation"), which keeps the beam width fixed: every beam row carries which
phrases it has produced, a hypothesis may stop only when it holds all of them, and the ``beam_size`` slots of a step are divided between
the candidates by how many constraint tokens they have met (cc_beam_lex_step: three launches; include/clipcap_hip.h states the rule).
The rest of a step is the beam decoders': the KV-cached forward, cc_logits_guide, cc_logits_constrain, cc_beam_advance.

Scores stay the model's own length-normalised log-probabilities: the stop token is banned as a candidate, not in the softmax.  A phrase is a
run of token ids, so "a dog" and " dog" are different phrases: the caller writes the leading space.  Not covered: alternatives ("giraffe"
or "giraffes"), and pruning hypotheses that can no longer finish within ``entry_length`` — a caption that runs out of positions may lack
phrases, which ``all_met`` reports."""
from __future__ import annotations

from typing import Callable, List, NamedTuple, Optional

import torch

from clipcap_amd import engine
from clipcap_amd.engine import DecodeSession, beam_lex_buffers, beam_lex_step
from clipcap_amd.inference.base import (_bans, _negative_context, _negative_rows, _persistent_decode_on, _stop_id, _with_text_prefix)
from clipcap_amd.inference.utils import unpack_lex_state, validate_phrases, validate_stochastic_beam


class ConstrainedBeams(NamedTuple):
    """tokens int64 (S, k, n); scores (S, k) length-normalised log-probabilities; seq_lengths (S, k); tokens_met int32 (S, k) = the constraint
    tokens a beam has produced (whole phrases, plus its progress into one); all_met bool (S, k).  Slot 0 has the largest tokens_met of its
    prefix; an empty slot (fewer than k hypotheses exist under extreme bans) has score -inf."""
    tokens: torch.Tensor
    scores: torch.Tensor
    seq_lengths: torch.Tensor
    tokens_met: torch.Tensor
    all_met: torch.Tensor


@torch.no_grad()
def generate_constrained_beam_tokens(model, embeds: torch.Tensor, phrases, beam_size: int = 5, entry_length: int = 67, temperature: float = 1.0,
                                     stop_token: int = 50256, *, no_repeat_ngram_size: int = 0, min_length: int = 0, suppress_tokens=None,
                                     guidance_scale: float = 1.0, negative_embeds: Optional[torch.Tensor] = None) -> ConstrainedBeams:
    """Token-level constrained beam search for a batch of prefixes, embeds fp32 (S, L, D).  ``phrases``: an int tensor (S, C, L) or (1, C, L)
    padded with -1, nested lists of ids per prefix, or one list of phrases for all prefixes; at most 8 phrases of at most 8 tokens per prefix
    (inference/utils.py validate_phrases).  The loop is generate_stochastic_beam_tokens' with cc_beam_lex_step reading the plain logits:
    prefill one row per prefix, the first update, the fan-out, then per position the forward(s), the guidance, the bans (stopped beams
    skipped), the update and cc_beam_advance (both sessions when guided), with the all-stopped poll every 4th step.
    ``no_repeat_ngram_size`` / ``min_length`` / ``suppress_tokens`` / ``guidance_scale`` with ``negative_embeds`` (needed here when the
    scale is not 1): as in the beam decoders (inference/base.py's docstring); a ban that removes a phrase's next token keeps that phrase
    from being produced at that step.
    Returns ConstrainedBeams(tokens int64 (S, k, n), scores (S, k), seq_lengths (S, k), tokens_met (S, k), all_met (S, k))."""
    validate_stochastic_beam(beam_size)                                         # an int in [1, 16]
    lm = model.language_model
    g = lm.engine
    V = g.dims["V"]
    dev = g.arena.device
    S, L0, D = embeds.shape
    table = validate_phrases(phrases, S, V, stop_token, suppress_tokens)
    embeds = embeds.to(dev, torch.float32)
    R = S * beam_size
    gs, neg = _negative_rows(negative_embeds, guidance_scale, S, D, dev, "generate_constrained_beam_tokens")
    guided = neg is not None
    bans = _bans(V, stop_token, no_repeat_ngram_size, min_length, suppress_tokens, dev)
    total = min(entry_length, g.dims["NPOS"] - L0)
    if total < 1:
        raise RuntimeError(f"a {L0}-position prefix leaves no room to generate (n_positions = {g.dims['NPOS']})")
    wte = lm.get_input_embeddings().weight.detach()
    table = table.to(dev)
    n_phr = int(table.shape[1])
    scores = torch.zeros(R, dtype=torch.float32, device=dev)
    seq_lengths = torch.ones(R, dtype=torch.float32, device=dev)
    has_stopped = torch.zeros(R, dtype=torch.uint8, device=dev)
    lex_state = torch.zeros(R, dtype=torch.int32, device=dev)
    fan = torch.arange(S, device=dev, dtype=torch.int32).repeat_interleave(beam_size)
    sess = DecodeSession(g, S, L0 + total)
    logits0 = sess.forward(embeds)                                              # (S, V)
    lg = torch.empty(R, V, dtype=torch.float32, device=dev)
    if guided:                                                                  # the unconditional stream: its own positions, from 0
        usess = DecodeSession(g, S, neg.shape[1] + total)
        engine.guide_logits(logits0, usess.forward(neg), gs, out=lg[::beam_size])
    else:
        lg[::beam_size] = logits0                                               # row 0 of every beam set
    bufs = beam_lex_buffers(dev, S, beam_size, n_phr, V)

    def update(logits, first):
        return beam_lex_step(logits, S, beam_size, temperature, first, stop_token, scores, seq_lengths, has_stopped, lex_state,
                             table if n_phr else None, bufs)

    if bans is not None:
        bans.apply(lg[::beam_size], 0)
    next_tok, src = update(lg, True)
    sess = sess.expand(fan, R)
    if guided:
        usess = usess.expand(fan, R)
    tok = [torch.zeros(R, total, dtype=torch.int32, device=dev) for _ in range(2)]
    x = torch.empty(R, 1, D, dtype=torch.float32, device=dev)
    sess.beam_advance(beam_size, next_tok, None, wte, 0, tok[1], tok[0], x)
    n = 1                                                                       # token columns written so far = the next position index
    for i in range(1, entry_length):
        # a step after every beam has stopped only appends token 0: scores, lengths, states and the slot order pass through bit for bit
        if i % 4 == 1 and bool(has_stopped.all()):
            break
        if n >= total:
            raise RuntimeError(f"generation reached n_positions = {g.dims['NPOS']} ({L0}-position prefix + {n} tokens)")
        logits = sess.forward(x, group=beam_size)
        if guided:
            engine.guide_logits(logits, usess.forward(x, group=beam_size), gs, skip_rows=has_stopped)
        if bans is not None:
            bans.apply(logits, n, tok[(n - 1) & 1], n, None, has_stopped)
        next_tok, src = update(logits, False)
        sess.beam_advance(beam_size, next_tok, src, wte, n, tok[(n - 1) & 1], tok[n & 1], x)
        if guided:
            usess.beam_advance(beam_size, next_tok, src, wte, n, tok[(n - 1) & 1], tok[n & 1], x)
        n += 1
    if _persistent_decode_on():
        sess.check()
    met, done = unpack_lex_state(lex_state, table)
    return ConstrainedBeams(tok[(n - 1) & 1][:, :n].to(torch.int64).view(S, beam_size, -1), (scores / seq_lengths).view(S, beam_size),
                            seq_lengths.view(S, beam_size).clone(), met, done)


def best_constrained_beams(scores: torch.Tensor, tokens_met: torch.Tensor, n: int = 1) -> torch.Tensor:
    """Indices (S, n) of the n best beams of every row: ``tokens_met`` (S, beam) descending, then ``scores`` (S, beam) descending, then the
    beam index ascending.  Pure torch."""
    by_score = torch.sort(scores, dim=1, descending=True, stable=True).indices
    by_met = torch.sort(tokens_met.gather(1, by_score), dim=1, descending=True, stable=True).indices
    return by_score.gather(1, by_met)[:, :n]


def generate_constrained_beam(model, tokenizer: Callable, embeds: torch.Tensor, force_words, text_prefix_tokens: Optional[torch.Tensor] = None,
                              beam_size: int = 5, entry_length: int = 67, temperature: float = 1.0, *, num_return_sequences: int = 1,
                              no_repeat_ngram_size: int = 0, min_length: int = 0, suppress_tokens=None, guidance_scale: float = 1.0,
                              negative_embeds: Optional[torch.Tensor] = None) -> List[str]:
    """Texts of generate_constrained_beam_tokens: for every prefix row its ``num_return_sequences`` best captions in best_constrained_beams
    order (most constraint tokens first, then the score), next to each other; empty slots are skipped.
    ``force_words``: a list of strings for all prefixes, or one list of strings per prefix.  Each string is encoded with
    tokenizer.encode(word) and must appear as that run of tokens, so the caller writes the leading space (" dog", not "dog", for a word
    inside a GPT-2 caption).  ``guidance_scale`` != 1: ``negative_embeds`` None = the embedding of tokenizer.bos_token, the text prefix after
    it, as generate_beam builds it."""
    validate_stochastic_beam(beam_size, num_return_sequences)
    stop = _stop_id(tokenizer)
    words = list(force_words)
    per_prefix = bool(words) and all(not isinstance(w, str) for w in words)
    phrases = [[list(tokenizer.encode(w)) for w in ws] for ws in words] if per_prefix else [list(tokenizer.encode(w)) for w in words]
    negative_embeds = _negative_context(model, tokenizer, negative_embeds, text_prefix_tokens, guidance_scale)
    embeds = _with_text_prefix(model, embeds, text_prefix_tokens)
    r = generate_constrained_beam_tokens(model, embeds, phrases, beam_size, entry_length, temperature, stop,
                                         no_repeat_ngram_size=no_repeat_ngram_size, min_length=min_length, suppress_tokens=suppress_tokens,
                                         guidance_scale=guidance_scale, negative_embeds=negative_embeds)
    tokens, scores, lengths = r.tokens.cpu(), r.scores.cpu(), r.seq_lengths.cpu()
    best = best_constrained_beams(scores, r.tokens_met.cpu(), int(num_return_sequences))
    out = []
    for s in range(tokens.shape[0]):
        for b in best[s].tolist():
            if scores[s, b] > float("-inf"):
                out.append(tokenizer.decode(tokens[s, b, :int(lengths[s, b])].numpy()))
    return out
