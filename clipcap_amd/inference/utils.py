"""Logit post-processing used by the sampling decoders — same names/semantics as the reference's helpers
(clipcap/inference/utils.py:5-51, duplicated in inference/base.py:9-55).  Unlike the reference these work on device tensors
of any batch shape (..., V) and do not modify their input."""
from __future__ import annotations

import torch
import torch.nn.functional as F


def top_k_top_p_filtering(logits: torch.Tensor, top_k: int = 0, top_p: float = 0.0, filter_value: float = -float("inf")) -> torch.Tensor:
    """Keep the top_k highest logits and/or the smallest sorted set whose cumulative probability exceeds top_p (the first
    token above the threshold is kept, utils.py:25-28)."""
    out = logits.clone()
    k = min(int(top_k), out.size(-1))
    if k > 0:
        kth = torch.topk(out, k, dim=-1).values[..., -1:]
        out = out.masked_fill(out < kth, filter_value)
    if top_p > 0.0:
        sorted_logits, sorted_idx = torch.sort(out, descending=True, dim=-1)
        cum = torch.cumsum(F.softmax(sorted_logits, dim=-1), dim=-1)
        drop_sorted = cum > top_p
        drop_sorted = torch.cat((torch.zeros_like(drop_sorted[..., :1]), drop_sorted[..., :-1]), dim=-1)
        drop = torch.zeros_like(drop_sorted).scatter(-1, sorted_idx, drop_sorted)
        out = out.masked_fill(drop, filter_value)
    return out


def repetition_penalty_apply(logits: torch.Tensor, tokens: torch.Tensor, penalty: float) -> torch.Tensor:
    """utils.py:33-37: already-generated tokens get logit*penalty if negative else logit/penalty."""
    out = logits.clone()
    t = torch.gather(out, -1, tokens)
    return out.scatter(-1, tokens, torch.where(t < 0, t * penalty, t / penalty))


def sentence_length_penalty_apply(logits: torch.Tensor, tokens: torch.Tensor, stop_token: int, current_length: int, desired_length: int,
                                  length_factor: float) -> torch.Tensor:
    """utils.py:39-49.  NB: like the reference this compares the gathered logit VALUES with ``stop_token`` (not token ids)."""
    out = logits.clone()
    penalty = (current_length / desired_length) * length_factor
    t = torch.gather(out, -1, tokens)
    return out.scatter(-1, tokens, torch.where(t == stop_token, t * penalty, t))


def nucleus_distribution(logits: torch.Tensor, top_p: float = 0.8, top_k=None) -> torch.Tensor:
    """Pre-sampling distribution of generate_nucleus_sampling (inference/base.py:165-181): probabilities sorted descending,
    cut at the first cumulative mass >= top_p (inclusive), renormalised, scattered back.  logits (n, V) -> (n, V)."""
    V = logits.shape[-1]
    top_k = V if top_k is None else top_k
    top_p = 1.0 if top_p is None else top_p
    p, idx = F.softmax(logits, dim=-1).topk(top_k, dim=-1)
    cum = p.cumsum(dim=-1)
    thr = torch.full((p.shape[0], 1), float(top_p), device=logits.device, dtype=cum.dtype)
    cut_i = torch.searchsorted(cum, thr).clamp(max=top_k - 1)
    cut = torch.gather(cum, -1, cut_i)
    kept = (cum <= cut) * p
    kept = kept / kept.sum(dim=-1, keepdim=True)
    return torch.zeros_like(logits).scatter(-1, idx, kept.to(logits.dtype))


# ---- constrained decoding (not in the reference: no_repeat_ngram_size / min_length / suppress_tokens of the decoders) ----------------
# A ban sets the token's logit to -inf BEFORE the softmax, the convention of top_k_top_p_filtering above: the banned mass is
# renormalised over the allowed tokens.  The device applies the bans in cc_logits_constrain; these two are its CPU side.

MAX_SUPPRESS_TOKENS = 1023      # the suppress list cc_logits_constrain accepts


def banned_tokens(history, no_repeat_ngram_size: int) -> set:
    """Tokens the no-repeat rule forbids as the next token of ``history`` (generated ids, oldest first; a sequence or a 1-D tensor):
    with g = no_repeat_ngram_size and n = len(history), h[i+g-1] for every i in [0, n-g] whose g-1 tokens h[i : i+g-1] equal the last
    g-1 tokens h[n-g+1 : n] — appending such a token would repeat an n-gram of the history.  g = 1 bans every token of the history,
    n < g bans nothing, 0 turns the rule off.  Plain Python: the statement of the rule that the device kernel is tested against."""
    h = [int(t) for t in (history.tolist() if hasattr(history, "tolist") else history)]
    g, n = int(no_repeat_ngram_size), len(h)
    if g <= 0 or n < g:
        return set()
    tail = h[n - g + 1:]
    return {h[i + g - 1] for i in range(n - g + 1) if h[i:i + g - 1] == tail}


def validate_constraints(vocab_size: int, stop_token: int, no_repeat_ngram_size: int = 0, min_length: int = 0, suppress_tokens=None) -> list:
    """Checks the three decoding constraints against a vocabulary of ``vocab_size`` ids and returns the suppress list as plain ints
    ([] for None).  ValueError for a negative size or length, an id outside [0, vocab_size), more than MAX_SUPPRESS_TOKENS ids, and a
    suppress list that holds the stop token while min_length == 0: such a decode could never stop.  Pure: touches no device."""
    g, m = int(no_repeat_ngram_size), int(min_length)
    if g < 0:
        raise ValueError(f"no_repeat_ngram_size must be >= 0, got {no_repeat_ngram_size}")
    if m < 0:
        raise ValueError(f"min_length must be >= 0, got {min_length}")
    ids = [] if suppress_tokens is None else [int(t) for t in (suppress_tokens.tolist() if hasattr(suppress_tokens, "tolist") else suppress_tokens)]
    if len(ids) > MAX_SUPPRESS_TOKENS:
        raise ValueError(f"suppress_tokens holds {len(ids)} ids; at most {MAX_SUPPRESS_TOKENS} are supported")
    bad = [t for t in ids if not 0 <= t < vocab_size]
    if bad:
        raise ValueError(f"suppress_tokens ids outside [0, {vocab_size}): {bad[:8]}")
    if (m > 0 or stop_token in ids) and not 0 <= int(stop_token) < vocab_size:
        raise ValueError(f"stop token {stop_token} is outside [0, {vocab_size})")
    if m == 0 and int(stop_token) in ids:
        raise ValueError(f"suppress_tokens contains the stop token {stop_token} and min_length is 0: this decode can never stop")
    return ids


# ---- classifier-free guidance (not in the reference: guidance_scale / negative_embeds of the beam and sampling decoders) ---------------

def validate_guidance(guidance_scale: float = 1.0) -> float:
    """Checks the guidance scale of the decoders and returns it as a float.  ValueError unless it is a finite number >= 0 (1: no guidance,
    the decoder as it is without the option; 0: the unconditional stream alone).  Pure: touches no device."""
    import math
    try:
        g = float(guidance_scale)
    except (TypeError, ValueError):
        raise ValueError(f"guidance_scale must be a finite number >= 0, got {guidance_scale!r}") from None
    if isinstance(guidance_scale, bool) or not math.isfinite(g) or g < 0:
        raise ValueError(f"guidance_scale must be finite and >= 0, got {guidance_scale!r}")
    return g


# ---- diverse beam search (not in the reference: num_beam_groups / diversity_penalty / num_return_sequences of the beam decoders) --------

def validate_beam_groups(beam_size: int, num_beam_groups: int = 1, diversity_penalty: float = 0.0, num_return_sequences: int = 1) -> None:
    """Checks the diverse-beam-search options of the beam decoders.  ValueError for num_beam_groups < 1 or not a divisor of beam_size, a
    penalty that is negative or not finite, beam groups without a penalty (with a penalty of 0 all beam groups would hold the same
    hypotheses after the first step), a penalty without beam groups (it would have nothing to act on), and num_return_sequences outside
    [1, beam_size].  Pure: touches no device."""
    import math
    b, g, n = int(beam_size), int(num_beam_groups), int(num_return_sequences)
    p = float(diversity_penalty)
    if g < 1:
        raise ValueError(f"num_beam_groups must be >= 1, got {num_beam_groups}")
    if b % g:
        raise ValueError(f"beam_size {beam_size} is not a multiple of num_beam_groups {num_beam_groups}")
    if not math.isfinite(p) or p < 0:
        raise ValueError(f"diversity_penalty must be finite and >= 0, got {diversity_penalty}")
    if g > 1 and p == 0:
        raise ValueError(f"num_beam_groups = {g} needs diversity_penalty > 0: without a penalty every beam group finds the same hypotheses")
    if g == 1 and p > 0:
        raise ValueError(f"diversity_penalty = {p} needs num_beam_groups > 1: the penalty acts between beam groups")
    if not 1 <= n <= b:
        raise ValueError(f"num_return_sequences must be in [1, beam_size = {beam_size}], got {num_return_sequences}")


# ---- contrastive search (not in the reference: top_k / penalty_alpha of generate_contrastive) ------------------------------------------

MAX_CONTRASTIVE_TOP_K = 8       # the candidates per caption cc_contrastive_topk / cc_contrastive_select accept


def validate_contrastive(top_k: int, penalty_alpha: float) -> None:
    """Checks the options of the contrastive-search decoders.  ValueError for a top_k that is not an int in [1, MAX_CONTRASTIVE_TOP_K] and
    for a penalty_alpha that is not finite or outside [0, 1] (0: no penalty, greedy decoding; 1: the model's probabilities are ignored).
    Pure: touches no device."""
    import math
    if isinstance(top_k, bool) or not isinstance(top_k, int) or not 1 <= top_k <= MAX_CONTRASTIVE_TOP_K:
        raise ValueError(f"top_k must be an int in [1, {MAX_CONTRASTIVE_TOP_K}], got {top_k!r}")
    try:
        a = float(penalty_alpha)
    except (TypeError, ValueError):
        raise ValueError(f"penalty_alpha must be a number in [0, 1], got {penalty_alpha!r}") from None
    if not math.isfinite(a) or not 0.0 <= a <= 1.0:
        raise ValueError(f"penalty_alpha must be finite and in [0, 1], got {penalty_alpha!r}")


# ---- truncation rules of the sampling decoders (not in the reference: min_p / typical_p / epsilon_cutoff / eta_cutoff) ------------------

def validate_truncation(min_p: float = 0.0, typical_p: float = 1.0, epsilon_cutoff: float = 0.0, eta_cutoff: float = 0.0) -> dict:
    """Checks the four truncation options of the sampling decoders and returns them as a dict of floats, keyed as engine.truncate_logits
    takes them.  ValueError unless min_p is in [0, 1] (0: off), typical_p in (0, 1] (1: off), epsilon_cutoff and eta_cutoff in [0, 1)
    (0: off); NaN and non-numbers are refused.  Pure: touches no device."""
    out = {}
    for name, val, ok, rng in (("min_p", min_p, lambda a: 0.0 <= a <= 1.0, "[0, 1]"), ("typical_p", typical_p, lambda a: 0.0 < a <= 1.0, "(0, 1]"),
                               ("epsilon_cutoff", epsilon_cutoff, lambda a: 0.0 <= a < 1.0, "[0, 1)"),
                               ("eta_cutoff", eta_cutoff, lambda a: 0.0 <= a < 1.0, "[0, 1)")):
        try:
            a = float(val)
        except (TypeError, ValueError):
            raise ValueError(f"{name} must be a number in {rng}, got {val!r}") from None
        if isinstance(val, bool) or not ok(a):                  # NaN fails every comparison
            raise ValueError(f"{name} must be in {rng}, got {val!r}")
        out[name] = a
    return out


def truncation_is_on(opts: dict) -> bool:
    """whether any rule of a validate_truncation result does anything"""
    return opts["min_p"] > 0.0 or opts["typical_p"] < 1.0 or opts["epsilon_cutoff"] > 0.0 or opts["eta_cutoff"] > 0.0


# ---- stochastic beam search (not in the reference: inference/stochastic_beam.py) ----------------------------------------------------------

MAX_STOCHASTIC_BEAM = 16        # the beam widths cc_beam_gumbel_step accepts


def validate_stochastic_beam(beam_size: int, num_return_sequences=None, seed=None) -> None:
    """Checks the options of the stochastic-beam-search decoders.  ValueError for a beam_size that is not an int in [1,
    MAX_STOCHASTIC_BEAM], a num_return_sequences that is neither None (all) nor an int in [1, beam_size], and a seed that is neither None
    (drawn from a generator) nor an int in [0, 2^64).  Pure: touches no device."""
    if isinstance(beam_size, bool) or not isinstance(beam_size, int) or not 1 <= beam_size <= MAX_STOCHASTIC_BEAM:
        raise ValueError(f"beam_size must be an int in [1, {MAX_STOCHASTIC_BEAM}], got {beam_size!r}")
    n = num_return_sequences
    if n is not None and (isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= beam_size):
        raise ValueError(f"num_return_sequences must be None or an int in [1, beam_size = {beam_size}], got {n!r}")
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64):
        raise ValueError(f"seed must be None or an int in [0, 2^64), got {seed!r}")


# ---- lexically constrained beam search (not in the reference: inference/lexical.py) ------------------------------------------------------

MAX_PHRASES = 8                 # the phrases per prefix and the tokens per phrase cc_beam_lex_step accepts
MAX_PHRASE_TOKENS = 8


def validate_phrases(phrases, samples: int, vocab_size: int, stop_token: int, suppress_tokens=None) -> torch.Tensor:
    """Checks the forced phrases of a constrained beam search over ``samples`` prefixes and returns them as the table cc_beam_lex_step
    reads: int32 (samples, C, L) on the CPU, -1 after a phrase's last token (a row of -1: no phrase; C = 0 when there is none at all).
    ``phrases``: an int tensor (samples, C, L) or (1, C, L) padded with negative ids, or nested lists of ids — one list of phrases per
    prefix, or one list of phrases for all prefixes.  ValueError for more than MAX_PHRASES phrases for a prefix, a phrase that is empty or
    longer than MAX_PHRASE_TOKENS, an id outside [0, vocab_size), the stop token inside a phrase, a phrase token in ``suppress_tokens``
    (it could never be produced), the same phrase twice for one prefix, and a batch dimension that is neither 1 nor ``samples``.  Pure:
    touches no device."""
    S = int(samples)
    if isinstance(phrases, torch.Tensor):
        if phrases.dim() != 3 or phrases.dtype in (torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.bool):
            raise ValueError(f"phrases must be an int tensor ({S}, C, L) or (1, C, L), got {phrases.dtype} {tuple(phrases.shape)}")
        rows = []
        for sample in phrases.tolist():
            kept = []
            for p in sample:
                n = next((i for i, t in enumerate(p) if t < 0), len(p))
                if any(t >= 0 for t in p[n:]):
                    raise ValueError(f"a phrase row has ids after its padding: {p}")
                if n:                                                          # a row that is all padding is no phrase
                    kept.append(p[:n])
            rows.append(kept)
    else:
        seq = (list, tuple, torch.Tensor)
        rows = [] if phrases is None else [p.tolist() if isinstance(p, torch.Tensor) else list(p) for p in phrases]
        # one list of phrases per prefix iff the elements hold lists themselves (or are all empty: no phrase for any prefix)
        if rows and not (any(isinstance(q, seq) for p in rows for q in p) or all(len(p) == 0 for p in rows)):
            rows = [rows]
        rows = [[[int(t) for t in (p.tolist() if isinstance(p, torch.Tensor) else p)] for p in sample] for sample in rows] or [[]]
    if len(rows) not in (1, S):
        raise ValueError(f"phrases are given for {len(rows)} prefixes; the batch has {S} (one list for all prefixes, or one per prefix)")
    if len(rows) == 1:
        rows = rows * S
    banned = set() if suppress_tokens is None else {int(t) for t in (suppress_tokens.tolist() if hasattr(suppress_tokens, "tolist") else suppress_tokens)}
    for sample in rows:
        if len(sample) > MAX_PHRASES:
            raise ValueError(f"{len(sample)} phrases for one prefix; at most {MAX_PHRASES} are supported")
        for p in sample:
            if not 1 <= len(p) <= MAX_PHRASE_TOKENS:
                raise ValueError(f"a phrase must hold 1 to {MAX_PHRASE_TOKENS} tokens, got {len(p)}: {p}")
            bad = [t for t in p if not 0 <= t < vocab_size]
            if bad:
                raise ValueError(f"phrase ids outside [0, {vocab_size}): {bad}")
            if int(stop_token) in p:
                raise ValueError(f"the stop token {stop_token} inside a phrase: {p}")
            if banned.intersection(p):
                raise ValueError(f"phrase tokens {sorted(banned.intersection(p))} are in suppress_tokens: the phrase {p} could never be produced")
        if len({tuple(p) for p in sample}) != len(sample):
            raise ValueError(f"the same phrase twice for one prefix: {sample}")
    C = max((len(sample) for sample in rows), default=0)
    L = max((len(p) for sample in rows for p in sample), default=1)
    table = torch.full((S, C, L), -1, dtype=torch.int32)
    for s, sample in enumerate(rows):
        for c, p in enumerate(sample):
            table[s, c, :len(p)] = torch.tensor(p, dtype=torch.int32)
    return table


def unpack_lex_state(lex_state: torch.Tensor, table: torch.Tensor):
    """(tokens_met int32, all_met bool), each (S, beam), of cc_beam_lex_step's row states ``lex_state`` int32 (S * beam,) under the phrase
    ``table`` (S, C, L) of validate_phrases: bits 0-7 of a state are the met phrases, bits 8-11 the phrase in progress + 1, bits 12-15 the
    tokens of it matched so far; tokens_met = the summed lengths of the met phrases plus that progress.  Pure torch, on the state's device."""
    S, C = table.shape[0], table.shape[1]
    st = lex_state.view(S, -1).to(torch.int64)
    table = table.to(st.device)
    lens = (table >= 0).to(torch.int64).cumprod(dim=2).sum(dim=2)                  # (S, C): a phrase ends at its first negative id
    bits = (st.unsqueeze(-1) >> torch.arange(C, device=st.device)) & 1             # (S, beam, C)
    progress = torch.where(((st >> 8) & 0xF) > 0, (st >> 12) & 0xF, torch.zeros_like(st))
    full = ((lens > 0).to(torch.int64) << torch.arange(C, device=st.device)).sum(dim=1, keepdim=True)
    return ((bits * lens.unsqueeze(1)).sum(dim=2) + progress).to(torch.int32), (st & 0xFF) == full
