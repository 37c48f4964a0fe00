"""Float64 statement of stochastic beam search's device step (cc_beam_gumbel_step, include/clipcap_hip.h) for ONE sample, with the noise
from the same bits: Philox4x32-10 in numpy, u = (h + 0.5) / 2^32, n = -ln(-ln u) in float64.  Two stages, as the header states them: per
parent row the `beam` best tokens by y = x + n; per sample the conditioned values Gamma_c of the kept candidates and the `beam` best of
them.  The GPU tests compare the kernels with this; tests/test_gumbel_ref.py pins it on the CPU (known answers, beam 1 = arg-max of the
perturbed logits, the sampling-without-replacement statistics)."""
import math
from collections import namedtuple

import numpy as np
import torch

GumbelStep = namedtuple("GumbelStep", "tokens src phi gam lengths stopped margin")

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
INF = float("inf")


def philox4x32_10(ctr, key):
    """ctr (..., 4), key (..., 2) of uint32 (broadcast against each other) -> (..., 4) uint32: ten rounds, the key bumped between rounds."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    key = np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = (ctr[..., i] for i in range(4))
    k0, k1 = key[..., 0], key[..., 1]
    for r in range(10):
        if r:
            k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2                    # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def noise_bits(seed: int, step: int, row: int, V: int) -> np.ndarray:
    """uint32 (V,): token v reads word v & 3 of philox(counter = (v >> 2, row, step, 0), key = (lo32(seed), hi32(seed)))."""
    q = np.arange((V + 3) // 4, dtype=np.uint64)
    ctr = np.stack((q, np.full_like(q, row), np.full_like(q, step), np.zeros_like(q)), axis=-1)
    return philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)).reshape(-1)[:V]


def gumbel_from_bits(h) -> np.ndarray:
    """float64 n = -ln(-ln u), u = (h + 0.5) / 2^32; the upper half of the words through log1p of the distance to 1, which is exact there."""
    h = np.asarray(h, dtype=np.uint64).astype(np.float64)
    lo = h < 2.0 ** 31
    e = np.where(lo, -np.log(np.where(lo, h + 0.5, 1.0) * 2.0 ** -32), -np.log1p(-np.where(lo, 1.0, 2.0 ** 32 - 1.0 - h + 0.5) * 2.0 ** -32))
    return -np.log(e)


def noise(seed: int, step: int, row: int, V: int) -> torch.Tensor:
    return torch.from_numpy(gumbel_from_bits(noise_bits(seed, step, row, V)))


def _log1mexp(d: float) -> float:
    """log(1 - exp(-d)), d >= 0"""
    if d <= 0.0:
        return -INF
    return math.log(-math.expm1(-d)) if d <= math.log(2.0) else math.log1p(-math.exp(-d))


def _gap(a: float, b: float) -> float:
    return 0.0 if a == b else a - b


def gumbel_step_ref(logits, phi, gam, seq_lengths, has_stopped, *, beam, seed, step, row0, temperature=1.0, first=False,
                    stop_token=50256, noise_rows=None) -> GumbelStep:
    """logits (beam, V) (first: only row 0 is read); phi, gam, seq_lengths (beam,) and has_stopped (beam,) bool are the state BEFORE the step
    (ignored when ``first``); row0 = the index of the sample's row 0 among the call's logits rows (s * beam), which the noise is keyed on
    (``noise_rows`` (beam, V): use this noise instead, for tests that draw many seeds' bits in one Philox call).
    Returns the new state in float64: tokens, src (source row inside the sample; 0 on the first step), phi, gam, lengths, stop flags, and
    the decision margin: the smallest gap between consecutive kept Gamma_c and to the first rejected one, and the smallest stage-1 gap in
    y between a row's last kept and first rejected token."""
    V = logits.shape[1]
    T = temperature if temperature > 0 else 1.0
    margin = INF
    cands = []                                                         # (Gamma_c, flat index, phi_c, b, v)
    for b in range(1 if first else beam):
        pb, gb = (0.0, 0.0) if first else (float(phi[b]), float(gam[b]))
        if not first and bool(has_stopped[b]):                         # exactly one candidate: the padding token, unperturbed
            cands.append((gb, b * V, pb, b, 0))
            continue
        x = logits[b].double() / T
        lp = torch.log_softmax(x, -1)
        nz = noise(seed, step, row0 + b, V) if noise_rows is None else noise_rows[b].double()
        y = x + nz
        live = torch.nonzero(x > -INF).flatten()
        if live.numel() == 0:
            continue
        k1 = min(beam + 1, live.numel())
        thr = torch.topk(y[live], k1).values[-1]
        idx = live[y[live] >= thr].tolist()
        order = sorted(idx, key=lambda v: (-float(y[v]), v))[:k1]
        if len(order) > beam:
            margin = min(margin, _gap(float(y[order[beam - 1]]), float(y[order[beam]])))
        Y = float(y[order[0]])
        for v in order[:beam]:
            pc = pb + float(lp[v])
            g = pc + float(nz[v])
            t = gb - g + _log1mexp(Y - float(y[v]))
            gc = gb - max(0.0, t) - math.log1p(math.exp(-abs(t))) if t > -INF else gb
            cands.append((gc, b * V + v, pc, b, v))
    cands = sorted((c for c in cands if c[0] > -INF), key=lambda c: (-c[0], c[1]))
    for a, b_ in zip(cands[:beam], cands[1:beam + 1]):
        margin = min(margin, _gap(a[0], b_[0]))
    tokens, src, nphi, ngam, nlen, nstop = [], [], [], [], [], []
    for k in range(beam):
        if k < len(cands):
            gc, _, pc, b, v = cands[k]
            st = False if first else bool(has_stopped[b])
            tokens.append(v); src.append(b); nphi.append(pc); ngam.append(gc)
            nlen.append(1.0 if first else float(seq_lengths[b]) + (0.0 if st else 1.0))
            nstop.append(st or v == stop_token)
        else:                                                          # an empty slot
            tokens.append(0); src.append(0); nphi.append(-INF); ngam.append(-INF)
            nlen.append(1.0 if first else float(seq_lengths[0]))
            nstop.append(True)
    return GumbelStep(torch.tensor(tokens), torch.tensor(src), torch.tensor(nphi, dtype=torch.float64), torch.tensor(ngam, dtype=torch.float64),
                      torch.tensor(nlen, dtype=torch.float64), torch.tensor(nstop), margin)


def stochastic_beam_search_ref(sd, embeds, *, n_head, n_layer, beam, entry_length, stop_token, seed, row0, temperature=1.0,
                               no_repeat_ngram_size=0, min_length=0, pre="language_model."):
    """Stochastic beam search for ONE prefix (1, L, D) on the CPU: the oracle's full re-forward per step (oracle.gpt2_logits, fp32), the bans
    of the constrained decoders masked into the logits of every beam that has not stopped, and gumbel_step_ref for the update, with the
    position index as the step.  -> (tokens (beam, n) int64, phi, gam, seq_lengths, the smallest decision margin at any step)."""
    from clipcap_amd.inference.utils import banned_tokens
    from oracle import clipcap_oracle as O
    wte = sd[pre + "transformer.wte.weight"]
    tokens, phi, gam, seql, stopped = None, None, None, None, None
    margin = INF
    for step in range(entry_length):
        logits = O.gpt2_logits(sd, embeds, n_head, n_layer, pre=pre)[:, -1, :].clone()
        for r in range(logits.shape[0]):
            if tokens is not None and bool(stopped[r]):
                continue
            ban = (banned_tokens(tokens[r], no_repeat_ngram_size) if tokens is not None else set()) | ({stop_token} if step < min_length else set())
            if ban:
                logits[r, sorted(ban)] = -INF
        first = tokens is None
        r = gumbel_step_ref(logits.expand(beam, -1) if first else logits, phi, gam, seql, stopped, beam=beam, seed=seed, step=step, row0=row0,
                            temperature=temperature, first=first, stop_token=stop_token)
        margin = min(margin, r.margin)
        phi, gam, seql, stopped = r.phi, r.gam, r.lengths, r.stopped
        if first:
            embeds = embeds.expand(beam, *embeds.shape[1:])
            tokens = r.tokens.unsqueeze(1)
        else:
            tokens = torch.cat((tokens[r.src], r.tokens.unsqueeze(1)), dim=1)
            embeds = embeds[r.src]
        embeds = torch.cat((embeds, wte[r.tokens].view(beam, 1, -1)), dim=1)
        if bool(stopped.all()):
            break
    return tokens, phi, gam, seql, margin
