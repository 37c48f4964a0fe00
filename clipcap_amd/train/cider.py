"""CIDEr-D as a reward that never leaves the device: the ``reward_fn`` of ``self_critical_step``.

The metric is the reference's ``eval/pycocoevalcap/cider/cider_scorer.py`` (CIDEr-D: clipped counts, Gaussian length penalty, its
bigram-counting length included) with one difference that matters: the words are TOKEN IDS.  Nothing is detokenised and no PTB tokenizer
runs, so the numbers are CIDEr-D over BPE tokens — a training signal, not the published word-level metric.  DESIGN.md states it exactly.

``CiderReward.from_corpus`` counts the document frequencies of a corpus once, on the host, and puts idf = log N - log max(1, df) into an
open-addressing table on the device (clipcap_amd/csrc/cider_table.h); ``score`` / ``for_batch`` are one launch of cc_cider_score each and
read no value back.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, Optional, Sequence, Tuple

import numpy as np
import torch

from clipcap_amd import _lib, engine

TOKEN_LIMIT = engine.CIDER_TOKEN_LIMIT
_EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def ngram_keys(tokens: np.ndarray, caption_of: np.ndarray, n: int) -> Tuple[np.ndarray, np.ndarray]:
    """Keys of every n-gram of a flat token array whose captions are told apart by ``caption_of`` (same length, non-decreasing): (keys
    uint64, start positions).  Token k of an n-gram sits in bits [16k, 16k + 16), the unused slots hold 0xFFFF (cider_table.h)."""
    T = tokens.shape[0]
    if T < n:
        return np.empty(0, np.uint64), np.empty(0, np.int64)
    start = np.nonzero(caption_of[:T - n + 1] == caption_of[n - 1:])[0]
    key = np.full(start.shape[0], _EMPTY, dtype=np.uint64)
    for k in range(n):
        sh = np.uint64(16 * k)
        key = (key & ~(np.uint64(0xFFFF) << sh)) | (tokens[start + k].astype(np.uint64) << sh)
    return key, start


def corpus_idf(docs: Sequence[Sequence[Sequence[int]]]) -> Tuple[np.ndarray, np.ndarray, int]:
    """(keys uint64, idf fp32, N) of a corpus of N documents, each a list of token-id lists: df(g) = the number of documents with g in at
    least one caption, idf = log N - log max(1, df) in float64, rounded once to fp32.  Vectorised: keys per position, unique over
    (document, key), unique over key.  ValueError for a token outside [0, 65535)."""
    N = len(docs)
    if N < 1:
        raise ValueError("the corpus must hold at least one document")
    caps = [np.asarray(c, dtype=np.int64).reshape(-1) for d in docs for c in d]
    doc_of_cap = np.repeat(np.arange(N, dtype=np.int64), [len(d) for d in docs])
    lens = np.array([c.shape[0] for c in caps], dtype=np.int64)
    tokens = np.concatenate(caps) if caps else np.empty(0, np.int64)
    if tokens.size and (tokens.min() < 0 or tokens.max() >= TOKEN_LIMIT):
        raise ValueError(f"token ids must lie in [0, {TOKEN_LIMIT}) to be packed 16 bits each; got {int(tokens.min())}..{int(tokens.max())}")
    caption_of = np.repeat(np.arange(len(caps), dtype=np.int64), lens)
    keys, dfs = [], []
    for n in range(1, 5):
        key, start = ngram_keys(tokens, caption_of, n)
        doc = doc_of_cap[caption_of[start]]
        order = np.lexsort((key, doc))
        key, doc = key[order], doc[order]
        keep = np.ones(key.shape[0], dtype=bool)
        keep[1:] = (key[1:] != key[:-1]) | (doc[1:] != doc[:-1])                       # one (document, key) pair each
        u, df = np.unique(key[keep], return_counts=True)
        keys.append(u)
        dfs.append(df)
    keys, df = np.concatenate(keys), np.concatenate(dfs).astype(np.float64)
    idf = (math.log(N) - np.log(np.maximum(1.0, df))).astype(np.float32)
    return keys, idf, N


def build_table(keys: np.ndarray, idf: np.ndarray, cap: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(tab_keys uint64 (cap,), tab_idf fp32 (cap,)) in host memory through the library's cider_table_build — the lines the kernel probes
    with.  cap: a power of two >= 2 * len(keys) (default: the smallest, at least 2).  ValueError when the build is refused."""
    keys, idf = np.ascontiguousarray(keys, dtype=np.uint64), np.ascontiguousarray(idf, dtype=np.float32)
    n = keys.shape[0]
    if cap is None:
        cap = 2
        while cap < 2 * n:
            cap *= 2
    tk, ti = np.empty(cap, np.uint64), np.empty(cap, np.float32)
    rc = _lib.lib().cc_cider_table_build(C.c_void_p(keys.ctypes.data), C.c_void_p(idf.ctypes.data), n, C.c_void_p(tk.ctypes.data),
                                         C.c_void_p(ti.ctypes.data), cap)
    if rc != 0:
        raise ValueError(f"cider table refused: {n} keys into {cap} slots (a power of two of at least twice the keys; keys distinct, none all-ones)")
    return tk, ti


class CiderReward:
    """CIDEr-D over token ids against a corpus's idf values, on the device.  Build with ``from_corpus``."""

    def __init__(self, tab_keys: torch.Tensor, tab_idf: torch.Tensor, n_docs: int, *, sigma: float = 6.0, count_stop: bool = False,
                 stop_token: int = 50256):
        sigma = float(sigma)
        if not (sigma > 0.0 and math.isfinite(sigma)):
            raise ValueError(f"sigma must be positive and finite, got {sigma}")
        if not 0 <= int(stop_token) < TOKEN_LIMIT:
            raise ValueError(f"stop_token must lie in [0, {TOKEN_LIMIT}), got {stop_token}")
        self.tab_keys, self.tab_idf = tab_keys, tab_idf            # int64 (cap,): the keys' bit patterns; fp32 (cap,)
        self.n_docs, self.log_ndocs = int(n_docs), math.log(int(n_docs))
        self.sigma, self.count_stop, self.stop_token = sigma, bool(count_stop), int(stop_token)

    @classmethod
    def from_corpus(cls, docs, *, sigma: float = 6.0, count_stop: bool = False, stop_token: int = 50256, device="cuda") -> "CiderReward":
        """``docs``: a list of documents, each the list of token-id lists that are one image's reference captions.  With ``count_stop``
        the stop token counts as the last word of every caption: it is appended to every corpus caption here, to every reference in
        ``for_batch``, and kept on every candidate by the kernel.  Tokens outside [0, 65535) raise ValueError."""
        if count_stop:
            docs = [[list(c) + [int(stop_token)] for c in d] for d in docs]
        keys, idf, N = corpus_idf(docs)
        tk, ti = build_table(keys, idf)
        return cls(torch.from_numpy(tk.view(np.int64)).to(device), torch.from_numpy(ti).to(device), N, sigma=sigma, count_stop=count_stop,
                   stop_token=stop_token)

    def score(self, cand: torch.Tensor, refs: torch.Tensor, ref_count: Optional[torch.Tensor] = None,
              cand_group: Optional[torch.Tensor] = None) -> torch.Tensor:
        """fp32 (C,) scores on the device of ``cand`` int64 (C, n) against ``refs`` int32 (G, Rmax, Lr) — ``engine.cider_score`` with this
        reward's table and options.  The references are taken as they are (``for_batch`` appends the stop token under ``count_stop``)."""
        return engine.cider_score(cand, refs, self.tab_keys, self.tab_idf, self.log_ndocs, sigma=self.sigma, stop_token=self.stop_token,
                                  count_stop=self.count_stop, ref_count=ref_count, cand_group=cand_group)

    def with_stop(self, refs: torch.Tensor) -> torch.Tensor:
        """``refs`` (G, Rmax, Lr) -> (G, Rmax, Lr + 1) with the stop token written after the last word of every row (device ops only)."""
        G, Rmax, Lr = refs.shape
        ext = torch.cat((refs, torch.full((G, Rmax, 1), -1, dtype=refs.dtype, device=refs.device)), dim=2)
        ended = (ext < 0).to(torch.int32).cumsum(dim=2) > 0                                    # at and after the first negative id
        first = ended & ~torch.cat((torch.zeros_like(ended[..., :1]), ended[..., :-1]), dim=2)
        minus, stop = torch.full_like(ext, -1), torch.full_like(ext, self.stop_token)
        return torch.where(first, stop, torch.where(ended, minus, ext)).contiguous()

    def for_batch(self, refs: torch.Tensor, ref_count: Optional[torch.Tensor] = None) -> Callable:
        """The ``reward_fn`` of ``self_critical_step`` for a batch whose row b has the references ``refs[b]`` (int32 (B, Rmax, Lr), -1
        after each row's last word; ``ref_count`` int32 (B,) rows in use, None = all): ``(sampled, greedy) -> (r_sampled, r_greedy)``, two
        fp32 (B,) device tensors.  The two id tensors, of different widths, are padded with -1 into one (2B, n) buffer and scored in one
        launch, candidate c against image c % B.  No value is read back."""
        if refs.dim() != 3 or refs.dtype != torch.int32:
            raise ValueError(f"refs must be int32 (B, Rmax, Lr), got {refs.dtype} {tuple(refs.shape)}")
        refs = self.with_stop(refs) if self.count_stop else refs.contiguous()
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
