"""Caption metrics on the device behind the Python surface of the reference's ``clipcap.eval.metrics``: BLEU-1..4, ROUGE-L and CIDEr(-D)
without the Java jars.  ``evaluate_metrics_from_lists`` and ``evaluate_metrics`` keep the reference's names and return shapes.

Not here, because the reference runs them in Java: METEOR, SPICE (and SPIDEr, which needs SPICE) and the PTB tokenizer.  The captions
are tokenised by ``normalise`` unless the caller passes a tokeniser of their own, so a score equals the reference's only when both sides
are given the same pre-tokenised strings.

Words become integers through a ``WordVocab`` built from the captions of the call; the three kernels compare integers (cc_bleu_stats,
cc_rouge_l, cc_cider_score: include/clipcap_hip.h states the metrics).  CIDEr's idf comes from the given references, as the reference's
``Cider`` takes it.
"""
from __future__ import annotations

import csv
import string
from collections import Counter
from pathlib import Path
from typing import Any, Callable, Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from clipcap_amd import engine

_PUNCT_TO_SPACE = str.maketrans({c: " " for c in string.punctuation})
METRIC_NAMES = ("Bleu", "ROUGE_L", "CIDEr")


def normalise(text: str) -> List[str]:
    """The words of a caption: lowercase, every punctuation character (``string.punctuation``) becomes a space, split on whitespace.

    This is NOT the PTB tokenizer the reference runs (a Java jar): it does not split contractions or keep hyphenated words the PTB
    way.  Scores equal the reference's only when both are given the same pre-tokenised strings (then pass ``tokenize=str.split``)."""
    return text.lower().translate(_PUNCT_TO_SPACE).split()


class WordVocab:
    """word -> id, ids assigned by DESCENDING frequency (ties: the word's own order), so that the ids CIDEr's 16-bit packing cannot hold
    (>= 65535) are the rarest words.  BLEU and ROUGE-L take any id."""

    def __init__(self, words_by_rank: Sequence[str]):
        self.words = list(words_by_rank)
        self.ids = {w: i for i, w in enumerate(self.words)}

    @classmethod
    def from_captions(cls, captions: Iterable[Sequence[str]]) -> "WordVocab":
        count = Counter(w for cap in captions for w in cap)
        return cls([w for w, _ in sorted(count.items(), key=lambda kv: (-kv[1], kv[0]))])

    def __len__(self) -> int:
        return len(self.words)

    def encode(self, words: Sequence[str]) -> List[int]:
        return [self.ids[w] for w in words]

    def require_cider(self) -> None:
        if len(self.words) > engine.CIDER_TOKEN_LIMIT:
            raise ValueError(f"CIDEr packs a word into 16 bits: at most {engine.CIDER_TOKEN_LIMIT} distinct words, the captions hold "
                             f"{len(self.words)}.  Leave \"CIDEr\" out of `metrics` (BLEU and ROUGE-L have no such limit) or score in parts.")


def _pad(cands: Sequence[Sequence[int]], refs: Sequence[Sequence[Sequence[int]]], device):
    n = max(1, max((len(c) for c in cands), default=1))
    Rmax = max(len(r) for r in refs)
    Lr = max(1, max(len(x) for r in refs for x in r))
    if n > engine.CIDER_MAX_LEN or Lr > engine.CIDER_MAX_LEN or Rmax * Lr > engine.CIDER_MAX_REF_TOKENS:
        raise ValueError(f"a caption may hold at most {engine.CIDER_MAX_LEN} words and an image's references at most "
                         f"{engine.CIDER_MAX_REF_TOKENS} padded positions; got {n}-word candidates, {Rmax} references of up to {Lr} words")
    cand = np.full((len(cands), n), -1, np.int64)
    for i, c in enumerate(cands):
        cand[i, :len(c)] = c
    arr = np.full((len(refs), Rmax, Lr), -1, np.int32)
    for g, rows in enumerate(refs):
        for r, row in enumerate(rows):
            arr[g, r, :len(row)] = row
    count = np.array([len(r) for r in refs], np.int32)
    return torch.from_numpy(cand).to(device), torch.from_numpy(arr).to(device), torch.from_numpy(count).to(device)


def score_ids(cands: Sequence[Sequence[int]], refs: Sequence[Sequence[Sequence[int]]], metrics: Sequence[str] = METRIC_NAMES,
              device="cuda") -> Tuple[Dict[str, float], List[Dict[str, float]]]:
    """Candidate i (a list of word ids >= 0) against ``refs[i]`` (1..Rmax lists of word ids): ({metric: corpus score}, [{metric: score
    of candidate i}]).  "Bleu" gives Bleu_1..Bleu_4 (corpus: from the summed counts; per candidate: the sentence scores), "ROUGE_L" and
    "CIDEr" the mean and the per-candidate scores.  One launch per metric; the ids have no stop token."""
    unknown = sorted(set(metrics) - set(METRIC_NAMES))
    if unknown:
        raise ValueError(f"unknown metrics {unknown}: choose from {list(METRIC_NAMES)}")
    if len(cands) != len(refs) or not cands:
        raise ValueError(f"one list of references per candidate, at least one; got {len(cands)} candidates and {len(refs)} lists")
    if any(len(r) < 1 for r in refs):
        raise ValueError("every candidate needs at least one reference")
    cand, arr, count = _pad(cands, refs, device)
    total: Dict[str, float] = {}
    per = [dict() for _ in cands]
    kw = dict(stop_token=-1, count_stop=False, ref_count=count)

    def put(name, corpus, values):
        total[name] = float(corpus)
        for d, v in zip(per, values):
            d[name] = float(v)

    if "Bleu" in metrics:
        stats, bleu = engine.bleu_stats(cand, arr, **kw)
        corpus, bleu = engine.bleu_corpus(stats), bleu.double().cpu()
        for n in range(4):
            put(f"Bleu_{n + 1}", corpus[n], bleu[:, n].tolist())
    if "ROUGE_L" in metrics:
        score = engine.rouge_l(cand, arr, **kw)[0].double()
        put("ROUGE_L", score.mean(), score.cpu().tolist())
    if "CIDEr" in metrics:
        from clipcap_amd.train.cider import CiderReward
        rw = CiderReward.from_corpus([list(map(list, r)) for r in refs], device=device)
        score = engine.cider_score(cand, arr, rw.tab_keys, rw.tab_idf, rw.log_ndocs, sigma=rw.sigma, **kw).double()
        put("CIDEr", score.mean(), score.cpu().tolist())
    return total, per


def evaluate_metrics_from_lists(predictions: List[str], ground_truths: List[List[str]], ids: Optional[List[Any]] = None, *,
                                tokenize: Callable[[str], List[str]] = normalise, metrics: Sequence[str] = METRIC_NAMES,
                                device="cuda") -> Tuple[Dict[str, float], Dict[Any, Dict[str, float]]]:
    """The reference's ``clipcap.eval.metrics.evaluate_metrics_from_lists`` for the metrics that need no Java: returns
    ({"Bleu_1": .., "Bleu_2": .., "Bleu_3": .., "Bleu_4": .., "ROUGE_L": .., "CIDEr": ..}, {id: {the same keys, for that file}}).
    ``predictions[i]`` is a caption (or a list whose first entry is taken, as in the reference), ``ground_truths[i]`` its 1..Rmax
    reference captions — ragged counts are allowed (the reference asserts exactly 5).  ``ids`` default to 0, 1, ...  ``tokenize`` turns a
    caption into words (``normalise``: not the PTB tokenizer, see there)."""
    if len(predictions) != len(ground_truths):
        raise ValueError(f"{len(predictions)} predictions for {len(ground_truths)} lists of references")
    ids = list(range(len(predictions))) if ids is None else list(ids)
    if len(ids) != len(predictions):
        raise ValueError(f"{len(ids)} ids for {len(predictions)} predictions")
    cand_words = [tokenize(p[0] if isinstance(p, (list, tuple)) else p) for p in predictions]
    ref_words = [[tokenize(r) for r in gt] for gt in ground_truths]
    vocab = WordVocab.from_captions(cand_words + [r for gt in ref_words for r in gt])
    if "CIDEr" in metrics:
        vocab.require_cider()
    total, per = score_ids([vocab.encode(c) for c in cand_words], [[vocab.encode(r) for r in gt] for gt in ref_words], metrics, device)
    return total, dict(zip(ids, per))


def check_and_read_csv(path: Union[str, Path, List[Dict[str, str]]]) -> List[Dict[str, str]]:
    """The rows of a CSV file as dicts (csv.DictReader), or the list itself if rows are given."""
    if isinstance(path, list):
        return path
    with Path(path).open("r", newline="") as f:
        return [row for row in csv.DictReader(f)]


def evaluate_metrics(prediction_file: Union[str, Path, List[Dict[str, str]]], reference_file: Union[str, Path, List[Dict[str, str]]],
                     nb_reference_captions: int = 5, **kw) -> Dict[str, Dict[str, Any]]:
    """The reference's ``clipcap.eval.metrics.evaluate_metrics``: ``prediction_file`` has the columns ``file_name`` and
    ``caption_predicted``, ``reference_file`` ``file_name`` and ``caption_reference_01`` .. ``caption_reference_NN`` (files, or their
    rows).  A reference column that a row leaves empty or does not have is skipped (at least one must remain).  Returns
    {metric.lower(): {"score": corpus score, "scores": {file_name: score}}}.  ``**kw`` goes to ``evaluate_metrics_from_lists``."""
    predictions = sorted(check_and_read_csv(prediction_file), key=lambda row: row["file_name"])
    reference = {row["file_name"]: row for row in check_and_read_csv(reference_file)}
    names = [row["file_name"] for row in predictions]
    missing = [n for n in names if n not in reference]
    if missing:
        raise ValueError(f"{len(missing)} predicted files have no row in the reference file, the first: {missing[0]!r}")
    columns = [f"caption_reference_{i:02d}" for i in range(1, nb_reference_captions + 1)]
    truths = [[reference[n][c] for c in columns if reference[n].get(c)] for n in names]
    total, per = evaluate_metrics_from_lists([row["caption_predicted"] for row in predictions], truths, **kw)
    return {m.lower(): {"score": s, "scores": {n: per[i][m] for i, n in enumerate(names)}} for m, s in total.items()}
