"""Decode a set of images and score the captions (``evaluate_model``), and the command line over two CSV files (``run_eval``)."""
from __future__ import annotations

import json
import sys
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import torch

from clipcap_amd.eval import metrics as M
from clipcap_amd.inference.base import best_beams, generate_beam


def _tokens_decoder(decoder: Callable) -> Callable:
    """The ``*_tokens`` form of a decoder: itself if it is one, else the function of that name in the decoder's own module."""
    if decoder.__name__.endswith("_tokens"):
        return decoder
    fn = getattr(sys.modules[decoder.__module__], decoder.__name__ + "_tokens", None)
    if fn is None:
        raise ValueError(f"level=\"token\" needs a decoder that returns ids: {decoder.__module__} has no {decoder.__name__}_tokens")
    return fn


def _best_ids(result, stop_token: int) -> List[List[int]]:
    """One id list per image from what a ``*_tokens`` decoder returned: a tensor or a tuple whose first entry is the ids, (S, n) or
    (S, beam, n) with the scores and lengths as second and third entry (then the best beam, cut at its length).  A row runs to its first
    stop token."""
    tokens = result[0] if isinstance(result, (tuple, list)) else getattr(result, "tokens", result)
    rows = []
    if tokens.dim() == 3:
        best = best_beams(result[1], 1)[:, 0].cpu().tolist()
        lengths = result[2].cpu().tolist()
        host = tokens.cpu().tolist()
        rows = [host[s][b][:int(lengths[s][b])] for s, b in enumerate(best)]
    else:
        rows = tokens.cpu().tolist()
    out = []
    for row in rows:
        ids = []
        for t in row:
            if t < 0 or t == stop_token:
                break
            ids.append(int(t))
        out.append(ids)
    return out


def evaluate_model(model, tokenizer, embeds: torch.Tensor, references: Sequence[Sequence[str]], *, batch_size: int = 64, level: str = "word",
                   decoder: Callable = generate_beam, metrics: Sequence[str] = M.METRIC_NAMES, tokenize: Callable = M.normalise,
                   **decoder_kw) -> Tuple[Dict[str, float], Dict[int, Dict[str, float]]]:
    """Decodes ``embeds`` (S, L, D) — the prefixes the decoders of clipcap_amd.inference take — ``batch_size`` rows at a time with
    ``decoder(model, tokenizer, rows, **decoder_kw)`` and scores the captions against ``references[i]`` (1..Rmax strings per image):
    what ``metrics.evaluate_metrics_from_lists`` returns.

    ``level="word"``: the decoder's strings and the reference strings are tokenised by ``tokenize`` (``metrics.normalise``).
    ``level="token"``: no string round trip — the decoder's ``*_tokens`` form is called as ``(model, rows, **decoder_kw)``, and its ids
    are scored against ``tokenizer.encode(reference)``: BLEU / ROUGE-L / CIDEr over BPE tokens, the quantities ``MetricReward`` trains
    on, not the published word-level metrics."""
    if level not in ("word", "token"):
        raise ValueError(f"level must be \"word\" or \"token\", got {level!r}")
    if embeds.shape[0] != len(references):
        raise ValueError(f"{embeds.shape[0]} rows of embeddings for {len(references)} lists of references")
    S = embeds.shape[0]
    if level == "word":
        captions: List[str] = []
        for lo in range(0, S, batch_size):
            captions += list(decoder(model, tokenizer, embeds[lo:lo + batch_size], **decoder_kw))
        if len(captions) != S:
            raise ValueError(f"the decoder returned {len(captions)} captions for {S} images: evaluate one caption per image")
        return M.evaluate_metrics_from_lists(captions, [list(r) for r in references], tokenize=tokenize, metrics=metrics, device=embeds.device)
    fn = _tokens_decoder(decoder)
    stop = tokenizer.encode(tokenizer.eos_token)[0] if getattr(tokenizer, "eos_token", None) else 50256
    ids: List[List[int]] = []
    for lo in range(0, S, batch_size):
        ids += _best_ids(fn(model, embeds[lo:lo + batch_size], **decoder_kw), stop)
    total, per = M.score_ids(ids, [[list(tokenizer.encode(r)) for r in refs] for refs in references], metrics, embeds.device)
    return total, dict(enumerate(per))


def run_eval(argv: Optional[List[str]] = None) -> int:
    """python -m clipcap_amd.eval --predictions P.csv --references R.csv [--nb-reference-captions 5] [--save-file out.json]"""
    parser = ArgumentParser(prog="python -m clipcap_amd.eval", formatter_class=ArgumentDefaultsHelpFormatter,
                            description="BLEU-1..4, ROUGE-L and CIDEr of predicted captions against reference captions, on the device.")
    parser.add_argument("--predictions", required=True, help="csv with the columns file_name and caption_predicted")
    parser.add_argument("--references", required=True, help="csv with the columns file_name and caption_reference_01 .. _NN")
    parser.add_argument("--nb-reference-captions", type=int, default=5, help="reference columns to read")
    parser.add_argument("--save-file", type=str, default=None, help="json file to write all scores to (optional)")
    parser.add_argument("--device", type=str, default="cuda", help="where the metrics run")
    args = parser.parse_args(argv)
    result: Dict[str, Any] = M.evaluate_metrics(args.predictions, args.references, args.nb_reference_captions, device=args.device)
    for name, entry in result.items():
        print(f"{name:8s} {entry['score']:.6f}")
    if args.save_file:
        with open(args.save_file, "w") as f:
            json.dump(result, f)
    return 0
