"""Inputs shared by the BLEU / ROUGE-L tests: the recorded cases of tests/golden/bleu_rouge_ref.npz (tools/gen_metrics_golden.py) as
Python lists, and the Python reference statement wrapped as stand-ins for the two launches."""
import functools
import os

import numpy as np
import torch

from tests import bleu_rouge_ref as ref
from tests import cider_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bleu_rouge_ref.npz")


@functools.lru_cache(maxsize=None)
def golden_cases():
    """[{images: [(candidate, [references])], counts: [[10 ints]], bleu: [[4]], rouge: [..], case_bleu: [4], case_rouge, case_cider}]"""
    z = np.load(GOLDEN)
    tokens, cap_start, case_img, img_cap = z["tokens"].astype(np.int64), z["cap_start"], z["case_img"], z["img_cap"]
    cases = []
    for c in range(len(case_img) - 1):
        lo, hi = int(case_img[c]), int(case_img[c + 1])
        images = []
        for i in range(lo, hi):
            caps = [tokens[cap_start[k]:cap_start[k + 1]].tolist() for k in range(img_cap[i], img_cap[i + 1])]
            images.append((caps[0], caps[1:]))
        cases.append(dict(images=images, counts=z["counts"][lo:hi].tolist(), bleu=z["bleu"][lo:hi].tolist(), rouge=z["rouge"][lo:hi].tolist(),
                          case_bleu=z["case_bleu"][c].tolist(), case_rouge=float(z["case_rouge"][c]), case_cider=float(z["case_cider"][c])))
    return cases


def lcs_fast(a, b):
    """bleu_rouge_ref.lcs with the DP's row taken at once: cur[j] = max(prev[j], prev[j - 1] + (a_i == b_j), cur[j - 1]), the last term as
    a running maximum (a row of the table never decreases).  tests/test_metrics_ref.py holds it to the plain DP."""
    b = np.asarray(b, dtype=np.int64)
    prev = np.zeros(len(b) + 1, dtype=np.int64)
    for x in a:
        cur = np.maximum(prev[1:], prev[:-1] + (b == x))
        prev = np.concatenate(([0], np.maximum.accumulate(cur)))
    return int(prev[-1])


def _rows(cand, refs, stop_token, count_stop, ref_count, cand_group):
    """(candidate words, reference word lists) per candidate row, cut as the kernels cut them"""
    G, Rmax, _ = refs.shape
    cand, refs = cand.cpu().tolist(), refs.cpu().tolist()
    out = []
    for c, row in enumerate(cand):
        g = c % G if cand_group is None else int(cand_group[c])
        if not 0 <= g < G:
            out.append(None)
            continue
        R = Rmax if ref_count is None else min(max(int(ref_count[g]), 1), Rmax)
        out.append((cider_ref.cut(row, stop_token if stop_token >= 0 else None, bool(count_stop)), [cider_ref.cut(r) for r in refs[g][:R]]))
    return out


def bleu_stats_stand_in(cand, refs, *, stop_token=50256, count_stop=False, ref_count=None, cand_group=None):
    """engine.bleu_stats computed by the reference statement, on the tensors' own device"""
    stats, bleu = [], []
    for item in _rows(cand, refs, stop_token, count_stop, ref_count, cand_group):
        counts = [0] * 10 if item is None else ref.bleu_counts(*item)
        stats.append(counts)
        bleu.append([0.0] * 4 if item is None else ref.bleu_from_counts(counts))
    return (torch.tensor(stats, dtype=torch.int32, device=cand.device).reshape(-1, 10),
            torch.tensor(bleu, dtype=torch.float64).to(torch.float32).to(cand.device).reshape(-1, 4))


def rouge_l_stand_in(cand, refs, *, stop_token=50256, count_stop=False, ref_count=None, cand_group=None, beta=ref.BETA):
    """engine.rouge_l computed by the reference statement"""
    Rmax = refs.shape[1]
    score, lcs = [], []
    for item in _rows(cand, refs, stop_token, count_stop, ref_count, cand_group):
        if item is None:
            score.append(0.0)
            lcs.append([-1] * Rmax)
            continue
        score.append(ref.rouge_l(*item, beta=beta))
        lcs.append([ref.lcs(item[0], r) for r in item[1]] + [-1] * (Rmax - len(item[1])))
    return (torch.tensor(score, dtype=torch.float64).to(torch.float32).to(cand.device),
            torch.tensor(lcs, dtype=torch.int32, device=cand.device).reshape(-1, Rmax))


def cider_score_stand_in(cand, refs, tab_keys, tab_idf, log_ndocs, *, sigma=6.0, stop_token=50256, count_stop=False, ref_count=None,
                         cand_group=None, out=None):
    """engine.cider_score computed by tests/cider_ref.py with the table's own fp32 idf values"""
    from tests.cider_cases import pack, table_find
    tk, ti = tab_keys.cpu().numpy().view(np.uint64), tab_idf.cpu().numpy()
    miss = float(np.float32(log_ndocs))
    idf = lambda g: miss if any(t >= 65535 for t in g) else table_find(tk, ti, pack(g), miss)  # noqa: E731
    score = [0.0 if item is None else cider_ref.cider_d(item[0], item[1], idf, sigma)
             for item in _rows(cand, refs, stop_token, count_stop, ref_count, cand_group)]
    return torch.tensor(score, dtype=torch.float64).to(torch.float32).to(cand.device)
