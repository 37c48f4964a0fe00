"""BLEU-1..4 and ROUGE-L over word ids in float64, with dicts and a plain DP: the statement cc_bleu_stats, cc_rouge_l and
clipcap_amd.eval are held to (include/clipcap_hip.h).

A caption is a list of non-negative integers.  For a candidate c of L words and its references r, n = 1..4:

    guess[n]   = max(0, L - n + 1)
    correct[n] = sum over the distinct n-grams g of c of min(tf_c(g), max_r tf_r(g))
    reflen     = the l among the reference lengths with the smallest (|l - L|, l)
    p = 1;  for n = 1..4:  p *= (correct[n] + 1e-15) / (guess[n] + 1e-9);  bleu_n = p ** (1 / n)
    ratio = (L + 1e-15) / (reflen + 1e-9);  if ratio < 1:  bleu_n *= exp(1 - 1 / ratio)
    corpus: the last two lines on the sums of L, reflen, guess[n], correct[n] over all candidates

    P = max_r lcs(c, r) / L_c,  R = max_r lcs(c, r) / L_r;  rouge_l = (1 + beta^2) P R / (R + beta^2 P), 0 if P = 0 or R = 0
    an empty candidate scores 0; an empty reference adds 0 to both maxima
"""
import math
from collections import Counter

TINY, SMALL, BETA = 1e-15, 1e-9, 1.2


def ngrams(words, n):
    return Counter(tuple(words[i:i + n]) for i in range(len(words) - n + 1))


def bleu_counts(cand, refs):
    """[L, reflen, guess[1..4], correct[1..4]]: ten integers"""
    cand, L = list(cand), len(cand)
    reflen = min((abs(len(r) - L), len(r)) for r in refs)[1]
    guess, correct = [], []
    for n in range(1, 5):
        most = {}
        for r in refs:
            for g, tf in ngrams(list(r), n).items():
                most[g] = max(most.get(g, 0), tf)
        guess.append(max(0, L - n + 1))
        correct.append(sum(min(tf, most.get(g, 0)) for g, tf in ngrams(cand, n).items()))
    return [L, reflen] + guess + correct


def bleu_from_counts(counts):
    """[bleu_1 .. bleu_4] from ten numbers — a sentence's counts, or a corpus's sums"""
    L, reflen, guess, correct = counts[0], counts[1], counts[2:6], counts[6:10]
    out, p = [], 1.0
    for n in range(4):
        p *= (float(correct[n]) + TINY) / (float(guess[n]) + SMALL)
        out.append(p ** (1.0 / (n + 1)))
    ratio = (L + TINY) / (reflen + SMALL)
    if ratio < 1:
        out = [b * math.exp(1 - 1 / ratio) for b in out]
    return out


def bleu_corpus(all_counts):
    return bleu_from_counts([sum(col) for col in zip(*all_counts)])


def lcs(a, b):
    """length of the longest common subsequence: the plain DP, one row at a time"""
    prev = [0] * (len(b) + 1)
    for x in a:
        cur = [0]
        for j, y in enumerate(b):
            cur.append(prev[j] + 1 if x == y else max(prev[j + 1], cur[j]))
        prev = cur
    return prev[len(b)]


def rouge_l(cand, refs, beta=BETA):
    cand = list(cand)
    if not cand:
        return 0.0
    prec, rec = 0.0, 0.0
    for r in refs:
        if len(r) == 0:
            continue
        l = lcs(cand, list(r))
        prec, rec = max(prec, l / float(len(cand))), max(rec, l / float(len(r)))
    if prec != 0 and rec != 0:
        return ((1 + beta ** 2) * prec * rec) / float(rec + beta ** 2 * prec)
    return 0.0
