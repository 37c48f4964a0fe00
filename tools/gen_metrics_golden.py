#!/usr/bin/env python
"""Records tests/golden/bleu_rouge_ref.npz: random word-id cases scored by the reference project's BLEU, ROUGE-L and CIDEr-D scorers.
CPU only; run once by hand, no test runs it.

    python tools/gen_metrics_golden.py PATH/TO/bleu_scorer.py PATH/TO/rouge.py PATH/TO/cider_scorer.py

(the three files of the reference's clipcap/eval/pycocoevalcap/{bleu,rouge,cider}/).  The scorers are loaded from those paths at run time
(nothing of them is copied here) and fed the space-joined decimal ids of every caption.  A case is a small corpus of its own: G images
with 1..5 references and one candidate each, by the recipe of tools/gen_cider_golden.py with three changes: NO caption is empty (the
reference's ROUGE-L splits "" into [""], so an empty caption would have to be left out of that comparison), the lengths are 1, 2, 3, 4,
5, 9, 17, 40, 63, 64, 65, and the vocabulary has 2, 6 or 40 words (8 cases each).  Recorded, as flat arrays with offsets (data only):
    tokens int16, cap_start int64 (captions + 1,)    every caption's words: caption k is tokens[cap_start[k]:cap_start[k + 1]]
    case_img int64 (cases + 1,)                      the images of a case: [case_img[c], case_img[c + 1])
    img_cap int64 (images + 1,)                      the captions of an image: the FIRST is the candidate, the others its references
    counts int64 (images, 10)                        BleuScorer's testlen, closest reflen, guess[1..4], correct[1..4]
    bleu float64 (images, 4), rouge float64 (images,)   the sentence BLEUs (option "closest") and Rouge.calc_score
    case_bleu float64 (cases, 4), case_rouge, case_cider float64 (cases,)   the corpus BLEUs, the mean ROUGE-L, the mean CIDEr-D
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "bleu_rouge_ref.npz")
LENGTHS = [1, 2, 3, 4, 5, 9, 17, 40]
LONG = [63, 64, 65]
VOCABS = [2, 6, 40]
CASES_PER_VOCAB = 8


def make_case(rng, V):
    """tools/gen_cider_golden.py's make_case with the vocabulary given and no empty caption"""
    G = int(rng.integers(2, 9))
    images = []
    for _ in range(G):
        refs = []
        for _ in range(int(rng.integers(1, 6))):
            L = int(rng.choice(LONG if rng.random() < 0.06 else LENGTHS))
            refs.append([int(t) for t in rng.integers(0, V, L)])
        kind = rng.random()
        if kind < 0.15:                                                 # an unrelated candidate, repeated tokens likely
            cand = [int(t) for t in rng.integers(0, max(2, V // 8), int(rng.choice(LENGTHS)))]
        else:                                                           # the longest reference with 0-2 substitutions, sometimes a deletion
            cand = list(max(refs, key=len))
            for _ in range(int(rng.integers(0, 3))):
                cand[int(rng.integers(0, len(cand)))] = int(rng.integers(0, V))
            if len(cand) > 1 and rng.random() < 0.3:
                del cand[int(rng.integers(0, len(cand)))]
        images.append((cand, refs))
    return images


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    bleu_mod, rouge_mod, cider_mod = (load(p, n) for p, n in zip(sys.argv[1:4], ("reference_bleu_scorer", "reference_rouge", "reference_cider_scorer")))
    rng = np.random.default_rng(20250207)
    text = lambda words: " ".join(str(t) for t in words)  # noqa: E731
    tokens, cap_start, case_img, img_cap = [], [0], [0], [0]
    counts, bleu, rouge, case_bleu, case_rouge, case_cider = [], [], [], [], [], []
    for V in VOCABS:
        for _ in range(CASES_PER_VOCAB):
            images = make_case(rng, V)
            bs, cs, rg = bleu_mod.BleuScorer(n=4), cider_mod.CiderScorer(n=4, sigma=6.0), rouge_mod.Rouge()
            per_rouge = []
            for cand, refs in images:
                bs += (text(cand), [text(r) for r in refs])
                cs += (text(cand), [text(r) for r in refs])
                per_rouge.append(float(rg.calc_score([text(cand)], [text(r) for r in refs])))
            corpus, per_bleu = bs.compute_score(option="closest", verbose=0)
            cider_mean, _ = cs.compute_score()
            for i, (cand, refs) in enumerate(images):
                for words in [cand] + refs:
                    tokens += words
                    cap_start.append(len(tokens))
                img_cap.append(len(cap_start) - 1)
                comps = bs.ctest[i]
                closest = bs._single_reflen(comps["reflen"], "closest", comps["testlen"])
                counts.append([comps["testlen"], closest] + list(comps["guess"]) + list(comps["correct"]))
                bleu.append([float(per_bleu[n][i]) for n in range(4)])
            rouge += per_rouge
            case_img.append(len(img_cap) - 1)
            case_bleu.append([float(b) for b in corpus])
            case_rouge.append(float(np.mean(np.array(per_rouge))))
            case_cider.append(float(cider_mean))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, tokens=np.array(tokens, np.int16), cap_start=np.array(cap_start, np.int64), case_img=np.array(case_img, np.int64),
                        img_cap=np.array(img_cap, np.int64), counts=np.array(counts, np.int64), bleu=np.array(bleu, np.float64),
                        rouge=np.array(rouge, np.float64), case_bleu=np.array(case_bleu, np.float64),
                        case_rouge=np.array(case_rouge, np.float64), case_cider=np.array(case_cider, np.float64))
    print(f"wrote {OUT}: {len(case_rouge)} cases, {len(rouge)} candidates, {os.path.getsize(OUT)} bytes; "
          f"{sum(r == 0 for r in rouge)} ROUGE-L scores and {sum(b[3] < 1e-6 for b in bleu)} BLEU-4 scores are (near) 0")


if __name__ == "__main__":
    main()
