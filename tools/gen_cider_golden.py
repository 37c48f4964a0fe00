#!/usr/bin/env python
"""Records tests/golden/cider_ref.npz: random token-id cases scored by the reference project's CIDEr-D scorer.  CPU only; run once by
hand, no test runs it.

    python tools/gen_cider_golden.py PATH/TO/clipcap/eval/pycocoevalcap/cider/cider_scorer.py

The reference's scorer is loaded from that path at run time (nothing of it is copied here) and fed the space-joined decimal ids of every
caption.  A case is a small corpus of its own, as the reference scorer builds it: G images with 1..5 references and one candidate each;
N = G.  Recorded per case, as flat arrays with offsets (data only):
    tokens int16, cap_start int64 (captions + 1,)    every caption's words: caption k is tokens[cap_start[k]:cap_start[k + 1]]
    case_img int64 (cases + 1,)                      the images of a case: [case_img[c], case_img[c + 1])
    img_cap int64 (images + 1,)                      the captions of an image: the FIRST is the candidate, the others its references
    score float64 (images,)                          the reference scorer's score of each image's candidate
    df_key uint64, df_count int32, case_df int64 (cases + 1,)   the reference scorer's own document frequencies of a case, the
                                                     n-gram as a key: token k in bits [16k, 16k + 16), unused slots 0xFFFF
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "cider_ref.npz")
LENGTHS = [0, 1, 2, 3, 4, 5, 9, 17, 40]
LONG = [63, 64, 65]


def make_case(rng):
    G, V = int(rng.integers(2, 9)), int(rng.choice([6, 40]))
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
                if cand:
                    cand[int(rng.integers(0, len(cand)))] = int(rng.integers(0, V))
            if cand and rng.random() < 0.3:
                del cand[int(rng.integers(0, len(cand)))]
        images.append((cand, refs))
    return images


def main():
    spec = importlib.util.spec_from_file_location("reference_cider_scorer", sys.argv[1])
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rng = np.random.default_rng(20250131)
    text = lambda words: " ".join(str(t) for t in words)  # noqa: E731
    tokens, cap_start, case_img, img_cap, score, df_key, df_count, case_df = [], [0], [0], [0], [], [], [], [0]
    n_cases = 0
    while n_cases < 24:
        images = make_case(rng)
        if not any(r for _, refs in images for r in refs):
            continue                                                    # (the reference scorer cannot take a corpus without a word)
        scorer = mod.CiderScorer(n=4, sigma=6.0)
        for cand, refs in images:
            scorer += (text(cand), [text(r) for r in refs])
        _, per_image = scorer.compute_score()
        for (cand, refs), s in zip(images, per_image):
            for words in [cand] + refs:
                tokens += words
                cap_start.append(len(tokens))
            img_cap.append(len(cap_start) - 1)
            score.append(float(s))
        case_img.append(len(img_cap) - 1)
        for gram, cnt in sorted(scorer.document_frequency.items()):
            if cnt <= 0:
                continue                                                # (looked up by the scorer, never counted)
            key = 0xFFFFFFFFFFFFFFFF
            for k, w in enumerate(gram):
                key = (key & ~(0xFFFF << (16 * k))) | (int(w) << (16 * k))
            df_key.append(key)
            df_count.append(int(cnt))
        case_df.append(len(df_key))
        n_cases += 1
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, tokens=np.array(tokens, np.int16), cap_start=np.array(cap_start, np.int64), case_img=np.array(case_img, np.int64),
                        img_cap=np.array(img_cap, np.int64), score=np.array(score, np.float64), df_key=np.array(df_key, np.uint64),
                        df_count=np.array(df_count, np.int32), case_df=np.array(case_df, np.int64))
    print(f"wrote {OUT}: {n_cases} cases, {len(score)} candidates, {len(df_key)} document frequencies, {os.path.getsize(OUT)} bytes; "
          f"{sum(s == 0 for s in score)} scores are 0, max {max(score):.3f}")


if __name__ == "__main__":
    main()
