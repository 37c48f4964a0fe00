"""Inputs shared by the CIDEr-D tests: the recorded cases of tests/golden/cider_ref.npz (tools/gen_cider_golden.py) as Python lists, the
key packing of clipcap_amd/csrc/cider_table.h restated in Python, and the random recipe of the device tests."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cider_ref.npz")
MUL, MASK64 = 0x9E3779B97F4A7C15, (1 << 64) - 1


def pack(gram):
    key = MASK64
    for k, w in enumerate(gram):
        key = (key & ~(0xFFFF << (16 * k))) | (int(w) << (16 * k))
    return key


def unpack(key):
    out = []
    for k in range(4):
        w = (int(key) >> (16 * k)) & 0xFFFF
        if w == 0xFFFF:
            break
        out.append(w)
    return tuple(out)


def table_find(tab_keys, tab_idf, key, miss):
    """cider_table_find in Python, on the arrays the library built (tab_keys as uint64)"""
    cap = len(tab_keys)
    lg = cap.bit_length() - 1
    s = ((key * MUL) & MASK64) >> (64 - lg) if lg else 0
    for _ in range(cap):
        k = int(tab_keys[s])
        if k == key:
            return float(tab_idf[s])
        if k == MASK64:
            return miss
        s = (s + 1) & (cap - 1)
    return miss


@functools.lru_cache(maxsize=None)
def golden_cases():
    """[{images: [(candidate, [references])], score: [float], df: {ngram tuple: count}}] — N of a case = len(images)"""
    z = np.load(GOLDEN)
    tokens, cap_start, case_img, img_cap = z["tokens"].astype(np.int64), z["cap_start"], z["case_img"], z["img_cap"]
    cases = []
    for c in range(len(case_img) - 1):
        images, score = [], []
        for i in range(case_img[c], case_img[c + 1]):
            caps = [tokens[cap_start[k]:cap_start[k + 1]].tolist() for k in range(img_cap[i], img_cap[i + 1])]
            images.append((caps[0], caps[1:]))
            score.append(float(z["score"][i]))
        lo, hi = z["case_df"][c], z["case_df"][c + 1]
        df = {unpack(k): int(n) for k, n in zip(z["df_key"][lo:hi], z["df_count"][lo:hi])}
        cases.append(dict(images=images, score=score, df=df))
    return cases


REF_LENGTHS = [0, 1, 2, 3, 4, 5, 9, 17, 40, 63, 64, 65]


def shared_inputs(seed=0, G=8, vocab=40, per_image=4):
    """The device tests' inputs: G images with 1-5 references of lengths drawn from REF_LENGTHS over `vocab` tokens; per image
    `per_image` candidates, each the image's longest reference with 0-2 substitutions and sometimes one deletion.
    Returns (refs: [[caption]] per image, cands: [(image, caption)])."""
    rng = np.random.default_rng(seed)
    refs, cands = [], []
    for g in range(G):
        rows = [[int(t) for t in rng.integers(0, vocab, int(rng.choice(REF_LENGTHS)))] for _ in range(int(rng.integers(1, 6)))]
        refs.append(rows)
        for _ in range(per_image):
            c = list(max(rows, key=len))
            for _ in range(int(rng.integers(0, 3))):
                if c:
                    c[int(rng.integers(0, len(c)))] = int(rng.integers(0, vocab))
            if c and rng.random() < 0.3:
                del c[int(rng.integers(0, len(c)))]
            cands.append((g, c))
    return refs, cands


def pad_rows(rows, width, fill=-1, dtype=np.int64):
    out = np.full((len(rows), width), fill, dtype=dtype)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def pad_refs(refs, Rmax, Lr, fill=-1):
    """(G, Rmax, Lr) int32 and ref_count (G,) int32"""
    out = np.full((len(refs), Rmax, Lr), fill, dtype=np.int32)
    for g, rows in enumerate(refs):
        for r, row in enumerate(rows):
            out[g, r, :len(row)] = row
    return out, np.array([len(rows) for rows in refs], dtype=np.int32)
