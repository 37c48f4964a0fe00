"""CIDEr-D over token ids in float64, with dicts: the statement cc_cider_score and clipcap_amd.train.cider are held to.

A caption is a list of token ids; its n-grams (n = 1..4) are the tuples w[i:i+n].  The idf is a FUNCTION of the n-gram tuple, so the same
code serves the check against the recorded reference scorer (idf from the case's own document frequencies, float64) and the check of the
device kernel (idf = the device table's fp32 values).

    v_x,n(g) = tf_x(g) idf(g);  norm_x,n = sqrt(sum_g v_x,n(g)^2)
    val_n(c, r) = sum_{g in c} min(v_c,n(g), v_r,n(g)) v_r,n(g), divided by norm_c,n norm_r,n only if both are non-zero
    score(c) = 10 / (4 R) sum_r exp(-(len(c) - len(r))^2 / (2 sigma^2)) sum_n val_n(c, r),  len(x) = max(L_x - 1, 0)
"""
import math
from collections import Counter


def ngrams(words, n):
    return Counter(tuple(words[i:i + n]) for i in range(len(words) - n + 1))


def vectors(words, idf):
    """([{ngram: tf * idf}] for n = 1..4, [norm_n], length) of one caption"""
    vec = [{g: tf * idf(g) for g, tf in ngrams(words, n).items()} for n in range(1, 5)]
    return vec, [math.sqrt(sum(v * v for v in d.values())) for d in vec], max(len(words) - 1, 0)


def cider_d(cand, refs, idf, sigma=6.0):
    """score of one candidate against the references of its image"""
    vc, nc, lc = vectors(list(cand), idf)
    total = 0.0
    for ref in refs:
        vr, nr, lr = vectors(list(ref), idf)
        s = 0.0
        for n in range(4):
            val = sum(min(v, vr[n].get(g, 0.0)) * vr[n].get(g, 0.0) for g, v in vc[n].items())
            if nc[n] != 0.0 and nr[n] != 0.0:
                val /= nc[n] * nr[n]
            s += val
        total += math.exp(-float(lc - lr) ** 2 / (2.0 * sigma * sigma)) * s
    return 10.0 * total / (4.0 * len(refs))


def doc_freq(docs):
    """{ngram: number of documents (lists of captions) with it in at least one caption}"""
    df = Counter()
    for doc in docs:
        df.update({g for cap in doc for n in range(1, 5) for g in ngrams(list(cap), n)})
    return df


def idf_from_df(df, n_docs):
    """idf(g) = log N - log max(1, df(g)); an n-gram the corpus does not hold gets log N"""
    ln = math.log(float(n_docs))
    return lambda g: ln - math.log(max(1.0, float(df.get(g, 0))))


def cut(ids, stop_token=None, count_stop=False):
    """the words of a candidate row: to the first stop token (kept with count_stop), else the first negative id, else the end"""
    out = []
    for t in ids:
        t = int(t)
        if t < 0:
            break
        if stop_token is not None and t == stop_token:
            if count_stop:
                out.append(t)
            break
        out.append(t)
    return out
