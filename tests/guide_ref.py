"""Float64 statement of classifier-free guidance on one step's logits (cc_logits_guide, include/clipcap_hip.h), the per-element bar a
device result is held to, an fp32 emulation of the kernel's rule with named defects the bar must reject, and a guided beam search for
one prefix on the CPU (the oracle's full re-forward of both streams) for the end-to-end tests.  tests/test_guide_ref.py pins all of it on
the CPU; tests/test_gpu_guide.py and tests/test_gpu_guide_decode.py compare the device with it.

The rule, per row over its V real columns:   out_i = g (c_i - lse_c) + (1 - g) (u_i - lse_u)
  * c_i or u_i = -inf  ->  out_i = -inf (a token banned in either stream stays banned; no inf - inf is formed);
  * a row whose cond or uncond is entirely -inf  ->  -inf everywhere (every element falls under the rule above).
The bar, per finite element:
    bound_i = (|g| + |1-g|) LOGP_TOL + 4 * 2^-24 (|g| (|c_i| + |lse_c|) + |1-g| (|u_i| + |lse_u|))
LOGP_TOL is what tests/test_gpu_contrastive.py already holds a device log-softmax to (each stream's log-softmax enters with weight |g| and
|1-g|); the second term is the fp32 roundings of the two subtractions, the two products and the sum on operands of those magnitudes."""
import numpy as np
import torch

LOGP_TOL = 4 * 2.626e-6
NEG = -np.inf

ROW_KINDS = ("gauss3", "gauss5", "grid", "far", "equal", "ban_cond", "ban_uncond", "ban_same", "ban_diff", "one_left_cond", "one_left_uncond",
             "dead_cond", "dead_uncond", "dead_both", "gauss3_b", "far_b")


def lse64(x):
    """log-sum-exp over the last axis in float64; -inf for a row without a finite entry (no warning, no nan)."""
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    ref = np.where(np.isfinite(m), m, 0.0)
    s = np.exp(x - ref).sum(axis=-1, keepdims=True)
    with np.errstate(divide="ignore"):
        return np.where(np.isfinite(m), ref + np.log(np.where(s > 0, s, 1.0)), NEG)[..., 0]


def guide_ref(cond, uncond, g):
    """cond, uncond (R, V) -> (out float64 (R, V), bound float64 (R, V)); bound is 0 where out is -inf (those must be -inf exactly)."""
    c, u = np.asarray(cond, dtype=np.float64), np.asarray(uncond, dtype=np.float64)
    g = float(g)
    lc, lu = lse64(c)[:, None], lse64(u)[:, None]
    banned = np.isneginf(c) | np.isneginf(u)
    cz, uz = np.where(banned, 0.0, c), np.where(banned, 0.0, u)
    lcz, luz = np.where(np.isfinite(lc), lc, 0.0), np.where(np.isfinite(lu), lu, 0.0)
    out = np.where(banned, NEG, g * (cz - lcz) + (1.0 - g) * (uz - luz))
    bound = (abs(g) + abs(1.0 - g)) * LOGP_TOL + 4 * 2.0 ** -24 * (abs(g) * (np.abs(cz) + np.abs(lcz)) + abs(1.0 - g) * (np.abs(uz) + np.abs(luz)))
    return out, np.where(banned, 0.0, bound)


def worst_ratio(dev, ref, bound):
    """Largest |dev - ref| / bound over the finite elements of ref; inf if dev is not -inf exactly where ref is, or holds a nan / +inf."""
    dev = np.asarray(dev, dtype=np.float64)
    dead = np.isneginf(ref)
    if not np.array_equal(np.isneginf(dev), dead) or not np.isfinite(dev[~dead]).all():
        return float("inf")
    if dead.all():
        return 0.0
    return float((np.abs(dev[~dead] - ref[~dead]) / bound[~dead]).max())


def random_rows(V, seed):
    """(cond, uncond) fp32 (len(ROW_KINDS), V): the row kinds of tests/sample_ref._random_rows, with the -inf patterns a pair of streams can
    show — five -inf in cond only, in uncond only, in both at the same and at different indices, one finite element left, all -inf."""
    rng = np.random.default_rng(seed)
    nb = min(5, V - 1)
    c, u = {}, {}
    for k in ROW_KINDS:
        c[k], u[k] = rng.standard_normal(V) * 3.0, rng.standard_normal(V) * 3.0
    c["gauss5"], u["gauss5"] = rng.standard_normal(V) * 5.0, rng.standard_normal(V) * 5.0
    c["grid"], u["grid"] = np.round(c["grid"] * 4.0) / 4.0, np.round(u["grid"] * 4.0) / 4.0
    c["far"][int(rng.integers(V))] = -1e4
    u["far_b"][int(rng.integers(V))] = -1e4
    c["equal"], u["equal"] = np.full(V, rng.standard_normal() * 3.0), np.full(V, rng.standard_normal() * 3.0)
    c["ban_cond"][rng.choice(V, size=nb, replace=False)] = NEG
    u["ban_uncond"][rng.choice(V, size=nb, replace=False)] = NEG
    same = rng.choice(V, size=nb, replace=False)
    c["ban_same"][same], u["ban_same"][same] = NEG, NEG
    perm = rng.permutation(V)
    c["ban_diff"][perm[:nb]] = NEG
    u["ban_diff"][perm[-nb:] if V >= 2 * nb else perm[nb:]] = NEG
    for name, d in (("one_left_cond", c), ("one_left_uncond", u)):
        keep = int(rng.integers(V))
        v = d[name][keep]
        d[name][:] = NEG
        d[name][keep] = v
    c["dead_cond"][:] = NEG
    u["dead_uncond"][:] = NEG
    c["dead_both"][:], u["dead_both"][:] = NEG, NEG
    f = lambda d: np.stack([d[k] for k in ROW_KINDS]).astype(np.float32)  # noqa: E731
    return f(c), f(u)


# ---- fp32 emulation of the kernel's rule on flat buffers, with defects --------------------------------------------------------------------
DEFECTS = ("softmax", "one_lse", "swapped", "ld_as_V", "skip_ignored", "inf_uncond")


def _lse32(x):
    F = np.float32
    m = x.max()
    if not np.isfinite(m):
        return F(NEG)
    return F(m + np.log(np.exp((x - m).astype(F)).sum(dtype=F), dtype=F))


def emulate(cond, ld_c, uncond, ld_u, R, V, scale, out, ld_o, skip=None, defect=None):
    """What cc_logits_guide does, in fp32 numpy on flat buffers (out is written in place and returned); ``defect``: one of DEFECTS."""
    F = np.float32
    assert defect is None or defect in DEFECTS
    g, h = F(scale), F(1.0) - F(scale)
    if defect == "swapped":
        g, h = h, g
    sc, su, so = (V, V, V) if defect == "ld_as_V" else (ld_c, ld_u, ld_o)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(R):
            if skip is not None and skip[r] and defect != "skip_ignored":
                continue
            c, u = cond[r * sc:r * sc + V].astype(F), uncond[r * su:r * su + V].astype(F)
            lc, lu = _lse32(c), _lse32(u)
            if defect == "one_lse":
                lu = lc
            if defect == "softmax":
                o = g * np.exp(c - lc, dtype=F) + h * np.exp(u - lu, dtype=F)
            else:
                o = g * (c - lc) + h * (u - lu)
            if defect != "inf_uncond":
                o = np.where(np.isneginf(c) | np.isneginf(u), F(NEG), o)
            out[r * so:r * so + V] = o.astype(F)
    return out


# ---- guided beam search for one prefix on the CPU --------------------------------------------------------------------------------------------

def _gap(a, b):
    return 0.0 if a == b else a - b


def _kept_margin(logp, scores, seql, stopped, beam):
    """The smallest gap between the last kept and the first rejected candidate of oracle.beam_update on these log-probabilities."""
    if scores is None:
        vals = logp[0]
    else:
        lp = logp.clone()
        lp[stopped] = float("-inf")
        lp[stopped, 0] = 0
        ln = seql.clone()
        ln[~stopped] += 1
        vals = ((scores[:, None] + lp) / ln[:, None]).view(-1)
    top = torch.topk(vals, min(beam + 1, vals.numel())).values
    return float("inf") if top.numel() <= beam else _gap(float(top[beam - 1]), float(top[beam]))


def guided_beam_search_ref(sd, embeds, negative, *, scale, n_head, n_layer, beam, entry_length, stop_token, rounds=1, groups=1, penalty=0.0,
                           no_repeat_ngram_size=0, min_length=0, pre="language_model."):
    """Guided beam search for ONE prefix (1, L, D) with the unconditional context ``negative`` (1, Ln, D): per step the oracle's full
    re-forward of both streams (oracle.gpt2_logits, fp32), the combination in float64 (guide_ref), the bans of the constrained decoders on
    every beam that has not stopped, then oracle.beam_update (groups == 1) or beam_group_step_ref.  ``rounds``: the reference's live rounds
    (oracle.generate_beam_tokens).  -> ([(tokens (beam, n) int64, length-normalised scores, seq_lengths) per round], margin): the smallest
    gap between the last kept and the first rejected candidate at any step (beam groups: beam_group_step_ref's margins)."""
    from clipcap_amd.inference.utils import banned_tokens
    from oracle import clipcap_oracle as O
    from tests.beam_group_ref import beam_group_step_ref
    wte = sd[pre + "transformer.wte.weight"]
    tokens, scores, stopped = None, None, torch.zeros(beam, dtype=torch.bool)
    seql = torch.ones(beam, dtype=torch.float64)
    margin, out, generated = float("inf"), [], 0
    for _ in range(max(1, rounds)):
        for _ in range(entry_length):
            lc = O.gpt2_logits(sd, embeds, n_head, n_layer, pre=pre)[:, -1, :]
            lu = O.gpt2_logits(sd, negative, n_head, n_layer, pre=pre)[:, -1, :]
            lg = torch.from_numpy(guide_ref(lc.numpy(), lu.numpy(), scale)[0])
            for r in range(lg.shape[0]):
                if tokens is not None and bool(stopped[r]):
                    continue
                ban = (banned_tokens(tokens[r], no_repeat_ngram_size) if tokens is not None else set()) | \
                    ({stop_token} if generated < min_length else set())
                if ban:
                    lg[r, sorted(ban)] = float("-inf")
            first = tokens is None
            if groups == 1:
                margin = min(margin, _kept_margin(torch.log_softmax(lg, -1), scores, seql, stopped, beam))
                nt, src, scores, seql, stopped = O.beam_update(lg, scores, seql, stopped, beam_size=beam, stop_token=stop_token)
            else:
                st = beam_group_step_ref(lg.expand(beam, -1) if first else lg, scores, seql, stopped, beam=beam, groups=groups, penalty=penalty,
                                         first=first, stop_token=stop_token)
                margin = min(margin, min(st.margins))
                nt, src, scores, seql, stopped = st.tokens, (None if first else st.src), st.scores, st.lengths, st.stopped
            if first:
                embeds, negative = embeds.expand(beam, *embeds.shape[1:]), negative.expand(beam, *negative.shape[1:])
                tokens = nt.unsqueeze(1)
            else:
                tokens = torch.cat((tokens[src], nt.unsqueeze(1)), dim=1)
                embeds, negative = embeds[src], negative[src]
            nxt = wte[nt].view(beam, 1, -1)
            embeds, negative = torch.cat((embeds, nxt), dim=1), torch.cat((negative, nxt), dim=1)
            generated += 1
            if bool(stopped.all()):
                break
        scores = scores / seql
        out.append((tokens.clone(), scores.clone(), seql.clone()))
    return out, margin
