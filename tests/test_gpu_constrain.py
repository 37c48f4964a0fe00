"""Constrained decoding on the device (cc_logits_constrain; no_repeat_ngram_size / min_length / suppress_tokens of the decoders).

There is no reference for this feature; the rule is "a banned token's logit is -inf before the softmax", so the expectation is always the
PINNED oracle applied to logits masked in torch: ``masked_fill`` with -inf on ``banned_tokens(history, g)`` + suppress list + ban token,
then oracle.beam_update / nucleus_final_p / top_k_top_p_filtering as they are.  ``banned_tokens`` is the CPU statement of the no-repeat
rule (clipcap_amd/inference/utils.py; hand cases in tests/test_constrain_surface.py).
"""
import math

import pytest
import torch

from clipcap_amd.engine import beam_step, constrain_logits, sample_step
from clipcap_amd.inference.utils import banned_tokens
from oracle import clipcap_oracle as O
from tests.test_gpu_beam import _oracle_step, _partials

pytestmark = pytest.mark.gpu

NEG = float("-inf")
SHAPES = [(4, 130, 136), (5, 50257, 50304)]         # (beam, V, ld): the last 64-column block of V = 130 has two real columns
STOP = 17
SUPPRESS = [5, 70]


# ---- a crafted step: logits, per-row histories, the global rules ------------------------------------------------------------------

def _history(plans, g, n, V):
    """int64 (R, n): row r's history bans exactly plans[r] under the no-repeat rule of size g >= 2.  The row ends with a key of g - 1
    tokens; every token to ban once followed an earlier copy of the key: [pads | key t1 key t2 ... key].  Pads are distinct and hold no
    key token, so they neither ban nor match; a row with an empty plan is pads only, and its last g - 1 tokens occur nowhere else."""
    key = [V - 3 - k for k in range(g - 1)]
    taken = set(key) | {t for p in plans for t in p}
    pads = [t for t in range(V) if t not in taken][:n]
    rows = []
    for p in plans:
        body = [x for t in p for x in (*key, t)] + key if p else []
        assert len(body) <= n
        rows.append(pads[:n - len(body)] + body)
    h = torch.tensor(rows, dtype=torch.int64)
    for r, p in enumerate(plans):
        assert banned_tokens(h[r], g) == set(p), r
    return h


class _Case:
    """One decoding step of S = 2 samples x beam rows, in which different rows meet the six situations of the issue:
       row 0  the banned token is the row's arg-max (hence the maximum of its 64-column block);
       row 1  two banned tokens share a block — the first two columns of the LAST block (V = 130: its only real columns, the block empties);
       row 2  the maximum of the last block is banned: the block maximum moves;
       row 3  all of the row's top-`beam` tokens are banned.  They are raised by 8 first, so that their blocks' stale partials would tower
              over every real candidate of the sample: without the repair the fused update's lower bound is wrong;
       row 4  one token is banned by two rules at once (the history and the suppress list; with the ban token a third time);
       row 5  is stopped: skipped, although its history would ban its arg-max;
       row 6  has nothing to ban in its history;
       rows 7+ ban two arbitrary tokens each.
    ``rules`` = "all": + ban token STOP + suppress list for every row;  "ngram": the history rule alone, so row 6 is banned nothing at all."""

    def __init__(self, beam, V, ld, g, rules, seed):
        gen = torch.Generator().manual_seed(seed)
        self.beam, self.V, self.ld, self.g = beam, V, ld, g
        self.S, self.R = 2, 2 * beam
        R = self.R
        buf = torch.randn(R, ld, generator=gen) * 3.0
        lg = buf[:, :V]
        last0 = (V - 1) // 64 * 64
        lg[3, lg[3].topk(beam).indices] += 8.0
        plans = [[] for _ in range(R)]
        plans[0] = [int(lg[0].argmax())]
        plans[1] = [last0, last0 + 1]
        plans[2] = [last0 + int(lg[2, last0:].argmax())]
        plans[3] = lg[3].topk(beam).indices.tolist()
        plans[4] = [SUPPRESS[0], int(lg[4].argmax())]
        plans[5] = [int(lg[5].argmax())]
        for r in range(7, R):
            plans[r] = torch.randint(0, V, (2,), generator=gen).tolist()
        self.plans = plans
        self.n = 2 * g * beam + 3
        self.hist = _history(plans, g, self.n, V)
        self.buf = buf
        self.skip = torch.zeros(R, dtype=torch.uint8)
        self.skip[5] = 1
        self.ban_token = STOP if rules == "all" else -1
        self.suppress = SUPPRESS if rules == "all" else []
        # the torch image: masked_fill with -inf on banned_tokens + suppress + ban token, rows that are not skipped
        self.banned = []
        img = buf.clone()
        for r in range(R):
            b = set() if self.skip[r] else banned_tokens(self.hist[r], g) | set(self.suppress) | ({self.ban_token} - {-1})
            self.banned.append(b)
            if b:
                img[r, sorted(b)] = NEG
        self.image = img
        # the situations really occur
        assert int(img[0, :V].argmax()) != plans[0][0] and lg[0, plans[0][0]] == lg[0, plans[0][0] // 64 * 64:(plans[0][0] // 64 + 1) * 64].max()
        assert plans[1][0] // 64 == plans[1][1] // 64 == (V - 1) // 64
        assert (V != 130) or bool((img[1, 128:130] == NEG).all())
        assert img[2, last0:V].max() < lg[2, last0:].max() and img[2, last0:V].max() > NEG
        assert set(lg[3].topk(beam).indices.tolist()) <= self.banned[3]
        assert rules != "all" or plans[4][0] in SUPPRESS
        assert torch.equal(img[5], buf[5]) and plans[5]
        assert rules != "ngram" or (not self.banned[6] and torch.equal(img[6], buf[6]))

    def run(self, hist_dtype=torch.int32, hist_pad=0, partials=True, extra_part=0):
        """The device call -> (logits buffer (R, ld), pmax, psum (R, npart) or None, the partials before the call)."""
        V, R = self.V, self.R
        d = self.buf.cuda()
        lg = d[:, :V]
        hbuf = torch.full((R, self.n + hist_pad), -7, dtype=hist_dtype)
        hbuf[:, :self.n] = self.hist.to(hist_dtype)
        hist = hbuf.cuda()[:, :self.n]                                   # hist_pad > 0: a row stride larger than the width
        lpart = before = None
        if partials:
            flat, npart = _partials(lg, V)
            if extra_part:                                               # npart larger than the block count: the row stride of the partials
                two = flat.view(2, R, npart)
                wide = torch.full((2, R, npart + extra_part), 123.0, device="cuda")
                wide[:, :, :npart] = two
                flat, npart = wide.reshape(-1).contiguous(), npart + extra_part
            before = flat.clone()
            lpart = (flat, npart)
        sup = torch.tensor(self.suppress, dtype=torch.int32, device="cuda") if self.suppress else None
        out = constrain_logits(lg, lpart=lpart, history=hist, hist_len=self.n, no_repeat_ngram=self.g, ban_token=self.ban_token, suppress=sup,
                               skip_rows=self.skip.cuda())
        torch.cuda.synchronize()
        assert out.data_ptr() == lg.data_ptr()
        if not partials:
            return d, None, None, None
        two = lpart[0].view(2, R, lpart[1])
        return d, two[0], two[1], before.view(2, R, lpart[1])


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("rules", ["all", "ngram"])
@pytest.mark.parametrize("variant", ["int32", "int64", "int32_strided", "int64_strided_g3", "wide_partials"])
@pytest.mark.parametrize("beam,V,ld", SHAPES)
def test_constrain_matches_the_torch_image(beam, V, ld, variant, rules):
    """Logits bit-equal to masked_fill(-inf) (padding columns and skipped rows bit-unchanged); pmax bit-equal to the maximum of the masked
    block; psum within rtol 1e-5 of the float64 sum (64 fp32 additions at 2^-24 each plus an expf of a couple of ulp per term stay under
    that); the partials of blocks without a ban bit-identical to the inputs."""
    g = 3 if variant.endswith("g3") else 2
    c = _Case(beam, V, ld, g, rules, seed=beam * 100 + V + g)
    d, pmax, psum, before = c.run(hist_dtype=torch.int64 if variant.startswith("int64") else torch.int32,
                                  hist_pad=5 if "strided" in variant else 0, extra_part=3 if variant == "wide_partials" else 0)
    assert torch.equal(_bits(d.cpu()), _bits(c.image))
    nblk = (V + 63) // 64
    pad = torch.full((c.R, nblk * 64), NEG, dtype=torch.float64)
    pad[:, :V] = c.image[:, :V].double()
    blk = pad.view(c.R, nblk, 64)
    want_max = blk.max(dim=2).values
    assert torch.equal(_bits(pmax[:, :nblk].cpu()), _bits(want_max.float()))
    want_sum = torch.where(want_max > NEG, torch.exp(blk - want_max.clamp_min(-1e30)[:, :, None]).sum(dim=2), torch.zeros_like(want_max))
    got_sum = psum[:, :nblk].cpu().double()
    assert torch.isfinite(got_sum).all()
    err = ((got_sum - want_sum).abs() / want_sum.clamp_min(1e-300)).where(want_sum > 0, (got_sum - want_sum).abs())
    print(f"psum: max relative error {err.max().item():.2e}")
    assert err.max().item() <= 1e-5
    touched = torch.zeros(c.R, nblk, dtype=torch.bool)
    for r, b in enumerate(c.banned):
        for t in b:
            touched[r, t // 64] = True
    assert touched[:5].any(dim=1).all() and not touched[5].any() and (rules == "all" or not touched[6].any())
    keep = ~touched
    assert torch.equal(_bits(pmax[:, :nblk].cpu())[keep], _bits(before[0][:, :nblk].cpu())[keep])
    assert torch.equal(_bits(psum[:, :nblk].cpu())[keep], _bits(before[1][:, :nblk].cpu())[keep])
    assert torch.equal(_bits(pmax[:, nblk:].cpu()), _bits(before[0][:, nblk:].cpu())) and torch.equal(_bits(psum[:, nblk:].cpu()), _bits(before[1][:, nblk:].cpu()))
    if V == 130:                                                     # the emptied block: (-inf, 0), which the beam update treats as empty
        assert pmax[1, 2].item() == NEG and psum[1, 2].item() == 0.0


@pytest.mark.parametrize("beam,V,ld", SHAPES)
def test_constrain_without_partials_and_with_nothing_to_do(beam, V, ld):
    c = _Case(beam, V, ld, 2, "all", seed=beam + V)
    d, *_ = c.run(partials=False)
    assert torch.equal(_bits(d.cpu()), _bits(c.image))
    # every rule off / a history shorter than the n-gram: nothing is written
    lg = c.buf.cuda()[:, :V]
    constrain_logits(lg)
    constrain_logits(lg, history=c.hist.cuda(), hist_len=2, no_repeat_ngram=3)
    torch.cuda.synchronize()
    assert torch.equal(_bits(lg.cpu()), _bits(c.buf[:, :V]))


def test_constrain_argument_errors_launch_nothing():
    from clipcap_amd._lib import CCError
    V = 130
    lg = torch.zeros(2, V, device="cuda")
    hist = torch.zeros(2, 1030, dtype=torch.int32, device="cuda")
    part = torch.zeros(2 * 2 * 2, device="cuda")
    for kw, code in ((dict(ban_token=V), -1), (dict(ban_token=-2), -1), (dict(no_repeat_ngram=-1), -1),
                     (dict(history=hist, hist_len=1025, no_repeat_ngram=2), -2),
                     (dict(suppress=torch.zeros(1024, dtype=torch.int32, device="cuda")), -2),
                     (dict(lpart=(part, 2), ban_token=3), -1)):
        with pytest.raises(CCError, match=rf"\({code}\)"):
            constrain_logits(lg, **kw)
    torch.cuda.synchronize()
    assert not lg.any()


# ---- the beam update behind the constrain step -------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ["fused_partials", "three_kernels"])
@pytest.mark.parametrize("beam,V,ld", SHAPES)
def test_beam_step_after_constrain_matches_oracle_on_masked_logits(beam, V, ld, route):
    """Five updates through stopping beams: a first step with the global rules only (no history yet), then crafted steps (class _Case).
    Tokens, source rows, lengths and flags equal oracle.beam_update on the masked logits; scores at tests/test_gpu_beam.py's tolerance.
    fused_partials: temperature 1 with the repaired partials (k_beam_fused); three_kernels: temperature 0.9 without partials."""
    temp = 1.0 if route == "fused_partials" else 0.9
    S, R = 2, 2 * beam
    scores = torch.zeros(R, device="cuda")
    seql = torch.ones(R, device="cuda")
    stopped = torch.zeros(R, dtype=torch.uint8, device="cuda")
    o_scores, o_seql, o_stopped = torch.zeros(R), torch.ones(R), torch.zeros(R, dtype=torch.bool)
    sup = torch.tensor(SUPPRESS, dtype=torch.int32, device="cuda")
    saw_row3 = False
    for step in range(5):
        c = _Case(beam, V, ld, 2, "all", seed=step * 7 + beam + V)
        buf = c.buf.clone()
        ban_token = STOP if step < 2 else -1                        # min_length = 2
        if step >= 2:
            buf[::3, STOP] += 25.0                                   # some beams pick the stop token and freeze
        d = buf.cuda()
        lg = d[:, :V]
        first = step == 0
        lpart = _partials(lg, V) if route == "fused_partials" else None
        if first:
            rows = lg[::beam]
            constrain_logits(rows, ban_token=ban_token, suppress=sup)       # what generate_beam_rounds does before the first update
            if lpart is not None:
                lpart = _partials(lg, V)                                     # (the decoder has no partials at step 0; the fused kernel is given consistent ones)
        else:
            constrain_logits(lg, lpart=lpart, history=c.hist.cuda(), hist_len=c.n, no_repeat_ngram=2, ban_token=ban_token, suppress=sup,
                             skip_rows=stopped)
        img = buf[:, :V].clone()
        for r in range(R):
            if first and r % beam:
                continue
            if not first and o_stopped[r]:
                continue
            b = (set() if first else banned_tokens(c.hist[r], 2)) | set(SUPPRESS) | ({ban_token} - {-1})
            img[r, sorted(b)] = NEG
        torch.cuda.synchronize()
        assert torch.equal(_bits(lg.cpu()), _bits(img)), step
        if not first and not o_stopped[3]:
            saw_row3 = True                                          # row 3: every top-`beam` token of a dominant row is banned
        nt, sr = beam_step(lg, S, beam, temp, first, STOP, scores, seql, stopped, None, lpart)
        ont, osr = _oracle_step(img, first, S, beam, temp, STOP, o_scores, o_seql, o_stopped)
        torch.cuda.synchronize()
        assert torch.equal(nt.cpu().long(), ont), step
        if not first:
            assert torch.equal(sr.cpu().long(), osr), step
        assert torch.allclose(scores.cpu(), o_scores, rtol=1e-5, atol=3e-5), step
        assert torch.equal(seql.cpu(), o_seql) and torch.equal(stopped.cpu().bool(), o_stopped), step
        assert step >= 2 or not o_stopped.any()                      # the stop token is banned while min_length holds
    assert o_stopped.any() and not o_stopped.all() and saw_row3


@pytest.mark.parametrize("V,ld", [(130, 136), (131, 131)])
def test_first_step_with_the_head_of_a_row_banned(V, ld):
    """The three-kernel route's row statistics (k_beam_rowstats) when a thread's FIRST elements are all -inf: tokens 0..3 banned is the whole
    first float4 group of thread 0 on the vector path (ld % 4 == 0) and the first element of threads 0..3 on the scalar path (ld = 131).
    Before the guard in that kernel such a thread computed -inf - -inf = NaN and the row's sum was NaN."""
    beam, S, temp = 4, 2, 0.9
    R = S * beam
    buf = torch.randn(R, ld, generator=torch.Generator().manual_seed(V)) * 3.0
    d = buf.cuda()
    lg = d[:, :V]
    sup = torch.tensor([0, 1, 2, 3], dtype=torch.int32, device="cuda")
    scores, seql = torch.zeros(R, device="cuda"), torch.ones(R, device="cuda")
    stopped = torch.zeros(R, dtype=torch.uint8, device="cuda")
    o_scores, o_seql, o_stopped = torch.zeros(R), torch.ones(R), torch.zeros(R, dtype=torch.bool)
    for first in (True, False):
        constrain_logits(lg[::beam] if first else lg, suppress=sup)
        img = buf[:, :V].clone()
        img[:, :4] = NEG                                             # (rows the first update does not read were banned by the second call)
        nt, sr = beam_step(lg, S, beam, temp, first, STOP, scores, seql, stopped)
        ont, osr = _oracle_step(img, first, S, beam, temp, STOP, o_scores, o_seql, o_stopped)
        torch.cuda.synchronize()
        assert torch.isfinite(scores).all() and torch.equal(nt.cpu().long(), ont)
        assert first or torch.equal(sr.cpu().long(), osr)
        assert torch.allclose(scores.cpu(), o_scores, rtol=1e-5, atol=3e-5)


def test_history_ids_outside_the_vocabulary_compare_by_value():
    """Two DIFFERENT out-of-range ids do not match in the suffix compare, equal ones do; neither is ever banned (nothing is written for it)."""
    V = 130
    hist = torch.tensor([[V + 5, 9, 3, V + 7], [V + 5, 9, 3, V + 5], [-4, 11, 3, -4], [7, V + 1, 3, 7]], dtype=torch.int64)
    for dt in (torch.int64, torch.int32):
        lg = torch.zeros(4, V, device="cuda")
        constrain_logits(lg, history=hist.to(dt).cuda(), hist_len=4, no_repeat_ngram=2)
        want = torch.zeros(4, V)
        want[1, 9] = want[2, 11] = NEG                               # row 0: V+5 != V+7, nothing; row 3: 7 is followed by V+1, which bans nothing
        assert torch.equal(_bits(lg.cpu()), _bits(want)), dt
        assert [banned_tokens(h, 2) & set(range(V)) for h in hist] == [set(), {9}, {11}, set()]


# ---- the samplers behind the constrain step ---------------------------------------------------------------------------------------

def _margin_ok(cum, top_p, tol=2e-5):
    return bool(((cum - top_p).abs() > tol).all())


@pytest.mark.parametrize("mode,top_p,top_k,temperature", [(0, 0.8, None, 1.0), (0, 0.5, 40, 0.7), (1, 0.9, 0, 1.0), (1, 0.5, 10, 0.9)])
@pytest.mark.parametrize("V", [130, 50257])
def test_sample_step_after_constrain(V, mode, top_p, top_k, temperature):
    """Banned tokens have probability exactly 0; the rest is the oracle's distribution on the masked logits, at the tolerance
    tests/test_gpu_sampling.py uses for the same comparison.  g = 1: a row's history IS its banned set; row 0 bans all but one token of a
    64-token window plus (V = 130) everything else, i.e. the all-but-one-banned row; row 1 bans its top 6; row 2 bans nothing (skipped)."""
    gen = torch.Generator().manual_seed(V + mode)
    R = 4
    logits = torch.randn(R, V, generator=gen) * 4.0
    n = V - 1 if V == 130 else 200
    plans = [[t for t in range(V) if t != 77][:n] if V == 130 else list(range(1000, 1000 + n)),
             logits[1].topk(6).indices.tolist(), logits[2].topk(3).indices.tolist(), torch.randint(0, V, (9,), generator=gen).tolist()]
    hist = torch.stack([torch.tensor((p * n)[:n]) for p in plans])                 # padded by repetition: g = 1 bans every entry
    skip = torch.tensor([0, 0, 1, 0], dtype=torch.uint8)
    d = logits.cuda()
    constrain_logits(d, history=hist.cuda(), hist_len=n, no_repeat_ngram=1, ban_token=STOP, skip_rows=skip.cuda())
    img = logits.clone()
    banned = []
    for r in range(R):
        b = set() if skip[r] else banned_tokens(hist[r], 1) | {STOP}
        banned.append(b)
        if b:
            img[r, sorted(b)] = NEG
    assert torch.equal(_bits(d.cpu()), _bits(img))
    if V == 130:
        assert int((img[0] > NEG).sum()) == 1
    u = torch.rand(R, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    nt, probs = sample_step(d, u, temperature=temperature, top_k=top_k or 0, top_p=top_p, mode=mode, return_probs=True)
    probs, nt = probs.cpu(), nt.cpu()
    checked = 0
    for r in range(R):
        assert all(probs[r, t] == 0 for t in banned[r]) and probs[r, int(nt[r])] > 0 and int(nt[r]) not in banned[r]
        x = img[r] / temperature
        if mode == 0:
            k = min(top_k, V) if top_k else None
            ref = O.nucleus_final_p(x[None], top_p=top_p, top_k=k)[0]
            ps = torch.softmax(x, -1).sort(descending=True).values
            cum = (ps[:k] if k else ps).cumsum(-1)
        else:
            ref = torch.softmax(O.top_k_top_p_filtering(x.clone(), top_k=top_k, top_p=top_p), -1)
            xs = x.clone()
            if top_k > 0:
                xs[xs < xs.topk(top_k).values[-1]] = NEG
            cum = torch.softmax(xs.sort(descending=True).values, -1).cumsum(-1)
        if not _margin_ok(cum, top_p):
            continue
        checked += 1
        assert torch.allclose(probs[r], ref, atol=2e-6, rtol=1e-4), (r, (probs[r] - ref).abs().max())
        assert (probs[r] > 0).sum() == (ref > 0).sum()
    assert checked >= R - 1
    assert torch.allclose(probs.sum(-1), torch.ones(R), atol=1e-5)
    if V == 130:
        assert int(nt[0]) == 77 and probs[0, 77] == 1.0


# ---- end to end: the decoders on a tiny GPT-2 against an oracle loop written here --------------------------------------------------
# The seed was chosen on the CPU with the oracle alone (asserted below, so the test cannot pass vacuously and a flip cannot be blamed on
# a tie): the oracle's UNCONSTRAINED search repeats a bigram, stops before min_length and emits the suppressed id in returned beams, and
# in the constrained search no step has its beam-th and (beam + 1)-th candidate values closer than 1e-3, the project's near-tie
# threshold for bf16 noise.  (The order INSIDE the best `beam` may be closer than that: it permutes rows, not what is kept, so the
# returned beams are compared as a set.)
E2E_D, E2E_NL, E2E_HEADS, E2E_V, E2E_NPOS = 64, 2, 4, 211, 48
E2E_SEED, E2E_WTE_SCALE, E2E_PREFIXES, E2E_L0, E2E_BEAM, E2E_ENTRY, E2E_STOP = 25, 40.0, 3, 4, 4, 20, 153
E2E_G, E2E_MIN, E2E_SUPPRESS = 2, 5, [71]


def _e2e_weights(seed=None, wte_scale=None):
    from tests import seeded
    gsd = seeded.state_dict(seeded.gpt2_shapes(E2E_D, E2E_NL, E2E_V, E2E_NPOS), E2E_SEED if seed is None else seed)
    gsd["transformer.wte.weight"] = gsd["transformer.wte.weight"] * (E2E_WTE_SCALE if wte_scale is None else wte_scale)
    pref = torch.randn(E2E_PREFIXES, E2E_L0, E2E_D, generator=torch.Generator().manual_seed(E2E_SEED if seed is None else seed)) * 0.5
    return gsd, pref


def _oracle_search(sd, embeds, g=0, m=0, suppress=()):
    """generate_beam (inference/base.py:55-132) for one prefix (1, L, D) as oracle.generate_beam_tokens restates it — full re-forward
    per step with oracle.gpt2_logits, the update by oracle.beam_update — with the bans masked into the logits of every beam that has not
    stopped.  -> (tokens (beam, n), length-normalised scores, seq_lengths, smallest gap between a step's beam-th and (beam + 1)-th value)."""
    beam, stop = E2E_BEAM, E2E_STOP
    wte = sd["language_model.transformer.wte.weight"]
    tokens, scores = None, None
    seql, stopped = torch.ones(beam), torch.zeros(beam, dtype=torch.bool)
    gap = math.inf
    for step in range(E2E_ENTRY):
        logits = O.gpt2_logits(sd, embeds, E2E_HEADS, E2E_NL, pre="language_model.")[:, -1, :].clone()
        for r in range(logits.shape[0]):
            if tokens is not None and stopped[r]:
                continue
            ban = set(suppress) | (banned_tokens(tokens[r], g) if tokens is not None else set()) | ({stop} if step < m else set())
            if ban:
                logits[r, sorted(ban)] = NEG
        if scores is None:                                              # the same update one candidate wider, for the gaps only
            wide = O.beam_update(logits.clone(), None, torch.ones(beam + 1), torch.zeros(beam + 1, dtype=torch.bool), beam_size=beam + 1, stop_token=stop)
        else:
            wide = O.beam_update(logits.clone(), scores.clone(), seql.clone(), stopped.clone(), beam_size=beam + 1, stop_token=stop)
        vals = wide[2] if scores is None else wide[2] / wide[3]
        gap = min(gap, float(vals[beam - 1] - vals[beam]))
        nxt, src, scores, seql, stopped = O.beam_update(logits, scores, seql, stopped, beam_size=beam, stop_token=stop)
        if src is None:
            embeds = embeds.expand(beam, *embeds.shape[1:])
            tokens = nxt.unsqueeze(1)
        else:
            tokens = torch.cat((tokens[src], nxt.unsqueeze(1)), dim=1)
            embeds = embeds[src]
        embeds = torch.cat((embeds, wte[nxt].view(beam, 1, -1)), dim=1)
        if stopped.all():
            break
    return tokens, scores / seql, seql, gap


def _beams(tokens, lengths):
    return sorted(tuple(int(t) for t in tokens[b, :int(lengths[b])]) for b in range(tokens.shape[0]))


def _repeats(seq, g):
    grams = [tuple(seq[i:i + g]) for i in range(len(seq) - g + 1)]
    return len(grams) != len(set(grams))


def _e2e_model():
    from types import SimpleNamespace
    from clipcap_amd.model.gpt2 import GPT2LM
    gsd, pref = _e2e_weights()
    lm = GPT2LM(n_embd=E2E_D, n_layer=E2E_NL, n_head=E2E_HEADS, vocab_size=E2E_V, n_positions=E2E_NPOS, precision=32)
    lm.load_state_dict({k: torch.from_numpy(v) for k, v in gsd.items()}, strict=False)
    sd = {"language_model." + k: torch.from_numpy(v) for k, v in gsd.items()}
    return SimpleNamespace(language_model=lm.to("cuda")), sd, pref


def test_constrained_beam_search_equals_the_constrained_oracle_search():
    """The returned beams equal the oracle's token for token, each with its score.  The ORDER of the beam rows is deliberately not
    pinned: the asserted 1e-3 gap separates what is kept from what is dropped, while two kept candidates may lie closer than the split-bf16
    logit noise, which permutes rows without changing any caption — so the beams are matched by content (_beams sorts them)."""
    from clipcap_amd.inference.base import generate_beam_tokens
    model, sd, pref = _e2e_model()
    kw = dict(no_repeat_ngram_size=E2E_G, min_length=E2E_MIN, suppress_tokens=E2E_SUPPRESS)
    toks, scores, lens = generate_beam_tokens(model, pref.cuda(), E2E_BEAM, E2E_ENTRY, 1.0, E2E_STOP, **kw)
    toks, scores, lens = toks.cpu(), scores.cpu(), lens.cpu()
    free_repeat = free_short = free_suppressed = False
    for s in range(E2E_PREFIXES):
        ft, fs, fl, _ = _oracle_search(sd, pref[s:s + 1])
        for seq in _beams(ft, fl):
            free_repeat |= _repeats(seq, E2E_G)
            free_short |= E2E_STOP in seq[:E2E_MIN]
            free_suppressed |= bool(set(seq) & set(E2E_SUPPRESS))
        ot, osc, ol, gap = _oracle_search(sd, pref[s:s + 1], E2E_G, E2E_MIN, E2E_SUPPRESS)
        assert gap > 1e-3, (s, gap)
        assert _beams(toks[s], lens[s]) == _beams(ot, ol), s
        mine = {tuple(toks[s, b, :int(lens[s, b])].tolist()): float(scores[s, b]) for b in range(E2E_BEAM)}
        for b in range(E2E_BEAM):                                     # split-bf16 logits are within ~1e-4 of fp32: so are the mean log-probabilities
            assert abs(mine[tuple(ot[b, :int(ol[b])].tolist())] - float(osc[b])) <= 1e-3, (s, b)
        # and, separately from the oracle, the three properties
        for seq in _beams(toks[s], lens[s]):
            assert not _repeats(seq, E2E_G), seq
            assert E2E_STOP not in seq[:E2E_MIN], seq
            assert not set(seq) & set(E2E_SUPPRESS), seq
    assert free_repeat and free_short and free_suppressed            # each constraint changes what the unconstrained search returns


def test_constrained_sampling_obeys_the_three_properties():
    from clipcap_amd.inference.base import sample_tokens
    model, _, pref = _e2e_model()
    head = torch.tensor([[9, 4]])
    for mode, kw in ((0, dict(top_p=0.9)), (1, dict(top_p=0.95, top_k=50, repetition_penalty=1.2, head_tokens=head))):
        gen = torch.Generator(device="cuda").manual_seed(5)
        toks, stop_pos = sample_tokens(model, pref.cuda().repeat(2, 1, 1), E2E_ENTRY, E2E_STOP, mode=mode, generator=gen, no_repeat_ngram_size=E2E_G,
                                       min_length=E2E_MIN, suppress_tokens=E2E_SUPPRESS, **kw)
        toks = toks.cpu()
        assert toks.shape[1] > E2E_MIN
        for r in range(toks.shape[0]):
            seq = (head[0].tolist() if "head_tokens" in kw else []) + toks[r].tolist()       # the history the rule sees: head ++ generated
            assert not _repeats(seq, E2E_G), (mode, seq)
            assert E2E_STOP not in toks[r, :E2E_MIN].tolist() and not set(toks[r].tolist()) & set(E2E_SUPPRESS), (mode, seq)


def test_options_off_make_no_constrain_call(monkeypatch):
    from clipcap_amd import engine
    from clipcap_amd.inference import base
    model, _, pref = _e2e_model()

    def boom(*a, **k):
        raise AssertionError("constrain_logits called with every option off")

    plain = base.generate_beam_tokens(model, pref.cuda(), E2E_BEAM, E2E_ENTRY, 1.0, E2E_STOP)
    gen = lambda: torch.Generator(device="cuda").manual_seed(3)  # noqa: E731
    plain_s = base.sample_tokens(model, pref.cuda(), E2E_ENTRY, E2E_STOP, generator=gen())
    monkeypatch.setattr(engine, "constrain_logits", boom)
    monkeypatch.setattr(base, "constrain_logits", boom)
    off = base.generate_beam_tokens(model, pref.cuda(), E2E_BEAM, E2E_ENTRY, 1.0, E2E_STOP, no_repeat_ngram_size=0, min_length=0, suppress_tokens=None)
    off_s = base.sample_tokens(model, pref.cuda(), E2E_ENTRY, E2E_STOP, generator=gen(), no_repeat_ngram_size=0, min_length=0, suppress_tokens=[])
    assert all(torch.equal(a, b) for a, b in zip(plain, off)) and all(torch.equal(a, b) for a, b in zip(plain_s, off_s))
    with pytest.raises(AssertionError, match="every option off"):          # ... and with an option on, the call is made
        base.generate_beam_tokens(model, pref.cuda(), E2E_BEAM, E2E_ENTRY, 1.0, E2E_STOP, min_length=1)
