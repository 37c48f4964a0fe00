"""CPU tests of tests/lm_ref.py itself: the float64 reference against torch autograd, the input families' stated properties in every
build's stored values, the defect emulations against the bounds, and the case list's coverage of the kernel paths."""
import functools
import math

import pytest
import torch

from tests import lm_ref as LM

@functools.lru_cache(maxsize=None)
def _ref(op, name):
    c = {k.name: k for k in LM.cases(op)}[name]
    x, gamma, beta, wte, tok = LM.make_inputs(c, op)
    T = c.L + c.cap
    ln = LM.ln_rows(x, gamma, beta, c.B, T, c.L, c.cap)
    hf = LM.store(ln["hf"], op)
    denom = LM.denom_of(c, tok)
    R = LM.chain(hf, wte, tok, c, op, denom)
    return c, (x, gamma, beta, wte, tok), hf, denom, R


def _names(op, pred=lambda c: True):
    return [c.name for c in LM.cases(op) if pred(c)]


_AUTO = [(op, n) for op, mode in (("x3", 2), ("x3", 1), ("bf16", 2), ("fp16", 2))
         for n in _names(op, lambda c: c.mode == mode and c.V < 5000 and c.family in ("flat", "confident", "wrong"))]


@pytest.mark.parametrize("op,name", _AUTO)
def test_reference_equals_autograd(op, name):
    """layer_norm -> matmul -> cross_entropy(ignore_index=0, pads -> 0) in float64 against chain() in both forms (split-bf16 mode 2 and
    fp16: logit form; split-bf16 mode 1 and bf16: exponential form, no row of these families clamps) and both operand branches.  Autograd
    multiplies the stored values exactly; the three-term product does so only for bf16-exact operands, so the split-bf16 cases round
    hf and wte to bf16 first."""
    c = {k.name: k for k in LM.cases(op)}[name]
    x, gamma, beta, wte, tok = LM.make_inputs(c, op)
    sdt = torch.bfloat16 if op == "x3" else LM.DT[op]
    wte = wte.to(sdt).float()
    T = c.L + c.cap
    xd = x.double().requires_grad_(True)
    g, b, w = gamma.double().requires_grad_(True), beta.double().requires_grad_(True), wte.double().requires_grad_(True)
    rows = LM.row_map(c.B, T, c.L, c.cap)
    hf_a = torch.nn.functional.layer_norm(xd, (c.D,), g, b, 1e-5)[rows]
    # the chain sees hf rounded to bf16-exact values; give autograd the same values without cutting the graph
    hf_q = hf_a + (hf_a.detach().float().to(sdt).double() - hf_a.detach())
    hf_q.retain_grad()
    logits = hf_q @ w.t()
    tgt = tok.reshape(-1).clamp_min(0)
    kept = int((tgt != 0).sum())
    loss = torch.nn.functional.cross_entropy(logits, tgt, ignore_index=0, reduction="sum")
    denom = LM.denom_of(c, tok)
    (loss * (c.ls or 1.0) / max(denom, 1.0)).backward()
    ln = LM.ln_rows(x, gamma, beta, c.B, T, c.L, c.cap)
    assert (ln["hf"] - hf_a.detach()).abs().max() <= 1e-10
    R = LM.chain(hf_q.detach().float() if op == "x3" else hf_q.detach().float().to(sdt), wte, tok, c, op, denom)
    assert not R["beyond"].any()
    assert abs(R["stats"][0].item() - loss.item()) <= 1e-10 * max(1.0, abs(loss.item())) and R["stats"][1].item() == kept
    assert (R["dhf"] - hf_q.grad).abs().max() <= 1e-10
    if c.mode == 2:
        assert (R["dwte"][:c.V] - w.grad).abs().max() <= 1e-10 and (R["dwte"][c.V:] == 0).all()
    W = LM.ln_bwd(ln, gamma, hf_q.grad)
    full = torch.zeros_like(xd)
    full[rows] = W["dx"]
    assert (full - xd.grad).abs().max() <= 1e-10
    assert (W["dgamma"] - g.grad).abs().max() <= 1e-10 and (W["dbeta"] - b.grad).abs().max() <= 1e-10
    lp = torch.log_softmax(logits.detach(), 1).gather(1, tgt.view(-1, 1)).squeeze(1)
    assert (torch.where(R["keep"], R["tgt"] - R["lse"], torch.zeros_like(lp)) - torch.where(tgt != 0, lp, torch.zeros_like(lp))).abs().max() <= 1e-10


@pytest.mark.parametrize("op", LM.OPS)
def test_family_properties(op):
    """each family is what lm_ref says it is, stated on the float64 reference of the build's stored values"""
    seen = set()
    for c in LM.cases(op):
        if c.mode == 2:
            continue
        c, (x, gamma, beta, wte, tok), hf, denom, R = _ref(op, c.name)
        z, tid = R["z"], R["tid"]
        kept = tid != 0
        tz = z.gather(1, tid.view(-1, 1)).squeeze(1)
        zmax = z.max(1).values
        assert (hf[:, 0].double() == 8.0).all(), c.name
        loss = R["lse"] - tz
        if c.family == "flat":
            assert ((loss - math.log(c.V)).abs() < 1.0).all(), (c.name, loss.min().item(), loss.max().item())
        if c.family == "confident":
            other = z.scatter(1, tid.view(-1, 1), -1e300).max(1).values
            assert ((tz - other)[kept] >= 30.0).all(), (c.name, (tz - other)[kept].min().item())
        if c.family == "wrong":
            gap = (zmax - tz)[kept]
            assert (gap >= 40.0).all() and (gap <= 70.0).all(), (c.name, gap.min().item(), gap.max().item())
            ign = (zmax - tz)[~kept]
            assert len(ign) == 0 or ign.max() >= 40.0, c.name      # ignored rows carry the family's spread
        if c.family == "offset":
            assert (z.min(1).values > LM.OFFSET[op] - 8).all() and (zmax < LM.OFFSET[op] + 8).all(), c.name
            w1 = wte.clone()      # the unshifted case: the same values apart from wte[:, 0]
            w1[:, 0] = 0
            R0 = LM.chain(hf, w1, tok, c, op, denom)
            key = "loss" if c.mode else "tlp"
            assert (R0[key] - R[key]).abs().max() <= 1e-9, c.name
            if c.mode:
                assert (R0["dhf"] - R["dhf"]).abs().max() <= 1e-9, c.name
        if c.family == "beyond":
            hit = (z - tz.unsqueeze(1)) > 80.0
            rows = hit.any(1)
            assert rows.any() or c.B * c.cap < 6, c.name
            gap = (z - tz.unsqueeze(1))[hit]
            if len(gap):
                assert (gap >= 85.0).all() and (gap <= 95.0).all(), (c.name, gap.min().item(), gap.max().item())
                assert hit.sum(1).max() <= 8
        flat = tok.reshape(-1)
        last = flat[(flat > 0) & (flat // 8 == (c.V - 1) // 8)]
        whole = bool((tok[:, -1] == -1).any() and (flat == 0).any() and (tok == -1).all(1).any() and (flat == c.V - 1).any() and len(last)
                     and flat[flat > 0].bincount().max() > 1 and max(r[r > 0].bincount().max() for r in tok if (r > 0).any()) > 1)
        # the whole inventory wherever the shape has room for it (lm_ref.make_tokens): three samples of three columns
        assert whole == (c.B >= 3 and c.cap >= 3), c.name
        if whole:
            seen.add(c.family)
    assert seen == set(LM.FAMILIES), seen       # every family has a case with the whole token inventory


@pytest.mark.parametrize("op", LM.OPS)
def test_finite_only_rows_stay_under_five_percent(op):
    rows = fin = 0
    for c in LM.cases(op):
        c, _, hf, denom, R = _ref(op, c.name)
        rows += hf.shape[0]
        fin += int(R["beyond"].sum())
    assert 0 < fin or op == "fp16"
    assert fin <= 0.05 * rows, (fin, rows)


@pytest.mark.parametrize("op", LM.OPS)
def test_every_path_is_reached(op):
    got = {LM.paths(c, op) for c in LM.cases(op)}
    assert LM.required_paths(op) <= got, sorted(LM.required_paths(op) - got)
    tiles = {c.tile for c in LM.cases(op)}
    assert tiles >= ({0, 3, 4, 5} | (set() if op == "x3" else {6, 7}))
    assert {c.B * c.cap for c in LM.cases(op)} >= {1, 5, 130, 257, 330} and {c.D for c in LM.cases(op)} == {64, 96, 256}


@pytest.mark.parametrize("op", LM.OPS)
def test_every_defect_leaves_the_bound(op):
    """every defect emulation leaves the bound of at least one checked quantity on at least one case of every form it can occur in, and the
    reference itself sits inside its own bounds"""
    met = {}
    for c in LM.cases(op):
        c, (x, gamma, beta, wte, tok), hf, denom, R = _ref(op, c.name)
        if LM.EXP2_POS_ULPS is not None:
            assert LM.EXP2_POS_ULPS <= LM.ALLOW_CEILING[0] and LM.LOGF_ULPS <= LM.ALLOW_CEILING[1]
        Bd = LM.bounds(R, c, op, allow=LM.ALLOW_CEILING)      # the loosest bounds any admissible allowance gives (lm_ref.ALLOW_CEILING)
        form = R["form"]
        assert LM.leaves_bound(R, R, Bd) is None
        for d in LM.DEFECTS:
            if not LM.defect_applies(d, form):
                continue
            if d == "row_map_plus_1":
                T = c.L + c.cap
                hf2 = LM.store(LM.ln_rows(x, gamma, beta, c.B, T, c.L, c.cap, shift=1)["hf"], op)
                Rd = LM.chain(hf2, wte, tok, c, op, denom)
            else:
                Rd = LM.chain(hf, wte, tok, c, op, denom, defect=d)
            q = LM.leaves_bound(Rd, R, Bd)
            if q is None and d == "dwte_pad_rows" and "dwte" in Rd:
                q = "dwte rows >= V" if (Rd["dwte"][c.V:] != 0).any() else None
            if q:
                met.setdefault((d, form), []).append((c.name, q))
                if d == "fold_last_batch":
                    met.setdefault((d, form, LM.paths(c, op)[2]), []).append((c.name, q))
    forms = {LM.form_of(op, m) for m in (0, 1, 2)}
    missing = [(d, f) for d in LM.DEFECTS for f in forms if LM.defect_applies(d, f) and (d, f) not in met]
    missing += [("fold_last_batch", f, fo) for f in forms for fo in ("fast", "generic") if ("fold_last_batch", f, fo) not in met]
    assert not missing, missing


def test_hooks_refuse_bad_calls_before_any_device_work():
    """cc_lmhead_put_x / cc_lmhead_get check their arguments before the first HIP call (this runs without a GPU)"""
    import ctypes as C
    from clipcap_amd import _lib
    from clipcap_amd.engine import Gpt2Engine
    l = _lib.lib()
    ge = Gpt2Engine(64, 1, 1, 97, 8)
    shp = ge.shape(2, 1, 3, 2, 1)
    p = C.c_void_p(4096)
    assert l.cc_lmhead_put_x(C.byref(ge.cfg), C.byref(shp), p, None, None) == -1
    assert l.cc_lmhead_put_x(None, C.byref(shp), p, p, None) == -1
    assert l.cc_lmhead_get(C.byref(ge.cfg), C.byref(shp), p, 6, p, 16, None) == -1
    assert l.cc_lmhead_get(C.byref(ge.cfg), C.byref(shp), p, -1, p, 16, None) == -1
    assert l.cc_lmhead_get(C.byref(ge.cfg), C.byref(shp), p, 0, None, 16, None) == -1
    assert l.cc_lmhead_get(C.byref(ge.cfg), C.byref(shp), p, 0, p, 15, None) == -2          # lse: 4 rows of fp32 = 16 bytes
    shp0 = ge.shape(2, 1, 3, 2, 0)
    assert l.cc_lmhead_get(C.byref(ge.cfg), C.byref(shp0), p, 2, p, 16, None) == -4         # a mode-0 pass carves no row_loss
    assert l.cc_lmhead_get(C.byref(ge.cfg), C.byref(shp0), p, 5, p, 16, None) == -4
    assert l.cc_lmhead_get(C.byref(ge.cfg), C.byref(ge.shape(2, 3, 3, 0, 1)), p, 3, p, 16, None) == -2   # T == L: no caption rows
