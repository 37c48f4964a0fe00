#!/usr/bin/env python3
"""Digest the raw output bytes of the decoders' selection steps over seeded cases, to compare two builds of the library bit for bit.

  * the beam update, cc_beam_step_p with and without the lm_head partials (k_beam_fused, and the k_beam_rowstats / k_beam_partial /
    k_beam_final chain): beam widths 1-8, V 130 / 1001 / 4099 / 50257, padded and unpadded rows, temperature 1 and 0.9, a first step and
    later steps with stopped beams, and the plateau case of tests/test_gpu_beam.py;
  * the same inputs through cc_beam_group_step (k_beam_group_partial / k_beam_group_final) wherever the beam divides: 1, 2 and `beam` beam
    groups, penalties 0 and 0.7; the plateau case (beam 5) through 1 and 5 beam groups, and all logits equal (the insertion-list overflow
    path) at beam 4 through 2 beam groups;
  * cc_contrastive_topk at the shapes of tests/test_gpu_contrastive.py, k 1-8, the first row and a selected row.

One library per process, each under its own time limit, nothing more after a failure:

    CLIPCAP_HIP_LIB=<other libclipcap_hip.so> timeout -k 10 400 tools/beam_step_bytes.py a.json && timeout -k 10 400 tools/beam_step_bytes.py b.json && cmp a.json b.json
"""
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clipcap_amd.engine import beam_group_step, beam_step, contrastive_topk
from tests import test_gpu_beam as T
from tests import test_gpu_contrastive as TC


def h(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def record(res, key, lg, S, beam, temp, first, stop, scores, seql, stopped, partials=False, groups=0, penalty=0.0):
    """groups = 0: cc_beam_step_p; else cc_beam_group_step with that many beam groups"""
    if groups:
        nt, sr = beam_group_step(lg, S, beam, groups, temp, penalty, first, stop, scores, seql, stopped)
    else:
        nt, sr = beam_step(lg, S, beam, temp, first, stop, scores, seql, stopped, None, T._partials(lg, lg.shape[1]) if partials else None)
    torch.cuda.synchronize()
    res[key] = [h(nt), h(sr), h(scores), h(seql), h(stopped)]


def state(R):
    return torch.zeros(R, device="cuda"), torch.ones(R, device="cuda"), torch.zeros(R, dtype=torch.uint8, device="cuda")


res = {}
S, stop = 3, 17
for beam in range(1, 9):
    for V, lds in ((130, (130, 136)), (1001, (1001, 1008)), (4099, (4099, 4104)), (50257, (50257, 50304))):
        for ld in lds:
            g = torch.Generator().manual_seed(beam * 100003 + V * 7 + ld)
            R = S * beam
            bufs = []
            for step in range(3):
                buf = (torch.randn(R, ld, generator=g) * 3.0).cuda()
                if step >= 1:
                    buf[::3, stop] += 25.0                 # some beams pick the stop token and freeze
                bufs.append(buf)
            for temp in (1.0, 0.9):
                for partials in (False, True):
                    st = state(R)
                    for step, buf in enumerate(bufs):
                        record(res, f"beam={beam} V={V} ld={ld} temp={temp} partials={partials} step={step}", buf[:, :V], S, beam, temp, step == 0,
                               stop, *st, partials=partials)
                for groups in sorted({G for G in (1, 2, beam) if beam % G == 0}):
                    for penalty in (0.0, 0.7):
                        st = state(R)
                        for step, buf in enumerate(bufs):
                            record(res, f"beam={beam} V={V} ld={ld} temp={temp} groups={groups} penalty={penalty} step={step}", buf[:, :V], S, beam,
                                   temp, step == 0, stop, *st, groups=groups, penalty=penalty)
for first in (True, False):
    for temp, partials in ((0.9, False), (1.0, True), (1.0, False)):
        buf, scores, seql, stopped = T._plateau_case(first)
        record(res, f"plateau first={first} temp={temp} partials={partials}", buf.cuda()[:, :T.PL_V], T.PL_S, T.PL_BEAM, temp, first, T.PL_STOP,
               scores.cuda(), seql.cuda(), stopped.to(torch.uint8).cuda(), partials=partials)
    for groups in (1, T.PL_BEAM):           # PL_BEAM = 5 has no 2 beam groups: the plateau case goes through 1 and 5, and ...
        for penalty in (0.0, 0.7):
            buf, scores, seql, stopped = T._plateau_case(first)
            record(res, f"plateau first={first} groups={groups} penalty={penalty}", buf.cuda()[:, :T.PL_V], T.PL_S, T.PL_BEAM, 0.9, first, T.PL_STOP,
                   scores.cuda(), seql.cuda(), stopped.to(torch.uint8).cuda(), groups=groups, penalty=penalty)
for penalty in (0.0, 1.0):      # ... all logits equal at GPT-2's vocabulary, beam 4, through 2: a first and a later step on the same state
    lg, st = torch.zeros(2 * 4, 50257, device="cuda"), state(2 * 4)
    for first in (True, False):
        record(res, f"all-equal groups=2 penalty={penalty} first={first}", lg, 2, 4, 1.0, first, 50256, *st, groups=2, penalty=penalty)
for V, ld in TC.TOPK_SHAPES:
    for k in range(1, 9):
        for rows_per in sorted({1, max(k, 2)}):
            g = torch.Generator().manual_seed(V * 10 + k + rows_per)
            lg = (torch.randn(TC.S * rows_per, ld, generator=g) * 3.0).cuda()
            sel = None if rows_per == 1 else torch.tensor([(2 * s + 1) % rows_per for s in range(TC.S)], dtype=torch.int32, device="cuda")
            tok = torch.full((TC.S * k,), -7, dtype=torch.int32, device="cuda")
            prob = torch.full((TC.S * k,), -7.0, device="cuda")
            contrastive_topk(lg[:, :V], TC.S, rows_per, sel, k, None, tok, prob)
            torch.cuda.synchronize()
            res[f"topk V={V} ld={ld} k={k} rows_per={rows_per}"] = [h(tok), h(prob)]
json.dump(res, open(sys.argv[1], "w"), indent=0, sort_keys=True)
print(len(res), "records ->", sys.argv[1])
