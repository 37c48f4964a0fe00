#!/usr/bin/env python3
"""Digest the raw output bytes of the beam update (cc_beam_step_p with and without the lm_head partials: k_beam_fused, and the
k_beam_rowstats / k_beam_partial / k_beam_final chain) over seeded cases, to compare two builds of the library bit for bit: beam widths
1-8, V 130 / 1001 / 4099 / 50257, padded and unpadded rows, temperature 1 and 0.9, a first step and later steps with stopped beams,
and the plateau case of tests/test_gpu_beam.py.  One library per process, each under its own time limit, nothing more after a failure:

    CLIPCAP_HIP_LIB=<other libclipcap_hip.so> timeout -k 10 170 tools/beam_step_bytes.py a.json && timeout -k 10 170 tools/beam_step_bytes.py b.json && cmp a.json b.json
"""
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clipcap_amd.engine import beam_step
from tests import test_gpu_beam as T


def h(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def record(res, key, lg, S, beam, temp, first, stop, scores, seql, stopped, partials):
    nt, sr = beam_step(lg, S, beam, temp, first, stop, scores, seql, stopped, None, T._partials(lg, lg.shape[1]) if partials else None)
    torch.cuda.synchronize()
    res[key] = [h(nt), h(sr), h(scores), h(seql), h(stopped)]


res = {}
S, stop = 3, 17
for beam in range(1, 9):
    for V, lds in ((130, (130, 136)), (1001, (1001, 1008)), (4099, (4099, 4104)), (50257, (50257, 50304))):
        for ld in lds:
            for temp in (1.0, 0.9):
                for partials in (False, True):
                    g = torch.Generator().manual_seed(beam * 100003 + V * 7 + ld)
                    R = S * beam
                    scores = torch.zeros(R, device="cuda")
                    seql = torch.ones(R, device="cuda")
                    stopped = torch.zeros(R, dtype=torch.uint8, device="cuda")
                    for step in range(3):
                        buf = (torch.randn(R, ld, generator=g) * 3.0).cuda()
                        if step >= 1:
                            buf[::3, stop] += 25.0                 # some beams pick the stop token and freeze
                        record(res, f"beam={beam} V={V} ld={ld} temp={temp} partials={partials} step={step}", buf[:, :V], S, beam, temp, step == 0,
                               stop, scores, seql, stopped, partials)
for first in (True, False):
    for temp, partials in ((0.9, False), (1.0, True), (1.0, False)):
        buf, scores, seql, stopped = T._plateau_case(first)
        record(res, f"plateau first={first} temp={temp} partials={partials}", buf.cuda()[:, :T.PL_V], T.PL_S, T.PL_BEAM, temp, first, T.PL_STOP,
               scores.cuda(), seql.cuda(), stopped.to(torch.uint8).cuda(), partials)
json.dump(res, open(sys.argv[1], "w"), indent=0, sort_keys=True)
print(len(res), "records ->", sys.argv[1])
