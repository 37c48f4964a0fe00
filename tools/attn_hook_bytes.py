#!/usr/bin/env python3
"""Digest the raw output bytes of the launcher hooks cc_attention_fwd_x / cc_attention_bwd_x over the case list of
tests/test_gpu_attention_ref.py (all three operand builds; the split-bf16 build also with operand-image outputs), to compare two builds
of the library bit for bit.  One library per process, each under its own time limit, nothing more after a failure:

    CLIPCAP_HIP_LIB=<other libclipcap_hip.so> timeout -k 10 170 tools/attn_hook_bytes.py a.json && timeout -k 10 170 tools/attn_hook_bytes.py b.json && cmp a.json b.json
"""
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import attn_ref as R
from tests import test_gpu_attention_ref as T

def h(t):
    return None if t is None else hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()

res = {}
for op in T.OPS:
    for c in list(R.plain_cases()) + list(R.dropout_cases(op)):
        r = T.Run(op, c)
        key = f"{op} {c.id} p={c.p}"
        rc, out, lse = r.fwd()
        res[key + " fwd"] = [rc, h(out), h(lse)]
        if c.bwd:
            rc, g = r.bwd()
            res[key + " bwd"] = [rc, h(g)]
        if op == "x3":
            rc, out, lse = r.fwd(img=r.D)
            res[key + " fwd img"] = [rc, h(out), h(lse)]
            if c.bwd:
                rc, g = r.bwd(img=3 * r.D)
                res[key + " bwd img"] = [rc, h(g)]
json.dump(res, open(sys.argv[1], "w"), indent=0, sort_keys=True)
print(len(res), "records ->", sys.argv[1])
