#!/usr/bin/env python3
"""Record what the library's host-only size, offset and refusal paths return, as tests/golden/host_layout.json.

    tools/record_host_layout.py [--lib clipcap_amd/libclipcap_hip.so] [--lab clipcap_amd/libclipcap_hip_lab.so] [--out tests/golden/host_layout.json]

Run it on the build whose answers are to be kept (the commit BEFORE a change to the arena layouts, the workspace carvers or the config
checks); tests/test_host_layout.py then asserts that the current build returns every recorded value.  Nothing here touches a GPU: the
size / offset functions are pure host arithmetic, and every refused call returns before the first HIP call.

A record is {"lib": "product" | "lab", "fn", "cfg": {...}, "args": [...], "ret"} (+ "offsets" for the *_param_offsets calls).  `args` are the
arguments after the config: integers, "PTR" / "PTR2" for two distinct non-null dummy pointers that no recorded call dereferences, null for
NULL, and a dict for a cc_gpt2_shape.
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clipcap_amd._lib import Gpt2Cfg, Gpt2Shape, LAB_SIGNATURES, MapperCfg, SIGNATURES  # noqa: E402

MAPPERS = {
    "tiny": dict(E=64, D=128, P=4, L=4, H=4, N=2, Hm=256, W=1, use_pos=0),
    "tiny_windowed": dict(E=64, D=128, P=4, L=4, H=4, N=2, Hm=256, W=3, use_pos=1),
    "d768_n8": dict(E=512, D=768, P=10, L=10, H=8, N=8, Hm=1536, W=1, use_pos=0),
    "d768_n8_windowed_pos": dict(E=512, D=768, P=10, L=10, H=8, N=8, Hm=1536, W=5, use_pos=1),
    "d768_n8_windowed_nopos": dict(E=512, D=768, P=10, L=10, H=8, N=8, Hm=1536, W=5, use_pos=0),
}
GPT2S = {
    "tiny": dict(D=128, H=4, NL=2, V=300, Vp=384, NPOS=32),
    "tiny_hd64": dict(D=128, H=2, NL=2, V=300, Vp=384, NPOS=32),
    "small": dict(D=768, H=12, NL=12, V=50257, Vp=50304, NPOS=1024),
    "medium": dict(D=1024, H=16, NL=24, V=50257, Vp=50304, NPOS=1024),
}
BATCHES = (1, 256, 4096)          # 4096 x 20 rows crosses the mapper's deferred-weight-gradient row limit
# refused somewhere: (name, overrides of GPT-2 small, does the DECODE side refuse it too?)
GPT2_REFUSED = (("NL=97", dict(NL=97), False), ("NPOS=0", dict(NPOS=0), False), ("D%8", dict(D=772, H=1), True), ("Vp%128", dict(Vp=50264), True))


def load(path, lab):
    lib = C.CDLL(path)
    for name, (res, args) in (dict(SIGNATURES, **LAB_SIGNATURES) if lab else SIGNATURES).items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def call(lib, fn, cfg, args):
    """one recorded call: cfg dict -> struct by the function's first argument type; "PTR" -> a dummy buffer, a dict -> cc_gpt2_shape"""
    f = getattr(lib, fn)
    c = (MapperCfg if f.argtypes[0]._type_ is MapperCfg else Gpt2Cfg)(**cfg)
    buf, buf2 = C.create_string_buffer(256), C.create_string_buffer(256)
    conv = [C.byref(Gpt2Shape(a["B"], a["L"], a["T"], a["cap"], a["mode"], 0.0, 0.0, 0.0, 0)) if isinstance(a, dict) else
            C.cast(buf, C.c_void_p) if a == "PTR" else C.cast(buf2, C.c_void_p) if a == "PTR2" else a for a in args]
    return int(f(C.byref(c), *conv))


def offsets(lib, fn, cfg, n):
    f = getattr(lib, fn)
    c = (MapperCfg if f.argtypes[0]._type_ is MapperCfg else Gpt2Cfg)(**cfg)
    out = (C.c_int64 * n)()
    return int(f(C.byref(c), out)), list(out)


def collect(lib, lab):
    recs = []

    def rec(which, fn, cfg, args):
        recs.append({"lib": which, "fn": fn, "cfg": cfg, "args": args, "ret": call(lab if which == "lab" else lib, fn, cfg, args)})

    def rec_offsets(fn, cfg, n):
        ret, offs = offsets(lib, fn, cfg, n)
        recs.append({"lib": "product", "fn": fn, "cfg": cfg, "args": [], "ret": ret, "offsets": offs})

    P = "PTR"
    shape = dict(B=4, L=4, T=12, cap=8, mode=1)
    for op in (0, 1, 2):
        for m in MAPPERS.values():
            cfg = dict(m, op_dtype=op)
            rec("product", "cc_mapper_param_count", cfg, [])
            rec_offsets("cc_mapper_param_offsets", cfg, 4 + 12 * m["N"])
            for B in BATCHES:
                for save in (0, 1):
                    rec("product", "cc_mapper_ws_bytes", cfg, [B, save])
        for g in GPT2S.values():
            cfg = dict(g, op_dtype=op)
            rec("product", "cc_gpt2_param_count", cfg, [])
            rec_offsets("cc_gpt2_param_offsets", cfg, 4 + 12 * g["NL"])
            for R in BATCHES:
                for Tn in (1, 10):
                    rec("product", "cc_decode_ws_bytes", cfg, [R, Tn])
                rec("product", "cc_decode_part_floats", cfg, [R])
            rec("lab", "cc_decode_image_bytes", cfg, [])
            rec("lab", "cc_decode_xt_image_bytes", cfg, [])
        # ---- refused configs: the status of every entry-point family, each call returning before any HIP call
        for _, over, decode_refuses in GPT2_REFUSED:
            cfg = dict(GPT2S["small"], op_dtype=op, **over)
            rec("product", "cc_gpt2_param_count", cfg, [])
            rec_offsets("cc_gpt2_param_offsets", cfg, 4 + 12 * 97)
            rec("product", "cc_gpt2_ws_bytes", cfg, [shape])
            rec("product", "cc_gpt2_sync_weights", cfg, [P, P, None])
            rec("product", "cc_gpt2_transpose_weights", cfg, [P, None])
            rec("product", "cc_gpt2_embed", cfg, [shape, P, P, P, P, None])
            rec("product", "cc_gpt2_fwd", cfg, [shape, P, P, P, None])
            rec("product", "cc_gpt2_logits", cfg, [shape, P, P, P, P, 50304, None])
            rec("product", "cc_lmhead_ce_fwd", cfg, [shape, P, P, P, P, P, None])
            rec("product", "cc_lmhead_ce_bwd", cfg, [shape, P, P, P, P, P, P, None])
            rec("product", "cc_gpt2_bwd", cfg, [shape, P, P, P, P, P, P, None])
            rec("product", "cc_gpt2_bwd_range", cfg, [shape, P, P, P, P, P, P, 1, 0, None])
            # decode side: the host-only entry points for every config, the launching ones only where the decode side refuses too
            rec("product", "cc_decode_ws_bytes", cfg, [5, 1])
            rec("product", "cc_decode_ws_bytes", cfg, [5, 10])
            rec("product", "cc_decode_part_floats", cfg, [5])
            rec("product", "cc_embed_tokens_bwd_ws_bytes", cfg, [5])
            rec("product", "cc_decode_reorder", cfg, [1, 1, 0, 1, P, "PTR2", P, None])      # ctx = 0: CC_OK without a launch where the config is accepted
            rec("lab", "cc_decode_image_bytes", cfg, [])
            rec("lab", "cc_decode_xt_image_bytes", cfg, [])
            if decode_refuses:
                rec("product", "cc_decode_fwd", cfg, [5, 1, 0, 16, P, P, P, P, None, P, P, 50304, None])
                rec("product", "cc_embed_tokens", cfg, [5, P, P, P, None])
                rec("product", "cc_beam_advance", cfg, [5, 5, P, P, P, 0, 16, None, None, 0, 1, None, None, P, None])
                rec("lab", "cc_decode_image", cfg, [P, P, None])
                rec("lab", "cc_decode_xt_image", cfg, [P, P, None])
        cfg = dict(MAPPERS["d768_n8"], op_dtype=op, N=97)
        rec("product", "cc_mapper_param_count", cfg, [])
        rec_offsets("cc_mapper_param_offsets", cfg, 4 + 12 * 97)
        rec("product", "cc_mapper_ws_bytes", cfg, [4, 1])
        rec("product", "cc_mapper_sync_weights", cfg, [P, P, None])
        rec("product", "cc_mapper_fwd", cfg, [4, P, P, P, P, P, 1, None])
        rec("product", "cc_mapper_bwd", cfg, [4, P, P, P, P, P, None])
        rec("product", "cc_mapper_bwd_range", cfg, [4, P, P, P, P, P, 1, 0, None])
        # R <= 0 / B <= 0 on valid configs
        small, mp = dict(GPT2S["small"], op_dtype=op), dict(MAPPERS["d768_n8"], op_dtype=op)
        for R in (0, -3):
            rec("product", "cc_decode_ws_bytes", small, [R, 1])
            rec("product", "cc_decode_part_floats", small, [R])
            rec("product", "cc_embed_tokens_bwd_ws_bytes", small, [R])
            rec("product", "cc_decode_fwd", small, [R, 1, 0, 16, P, P, P, P, None, P, P, 50304, None])
            rec("product", "cc_embed_tokens", small, [R, P, P, P, None])
            rec("product", "cc_mapper_ws_bytes", mp, [R, 1])
            rec("product", "cc_mapper_fwd", mp, [R, P, P, P, P, P, 1, None])
        rec("product", "cc_decode_ws_bytes", small, [5, 0])
    return recs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", default=os.path.join(ROOT, "clipcap_amd", "libclipcap_hip.so"))
    ap.add_argument("--lab", default=os.path.join(ROOT, "clipcap_amd", "libclipcap_hip_lab.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "host_layout.json"))
    a = ap.parse_args()
    recs = collect(load(a.lib, False), load(a.lab, True))
    with open(a.out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in recs) + "\n]\n")
    print(f"{a.out}: {len(recs)} records")


if __name__ == "__main__":
    main()
