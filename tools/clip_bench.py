#!/usr/bin/env python
"""Times global gradient-norm clipping on one box:

  (a) the training step of bench.py's config 2 (frozen GPT-2-small, B = 256) and config 4 (GPT-2-medium full finetune, B = 128, GPT-2
      dropout on), each with clipping off, at max_grad_norm = inf (report only) and at a finite value;
  (b) the cc_grad_sqnorm launches alone (partials + fold) over each configuration's trained arenas, against the bytes they read.

Method: every variant is warmed up first; the three variants ALTERNATE inside one process (off, inf, finite, off, ...), each step timed
with HIP events; medians are reported, with the spread of the per-block medians of ONE variant over --blocks blocks as the same-box noise
figure.  The "off" variant launches exactly what a step launched before clipping existed, so it is the line to hold against the parent
commit's step on the same box.  Prints one JSON line per configuration and, with --markdown, the table for profiles/.

    python tools/clip_bench.py [--reps 10] [--blocks 3] [--configs 2,4] [--clip 1.0] [--markdown out.md]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bench import CONFIGS, init_engines  # noqa: E402
from clipcap_amd.engine import GradClipper  # noqa: E402

VARIANTS = ("off", "inf", "finite")


def timed(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def mid(v):
    return statistics.median(v)


def spread(v):
    return (max(v) - min(v)) / mid(v) if len(v) > 1 else 0.0


def run(key, reps, blocks, clip):
    device = torch.device("cuda", 0)
    c = dict(CONFIGS[key])
    me, ge, eng = init_engines(c, device)
    gen = torch.Generator(device=device).manual_seed(4321)
    embeds = torch.randn(c["B"], c["E"], generator=gen, device=device)
    tokens = torch.randint(1, c["V"], (c["B"], c["cap"]), generator=gen, device=device)
    stream = torch.cuda.current_stream()
    n = {"i": 0}
    kw = {"off": {}, "inf": {"max_grad_norm": float("inf")}, "finite": {"max_grad_norm": clip}}

    def step(variant):
        i = n["i"] = n["i"] + 1
        eng.zero_grad()
        eng.forward_backward(tokens, embeds, dropout=(0.1, 0.1, 0.1, 1000003 * i) if c["train_lm"] else None)
        eng.optimizer_step(1e-6, i, **kw[variant])

    for _ in range(2):
        for v in VARIANTS:
            step(v)
    torch.cuda.synchronize()
    norm = float(eng.last_grad_norm)
    med = {v: [] for v in VARIANTS}
    for _ in range(blocks):
        t = {v: [] for v in VARIANTS}
        for _ in range(reps):
            for v in VARIANTS:
                t[v].append(timed(lambda: step(v), stream))
        for v in VARIANTS:
            med[v].append(mid(t[v]))

    # (b) the norm pass alone: cc_grad_sqnorm over every trained arena (two launches each) + the zeroing of sumsq
    cl = GradClipper(device, float("inf"))
    arenas = eng.arenas()
    nbytes = 4 * sum(a.n for a in arenas)

    def norm_pass():
        cl.begin()
        for a in arenas:
            cl.add(a)

    for _ in range(5):
        norm_pass()
    nm = []
    for _ in range(blocks):
        nm.append(mid([timed(norm_pass, stream) for _ in range(max(5, reps))]))
    out = dict(config=key, name=c["name"], B=c["B"], trained_params=sum(a.n for a in arenas), reps=reps, blocks=blocks, clip=clip, grad_norm=norm,
               norm_pass_ms=mid(nm), norm_pass_spread=spread(nm), norm_pass_bytes=nbytes, norm_pass_TBps=nbytes / (mid(nm) * 1e-3) / 1e12)
    for v in VARIANTS:
        out[f"step_{v}_ms"] = mid(med[v])
        out[f"step_{v}_spread"] = spread(med[v])
    del me, ge, eng, cl
    torch.cuda.empty_cache()
    return out


def markdown(rows):
    out = ["# Global gradient-norm clipping: step time and the norm pass alone", "",
           "`tools/clip_bench.py`: the three variants of a step alternate in one process, HIP events, medians of per-block medians; spread =",
           "(max - min) / median of the per-block medians of ONE variant (same-box noise).  off = no clipping (the launches of a step before",
           "clipping existed), inf = report the norm only, finite = clip to the given norm.  The norm pass = cc_grad_sqnorm over every trained",
           "arena (partials + fold launches) and the zeroing of sumsq, against the gradient bytes it reads.", "",
           "| config | trained parameters | step off, ms | step inf, ms | step finite, ms | inf / off | finite / off | spread off / inf / finite | norm pass, ms | bytes read | TB/s | spread | grad norm |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['config']} ({r['name']}, B = {r['B']}) | {r['trained_params'] / 1e6:.1f} M | {r['step_off_ms']:.3f} | {r['step_inf_ms']:.3f} | "
                   f"{r['step_finite_ms']:.3f} | {r['step_inf_ms'] / r['step_off_ms']:.4f} | {r['step_finite_ms'] / r['step_off_ms']:.4f} | "
                   f"{100 * r['step_off_spread']:.1f} % / {100 * r['step_inf_spread']:.1f} % / {100 * r['step_finite_spread']:.1f} % | {r['norm_pass_ms']:.4f} | "
                   f"{r['norm_pass_bytes'] / 1e6:.1f} MB | {r['norm_pass_TBps']:.2f} | {100 * r['norm_pass_spread']:.1f} % | {r['grad_norm']:.4g} (clip at {r['clip']:g}) |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10, help="alternating repetitions per block")
    ap.add_argument("--blocks", type=int, default=3, help="blocks (their medians give the same-box spread)")
    ap.add_argument("--configs", default="2,4")
    ap.add_argument("--clip", type=float, default=1.0, help="max_grad_norm of the finite variant")
    ap.add_argument("--markdown", default="", help="also write the table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_bench.py measures on an MI355X; no GPU found (nothing is estimated on the CPU)")
    rows = []
    for key in args.configs.split(","):
        rows.append(run(key.strip(), args.reps, args.blocks, args.clip))
        print(json.dumps(rows[-1]), flush=True)
    if args.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(args.markdown)), exist_ok=True)
        open(args.markdown, "w").write(markdown(rows))


if __name__ == "__main__":
    main()
