#!/usr/bin/env python
"""Times the weight average inside the AdamW step on one box: the training step of bench.py's config 2 (frozen GPT-2-small, B = 256) and
config 3 (GPT-2-small full finetune, B = 256, GPT-2 dropout on), with bf16 and with split-bf16 operands, in three variants:

    plain   ema_decay = None: exactly what a step launched before the option existed (the line to hold against the parent commit)
    fused   ema_decay = 0.999: the average updated inside the AdamW launch (cc_adamw_step_ema)
    lerp    the unfused alternative: the plain step, then torch's ``ema.lerp_(w32, 1 - d)`` over every trained arena

Method: all variants are warmed up first, then ALTERNATE inside one process (plain, fused, lerp, plain, ...), each step (zero_grad,
forward_backward, optimizer_step [, lerp_]) timed with HIP events; medians of per-block medians are reported, with the spread of ONE
variant's per-block medians over --blocks blocks as the same-box noise figure.  The optimizer step alone (the AdamW launches and the
operand-copy refresh, on gradients left in place) is timed the same way, because the whole step's noise is larger than the effect.
Beside the times: the bytes the averaged step adds (8 B x trained parameters: 4 read + 4 written; the separate pass moves 12 B) and the
AdamW kernel's 28 B per parameter, from which the expectation 8 / 28 of the kernel's time follows.  One JSON line per (configuration,
precision); --markdown writes the table.

    python tools/ema_bench.py [--reps 10] [--blocks 3] [--configs 2,3] [--precisions bf16,32] [--markdown out.md]
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

DECAY = 0.999
VARIANTS = ("plain", "fused", "lerp")


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


def alternate(fns, reps, blocks, stream):
    """{variant: per-block medians} of the callables, alternating inside every repetition"""
    med = {v: [] for v in fns}
    for _ in range(blocks):
        t = {v: [] for v in fns}
        for _ in range(reps):
            for v, fn in fns.items():
                t[v].append(timed(fn, stream))
        for v in fns:
            med[v].append(mid(t[v]))
    return med


def run(key, precision, reps, blocks):
    device = torch.device("cuda", 0)
    c = dict(CONFIGS[key])
    me, ge, eng = init_engines(c, device)
    if precision != "bf16":
        me.set_precision(int(precision))
        ge.set_precision(int(precision))
    gen = torch.Generator(device=device).manual_seed(4321)
    embeds = torch.randn(c["B"], c["E"], generator=gen, device=device)
    tokens = torch.randint(1, c["V"], (c["B"], c["cap"]), generator=gen, device=device)
    stream = torch.cuda.current_stream()
    arenas = eng.arenas()
    for a in arenas:
        a.enable_ema()
    n = {"i": 0}

    def optimizer(variant):
        i = n["i"] = n["i"] + 1
        eng.optimizer_step(1e-6, i, **({"ema_decay": DECAY} if variant == "fused" else {}))
        if variant == "lerp":
            for a in arenas:
                a.ema.lerp_(a.w32, 1.0 - DECAY)

    def step(variant):
        eng.zero_grad()
        loss = eng.forward_backward(tokens, embeds, dropout=(0.1, 0.1, 0.1, 1000003 * (n["i"] + 1)) if c["train_lm"] else None)
        optimizer(variant)
        return loss

    for _ in range(3):
        for v in VARIANTS:
            step(v)
    torch.cuda.synchronize()
    whole = alternate({v: (lambda v=v: step(v)) for v in VARIANTS}, reps, blocks, stream)
    opt = alternate({v: (lambda v=v: optimizer(v)) for v in VARIANTS}, reps, blocks, stream)
    loss = float(step("fused"))
    trained = sum(a.n for a in arenas)
    out = dict(config=key, name=c["name"], B=c["B"], precision=precision, reps=reps, blocks=blocks, loss=loss, trained_params=trained,
               extra_bytes_fused=8 * trained, extra_bytes_lerp=12 * trained, adamw_bytes=28 * trained)
    for v in VARIANTS:
        out[f"step_{v}_ms"], out[f"step_{v}_spread"] = mid(whole[v]), spread(whole[v])
        out[f"opt_{v}_ms"], out[f"opt_{v}_spread"] = mid(opt[v]), spread(opt[v])
    out["fused_extra_ms"] = out["opt_fused_ms"] - out["opt_plain_ms"]
    out["lerp_extra_ms"] = out["opt_lerp_ms"] - out["opt_plain_ms"]
    out["step_ratio_fused"] = out["step_fused_ms"] / out["step_plain_ms"]
    out["step_ratio_lerp"] = out["step_lerp_ms"] / out["step_plain_ms"]
    del me, ge, eng
    torch.cuda.empty_cache()
    return out


def markdown(rows):
    out = ["# Weight average inside the AdamW step: step time", "",
           "`tools/ema_bench.py`: plain (no average), fused (ema_decay = 0.999 inside the AdamW launch) and lerp (plain step + `torch.lerp_` per arena)",
           "alternate in one process, HIP events around a whole step and around the optimizer step alone, medians of per-block medians;",
           "spread = (max - min) / median of the plain variant's per-block medians (same-box noise).  Extra bytes: 8 B (fused) / 12 B (lerp) x trained parameters.", "",
           "| config | operands | trained | step plain / fused / lerp, ms | step spread | optimizer plain / fused / lerp, ms | fused - plain, ms | lerp - plain, ms | extra bytes fused / lerp |",
           "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['config']} ({r['name']}, B = {r['B']}) | {r['precision']} | {r['trained_params'] / 1e6:.1f} M | {r['step_plain_ms']:.3f} / {r['step_fused_ms']:.3f} / "
                   f"{r['step_lerp_ms']:.3f} | {100 * r['step_plain_spread']:.1f} % | {r['opt_plain_ms']:.3f} / {r['opt_fused_ms']:.3f} / {r['opt_lerp_ms']:.3f} | "
                   f"{r['fused_extra_ms']:+.3f} | {r['lerp_extra_ms']:+.3f} | {r['extra_bytes_fused'] / 1e6:.0f} / {r['extra_bytes_lerp'] / 1e6:.0f} MB |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10, help="alternating repetitions per block")
    ap.add_argument("--blocks", type=int, default=3, help="blocks (their medians give the same-box spread)")
    ap.add_argument("--configs", default="2,3")
    ap.add_argument("--precisions", default="bf16,32")
    ap.add_argument("--markdown", default="", help="also write the table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ema_bench.py measures on an MI355X; no GPU found (nothing is estimated on the CPU)")
    rows = []
    for key in args.configs.split(","):
        for prec in args.precisions.split(","):
            rows.append(run(key.strip(), prec.strip(), args.reps, args.blocks))
            print(json.dumps(rows[-1]), flush=True)
    if args.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(args.markdown)), exist_ok=True)
        open(args.markdown, "w").write(markdown(rows))


if __name__ == "__main__":
    main()
