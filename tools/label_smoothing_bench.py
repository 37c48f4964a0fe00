#!/usr/bin/env python
"""Times label smoothing in the fused lm_head loss on one box: the training step of bench.py's config 2 (frozen GPT-2-small, B = 256) and
config 3 (GPT-2-small full finetune, B = 256, GPT-2 dropout on), with bf16 and with split-bf16 operands, each at eps = 0 and eps = 0.1.

Method: both variants are warmed up first, then ALTERNATE inside one process (0, 0.1, 0, 0.1, ...), each step (zero_grad, forward_backward,
optimizer_step) timed with HIP events; medians of per-block medians are reported, with the spread of ONE variant's per-block medians over
--blocks blocks as the same-box noise figure.  eps = 0 launches exactly what a step launched before the option existed, so it is the line
to hold against the parent commit's step on the same box.  The extra bytes of a smoothed step (computed from the shapes: one read of the V
real rows of wte for the column mean, the row passes over hf / d hf, and in a full finetune the read-modify-write of the V rows of the fp32
wte gradient) are printed beside the measured difference.  One JSON line per (configuration, precision); --markdown writes the table.

    python tools/label_smoothing_bench.py [--reps 10] [--blocks 3] [--configs 2,3] [--precisions bf16,32] [--markdown out.md]
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

VARIANTS = (0.0, 0.1)


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


def extra_bytes(c, precision):
    """bytes a smoothed step moves beyond the plain one, from the shapes"""
    w = 4 if precision == "32" else 2                      # a wte row as it is read; a stored activation
    rows, D, V = c["B"] * c["cap"], c["D"], c["V"]
    n = V * D * w + rows * D * w + 3 * rows * D * w        # column mean; zbar; d hf read + write + the gathered wte rows
    if c["train_lm"]:
        n += 2 * rows * D * w + 2 * V * D * 4              # the scatter's and the row sum's reads of hf; the broadcast's read-modify-write
    return n


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
    n = {"i": 0}

    def step(eps):
        i = n["i"] = n["i"] + 1
        eng.zero_grad()
        loss = eng.forward_backward(tokens, embeds, dropout=(0.1, 0.1, 0.1, 1000003 * i) if c["train_lm"] else None, label_smoothing=eps)
        eng.optimizer_step(1e-6, i)
        return loss

    for _ in range(3):
        for v in VARIANTS:
            step(v)
    torch.cuda.synchronize()
    med = {v: [] for v in VARIANTS}
    for _ in range(blocks):
        t = {v: [] for v in VARIANTS}
        for _ in range(reps):
            for v in VARIANTS:
                t[v].append(timed(lambda: step(v), stream))
        for v in VARIANTS:
            med[v].append(mid(t[v]))
    loss = float(step(0.1))
    out = dict(config=key, name=c["name"], B=c["B"], precision=precision, reps=reps, blocks=blocks, loss_smoothed=loss, nll=float(eng.last_nll),
               step_plain_ms=mid(med[0.0]), step_plain_spread=spread(med[0.0]), step_smooth_ms=mid(med[0.1]), step_smooth_spread=spread(med[0.1]),
               extra_bytes=extra_bytes(c, precision))
    out["extra_ms"] = out["step_smooth_ms"] - out["step_plain_ms"]
    out["ratio"] = out["step_smooth_ms"] / out["step_plain_ms"]
    del me, ge, eng
    torch.cuda.empty_cache()
    return out


def markdown(rows):
    out = ["# Label smoothing in the fused lm_head loss: step time", "",
           "`tools/label_smoothing_bench.py`: eps = 0 and eps = 0.1 alternate in one process, HIP events around a whole step, medians of per-block",
           "medians; spread = (max - min) / median of ONE variant's per-block medians (same-box noise).  Extra bytes: from the shapes.", "",
           "| config | operands | step eps = 0, ms | step eps = 0.1, ms | difference, ms | ratio | spread 0 / 0.1 | extra bytes |",
           "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['config']} ({r['name']}, B = {r['B']}) | {r['precision']} | {r['step_plain_ms']:.3f} | {r['step_smooth_ms']:.3f} | {r['extra_ms']:+.3f} | "
                   f"{r['ratio']:.4f} | {100 * r['step_plain_spread']:.1f} % / {100 * r['step_smooth_spread']:.1f} % | {r['extra_bytes'] / 1e6:.0f} MB |")
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
        raise SystemExit("label_smoothing_bench.py measures on an MI355X; no GPU found (nothing is estimated on the CPU)")
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
