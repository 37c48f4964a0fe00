#!/usr/bin/env python
"""What the sampling truncation rules (cc_logits_truncate: min_p / typical_p / epsilon_cutoff / eta_cutoff) cost at decode time, on one box.

One sampling step at the decode benchmark's step shape (R = 320 rows, V = 50257, ld = Vp = 50304, temperature 0.8, mode-0 top_p 0.9, no
history), with each rule on alone and with all four on.  Four routes per configuration, alternating inside one process after a warm-up:

    step         cc_sample_step_lp alone: the step as it is without the rules
    kernel       engine.truncate_logits alone
    kernel+step  the two launches a decoder makes with the rules on
    torch        the same rules written in torch on the same logits: log_softmax, entropy, a full sort of [R][V], gather, cumsum, masked_fill

Every timed sample runs a route over `--bufs` separate copies of the logits between two device events (truncation works in place, so every
copy is restored from the source before the sample, outside the timed region); the copies together exceed the Infinity Cache, so a route's
first pass over a row comes from HBM — a decode step, whose lm_head has just written the logits, is no worse off.  Reported: the median of
the per-block medians per launch, the spread of the block medians as the same-box noise, the tokens the kernel and the torch route decide
differently (fp32 torch against the kernel's fp64 statistics: a handful at the thresholds), and the bytes the kernel's passes move.
No threshold is asserted: it is a record.

    python tools/truncate_bench.py [--reps 10] [--blocks 3] [--bufs 6] [--markdown out.md]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

R, V, VP, TEMP, TOP_P = 320, 50257, 50304, 0.8, 0.9
CONFIGS = {"min_p": dict(min_p=0.05), "typical_p": dict(typical_p=0.9), "epsilon_cutoff": dict(epsilon_cutoff=3e-4),
           "eta_cutoff": dict(eta_cutoff=6e-4), "all four": dict(min_p=0.05, typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=6e-4)}
# row sweeps of the kernel: maximum, [sums], [typical: 4], [typical and a threshold rule: 1], the write sweep
PASSES = {"min_p": 2, "typical_p": 7, "epsilon_cutoff": 3, "eta_cutoff": 3, "all four": 8}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def spread(v):
    return (max(v) - min(v)) / statistics.median(v) if len(v) > 1 else 0.0


def torch_rules(x, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0):
    """the rules of include/clipcap_hip.h cc_logits_truncate in torch, in place on fp32 x (R, V); no history"""
    v = x * (1.0 / TEMP)
    lp = torch.log_softmax(v, -1)
    p = lp.exp()
    keep = torch.ones_like(x, dtype=torch.bool)
    if min_p > 0:
        keep &= p >= min_p * p.max(-1, keepdim=True).values
    if epsilon_cutoff > 0:
        keep &= p >= epsilon_cutoff
    if eta_cutoff > 0 or typical_p < 1:
        H = -torch.nansum(p * lp, -1, keepdim=True)
    if eta_cutoff > 0:
        keep &= p >= torch.clamp(math.sqrt(eta_cutoff) * torch.exp(-H), max=eta_cutoff)
    if typical_p < 1:
        d = (-lp - H).abs()
        sd, si = torch.sort(d, -1)
        cum = p.gather(-1, si).cumsum(-1)
        last = (cum < typical_p).sum(-1, keepdim=True).clamp_(max=x.shape[1] - 1)
        keep &= d <= sd.gather(-1, last)
    keep |= ~keep.any(-1, keepdim=True) & (v == v.max(-1, keepdim=True).values)
    return x.masked_fill_(~keep, float("-inf"))


def measure(name, opts, src, bufs, u, reps, blocks):
    from clipcap_amd.engine import sample_step, truncate_logits
    views = [b[:, :V] for b in bufs]
    step = lambda x: sample_step(x, u, temperature=TEMP, top_p=TOP_P, mode=0)  # noqa: E731
    routes = {"step": lambda x: step(x), "kernel": lambda x: truncate_logits(x, temperature=TEMP, **opts),
              "kernel+step": lambda x: step(truncate_logits(x, temperature=TEMP, **opts)), "torch": lambda x: torch_rules(x, **opts)}

    def restore():
        for b in bufs:
            b.copy_(src)

    restore()
    a = torch.isfinite(truncate_logits(views[0], temperature=TEMP, **opts))
    b = torch.isfinite(torch_rules(views[1], **opts))
    differ, kept = int((a != b).sum()), int(a.sum())
    for fn in routes.values():                                   # warm-up
        restore()
        for x in views:
            fn(x)
    med = {k: [] for k in routes}
    for _ in range(blocks):
        t = {k: [] for k in routes}
        for _ in range(reps):
            for k, fn in routes.items():                         # alternating
                restore()
                t[k].append(timed(lambda: [fn(x) for x in views]) / len(views))
        for k in routes:
            med[k].append(statistics.median(t[k]))
    out = dict(config=name, options=opts, kept_per_row=round(kept / R, 1), tokens_decided_differently_by_torch=differ, passes=PASSES[name],
               bytes_swept=PASSES[name] * R * V * 4)
    for k in routes:
        out[f"{k}_us"], out[f"{k}_spread"] = round(statistics.median(med[k]) * 1e6, 2), round(spread(med[k]), 4)
    out["torch_over_kernel"] = round(out["torch_us"] / out["kernel_us"], 2)
    out["kernel+step_over_step"] = round(out["kernel+step_us"] / out["step_us"], 3)
    return out


def markdown(rows, args):
    head = [f"R = {R}, V = {V}, ld = {VP}, temperature {TEMP}, mode-0 top_p {TOP_P}, gaussian logits x 3, no history; {args.blocks} blocks x {args.reps} "
            f"alternating samples over {args.bufs} copies of the logits; time per launch, median of block medians (spread of the block medians).", "",
            "| rules on | kept per row | step alone, us | kernel alone, us | kernel + step, us | torch rules alone, us | torch / kernel | "
            "(kernel + step) / step | row sweeps, MB swept | tokens torch decides differently |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        head.append(f"| {r['config']} {r['options']} | {r['kept_per_row']} | {r['step_us']} ({100 * r['step_spread']:.1f} %) | {r['kernel_us']} "
                    f"({100 * r['kernel_spread']:.1f} %) | {r['kernel+step_us']} ({100 * r['kernel+step_spread']:.1f} %) | {r['torch_us']} "
                    f"({100 * r['torch_spread']:.1f} %) | {r['torch_over_kernel']} | {r['kernel+step_over_step']} | {r['passes']}, "
                    f"{r['bytes_swept'] / 1e6:.0f} | {r['tokens_decided_differently_by_torch']} of {R * V} |")
    return "\n".join(head + [""])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--bufs", type=int, default=6)
    ap.add_argument("--markdown", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("truncate_bench.py measures on an MI355X; no GPU found (nothing is estimated on the CPU)")
    gen = torch.Generator(device="cuda").manual_seed(11)
    src = torch.randn(R, VP, device="cuda", generator=gen) * 3.0
    bufs = [src.clone() for _ in range(args.bufs)]
    u = torch.rand(R, device="cuda", generator=gen)
    rows = []
    for name, opts in CONFIGS.items():
        rows.append(measure(name, opts, src, bufs, u, args.reps, args.blocks))
        print(json.dumps(rows[-1]), flush=True)
    if args.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(args.markdown)), exist_ok=True)
        open(args.markdown, "w").write(markdown(rows, args))


if __name__ == "__main__":
    main()
