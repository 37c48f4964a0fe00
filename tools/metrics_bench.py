#!/usr/bin/env python
"""What BLEU and ROUGE-L cost next to CIDEr-D, on one box: each launch alone, and self_critical_step with MetricReward (cider + bleu4)
against the same step with CiderReward alone.

The model, the shape and the references are tools/cider_bench.py's: bench.py's config 2 (TransformerMapper 8 layers, P = L = 10, frozen
GPT-2-small, B = 256, random weights), lr = 0 and the same sampling seed in every step, captions of `--entry-length` words (default 20),
5 references per image built from the model's own greedy caption.  The two rewards alternate inside one process after a warm-up; a step
is timed on the host clock between two device synchronisations.  Each launch alone: device events over `--launches` back-to-back launches
on the step's own (2 B, n) buffer.  Reported: the median of the per-block medians and the spread of the block medians as the same-box
noise.  No threshold is asserted: it is a record.

    python tools/metrics_bench.py [--reps 5] [--blocks 3] [--entry-length 20] [--markdown out.md]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools.cider_bench import SHAPE, STOP, build_model, references, spread  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--entry-length", type=int, default=20)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--markdown", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench.py measures on an MI355X; no GPU found (nothing is estimated on the CPU)")
    from clipcap_amd import engine
    from clipcap_amd.train import CiderReward, MetricReward, self_critical_step
    from tests.cider_cases import pad_refs
    model, embeds = build_model()
    B, entry = SHAPE["B"], args.entry_length
    docs = references(model, embeds, entry)
    arr, count = pad_refs(docs, 5, entry + 1)
    refs_d, count_d = torch.from_numpy(arr).cuda(), torch.from_numpy(count).cuda()
    cider = CiderReward.from_corpus(docs, stop_token=STOP)
    mix = MetricReward({"cider": 1.0, "bleu4": 0.5}, cider=cider, stop_token=STOP)
    arms = {"cider": cider.for_batch(refs_d, count_d), "cider_bleu4": mix.for_batch(refs_d, count_d)}
    last = {}

    def capture(sampled, greedy):
        last.update(sampled=sampled.clone(), greedy=greedy.clone())
        return arms["cider_bleu4"](sampled, greedy)

    def step(fn):
        gen = torch.Generator(device="cuda").manual_seed(7)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = self_critical_step(model, embeds, fn, 0.0, entry_length=entry, stop_token=STOP, generator=gen)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    _, (_, ms_mix, mg_mix) = step(capture)                                                   # warm-up, both arms
    _, (_, ms_cider, mg_cider) = step(arms["cider"])
    med = {k: [] for k in arms}
    for _ in range(args.blocks):
        t = {k: [] for k in arms}
        for _ in range(args.reps):
            for k, fn in arms.items():                                                      # alternating
                t[k].append(step(fn)[0])
        for k in arms:
            med[k].append(statistics.median(t[k]))
    # each launch alone, on the step's own candidates
    n = max(last["sampled"].shape[1], last["greedy"].shape[1])
    cand = torch.full((2 * B, n), -1, dtype=torch.int64, device="cuda")
    cand[:B, :last["sampled"].shape[1]] = last["sampled"]
    cand[B:, :last["greedy"].shape[1]] = last["greedy"]
    kw = dict(stop_token=STOP, ref_count=count_d)
    launches = {"cc_cider_score": lambda: cider.score(cand, refs_d, count_d), "cc_bleu_stats": lambda: engine.bleu_stats(cand, refs_d, **kw),
                "cc_rouge_l": lambda: engine.rouge_l(cand, refs_d, **kw)}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    alone = {}
    for name, fn in launches.items():
        for _ in range(3):
            fn()
        ts = []
        for _ in range(args.blocks):
            a.record()
            for _ in range(args.launches):
                fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e-3 / args.launches)
        alone[name] = ts
    out = dict(shape=SHAPE, entry_length=entry, candidates=2 * B, candidate_width=n, refs_per_image=5, ref_width=entry + 1, blocks=args.blocks,
               reps=args.reps, step_cider_ms=round(statistics.median(med["cider"]) * 1e3, 3), step_cider_spread=round(spread(med["cider"]), 4),
               step_cider_bleu4_ms=round(statistics.median(med["cider_bleu4"]) * 1e3, 3),
               step_cider_bleu4_spread=round(spread(med["cider_bleu4"]), 4),
               launch_alone_us={k: round(statistics.median(v) * 1e6, 2) for k, v in alone.items()},
               launch_alone_spread={k: round(spread(v), 4) for k, v in alone.items()},
               mean_reward_sampled=dict(cider=round(float(ms_cider), 5), cider_bleu4=round(float(ms_mix), 5)),
               mean_reward_greedy=dict(cider=round(float(mg_cider), 5), cider_bleu4=round(float(mg_mix), 5)))
    out["mix_over_cider_step"] = round(out["step_cider_bleu4_ms"] / out["step_cider_ms"], 4)
    print(json.dumps(out), flush=True)
    if args.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(args.markdown)), exist_ok=True)
        rows = "".join(f"| {k} | {out['launch_alone_us'][k]} ({100 * out['launch_alone_spread'][k]:.1f} %) | "
                       f"{100 * out['launch_alone_us'][k] * 1e-3 / out['step_cider_ms']:.3f} % |\n" for k in launches)
        open(args.markdown, "w").write(
            f"self_critical_step at bench.py config 2's shape (B = {B}, frozen GPT-2-small, random weights), entry_length {entry}, {2 * B} candidates x "
            f"{n} positions, 5 references x {entry + 1} positions per image; {args.blocks} blocks x {args.reps} alternating steps; median of block "
            "medians (spread of the block medians).  A launch alone: device events over back-to-back launches (the engine wrapper's output "
            "allocations included).\n\n"
            "| reward | step, ms |\n|---|---|\n"
            f"| CiderReward.for_batch | {out['step_cider_ms']} ({100 * out['step_cider_spread']:.1f} %) |\n"
            f"| MetricReward(cider + 0.5 bleu4).for_batch | {out['step_cider_bleu4_ms']} ({100 * out['step_cider_bleu4_spread']:.1f} %) |\n\n"
            f"mix / cider step time: {out['mix_over_cider_step']}\n\n"
            "| launch alone | us | of the CIDEr-only step |\n|---|---|---|\n" + rows + f"\n```\n{json.dumps(out)}\n```\n")


if __name__ == "__main__":
    main()
