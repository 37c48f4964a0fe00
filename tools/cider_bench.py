#!/usr/bin/env python
"""What the reward costs in a self-critical step, on one box: CiderReward.for_batch (one launch of cc_cider_score, nothing read back)
against a host reward_fn that copies both decodes to the CPU, runs the float64 dict statement tests/cider_ref.py over the 2 B captions
and hands two vectors back.

The step is clipcap_amd.train.self_critical_step at the shape of bench.py's config 2 (TransformerMapper 8 layers, P = L = 10, frozen
GPT-2-small, B = 256, random weights), lr = 0 and the same sampling seed in every step, so every step of both arms decodes the same
captions and does the same work.  A random model never stops, so captions have `--entry-length` words (default 20, a caption's length).
References: 5 per image — the model's own greedy caption with one, two and three substitutions, one with a deletion and one unrelated row
— so that n-grams do match; the corpus is these references.  The two arms alternate inside one process after a warm-up; a step is timed
on the host clock between two device synchronisations (the host arm's cost is host time).  Reported: the median of the per-block medians,
the spread of the block medians as the same-box noise, the time spent inside the host callback, and the launch alone (device events
over `--launches` back-to-back launches on the step's own (2 B, n) buffer).  No threshold is asserted: it is a record.

    python tools/cider_bench.py [--reps 5] [--blocks 3] [--entry-length 20] [--markdown out.md]
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPE = dict(E=512, P=10, L=10, H=8, N=8, D=768, n_head=12, n_layer=12, V=50257, npos=1024, B=256)     # bench.py CONFIGS["2"]
STOP = 50256


def spread(v):
    return (max(v) - min(v)) / statistics.median(v) if len(v) > 1 else 0.0


def build_model():
    from clipcap_amd.encoders import EncoderConfig
    from clipcap_amd.model import ClipCapModel, Config, TrainingConfig
    from clipcap_amd.model.gpt2 import GPT2LM
    s = SHAPE
    torch.manual_seed(0)
    lm = GPT2LM(n_embd=s["D"], n_layer=s["n_layer"], n_head=s["n_head"], vocab_size=s["V"], n_positions=s["npos"])
    cfg = Config(language_model="unused", train_language_model=False, prefix_length=s["L"], projection_length=s["P"], transformer_layers=s["N"],
                 transformer_attention_heads=s["H"], encoder_config=EncoderConfig(encoder_embedding_size=s["E"]),
                 training_config=TrainingConfig(optimizer_lr=0.0, use_deepspeed_optimisers=False, scheduler_warmup_steps=1, total_steps=4))
    model = ClipCapModel(cfg, language_model=lm).to("cuda").eval()
    embeds = torch.randn(s["B"], s["E"], generator=torch.Generator().manual_seed(1)).cuda()
    return model, embeds


def references(model, embeds, entry):
    from clipcap_amd.inference.base import sample_tokens
    from tests import cider_ref
    with torch.no_grad():
        prefix = model.engine.mapper.forward(embeds, save=False)
        greedy, _ = sample_tokens(model, prefix, entry_length=entry, stop_token=STOP, mode=0, top_p=1.0, top_k=1, suppress_tokens=[0])
    rng = np.random.default_rng(2)
    docs = []
    for row in greedy.cpu().tolist():
        words = cider_ref.cut(row, STOP) or [1]
        rows = []
        for subs in (1, 2, 3):
            r = list(words)
            for _ in range(subs):
                r[int(rng.integers(0, len(r)))] = int(rng.integers(1, STOP))
            rows.append(r)
        rows.append(words[:len(words) // 2] + words[len(words) // 2 + 1:])
        rows.append([int(t) for t in rng.integers(1, STOP, len(words))])
        docs.append(rows)
    return docs


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--entry-length", type=int, default=20)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--markdown", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cider_bench.py measures on an MI355X; no GPU found (nothing is estimated on the CPU)")
    from clipcap_amd.train import CiderReward, self_critical_step
    from tests import cider_ref
    from tests.cider_cases import pad_refs
    model, embeds = build_model()
    B, entry = SHAPE["B"], args.entry_length
    docs = references(model, embeds, entry)
    arr, count = pad_refs(docs, 5, entry + 1)
    rw = CiderReward.from_corpus(docs, stop_token=STOP)
    device_fn = rw.for_batch(torch.from_numpy(arr).cuda(), torch.from_numpy(count).cuda())
    idf = cider_ref.idf_from_df(cider_ref.doc_freq(docs), len(docs))
    inside, last = [], {}

    def host_fn(sampled, greedy):
        t0 = time.perf_counter()
        out = []
        for ids in (sampled, greedy):
            rows = ids.cpu().tolist()                                                       # the copy to the host: a synchronisation
            out.append(torch.tensor([cider_ref.cider_d(cider_ref.cut(r, STOP), docs[b], idf) for b, r in enumerate(rows)], dtype=torch.float32))
        inside.append(time.perf_counter() - t0)
        return out

    def capture(sampled, greedy):
        last.update(sampled=sampled.clone(), greedy=greedy.clone())
        return device_fn(sampled, greedy)

    def step(fn):
        gen = torch.Generator(device="cuda").manual_seed(7)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = self_critical_step(model, embeds, fn, 0.0, entry_length=entry, stop_token=STOP, generator=gen)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    arms = {"device": device_fn, "host": host_fn}
    _, (_, ms_dev, mg_dev) = step(capture)                                                   # warm-up, and the two arms' rewards side by side
    _, (_, ms_host, mg_host) = step(host_fn)
    inside.clear()
    med = {k: [] for k in arms}
    for _ in range(args.blocks):
        t = {k: [] for k in arms}
        for _ in range(args.reps):
            for k, fn in arms.items():                                                      # alternating
                t[k].append(step(fn)[0])
        for k in arms:
            med[k].append(statistics.median(t[k]))
    # the launch alone, on the step's own candidates
    n = max(last["sampled"].shape[1], last["greedy"].shape[1])
    for _ in range(3):
        device_fn(last["sampled"], last["greedy"])
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cand = torch.full((2 * B, n), -1, dtype=torch.int64, device="cuda")
    cand[:B, :last["sampled"].shape[1]] = last["sampled"]
    cand[B:, :last["greedy"].shape[1]] = last["greedy"]
    refs_d, count_d = torch.from_numpy(arr).cuda(), torch.from_numpy(count).cuda()
    rw.score(cand, refs_d, count_d)
    launch = []
    for _ in range(args.blocks):
        a.record()
        for _ in range(args.launches):
            rw.score(cand, refs_d, count_d)
        b.record()
        b.synchronize()
        launch.append(a.elapsed_time(b) * 1e-3 / args.launches)
    out = dict(shape=SHAPE, entry_length=entry, candidates=2 * B, candidate_width=n, refs_per_image=5, ref_width=entry + 1,
               table_slots=rw.tab_keys.numel(), blocks=args.blocks, reps=args.reps,
               step_device_reward_ms=round(statistics.median(med["device"]) * 1e3, 3), step_device_reward_spread=round(spread(med["device"]), 4),
               step_host_reward_ms=round(statistics.median(med["host"]) * 1e3, 3), step_host_reward_spread=round(spread(med["host"]), 4),
               host_callback_ms=round(statistics.median(inside) * 1e3, 3), launch_alone_us=round(statistics.median(launch) * 1e6, 2),
               launch_alone_spread=round(spread(launch), 4), mean_reward_sampled=[round(float(ms_dev), 5), round(float(ms_host), 5)],
               mean_reward_greedy=[round(float(mg_dev), 5), round(float(mg_host), 5)])
    out["host_over_device_step"] = round(out["step_host_reward_ms"] / out["step_device_reward_ms"], 3)
    print(json.dumps(out), flush=True)
    if args.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(args.markdown)), exist_ok=True)
        open(args.markdown, "w").write(
            f"self_critical_step at bench.py config 2's shape (B = {B}, frozen GPT-2-small, random weights), entry_length {entry}, {2 * B} candidates x "
            f"{n} positions, 5 references x {entry + 1} positions per image, table of {out['table_slots']} slots; {args.blocks} blocks x {args.reps} "
            "alternating steps; median of block medians (spread of the block medians).\n\n"
            "| reward | step, ms | inside the callback, ms | launch alone, us |\n|---|---|---|---|\n"
            f"| CiderReward.for_batch (device) | {out['step_device_reward_ms']} ({100 * out['step_device_reward_spread']:.1f} %) | - | "
            f"{out['launch_alone_us']} ({100 * out['launch_alone_spread']:.1f} %) |\n"
            f"| host reward_fn (copy, tests/cider_ref.py, copy back) | {out['step_host_reward_ms']} ({100 * out['step_host_reward_spread']:.1f} %) | "
            f"{out['host_callback_ms']} | - |\n\nhost / device step time: {out['host_over_device_step']}\n\n```\n{json.dumps(out)}\n```\n")


if __name__ == "__main__":
    main()
