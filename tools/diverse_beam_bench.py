#!/usr/bin/env python
"""What diverse beam search costs: plain beam 6 against beam 6 in 3 and in 6 beam groups, at the decode benchmark's shape (GPT-2-medium
geometry, random weights, 64 prefixes of 10 rows, 67 generated tokens).  The stop token is an id outside the vocabulary, which no beam can
pick, so every run takes all its steps.  The configurations alternate inside one process, each decode timed with device events after a
warm-up; the beam update alone (cc_beam_step_p on the lm_head partials for the plain decode, cc_beam_group_step for the grouped ones) is
timed the same way on the logits of a real decode step.  Prints one JSON line.

    python tools/diverse_beam_bench.py [--rounds 5] [--warmup 1] [--batch 64] [--plain-only]

--plain-only times the plain decode alone: it runs on a checkout that predates the beam groups (the parent of the commit that added them).
"""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BEAM, ENTRY, L0, PENALTY = 6, 67, 10, 1.0


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3, out


def update_seconds(model, prefix, groups, stop, reps=200):
    """Seconds per beam update, on the logits of the decode's second step (the first with `beam` rows per prefix)."""
    from clipcap_amd import engine as E
    g = model.language_model.engine
    S, V, R = prefix.shape[0], g.dims["V"], prefix.shape[0] * BEAM
    sess = E.DecodeSession(g, S, L0 + 2)
    sess.forward(prefix)
    base = torch.arange(R, device=prefix.device, dtype=torch.int32) // BEAM
    sess = sess.expand(base, R)
    x = torch.randn(R, 1, g.dims["D"], device=prefix.device) * 0.5
    logits = sess.forward(x, partials=groups == 1, group=BEAM)
    scores = -torch.rand(R, device=prefix.device)
    seql = torch.ones(R, device=prefix.device)
    stopped = torch.zeros(R, dtype=torch.uint8, device=prefix.device)
    if groups == 1:
        bufs = E.beam_buffers(prefix.device, S, BEAM, V)
        step = lambda: E.beam_step(logits, S, BEAM, 1.0, False, stop, scores, seql, stopped, bufs, sess.lpart)  # noqa: E731
    else:
        bufs = E.beam_group_buffers(prefix.device, S, BEAM, groups, V)
        step = lambda: E.beam_group_step(logits, S, BEAM, groups, 1.0, PENALTY, False, stop, scores, seql, stopped, bufs)  # noqa: E731
    for _ in range(10):
        step()
    return timed(lambda: [step() for _ in range(reps)])[0] / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--plain-only", action="store_true")
    args = ap.parse_args()
    from clipcap_amd.inference.base import generate_beam_tokens
    from clipcap_amd.model.gpt2 import GPT2LM
    torch.manual_seed(1234)
    lm = GPT2LM(n_embd=1024, n_layer=24, n_head=16, vocab_size=50257, n_positions=1024).to("cuda")
    model = SimpleNamespace(language_model=lm)
    stop = lm.engine.dims["V"]                      # outside the vocabulary: never picked, every decode takes ENTRY steps
    prefix = torch.randn(args.batch, L0, 1024, device="cuda") * 0.5
    configs = {"plain": {}} if args.plain_only else {"plain": {}, "groups3": dict(num_beam_groups=3, diversity_penalty=PENALTY),
                                                     "groups6": dict(num_beam_groups=6, diversity_penalty=PENALTY)}
    run = lambda kw: generate_beam_tokens(model, prefix, BEAM, ENTRY, 1.0, stop, **kw)  # noqa: E731
    for _ in range(max(1, args.warmup)):
        for kw in configs.values():
            run(kw)
    times = {k: [] for k in configs}
    for _ in range(args.rounds):
        for k, kw in configs.items():              # alternating: drift of the box hits every configuration alike
            dt, (toks, _, lens) = timed(lambda: run(kw))
            assert toks.shape[2] == ENTRY and bool((lens == ENTRY).all())
            times[k].append(dt)
    out = {"shape": f"GPT-2-medium random init, {args.batch} prefixes x {L0} rows, beam {BEAM}, {ENTRY} tokens, penalty {PENALTY}", "rounds": args.rounds}
    for k, ts in times.items():
        dt = statistics.median(ts)
        rec = {"decode_s": round(dt, 4), "min_s": round(min(ts), 4), "max_s": round(max(ts), 4), "tokens_per_s": round(args.batch * ENTRY / dt, 1),
               "step_ms": round(dt / ENTRY * 1e3, 3)}
        if not args.plain_only:
            groups = configs[k].get("num_beam_groups", 1)
            us = update_seconds(model, prefix, groups, stop) * 1e6
            rec.update(update_us=round(us, 1), update_share_of_step=round(us * 1e-6 / (dt / ENTRY), 4), launches_per_update=3 if groups == 1 else 1 + 2 * groups)      # width 6 has no fused kernel: three kernels
        out[k] = rec
    if not args.plain_only:
        for k in ("groups3", "groups6"):
            out[k]["tokens_per_s_vs_plain"] = round(out[k]["tokens_per_s"] / out["plain"]["tokens_per_s"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
