#!/usr/bin/env python
"""What stochastic beam search costs.  (1) The update alone: cc_beam_gumbel_step against the three-kernel cc_beam_step (no lm_head
partials: both read the logits once) at S = 64, beam 5, V = 50257, ld = 50304 on random logits, alternating on one box under device
events; what the noise adds is the difference, also per token.  (2) A whole generate_stochastic_beam_tokens against generate_beam_tokens
at the decode benchmark's shape (GPT-2-medium geometry, random weights, 64 prefixes of 10 rows, beam 5, 67 generated tokens; the stop
token is an id outside the vocabulary, so every run takes all its steps; the plain decode uses the lm_head partials and the one-launch
update, as the product does).  Prints one JSON line; nothing passes or fails on it.

    python tools/stochastic_beam_bench.py [--rounds 5] [--warmup 1] [--batch 64] [--reps 100] [--update-only]
"""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BEAM, ENTRY, L0, V, LD, SEED = 5, 67, 10, 50257, 50304, 0x9E3779B97F4A7C15


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3, out


def update_us(S, reps, blocks=5):
    """Median over alternating blocks of the microseconds per update, on 4 copies of the logits so that a call does not find its rows in L2
    from the call before.  The state is reset before every block; no row has stopped."""
    from clipcap_amd import engine as E
    dev = "cuda"
    R = S * BEAM
    g = torch.Generator(device=dev).manual_seed(7)
    copies = [(torch.randn(R, LD, device=dev, generator=g) * 3.0)[:, :V] for _ in range(4)]
    phi, gam = torch.zeros(R, device=dev), torch.zeros(R, device=dev)
    seql, stopped = torch.ones(R, device=dev), torch.zeros(R, dtype=torch.uint8, device=dev)
    gb, pb = E.beam_gumbel_buffers(dev, S, BEAM, V), E.beam_buffers(dev, S, BEAM, V)
    stop = V                                                                    # never picked

    def reset():
        phi.copy_(-torch.rand(R, device=dev))
        gam.copy_(-torch.rand(R, device=dev).sort(descending=True).values)
        seql.fill_(1.0)
        stopped.zero_()

    runs = {"gumbel": lambda i: E.beam_gumbel_step(copies[i & 3], S, BEAM, 1.0, False, stop, SEED, 1 + (i & 15), phi, gam, seql, stopped, gb),
            "beam3": lambda i: E.beam_step(copies[i & 3], S, BEAM, 1.0, False, stop, phi, seql, stopped, pb)}
    times = {k: [] for k in runs}
    for blk in range(blocks + 1):
        for k, fn in runs.items():                                              # alternating: drift of the box hits both alike
            reset()
            for i in range(4):
                fn(i)
            dt = timed(lambda: [fn(i) for i in range(reps)])[0] / reps
            if blk:                                                             # block 0 is the warm-up
                times[k].append(dt * 1e6)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--update-only", action="store_true")
    args = ap.parse_args()
    out = {"update_shape": f"S {args.batch}, beam {BEAM}, V {V}, ld {LD}, T 1, no row stopped, {args.reps} calls per block, 5 blocks"}
    u = update_us(args.batch, args.reps)
    tokens = args.batch * BEAM * V
    for k, (med, lo, hi) in u.items():
        out[k + "_update_us"] = {"median": round(med, 1), "min": round(lo, 1), "max": round(hi, 1),
                                 "logits_GBps": round(tokens * 4 / (med * 1e-6) / 1e9, 1), "ps_per_token": round(med * 1e-6 / tokens * 1e12, 2)}
    out["noise_adds_us"] = round(u["gumbel"][0] - u["beam3"][0], 1)
    out["noise_adds_ps_per_token"] = round((u["gumbel"][0] - u["beam3"][0]) * 1e-6 / tokens * 1e12, 2)
    if not args.update_only:
        from clipcap_amd.inference import generate_beam_tokens, generate_stochastic_beam_tokens
        from clipcap_amd.model.gpt2 import GPT2LM
        torch.manual_seed(1234)
        lm = GPT2LM(n_embd=1024, n_layer=24, n_head=16, vocab_size=V, n_positions=1024).to("cuda")
        model = SimpleNamespace(language_model=lm)
        stop = lm.engine.dims["V"]                  # outside the vocabulary: never picked, every decode takes ENTRY steps
        prefix = torch.randn(args.batch, L0, 1024, device="cuda") * 0.5
        runs = {"beam": lambda: generate_beam_tokens(model, prefix, BEAM, ENTRY, 1.0, stop),
                "stochastic": lambda: generate_stochastic_beam_tokens(model, prefix, BEAM, ENTRY, 1.0, stop, seed=SEED)}
        for _ in range(max(1, args.warmup)):
            for fn in runs.values():
                fn()
        times = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, fn in runs.items():
                dt, r = timed(fn)
                assert r[0].shape[2] == ENTRY
                times[k].append(dt)
        out["decode_shape"] = f"GPT-2-medium random init, {args.batch} prefixes x {L0} rows, beam {BEAM}, {ENTRY} tokens, {args.rounds} rounds"
        for k, ts in times.items():
            dt = statistics.median(ts)
            out[k + "_decode"] = {"s": round(dt, 4), "min_s": round(min(ts), 4), "max_s": round(max(ts), 4),
                                  "tokens_per_s": round(args.batch * ENTRY / dt, 1), "step_ms": round(dt / ENTRY * 1e3, 3)}
        out["stochastic_vs_beam_tokens_per_s"] = round(out["stochastic_decode"]["tokens_per_s"] / out["beam_decode"]["tokens_per_s"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
