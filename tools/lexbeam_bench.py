#!/usr/bin/env python
"""What lexically constrained beam search costs.  (1) The update alone: cc_beam_lex_step with 0, 2 and 8 phrases per sample against the
three-kernel cc_beam_step (no lm_head partials) at S = 64, beam 5, V = 50257, ld = 50304 on the same random logits, alternating on one box
under device events.  (2) A whole generate_constrained_beam_tokens (2 phrases per prefix) against generate_beam_tokens at the decode
benchmark's shape (GPT-2-medium geometry, random weights, 64 prefixes of 10 rows, beam 5, 67 generated tokens; the stop token is an id
outside the vocabulary, so every run takes all its steps; the plain decode uses the lm_head partials and the one-launch update, as the
product does).  Prints one JSON line; nothing passes or fails on it.

    python tools/lexbeam_bench.py [--rounds 5] [--warmup 1] [--batch 64] [--reps 100] [--update-only]
"""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BEAM, ENTRY, L0, V, LD = 5, 67, 10, 50257, 50304
PHRASES = [[101, 102, 103], [2000], [301, 302], [4000, 4001, 4002, 4003, 4004, 4005, 4006, 4007], [501], [601, 602], [701, 702, 703, 704], [801, 802]]


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
    from clipcap_amd.inference.utils import validate_phrases
    dev = "cuda"
    R = S * BEAM
    g = torch.Generator(device=dev).manual_seed(7)
    copies = [(torch.randn(R, LD, device=dev, generator=g) * 3.0)[:, :V] for _ in range(4)]
    scores, seql = torch.zeros(R, device=dev), torch.ones(R, device=dev)
    stopped, state = torch.zeros(R, dtype=torch.uint8, device=dev), torch.zeros(R, dtype=torch.int32, device=dev)
    stop = V                                                                    # never picked
    pb = E.beam_buffers(dev, S, BEAM, V)

    def reset():
        scores.copy_(-torch.rand(R, device=dev))
        seql.fill_(1.0)
        stopped.zero_()
        state.zero_()

    runs = {"beam3": lambda i: E.beam_step(copies[i & 3], S, BEAM, 1.0, False, stop, scores, seql, stopped, pb)}
    for n in (0, 2, 8):
        tab = validate_phrases(PHRASES[:n], S, V, stop).to(dev) if n else None
        lb = E.beam_lex_buffers(dev, S, BEAM, n, V)
        runs[f"lex{n}"] = lambda i, tab=tab, lb=lb: E.beam_lex_step(copies[i & 3], S, BEAM, 1.0, False, stop, scores, seql, stopped, state, tab, lb)
    times = {k: [] for k in runs}
    for blk in range(blocks + 1):
        for k, fn in runs.items():                                              # alternating: drift of the box hits all alike
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
    nbytes = args.batch * BEAM * V * 4
    for k, (med, lo, hi) in u.items():
        # passes over the logits: the row statistics and one selection pass; cc_beam_step's two-pass selection scans them twice
        reads = (3 if k == "beam3" else 2) * nbytes
        out[k + "_update_us"] = {"median": round(med, 1), "min": round(lo, 1), "max": round(hi, 1), "logits_MB_requested": round(reads / 1e6, 1),
                                 "requested_GBps": round(reads / (med * 1e-6) / 1e9, 1)}
    if not args.update_only:
        from clipcap_amd.inference import generate_beam_tokens, generate_constrained_beam_tokens
        from clipcap_amd.model.gpt2 import GPT2LM
        torch.manual_seed(1234)
        lm = GPT2LM(n_embd=1024, n_layer=24, n_head=16, vocab_size=V, n_positions=1024).to("cuda")
        model = SimpleNamespace(language_model=lm)
        stop = lm.engine.dims["V"]                  # outside the vocabulary: never picked, every decode takes ENTRY steps
        prefix = torch.randn(args.batch, L0, 1024, device="cuda") * 0.5
        runs = {"beam": lambda: generate_beam_tokens(model, prefix, BEAM, ENTRY, 1.0, stop)[0],
                "constrained": lambda: generate_constrained_beam_tokens(model, prefix, PHRASES[:2], BEAM, ENTRY, 1.0, stop).tokens}
        for _ in range(max(1, args.warmup)):
            for fn in runs.values():
                fn()
        times = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, fn in runs.items():
                dt, r = timed(fn)
                assert r.shape[2] == ENTRY
                times[k].append(dt)
        out["decode_shape"] = f"GPT-2-medium random init, {args.batch} prefixes x {L0} rows, beam {BEAM}, {ENTRY} tokens, {args.rounds} rounds"
        for k, ts in times.items():
            dt = statistics.median(ts)
            out[k + "_decode"] = {"s": round(dt, 4), "min_s": round(min(ts), 4), "max_s": round(max(ts), 4),
                                  "tokens_per_s": round(args.batch * ENTRY / dt, 1), "step_ms": round(dt / ENTRY * 1e3, 3)}
        out["constrained_vs_beam_tokens_per_s"] = round(out["constrained_decode"]["tokens_per_s"] / out["beam_decode"]["tokens_per_s"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
