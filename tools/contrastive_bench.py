#!/usr/bin/env python
"""What contrastive search costs next to a beam of the same width: generate_contrastive_tokens(top_k=4) against generate_beam_tokens(beam 4)
at the decode benchmark's shape (GPT-2-medium geometry, random weights, 64 prefixes of 10 rows, 67 generated tokens).  The stop token is
an id outside the vocabulary, which nothing can pick, so every run takes all its steps.  The two decoders alternate inside one process,
each decode timed with device events after a warm-up.  A beam decode takes one forward fewer than it generates tokens (its first token
comes from the prefill), a contrastive decode one forward per token (a token is kept only after its candidates have been run): both
are reported per generated position.  The three launches a contrastive step adds (hidden_unit, contrastive_select, contrastive_topk) are
timed alone on the buffers of a real decode, with the history as long as at the decode's middle step.  Prints one JSON line.

    python tools/contrastive_bench.py [--rounds 5] [--warmup 1] [--batch 64]
"""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K, ENTRY, L0, ALPHA = 4, 67, 10, 0.6


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3, out


def added_launch_seconds(model, prefix, stop, reps=200):
    """Seconds per call of the three launches a contrastive step adds to a width-K beam step's forward, each timed alone."""
    from clipcap_amd import engine as E
    g = model.language_model.engine
    S, V, D, R = prefix.shape[0], g.dims["V"], g.dims["D"], prefix.shape[0] * K
    n_hist = L0 + ENTRY // 2
    b = E.contrastive_buffers(prefix.device, S, K, D, L0 + ENTRY, ENTRY)
    sess = E.DecodeSession(g, S, L0 + 2)
    sess.forward(prefix)
    sess = sess.expand(torch.arange(R, device=prefix.device, dtype=torch.int32) // K, R)
    logits = sess.forward(torch.randn(R, 1, D, device=prefix.device) * 0.5, group=K)
    b.hist.copy_(torch.nn.functional.normalize(torch.randn_like(b.hist), dim=-1))
    E.contrastive_topk(logits, S, K, b.sel, K, None, b.cand_tok, b.cand_prob)

    def select():
        b.stopped.zero_()                                # queued memset: a caption that "stopped" would skip the work
        E.contrastive_select(b, K, 0, n_hist, ALPHA, stop, 0)

    steps = {"hidden_unit": lambda: sess.hidden_unit(b.cand_h, D, D), "select": select,
             "topk": lambda: E.contrastive_topk(logits, S, K, b.sel, K, None, b.cand_tok, b.cand_prob)}
    out = {}
    for name, fn in steps.items():
        for _ in range(10):
            fn()
        out[name] = timed(lambda: [fn() for _ in range(reps)])[0] / reps
    return out, n_hist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=64)
    args = ap.parse_args()
    from clipcap_amd.inference import generate_beam_tokens, generate_contrastive_tokens
    from clipcap_amd.model.gpt2 import GPT2LM
    torch.manual_seed(1234)
    lm = GPT2LM(n_embd=1024, n_layer=24, n_head=16, vocab_size=50257, n_positions=1024).to("cuda")
    model = SimpleNamespace(language_model=lm)
    stop = lm.engine.dims["V"]                      # outside the vocabulary: never picked, every decode takes ENTRY steps
    prefix = torch.randn(args.batch, L0, 1024, device="cuda") * 0.5
    runs = {"beam4": lambda: generate_beam_tokens(model, prefix, K, ENTRY, 1.0, stop)[0][:, 0],
            "contrastive4": lambda: generate_contrastive_tokens(model, prefix, K, ALPHA, ENTRY, stop)[0]}
    for _ in range(max(1, args.warmup)):
        for fn in runs.values():
            fn()
    times = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, fn in runs.items():                  # alternating: drift of the box hits both decoders alike
            dt, toks = timed(fn)
            assert toks.shape == (args.batch, ENTRY)
            times[k].append(dt)
    out = {"shape": f"GPT-2-medium random init, {args.batch} prefixes x {L0} rows, width {K}, {ENTRY} tokens, alpha {ALPHA}", "rounds": args.rounds}
    for k, ts in times.items():
        dt = statistics.median(ts)
        out[k] = {"decode_s": round(dt, 4), "min_s": round(min(ts), 4), "max_s": round(max(ts), 4), "ms_per_position": round(dt / ENTRY * 1e3, 3),
                  "forwards_at_width": ENTRY - 1 if k == "beam4" else ENTRY}
    out["contrastive4"]["ms_per_position_vs_beam4"] = round(out["contrastive4"]["ms_per_position"] / out["beam4"]["ms_per_position"], 4)
    added, n_hist = added_launch_seconds(model, prefix, stop)
    out["added_launches_us"] = {k: round(v * 1e6, 1) for k, v in added.items()}
    out["added_launches_us"]["history_rows"] = n_hist
    print(json.dumps(out))


if __name__ == "__main__":
    main()
