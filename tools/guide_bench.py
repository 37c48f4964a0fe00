#!/usr/bin/env python
"""What classifier-free guidance costs at decode time, on one box:

  (a) the combination alone at the decode benchmark's step shape (R = 320 rows, V = 50257, ld = Vp = 50304): cc_logits_guide, in place as
      the decoders call it, against the torch composition ``torch.lerp(log_softmax(uncond), log_softmax(cond), g)`` on the same views.
      The two alternate inside one process after a warm-up; every sample is `--inner` calls between two device events; the median of the
      per-block medians is reported, with the spread of the per-block medians as the same-box noise.  Beside the times: the bytes the
      launch has to move (2 rows read twice, 1 written: 5 * R * V * 4, of which 3 * R * V * 4 cannot be served by a cache) and the peak
      device memory each route allocates on top of its inputs (torch.cuda.max_memory_allocated).
  (b) a beam-5 decode of the benchmark's decode shape (GPT-2-medium geometry, random weights, 64 prefixes of 10 rows, 67 generated tokens,
      a stop token outside the vocabulary so that every decode takes all its steps) with guidance_scale 1 (today's decoder: the fused
      beam update on the lm_head partials, one forward per step) and 1.5 (two forwards per step, cc_logits_guide, the beam update on the
      logits), one random position as the negative context.  The two alternate; each decode is timed with device events.

Prints one JSON line per part; --markdown also writes the tables.

    python tools/guide_bench.py [--reps 20] [--blocks 3] [--inner 20] [--rounds 5] [--markdown out.md]
"""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

R, V, VP, SCALE = 320, 50257, 50304, 1.5
BEAM, ENTRY, L0, BATCH = 5, 67, 10, 64


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3, out


def spread(v):
    return (max(v) - min(v)) / statistics.median(v) if len(v) > 1 else 0.0


def peak_extra(fn):
    """Bytes allocated at the peak of fn() on top of what was allocated before it."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - before


def kernel_part(reps, blocks, inner):
    from clipcap_amd.engine import guide_logits
    gen = torch.Generator(device="cuda").manual_seed(7)
    src = torch.randn(R, VP, device="cuda", generator=gen) * 3.0
    cond, uncond = src.clone(), torch.randn(R, VP, device="cuda", generator=gen) * 3.0
    c, u = cond[:, :V], uncond[:, :V]
    routes = {"kernel": lambda: guide_logits(c, u, SCALE),                                           # in place, as the decoders call it
              "torch": lambda: torch.lerp(torch.log_softmax(u, -1), torch.log_softmax(c, -1), SCALE)}
    ref = routes["torch"]()
    err = (guide_logits(c, u, SCALE, out=torch.empty(R, V, device="cuda")) - ref).abs().max().item()
    peaks = {k: peak_extra(fn) for k, fn in routes.items()}
    for fn in routes.values():
        for _ in range(5):
            fn()
    med = {k: [] for k in routes}
    for _ in range(blocks):
        t = {k: [] for k in routes}
        for _ in range(reps):
            for k, fn in routes.items():                                                            # alternating
                cond.copy_(src)                                                                      # the kernel works in place: same inputs every sample
                t[k].append(timed(lambda: [fn() for _ in range(inner)])[0] / inner)
        for k in routes:
            med[k].append(statistics.median(t[k]))
    out = dict(part="kernel", R=R, V=V, ld=VP, scale=SCALE, reps=reps, blocks=blocks, inner=inner, bytes_moved=5 * R * V * 4, bytes_compulsory=3 * R * V * 4,
               max_abs_difference=err)
    for k in routes:
        us = statistics.median(med[k]) * 1e6
        out[f"{k}_us"], out[f"{k}_spread"], out[f"{k}_peak_extra_bytes"] = round(us, 2), round(spread(med[k]), 4), peaks[k]
        out[f"{k}_GBps_of_bytes_moved"] = round(out["bytes_moved"] / us * 1e-3, 1)
    out["torch_over_kernel"] = round(out["torch_us"] / out["kernel_us"], 2)
    return out


def decode_part(rounds, warmup):
    from clipcap_amd.inference.base import generate_beam_tokens
    from clipcap_amd.model.gpt2 import GPT2LM
    torch.manual_seed(1234)
    lm = GPT2LM(n_embd=1024, n_layer=24, n_head=16, vocab_size=V, n_positions=1024).to("cuda")
    model = SimpleNamespace(language_model=lm)
    stop = lm.engine.dims["V"]                                                                       # outside the vocabulary: never picked
    prefix = torch.randn(BATCH, L0, 1024, device="cuda") * 0.5
    neg = torch.randn(1, 1, 1024, device="cuda") * 0.5
    configs = {"g1": dict(guidance_scale=1.0), "g1.5": dict(guidance_scale=SCALE, negative_embeds=neg)}
    run = lambda kw: generate_beam_tokens(model, prefix, BEAM, ENTRY, 1.0, stop, **kw)  # noqa: E731
    for _ in range(max(1, warmup)):
        for kw in configs.values():
            run(kw)
    times = {k: [] for k in configs}
    for _ in range(rounds):
        for k, kw in configs.items():                                                                # alternating
            dt, (toks, _, lens) = timed(lambda: run(kw))
            assert toks.shape[2] == ENTRY and bool((lens == ENTRY).all())
            times[k].append(dt)
    out = dict(part="decode", shape=f"GPT-2-medium random init, {BATCH} prefixes x {L0} rows, beam {BEAM}, {ENTRY} tokens", rounds=rounds)
    for k, ts in times.items():
        dt = statistics.median(ts)
        out[k] = dict(decode_s=round(dt, 4), min_s=round(min(ts), 4), max_s=round(max(ts), 4), step_ms=round(dt / ENTRY * 1e3, 3),
                      tokens_per_s=round(BATCH * ENTRY / dt, 1))
    out["guided_over_plain"] = round(out["g1.5"]["decode_s"] / out["g1"]["decode_s"], 3)
    return out


def markdown(k, d):
    mb = lambda b: f"{b / 1e6:.1f} MB"  # noqa: E731
    return "\n".join([
        "## (a) the combination alone", "",
        f"R = {k['R']}, V = {k['V']}, ld = {k['ld']}, g = {k['scale']}; {k['blocks']} blocks x {k['reps']} alternating samples of {k['inner']} calls; largest difference "
        f"between the two routes {k['max_abs_difference']:.2e}.", "",
        "| route | time per call, us | spread of block medians | bytes moved (5 R V 4) / time | peak extra memory |", "|---|---|---|---|---|",
        f"| cc_logits_guide, in place | {k['kernel_us']} | {100 * k['kernel_spread']:.1f} % | {k['kernel_GBps_of_bytes_moved']} GB/s | {mb(k['kernel_peak_extra_bytes'])} |",
        f"| log_softmax x 2 + lerp | {k['torch_us']} | {100 * k['torch_spread']:.1f} % | (moves more) | {mb(k['torch_peak_extra_bytes'])} |", "",
        f"torch / kernel = {k['torch_over_kernel']}.  Bytes the launch moves: {mb(k['bytes_moved'])}, of which {mb(k['bytes_compulsory'])} are compulsory.", "",
        "## (b) beam-5 decode", "", f"{d['shape']}; {d['rounds']} alternating rounds, median (min .. max).", "",
        "| guidance_scale | decode, s | step, ms | tokens/s |", "|---|---|---|---|"] + [
        f"| {n} | {d[n]['decode_s']} ({d[n]['min_s']} .. {d[n]['max_s']}) | {d[n]['step_ms']} | {d[n]['tokens_per_s']} |" for n in ("g1", "g1.5")] + [
        "", f"guided / plain = {d['guided_over_plain']}", ""])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--markdown", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("guide_bench.py measures on an MI355X; no GPU found (nothing is estimated on the CPU)")
    k = kernel_part(args.reps, args.blocks, args.inner)
    print(json.dumps(k), flush=True)
    d = decode_part(args.rounds, args.warmup)
    print(json.dumps(d), flush=True)
    if args.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(args.markdown)), exist_ok=True)
        open(args.markdown, "w").write(markdown(k, d))


if __name__ == "__main__":
    main()
