#!/usr/bin/env python
"""Times per-token loss weights in the fused lm_head loss on one box: the training step of bench.py's config 2 (frozen GPT-2-small,
B = 256) and config 3 (GPT-2-small full finetune, B = 256, GPT-2 dropout on), with bf16 and with split-bf16 operands, under four settings:

    parent      without weights, on the PARENT commit's library (--parent-lib: a libclipcap_hip.so built from the parent commit)
    plain       without weights, on this build
    weighted    token_weights, eps = 0
    weighted+ls token_weights, eps = 0.1

Method: a library is chosen when a process starts, so the settings run in worker processes that ALTERNATE (parent, plain, weighted, parent,
plain, weighted, ... --rounds times, at least three).  The parent and the plain worker follow one protocol: nothing but steps without
weights.  The weighted worker alternates its two settings and a step without weights step by step, which gives the in-process difference
"weighted - plain".  Each step (zero_grad, forward_backward, optimizer_step) is timed with HIP events; a worker reports the median per
setting, and the table gives the median over the rounds with each setting's spread (max - min) / median over the rounds.  The one
pass/fail figure: the plain step of this build must lie inside the parent's own run-to-run spread on this box, i.e. its median may exceed
the parent's by no more than the parent's (max - min) over the rounds.  The weighted step's cost is reported beside the bytes it adds
(two reads of B * cap fp32 weights: 8 * B * cap), not bounded.  One JSON line per (configuration, precision); --markdown writes the table.

    python tools/token_weights_bench.py --parent-lib /path/to/parent/libclipcap_hip.so [--reps 20] [--rounds 3] [--markdown out.md]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NEW = ("cc_lmhead_ce_fwd_w", "cc_lmhead_ce_bwd_w")
SETTINGS = ("inproc_plain", "weighted", "weighted+ls")


def mid(v):
    return statistics.median(v)


def spread(v):
    return (max(v) - min(v)) / mid(v) if len(v) > 1 else 0.0


def extra_bytes(c):
    """bytes a weighted step moves beyond the plain one: the fp32 weights, read by the forward's stats block and by the backward's row factors"""
    return 2 * 4 * c["B"] * c["cap"]


def worker(configs, precisions, reps, with_weights):
    """one process = one library (CLIPCAP_HIP_LIB): per (config, precision) the median step time of each setting, alternating"""
    from clipcap_amd import _lib
    have = C.CDLL(_lib.LIB_PATH)
    for name in NEW:                                   # the parent's library has no weighted entry points: bind what it exports
        if not hasattr(have, name):
            assert not with_weights, f"{_lib.LIB_PATH} does not export {name}"
            _lib.SIGNATURES.pop(name, None)
    import torch
    from bench import CONFIGS, init_engines

    def timed(fn, stream):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)

    device = torch.device("cuda", 0)
    for key in configs:
        for precision in precisions:
            c = dict(CONFIGS[key])
            me, ge, eng = init_engines(c, device)
            if precision != "bf16":
                me.set_precision(int(precision))
                ge.set_precision(int(precision))
            gen = torch.Generator(device=device).manual_seed(4321)
            embeds = torch.randn(c["B"], c["E"], generator=gen, device=device)
            tokens = torch.randint(1, c["V"], (c["B"], c["cap"]), generator=gen, device=device)
            weights = torch.randn(c["B"], c["cap"], generator=gen, device=device)
            stream = torch.cuda.current_stream()
            n = {"i": 0}

            def step(setting):
                i = n["i"] = n["i"] + 1
                kw = {} if setting in ("plain", "inproc_plain") else dict(token_weights=weights, label_smoothing=0.1 if setting == "weighted+ls" else 0.0)
                eng.zero_grad()
                loss = eng.forward_backward(tokens, embeds, dropout=(0.1, 0.1, 0.1, 1000003 * i) if c["train_lm"] else None, **kw)
                eng.optimizer_step(1e-6, i)
                return loss

            settings = SETTINGS if with_weights else ("plain",)
            for _ in range(3):
                for s in settings:
                    step(s)
            torch.cuda.synchronize()
            t = {s: [] for s in settings}
            for _ in range(reps):
                for s in settings:
                    t[s].append(timed(lambda: step(s), stream))
            print(json.dumps(dict(config=key, name=c["name"], B=c["B"], cap=c["cap"], precision=precision, extra_bytes=extra_bytes(c),
                                  ms={s: mid(t[s]) for s in settings})), flush=True)
            del me, ge, eng
            torch.cuda.empty_cache()


def run_worker(lib, args, with_weights):
    env = dict(os.environ)
    if lib:
        env["CLIPCAP_HIP_LIB"] = lib
    else:
        env.pop("CLIPCAP_HIP_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--configs", args.configs, "--precisions", args.precisions, "--reps", str(args.reps)]
    if with_weights:
        cmd.append("--with-weights")
    out = subprocess.run(cmd, env=env, check=True, stdout=subprocess.PIPE, text=True, timeout=600).stdout
    return [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]


def markdown(rows, rounds):
    out = ["# Per-token loss weights in the fused lm_head loss: step time", "",
           f"`tools/token_weights_bench.py`: the parent commit's library and this build in worker processes that alternate {rounds} times on one box; inside",
           "a worker of this build the settings alternate step by step; HIP events around a whole step; each figure is the median over the rounds of",
           "the workers' medians, +- its spread (max - min) / median over the rounds.  parent and plain: workers that run nothing but steps without",
           "weights; weighted - plain: against the steps without weights interleaved in the weighted worker.  Verdict: plain - parent against the",
           "parent's own (max - min) over the rounds.  Extra bytes of a weighted step: two reads of the B * cap fp32 weights.", "",
           "| config | operands | parent, ms | plain, ms | weighted, ms | weighted + eps 0.1, ms | plain - parent | weighted - plain | extra bytes | plain within the parent's spread |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        f = lambda k: f"{r[k + '_ms']:.3f} +- {100 * r[k + '_spread']:.1f} %"      # noqa: E731
        out.append(f"| {r['config']} ({r['name']}, B = {r['B']}) | {r['precision']} | {f('parent')} | {f('plain')} | {f('weighted')} | {f('weighted+ls')} | "
                   f"{r['plain_ms'] - r['parent_ms']:+.3f} ms | {r['weighted_ms'] - r['inproc_plain_ms']:+.3f} ms | {r['extra_bytes'] / 1e3:.0f} kB | "
                   f"{'yes' if r['plain_within_parent_range'] else 'NO'} (parent {r['parent_min_ms']:.3f} .. {r['parent_max_ms']:.3f}) |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-lib", default="", help="libclipcap_hip.so built from the parent commit")
    ap.add_argument("--reps", type=int, default=20, help="alternating repetitions per worker")
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the two libraries (at least 3)")
    ap.add_argument("--configs", default="2,3")
    ap.add_argument("--precisions", default="bf16,32")
    ap.add_argument("--markdown", default="", help="also write the table to this file")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--with-weights", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("token_weights_bench.py measures on an MI355X; no GPU found (nothing is estimated on the CPU)")
        worker([k.strip() for k in args.configs.split(",")], [p.strip() for p in args.precisions.split(",")], args.reps, args.with_weights)
        return
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        raise SystemExit("--parent-lib: build the parent commit's library first and hand its path in")
    if args.rounds < 3:
        raise SystemExit("--rounds: at least 3")
    acc = {}
    for i in range(args.rounds):
        for label, lib, with_weights in (("parent", os.path.abspath(args.parent_lib), False), ("plain", "", False), ("weighted", "", True)):
            print(f"round {i + 1} of {args.rounds}: {label}", file=sys.stderr, flush=True)
            for r in run_worker(lib, args, with_weights):
                e = acc.setdefault((r["config"], r["precision"]), dict(r, ms={}))
                for s, v in r["ms"].items():
                    e["ms"].setdefault(s if with_weights else label, []).append(v)
    rows = []
    for (key, prec), e in acc.items():
        row = {k: e[k] for k in ("config", "name", "B", "cap", "precision", "extra_bytes")}
        for s, v in e["ms"].items():
            row[s + "_ms"], row[s + "_spread"], row[s + "_rounds"] = mid(v), spread(v), v
        row["parent_min_ms"], row["parent_max_ms"] = min(e["ms"]["parent"]), max(e["ms"]["parent"])
        row["plain_within_parent_range"] = row["plain_ms"] - row["parent_ms"] <= row["parent_max_ms"] - row["parent_min_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(args.markdown)), exist_ok=True)
        open(args.markdown, "w").write(markdown(rows, args.rounds))
    if not all(r["plain_within_parent_range"] for r in rows):
        raise SystemExit("the plain step of this build lies outside the parent's run-to-run spread")


if __name__ == "__main__":
    main()
