#!/usr/bin/env python
"""Times caption scoring at GPT-2-small, B = 256, L = 10, cap = 40 (10 240 lm_head rows x 50 304 columns), in bf16 and split-bf16:

  (a) the scoring pass end to end: ClipCapEngine.score from a mapped prefix (cc_gpt2_embed + cc_gpt2_fwd + cc_lmhead_score);
  (b) the route to the same numbers that needs no scoring entry point: Gpt2Engine.logits on all B T rows, then log_softmax and
      gather in torch;
  (c) the lm_head launch alone (CC_SITE_LMHEAD_FWD, HIP events recorded by the library around the launch): the storing form of
      cc_lmhead_ce_fwd against the store-free form of cc_lmhead_score.

Method: every variant is warmed up first; the variants of a comparison ALTERNATE inside one process (a, b, a, b, ...), each
repetition timed with HIP events; medians are reported, with the spread of repeated same-variant medians over --blocks blocks as the
same-box noise figure.  Also reports the peak workspace bytes of (a) and (b).  Parameters are random (the timing does not depend on
them).  Prints one JSON line per precision and, with --markdown, the table for profiles/.

    python tools/score_bench.py [--reps 20] [--blocks 3] [--precisions bf16,32] [--markdown out.md]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from clipcap_amd import _lib  # noqa: E402
from clipcap_amd.engine import ClipCapEngine, Gpt2Engine, MapperEngine  # noqa: E402

B, L, CAP, D, H, NL, V, NPOS, E = 256, 10, 40, 768, 12, 12, 50257, 1024, 512


def timed(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def site_ms(lib, fn, reps):
    """durations of the CC_SITE_LMHEAD_FWD launches of `reps` calls of fn (one launch per call)"""
    lib.cc_prof_start(_lib.SITES["lmhead_fwd"], reps)
    torch.cuda.synchronize()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    n = C.c_int32(reps)
    ms = (C.c_float * reps)()
    lib.cc_prof_stop(ms, None, C.byref(n))
    return [ms[i] for i in range(n.value)]


def run(precision, reps, blocks):
    lib = _lib.lib()
    torch.manual_seed(0)
    me = MapperEngine(E, D, L, L, 8, 8, device="cuda", precision=precision)
    ge = Gpt2Engine(D, H, NL, V, NPOS, device="cuda", precision=precision)
    for eng in (me, ge):
        for k, v in eng.views(eng.arena.w32).items():
            v.copy_(1.0 + 0.05 * torch.randn(v.shape) if ("ln_" in k or "norm" in k) and k.endswith("weight") else 0.02 * torch.randn(v.shape))
    eng = ClipCapEngine(me, ge, train_lm=False)
    gen = torch.Generator().manual_seed(1)
    tokens = torch.randint(1, V, (B, CAP), generator=gen)
    lengths = torch.randint(8, CAP + 1, (B,), generator=gen)
    tokens[torch.arange(CAP).view(1, -1) >= lengths.view(-1, 1)] = -1
    tokens = tokens.cuda()
    prefix = me.forward(torch.randn(B, E, generator=gen).cuda()).clone()
    wte = ge.views(ge.arena.w32)["transformer.wte.weight"]
    stream = torch.cuda.current_stream()

    def new_route():
        return eng.score(tokens, prefix=prefix)

    def old_route():
        x = torch.cat((prefix, wte[tokens.clamp_min(0)]), dim=1)
        lg = ge.logits(x)[:, L - 1:-1]
        lp = torch.log_softmax(lg, dim=-1).gather(2, tokens.clamp_min(0).unsqueeze(-1)).squeeze(-1)
        lp = torch.where(tokens >= 0, lp, torch.zeros_like(lp))
        return lp, lp.sum(dim=1), (tokens >= 0).sum(dim=1)

    # same numbers first (measuring-on-mi355x: faster and different is not faster)
    a, b = new_route(), old_route()
    torch.cuda.synchronize()
    diff = float((a[0] - b[0]).abs().max())
    # peak bytes of each route beyond what is resident before it (parameters, inputs)
    peaks = {}
    for name, fn in (("a", new_route), ("b", old_route)):
        eng._score_ws = None
        ge._ws.clear()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated() - base
        del out
    shp = ge.shape(B, L, L + CAP, CAP, 0)
    ws_a = lib.cc_gpt2_ws_bytes(C.byref(ge.cfg), C.byref(shp))
    shp_b = ge.shape(B, L + CAP, L + CAP, 0, 0)
    ws_b = lib.cc_gpt2_ws_bytes(C.byref(ge.cfg), C.byref(shp_b))
    for _ in range(3):
        new_route()
        old_route()
    torch.cuda.synchronize()
    med = {"a": [], "b": []}
    for _ in range(blocks):
        ta, tb = [], []
        for _ in range(reps):
            ta.append(timed(new_route, stream))
            tb.append(timed(old_route, stream))
        med["a"].append(statistics.median(ta))
        med["b"].append(statistics.median(tb))

    # (c) the lm_head launch alone: a mode-1 pass for the storing form, the mode-0 scoring pass for the store-free form
    shp1 = ge.shape(B, L, L + CAP, CAP, 1)
    ws1 = ge.workspace(shp1)
    st = C.c_void_p(stream.cuda_stream)
    ga = ge.arena
    stats = torch.zeros(2, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    _lib.check(lib.cc_gpt2_embed(C.byref(ge.cfg), C.byref(shp1), p(ga.w32), p(prefix), p(tokens), p(ws1), st))
    _lib.check(lib.cc_gpt2_fwd(C.byref(ge.cfg), C.byref(shp1), p(ga.w32), p(ga.w16), p(ws1), st))
    ws0 = eng._score_workspace(shp)
    _lib.check(lib.cc_gpt2_embed(C.byref(ge.cfg), C.byref(shp), p(ga.w32), p(prefix), p(tokens), p(ws0), st))
    _lib.check(lib.cc_gpt2_fwd(C.byref(ge.cfg), C.byref(shp), p(ga.w32), p(ga.w16), p(ws0), st))
    out = torch.empty(B, CAP, device="cuda")
    sst = torch.empty(B, 2, device="cuda")

    def storing():
        _lib.check(lib.cc_lmhead_ce_fwd(C.byref(ge.cfg), C.byref(shp1), p(ga.w32), p(ga.w16), p(ws1), p(tokens), p(stats), st))

    def store_free():
        _lib.check(lib.cc_lmhead_score(C.byref(ge.cfg), C.byref(shp), p(ga.w32), p(ga.w16), p(ws0), p(tokens), 0, p(out), p(sst), st))
    for _ in range(3):
        storing()
        store_free()
    lm = {"storing": [], "store_free": []}
    for _ in range(blocks):
        s1, s2 = [], []
        for _ in range(max(1, reps // 5)):          # alternate in groups of 5 launches
            s1 += site_ms(lib, storing, 5)
            s2 += site_ms(lib, store_free, 5)
        lm["storing"].append(statistics.median(s1))
        lm["store_free"].append(statistics.median(s2))

    def mid(v):
        return statistics.median(v)

    def spread(v):
        return (max(v) - min(v)) / mid(v) if len(v) > 1 else 0.0
    return dict(precision=str(precision), B=B, L=L, cap=CAP, reps=reps, blocks=blocks, max_abs_diff_a_vs_b=diff,
                score_ms=mid(med["a"]), logits_route_ms=mid(med["b"]), score_spread=spread(med["a"]), logits_route_spread=spread(med["b"]),
                lmhead_storing_ms=mid(lm["storing"]), lmhead_store_free_ms=mid(lm["store_free"]), lmhead_storing_spread=spread(lm["storing"]),
                lmhead_store_free_spread=spread(lm["store_free"]), score_ws_bytes=int(ws_a), logits_route_ws_bytes=int(ws_b),
                score_peak_bytes=int(peaks["a"]), logits_route_peak_bytes=int(peaks["b"]))


def markdown(rows):
    out = ["# Caption scoring: store-free lm_head against the logits route", "",
           f"GPT-2 small, B = {B}, L = {L}, cap = {CAP} ({B * CAP} lm_head rows x 50 304 columns).  `tools/score_bench.py`: variants alternate in one",
           "process, HIP events, medians of medians over blocks; spread = (max - min) / median of the per-block medians of ONE variant (same-box noise).", "",
           "| precision | (a) score, ms | (b) logits + log_softmax + gather, ms | b / a | spread a / b | lm_head storing, ms | lm_head store-free, ms | store-free / storing | spread | peak bytes a | peak bytes b | max abs diff a vs b |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['precision']} | {r['score_ms']:.3f} | {r['logits_route_ms']:.3f} | {r['logits_route_ms'] / r['score_ms']:.2f} | "
                   f"{100 * r['score_spread']:.1f} % / {100 * r['logits_route_spread']:.1f} % | {r['lmhead_storing_ms']:.4f} | {r['lmhead_store_free_ms']:.4f} | "
                   f"{r['lmhead_store_free_ms'] / r['lmhead_storing_ms']:.3f} | {100 * r['lmhead_storing_spread']:.1f} % / {100 * r['lmhead_store_free_spread']:.1f} % | "
                   f"{r['score_peak_bytes'] / 1e9:.3f} GB (workspace {r['score_ws_bytes'] / 1e9:.3f}) | {r['logits_route_peak_bytes'] / 1e9:.3f} GB (workspace "
                   f"{r['logits_route_ws_bytes'] / 1e9:.3f}) | {r['max_abs_diff_a_vs_b']:.2e} |")
    out += ["", "The lm_head columns time the one launch inside `CC_SITE_LMHEAD_FWD`.  In bf16 the storing launch is the training path's exponential-form",
            "epilogue, whose target-logit pre-kernel (`lm_tgt_ref`) runs outside the timed site: the comparison is between the two launches as the",
            "library issues them, slightly in the storing form's favour, not between two epilogues of equal arithmetic.  Peak bytes: torch's peak",
            "allocation during one call above what was resident before it (workspace + outputs + torch temporaries)."]
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20, help="alternating repetitions per block")
    ap.add_argument("--blocks", type=int, default=3, help="blocks (their medians give the same-box spread)")
    ap.add_argument("--precisions", default="bf16,32")
    ap.add_argument("--markdown", default="", help="also write the table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("score_bench.py measures on an MI355X; no GPU found (nothing is estimated on the CPU)")
    rows = []
    for pr in args.precisions.split(","):
        pr = pr.strip()
        rows.append(run(int(pr) if pr.isdigit() else pr, args.reps, args.blocks))
        print(json.dumps(rows[-1]), flush=True)
        torch.cuda.empty_cache()
    if args.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(args.markdown)), exist_ok=True)
        open(args.markdown, "w").write(markdown(rows))


if __name__ == "__main__":
    main()
