#!/usr/bin/env python
"""What the MLP mapping network costs at the shape of the original ClipCap checkpoints: E = 512, D = 768, L = 10 (Hd = 3840, 31 468 800
parameters), B in {16, 256, 1024}, bf16 and split-bf16 operands.

Per (precision, B): the forward (MlpMapperEngine.forward, save = False), and forward (save = True) + backward into the gradient arena, each timed
with HIP events around `--reps` back-to-back engine calls after a warm-up, the median of `--blocks` such blocks reported with the spread
of the block figures as the same-box noise.  Beside it the same MLP through torch.nn (Linear, Tanh, Linear under autocast to bf16 for the
bf16 row, plain fp32 for the split-bf16 row) in the same process, as a yardstick, not a target.

Bytes a pass must move (the algorithmic minimum, computed here from the shapes; n = parameter count, |W2| = L D x Hd):
    forward    the weight operands once: 2 n bytes in bf16 (6 n in split-bf16: three 16-bit planes), + activations x16, h, out
    backward   W2's transposed operand copy once (2 |W2|, split-bf16 6 |W2|), the fp32 gradient arena read and written (8 n), + activations
               g16, h, t, dU, x16 once each
and the fraction of 6.3 TB/s (the achievable HBM rate DESIGN.md uses) that the measured time leaves of them.  Nothing is asserted: it is a
record, and nothing is tuned to it.

    python tools/mlp_mapper_bench.py [--reps 20] [--blocks 5] [--markdown profiles/mlp_mapper_bench.md]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

E, D, L = 512, 768, 10
BATCHES = (16, 256, 1024)
HBM = 6.3e12


def pass_bytes(B, x3):
    """(forward, forward + backward) algorithmic bytes"""
    Hd, LD = L * D // 2, L * D
    n = Hd * E + Hd + LD * Hd + LD
    w2 = LD * Hd
    op, act = (6, 4) if x3 else (2, 2)
    fwd = op * n + B * (4 * E + act * E + act * Hd + 4 * LD)                      # emb in, x16 out; h out (read back from cache); out
    bwd = op * w2 + 8 * n + B * (4 * LD + act * LD + act * (3 * Hd) + act * E)     # dout in, g16; h, t, dU; x16
    return fwd, fwd + B * act * Hd + bwd                                           # (the saving forward also writes t)


def spread(v):
    return (max(v) - min(v)) / statistics.median(v) if len(v) > 1 else 0.0


def time_blocks(fn, reps, blocks):
    """median over `blocks` of (HIP-event time of `reps` back-to-back calls) / reps, in microseconds, and the blocks' spread"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        per.append(a.elapsed_time(b) * 1e3 / reps)
    return statistics.median(per), spread(per)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--markdown", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mlp_mapper_bench needs an MI355X: nothing here is measured on the CPU")
    from clipcap_amd.engine import MlpMapperEngine
    rows = []
    for prec, x3 in (("bf16", False), (32, True)):
        eng = MlpMapperEngine(E, D, L, device="cuda", precision=prec)
        g = torch.Generator().manual_seed(0)
        for k, v in eng.views(eng.arena.w32).items():
            v.copy_(torch.randn(v.shape, generator=g) * (0.02 if k.endswith("bias") else 1.0 / v.shape[-1] ** 0.5))
        ref = torch.nn.Sequential(torch.nn.Linear(E, L * D // 2), torch.nn.Tanh(), torch.nn.Linear(L * D // 2, L * D)).cuda()
        ref.load_state_dict({k[len("model."):]: v for k, v in eng.views(eng.arena.w32).items()})
        assert eng.arena.n == 31_468_800
        for B in BATCHES:
            emb = torch.randn(B, E, generator=g).cuda()
            dout = (torch.randn(B, L, D, generator=g) * 0.01).cuda()
            eng.arena.grads().zero_()

            def fwd():
                eng.forward(emb, save=False)

            def step():
                eng.forward(emb, save=True)
                eng.backward(dout)

            def tfwd():
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=not x3):
                    ref(emb)

            def tstep():
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=not x3):
                    out = ref(emb)
                out.backward(dout.view(B, -1).to(out.dtype))      # gradients accumulate into .grad, as the engine's do into its arena
            out = eng.forward(emb, save=False)
            with torch.no_grad():
                want = ref(emb).view(B, L, D)
            err = float((out - want).abs().max() / want.abs().max())
            f_us, f_sp = time_blocks(fwd, args.reps, args.blocks)
            s_us, s_sp = time_blocks(step, args.reps, args.blocks)
            tf_us, _ = time_blocks(tfwd, args.reps, args.blocks)
            ts_us, _ = time_blocks(tstep, args.reps, args.blocks)
            fb, sb = pass_bytes(B, x3)
            row = dict(precision="split-bf16" if x3 else "bf16", B=B, fwd_us=round(f_us, 1), fwd_spread=round(f_sp, 3), step_us=round(s_us, 1),
                       step_spread=round(s_sp, 3), fwd_MB=round(fb / 1e6, 1), step_MB=round(sb / 1e6, 1),
                       fwd_hbm_frac=round(fb / HBM / (f_us * 1e-6), 3), step_hbm_frac=round(sb / HBM / (s_us * 1e-6), 3),
                       torch_fwd_us=round(tf_us, 1), torch_step_us=round(ts_us, 1), rel_err_vs_torch_fp32=float(f"{err:.2e}"))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.markdown:
        os.makedirs(os.path.dirname(os.path.abspath(args.markdown)), exist_ok=True)
        with open(args.markdown, "w") as f:
            f.write("# MLP mapping network at E = 512, D = 768, L = 10 (31 468 800 parameters)\n\n"
                    f"`python tools/mlp_mapper_bench.py --reps {args.reps} --blocks {args.blocks}` on one MI355X; HIP events around {args.reps} back-to-back "
                    f"engine calls, median of {args.blocks} blocks (spread = (max - min) / median of the blocks).  MB = the bytes the pass must move "
                    "(tools/mlp_mapper_bench.py pass_bytes); HBM = those bytes / 6.3 TB/s / the measured time.  torch = the same MLP through "
                    "torch.nn in the same process (bf16 autocast for the bf16 rows, fp32 for the split-bf16 rows).\n\n"
                    "| operands | B | fwd us (spread) | fwd MB | fwd HBM | fwd+bwd us (spread) | fwd+bwd MB | fwd+bwd HBM | torch fwd us | torch fwd+bwd us |\n"
                    "|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                f.write(f"| {r['precision']} | {r['B']} | {r['fwd_us']} ({r['fwd_spread']}) | {r['fwd_MB']} | {r['fwd_hbm_frac']} | {r['step_us']} "
                        f"({r['step_spread']}) | {r['step_MB']} | {r['step_hbm_frac']} | {r['torch_fwd_us']} | {r['torch_step_us']} |\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
