#!/usr/bin/env python
"""bench.py — ClipCap training-step throughput on MI355X (BASELINE.json metric: train samples/sec, 512-d prefix input,
40-token captions), one process per GPU, weak scaling (per-GPU batch fixed).

    python bench.py --gpus 1 --steps 10 --warmup 3
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

A "step" = one pass of the hot path over one batch of synthetic (embedding, caption) pairs already resident in HBM:
mapper forward -> [prefix ; tokens] -> GPT-2 forward -> fused lm_head + cross-entropy -> backward through GPT-2 (dgrad;
+wgrad when --config 3) -> mapper backward -> (N>1: RCCL all-reduce of the gradient arena) -> fused AdamW + LR schedule.
Nothing is skipped inside the timed region.  Rank 0 prints ONE JSON line (see DESIGN.md §Measurement for every field).

A plain run sets up, warms up, times the --steps steps, writes --dump-outputs and prints the headline line.  --full adds everything else
the line can carry: the exposed all-reduce pass (N > 1), the event-bracketed roofline passes, the sub-benches (mapper, decode, configs[2] /
[3], e2e input path, the other precisions) and the CPU baselines (--no-roofline-pass / --no-sub-benches / --no-cpu-baseline drop parts of it).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIGS = {
    # BASELINE.json configs[1]: TransformerMapper (8 layers, prefix_len=10) + frozen GPT-2-small, bf16, batch 256
    "2": dict(name="TransformerMapper(8L,P=L=10,H=8)+frozen GPT-2-small", E=512, P=10, L=10, H=8, N=8, D=768, n_head=12, n_layer=12,
              V=50257, npos=1024, B=256, cap=40, train_lm=False),
    # configs[2]: same mapper, GPT-2-small unfrozen
    "3": dict(name="TransformerMapper(8L)+GPT-2-small full finetune", E=512, P=10, L=10, H=8, N=8, D=768, n_head=12, n_layer=12, V=50257,
              npos=1024, B=256, cap=40, train_lm=True),
    # configs[3]: CLAP 1024-d -> GPT-2-medium
    "4": dict(name="TransformerMapper(8L,E=1024)+GPT-2-medium full finetune", E=1024, P=10, L=10, H=8, N=8, D=1024, n_head=16, n_layer=24,
              V=50257, npos=1024, B=128, cap=40, train_lm=True),
    # configs[0]-like small case (what the CPU baseline runs): B=16
    "1": dict(name="TransformerMapper(8L)+frozen GPT-2-small, B=16", E=512, P=10, L=10, H=8, N=8, D=768, n_head=12, n_layer=12, V=50257,
              npos=1024, B=16, cap=40, train_lm=False),
}

PEAK_BF16_TFLOPS = 2500.0   # MI355X dense bf16 MFMA peak (/opt/skills/guides/MI355X_MICROARCH.md)
# Offline PMC measurements quoted in the JSON line (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate passes, FETCH x2 gfx950
# correction; tools/profile_round.sh writes them to profiles/pmc_constants.json together with a hash of the kernel sources they were
# measured on).  bench.py does not read counters itself: when the sources have changed since the passes were taken, the numbers would
# describe another build, and the fields are reported as null (with the reason) instead of silently going stale.
ROOT = os.path.dirname(os.path.abspath(__file__))
DUMP_BYTES = 64 << 20         # --dump-outputs: at most this much in all
DUMP_SAMPLE = 2 << 20         # a tensor larger than this many elements is dumped as a fixed, seeded sample of this size


def region_sizes(steps, regions):
    """--steps timed steps in all, split into at most --regions back-to-back regions of near-equal length."""
    n = max(1, min(regions, steps))
    return [steps // n + (1 if r < steps % n else 0) for r in range(n)]


def dump_sample(t, seed):
    """t flattened; if longer than DUMP_SAMPLE, the elements at DUMP_SAMPLE indices drawn (sorted, no repeats) by numpy's seeded
    generator: the same positions for the same seed and length in every run and build."""
    t = t.detach().reshape(-1)
    if t.numel() <= DUMP_SAMPLE:
        return t
    idx = np.sort(np.random.default_rng(seed).choice(t.numel(), DUMP_SAMPLE, replace=False))
    return t[torch.from_numpy(idx).to(t.device)]


def dump_outputs(dirname, arrays):
    """--dump-outputs: {name: tensor} -> dirname/<name>.npy, float64 kept as float64, everything else as float32."""
    out = {}
    for name, t in arrays.items():
        t = torch.as_tensor(t).detach().cpu()
        out[name] = t.numpy() if t.dtype == torch.float64 else t.float().numpy()
    total = sum(a.nbytes for a in out.values())
    if total > DUMP_BYTES:
        raise RuntimeError(f"--dump-outputs: {total} bytes exceed the {DUMP_BYTES}-byte budget")
    os.makedirs(dirname, exist_ok=True)
    for name, a in out.items():
        np.save(os.path.join(dirname, f"{name}.npy"), a)


def train_step_outputs(loss, eng):
    """What a caller of the training step receives: the loss, and per trained arena the gradients of the step and the weights after its
    optimizer update (samples of them when large)."""
    out = {"loss": loss.reshape(1)}
    if eng is not None:
        for k, a in enumerate(eng.arenas()):
            name = "mapper" if k == 0 else "gpt2"
            out[f"{name}_grads"] = dump_sample(a.grads(), 100 + k)
            out[f"{name}_weights"] = dump_sample(a.w32, 200 + k)
    return out


def kernel_source_hash():
    """sha256 over the kernel sources + the public header (what decides the machine code of libclipcap_hip.so)."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "clipcap_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".h", ".cpp")) or f == "Makefile":
            h.update(f.encode())
            h.update(open(os.path.join(d, f), "rb").read())
    h.update(open(os.path.join(ROOT, "include", "clipcap_hip.h"), "rb").read())
    return h.hexdigest()[:16]


def mfma_busy_constant(label, symbol_substr=None):
    """Offline MFMA-pipe utilisation (SQ_VALU_MFMA_BUSY_CYCLES / 32 / GRBM_GUI_ACTIVE, tools/mfma_util.py via tools/profile_round.sh) from
    profiles/pmc_constants.json: the GEMM family's cycle-weighted figure of run `label` ("train", "x3_train", "decode"), or one kernel's
    (first symbol containing symbol_substr).  {"value": float | None, "source", "stale"}: None when absent or measured on other kernel sources."""
    try:
        with open(os.path.join(ROOT, "profiles", "pmc_constants.json")) as f:
            e = json.load(f)["mfma_busy"]
        run = e[label]
    except (OSError, KeyError, ValueError):
        return {"value": None, "source": None, "stale": "no offline MFMA-utilisation pass recorded (profiles/pmc_constants.json)"}
    cur = kernel_source_hash()
    if e.get("kernel_source_hash") != cur:
        return {"value": None, "source": e.get("source"), "stale": f"kernel sources changed since the counter pass (pass: {e.get('kernel_source_hash')}, now: {cur})"}
    if symbol_substr is None:
        v = run.get("gemm_family")
    else:
        v = next((b for k, b in run.get("per_kernel", {}).items() if symbol_substr in k), None)
    return {"value": round(v, 4) if v is not None else None, "source": e.get("source"), "stale": None}


def pmc_constant(name):
    """{"bytes": int | None, "source": str, ...} for one offline counter measurement; bytes = None when absent or stale."""
    path = os.path.join(ROOT, "profiles", "pmc_constants.json")
    try:
        with open(path) as f:
            all_ = json.load(f)
        e = dict(all_[name])
    except (OSError, KeyError, ValueError):
        return {"bytes": None, "source": None, "stale": "no offline PMC pass recorded (profiles/pmc_constants.json)"}
    cur = kernel_source_hash()
    if e.get("kernel_source_hash") != cur:
        return {"bytes": None, "source": e.get("source"), "stale": f"kernel sources changed since the PMC pass (pass: {e.get('kernel_source_hash')}, now: {cur})"}
    return e


def mapper_flops_fwd(c):   # 2*E*P*D + N*[S*2*D*(D+2D+D+rD+rD) + 4*S^2*D], r=2
    S = c["P"] + c["L"]
    D = c["D"]
    return 2 * c["E"] * c["P"] * D + c["N"] * (S * 2 * D * (D + 2 * D + D + 2 * D + 2 * D) + 4 * S * S * D)


def gpt2_flops_fwd(c):     # n_layer*[T*24*D^2 + 4*T^2*D] + 2*D*V*T
    T = c["L"] + c["cap"]
    D = c["D"]
    return c["n_layer"] * (T * 24 * D * D + 4 * T * T * D) + 2 * D * c["V"] * T


def step_flops(c):         # frozen: 3*mapper + 2*LM ; full: 3*(mapper+LM)   (per sample)
    m, g = mapper_flops_fwd(c), gpt2_flops_fwd(c)
    return 3 * m + (3 if c["train_lm"] else 2) * g


def gemm_family_algorithmic_bytes(c):
    """HBM bytes one training step's GEMM launches need if every operand is read once and every output written once (the yardstick for
    the counter-measured `traffic` of the GEMM family).  Accounting per launch: A + B operands (16-bit), the output (16-bit, or fp32 for
    residual streams / weight gradients), and what the fused epilogue reads (fp32 residual, the stored gelu' tensor)."""
    B, cap, D, NL, V = c["B"], c["cap"], c["D"], c["n_layer"], c["V"]
    Vp = (V + 127) // 128 * 128
    M, Mc = B * (c["L"] + cap), B * cap                        # GPT-2 rows, lm_head rows
    h, f = 2, 4                                                # bytes: 16-bit operand, fp32

    def lin(m, k, n, out_b, extra=0):                          # forward-shaped launch: A [m,k], W [n,k], out [m,n]
        return m * k * h + n * k * h + m * n * out_b + extra

    fwd = NL * (lin(M, D, 3 * D, h) + lin(M, D, D, f, M * D * f) + lin(M, D, 4 * D, h, M * 4 * D * h) + lin(M, 4 * D, D, f, M * D * f))
    dgrad = NL * (lin(M, D, 4 * D, h, M * 4 * D * h) + lin(M, 4 * D, D, h) + lin(M, D, D, h) + lin(M, 3 * D, D, h))
    wgrad = NL * sum(M * (k + n) * h + k * n * f for k, n in ((D, 3 * D), (D, D), (D, 4 * D), (4 * D, D))) if c["train_lm"] else 0
    head = lin(Mc, D, Vp, h) + (Mc * Vp * h + Vp * D * h + Mc * D * h + 2 * Mc * D * f) + ((Mc * (Vp + D)) * h + Vp * D * f if c["train_lm"] else 0)
    Mm, Dm, r = B * (c["P"] + c["L"]), D, 2
    m_fwd = c["N"] * (lin(Mm, Dm, 3 * Dm, h) + lin(Mm, Dm, Dm, f, Mm * Dm * f) + lin(Mm, Dm, r * Dm, h) + lin(Mm, r * Dm, Dm, f, Mm * Dm * f))
    m_dgrad = c["N"] * (lin(Mm, Dm, r * Dm, h, Mm * r * Dm * h) + lin(Mm, r * Dm, Dm, h) + lin(Mm, Dm, Dm, h) + lin(Mm, 3 * Dm, Dm, h))
    m_wgrad = c["N"] * sum(Mm * (k + n) * h + k * n * f for k, n in ((Dm, 3 * Dm), (Dm, Dm), (Dm, r * Dm), (r * Dm, Dm)))
    m_lin = 3 * (B * c["E"] * h + c["E"] * c["P"] * Dm * h + B * c["P"] * Dm * f)
    return {"gpt2_forward": int(fwd), "gpt2_input_gradients": int(dgrad), "gpt2_weight_gradients": int(wgrad), "lm_head": int(head),
            "mapper": int(m_fwd + m_dgrad + m_wgrad + m_lin), "total": int(fwd + dgrad + wgrad + head + m_fwd + m_dgrad + m_wgrad + m_lin)}


def init_engines(c, device, seed=1234):
    from clipcap_amd.engine import ClipCapEngine, Gpt2Engine, MapperEngine
    gen = torch.Generator(device=device).manual_seed(seed)
    me = MapperEngine(c["E"], c["D"], c["L"], c["P"], c["H"], c["N"], device=device)
    ge = Gpt2Engine(c["D"], c["n_head"], c["n_layer"], c["V"], c["npos"], device=device)
    for k, v in me.views(me.arena.w32).items():   # torch default init of the reference modules (mapper.py:118-120)
        if "norm" in k:
            v.fill_(1.0 if k.endswith("weight") else 0.0)
        elif k == "prefix_const":
            v.copy_(torch.randn(v.shape, generator=gen, device=device))
        else:
            fan_in = v.shape[-1] if v.dim() == 2 else {"linear.bias": c["E"]}.get(k, c["D"])
            bound = 1.0 / fan_in ** 0.5
            v.copy_((torch.rand(v.shape, generator=gen, device=device) * 2 - 1) * bound)
    for k, v in ge.views(ge.arena.w32).items():   # GPT2Config init: N(0, 0.02), LN = identity, biases 0
        if "ln_" in k:
            v.fill_(1.0 if k.endswith("weight") else 0.0)
        elif k.endswith(".bias"):
            v.zero_()
        else:
            v.copy_(torch.randn(v.shape, generator=gen, device=device) * 0.02)
    return me, ge, ClipCapEngine(me, ge, c["train_lm"])


def cpu_baseline(c, warm=3, timed=10, max_seconds=75.0):
    """The CPU oracle (oracle/clipcap_oracle.py, fp32 torch-CPU restatement pinned to the reference's golden outputs) timed on
    this box's host cores on a bounded sample of the same workload: the same model at batch 16 (BASELINE configs[0] size),
    BASELINE.md 3: 3 warm-up + 10 timed training steps (fwd + bwd + AdamW + schedule), median step time; stops early at max_seconds."""
    from oracle import clipcap_oracle as O
    torch.manual_seed(0)
    Bc = 16
    from clipcap_amd.engine import Gpt2Engine, MapperEngine
    me = MapperEngine(c["E"], c["D"], c["L"], c["P"], c["H"], c["N"], device="cpu")
    ge = Gpt2Engine(c["D"], c["n_head"], c["n_layer"], c["V"], c["npos"], device="cpu")
    sd = {}
    for pre, eng in (("transformer_mapper.", me), ("language_model.", ge)):
        for k, v in eng.views(eng.arena.w32).items():
            if "norm" in k or "ln_" in k:
                v.fill_(1.0 if k.endswith("weight") else 0.0)
            else:
                v.normal_(0, 0.02)
            sd[pre + k] = v
    train = [k for k in sd if k.startswith("transformer_mapper.") or c["train_lm"]]
    for k in train:
        sd[k].requires_grad_(True)
    tokens = torch.randint(1, c["V"], (Bc, c["cap"]))
    embeds = torch.randn(Bc, c["E"])
    cfg = dict(projection_length=c["P"], prefix_length=c["L"], heads=c["H"], layers=c["N"], n_head=c["n_head"], n_layer=c["n_layer"])
    m = {k: torch.zeros_like(sd[k]) for k in train}
    v = {k: torch.zeros_like(sd[k]) for k in train}
    times = []
    t_begin = time.time()
    for step in range(warm + timed):
        t0 = time.time()
        for k in train:
            sd[k].grad = None
        loss = O.clipcap_loss(sd, tokens, embeds, cfg=cfg)
        loss.backward()
        lr = 2e-5 * O.linear_schedule_factor(step, 2, warm + timed + 1)
        with torch.no_grad():
            for k in train:
                pn, m[k], v[k] = O.adamw_step(sd[k], sd[k].grad, m[k], v[k], step + 1, lr)
                sd[k].copy_(pn)
        times.append(time.time() - t0)
        if time.time() - t_begin > max_seconds and len(times) > warm + 1:
            break
    steady = sorted(times[warm:])
    med = steady[len(steady) // 2]
    return {"value": round(Bc / med, 3), "unit": "samples/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"oracle fp32 torch-CPU training step (fwd+bwd+AdamW+schedule), same model, batch {Bc}: {warm} warm-up + "
                      f"{len(steady)} timed steps, median {med * 1e3:.0f} ms (min {steady[0] * 1e3:.0f}, max {steady[-1] * 1e3:.0f})"}


def cpu_decode_baseline(max_seconds=14.0):
    """CPU decode baselines of BASELINE.md 3 on the oracle: beam 5, GPT-2-medium (random init), ONE prefix of 10 rows, reference
    semantics (no KV cache: the whole sequence is re-forwarded every step, inference/base.py:80-121) and the same search with a
    KV cache.  Bounded: 16 generated positions (no-cache) / 32 (cached); generated best-beam tokens per second."""
    from oracle import clipcap_oracle as O
    from clipcap_amd.engine import Gpt2Engine
    torch.manual_seed(0)
    D, NL, H = 1024, 24, 16
    ge = Gpt2Engine(D, H, NL, 50257, 1024, device="cpu")
    sd = {}
    for k, v in ge.views(ge.arena.w32).items():
        if "ln_" in k:
            v.fill_(1.0 if k.endswith("weight") else 0.0)
        else:
            v.normal_(0, 0.02)
        sd["language_model." + k] = v
    pref = torch.randn(1, 10, D) * 0.5
    out = {}
    with torch.no_grad():
        for name, n, kv in (("no_cache", 16, False), ("kv_cache", 32, True)):
            O.generate_beam_tokens(sd, pref, n_head=H, n_layer=NL, beam_size=5, entry_length=2, stop_token=50256, kv_cache=kv)   # warm-up
            t0 = time.time()
            toks, sc, lens, order = O.generate_beam_tokens(sd, pref, n_head=H, n_layer=NL, beam_size=5, entry_length=n, stop_token=50256,
                                                           kv_cache=kv)
            dt = time.time() - t0
            out[name] = {"value": round(float(lens[order[0]]) / dt, 2), "unit": "tokens/s", "generated_positions": int(toks.shape[1]),
                         "seconds": round(dt, 2)}
    out.update(cores=torch.get_num_threads(), kind="port",
               sample="oracle beam-5 decode, GPT-2-medium random init, 1 prefix x 10 rows; no_cache = the reference's full re-forward per step")
    return out


def decode_bench(args, device):
    """BASELINE configs[4]: beam-search (beam=5) caption decode, GPT-2-medium, KV-cached HIP kernels, 64 prefixes per step.
    A "step" = decoding the whole batch (prefill of the 10-row prefix + up to 67 generated tokens per beam).
    traffic: HBM bytes per generated position from offline PMC passes (tagged with their source) — not measured by this run."""
    from types import SimpleNamespace
    from clipcap_amd.inference.base import generate_beam_tokens
    from clipcap_amd.model.gpt2 import GPT2LM
    torch.manual_seed(1234)
    lm = GPT2LM(n_embd=1024, n_layer=24, n_head=16, vocab_size=50257, n_positions=1024).to(device)
    model = SimpleNamespace(language_model=lm)
    S, L, beam, entry = args.batch or 64, 10, 5, 67
    prefix = torch.randn(S, L, 1024, device=device) * 0.5
    for _ in range(max(1, args.warmup)):
        generate_beam_tokens(model, prefix, beam, entry, 1.0, 50256)
    # `steps` timed decodes in all, split into up to `regions` timed regions (box-to-box and run-to-run spread of this number exceeds most
    # decode changes: the median region's time per decode is reported, min / max beside it)
    sizes = region_sizes(args.steps, max(1, int(getattr(args, "regions", 3) or 3)))
    regions = len(sizes)
    each = []
    for k in sizes:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            toks, scores, lens = generate_beam_tokens(model, prefix, beam, entry, 1.0, 50256)
            best = scores.argmax(dim=1)
            gen = int(lens.gather(1, best[:, None]).sum())      # tokens of one decode (every decode runs the same inputs)
        torch.cuda.synchronize()
        each.append((time.perf_counter() - t0) / k)
    if getattr(args, "dump_outputs", None):
        dump_outputs(args.dump_outputs, {"tokens": toks.double(), "scores": scores, "seq_lengths": lens})
    dt = sorted(each)[len(each) // 2]
    steps_per_decode = toks.shape[2]
    wbytes = 2.0 * (lm.engine.arena.n - (lm.engine.dims["NPOS"] * 1024))     # bf16 weights read once per decode step
    # + the KV cache rows the step attends to.  Upper bound: every beam row reads its whole history (what a per-row
    # attention kernel fetches): 2 * n_layer * ctx * D * 2 B per row.  MEASURED: the beam-group attention step reads every distinct
    # (cache row, position) of a caption's beams once — counted from the ancestry tables of one extra, untimed decode.
    ctx_avg = L + (steps_per_decode - 1) / 2.0
    kvbytes_ub = 2.0 * 24 * ctx_avg * 1024 * 2 * S * beam
    rows_distinct = decode_distinct_rows(model, prefix, beam, entry)
    kvbytes = 2.0 * 24 * rows_distinct * 1024 * 2
    tr = pmc_constant("decode_bytes_per_position") if S == 64 else {"bytes": None, "source": None, "stale": "offline pass is for 64 prefixes"}
    per_pos_s = dt / steps_per_decode
    return {"metric": "decode tok/s (beam=5, GPT-2-medium, KV cache)", "value": round(gen / dt, 1), "unit": "tokens/s", "n_gpus": 1,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt * 1e3, 2), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
            "config": {"workload": "BASELINE configs[4]: beam=5 decode, GPT-2-medium random init, 64 prefixes x 10 rows, 67 new tokens",
                       "prefixes": S, "beam": beam, "entry_length": entry, "generated_steps": steps_per_decode},
            "beam_tokens_per_s": round(gen * beam / dt, 1),
            "timed_regions": {"regions": regions, "decodes_per_region": sizes, "statistic": "median region",
                              "ms_per_batch_each": [round(e * 1e3, 2) for e in each],
                              "tokens_per_s_min": round(gen / max(each), 1), "tokens_per_s_max": round(gen / min(each), 1)},
            "roofline": {"bound": "hbm", "kernel": "whole decode step (weights once per generated position + the distinct KV rows of every beam group)",
                         "achieved": round((wbytes + kvbytes) / per_pos_s / 1e9, 1), "peak": 8000.0, "unit": "GB/s",
                         "frac": round((wbytes + kvbytes) / per_pos_s / 8e12, 4),
                         "frac_weights_only": round(wbytes / per_pos_s / 8e12, 4),
                         "algorithmic_bytes_per_position": int(wbytes + kvbytes),
                         "weight_bytes_per_position": int(wbytes),
                         "kv_read_bytes_per_position": int(kvbytes),
                         "kv_read_bytes_per_position_per_row_kernel": int(kvbytes_ub),
                         "us_per_position": round(per_pos_s * 1e6, 1),
                         # fabric bytes per generated position from separate PMC passes (FETCH_SIZE x2 on gfx950 + WRITE_SIZE, summed over the
                         # step's kernels): an OFFLINE measurement, null unless it was taken on this build's kernel sources
                         "traffic": tr["bytes"], "traffic_source": tr.get("source"), "traffic_stale": tr.get("stale"),
                         "traffic_over_weights": round(tr["bytes"] / wbytes, 2) if tr["bytes"] else None,
                         "traffic_over_weights_plus_kv": round(tr["bytes"] / (wbytes + kvbytes), 2) if tr["bytes"] else None}}


@torch.no_grad()
def decode_distinct_rows(model, prefix, beam, entry):
    """Mean number of distinct (cache row, position) pairs — summed over the beam groups — that one generated position of the beam decode
    attends to (what k_decode_attn_group reads per layer and K / V): one untimed decode with the ancestry tables inspected after every step."""
    from clipcap_amd.engine import DecodeSession, beam_buffers, beam_step
    lm = model.language_model
    g = lm.engine
    dev = prefix.device
    S, L0, D = prefix.shape
    R, V = S * beam, g.dims["V"]
    wte = lm.get_input_embeddings().weight.detach()
    scores = torch.zeros(R, device=dev)
    seq_lengths = torch.ones(R, device=dev)
    has_stopped = torch.zeros(R, dtype=torch.uint8, device=dev)
    base = (torch.arange(S, device=dev, dtype=torch.int32) * beam).repeat_interleave(beam)
    sess = DecodeSession(g, S, L0 + entry)
    lg = torch.empty(R, V, device=dev)
    lg[::beam] = sess.forward(prefix)
    bufs = beam_buffers(dev, S, beam, V)
    next_tok, src = beam_step(lg, S, beam, 1.0, True, 50256, scores, seq_lengths, has_stopped, bufs)
    sess = sess.expand((base // beam).to(torch.int32), R)
    tok = [torch.zeros(R, entry, dtype=torch.int32, device=dev) for _ in range(2)]
    x = torch.empty(R, 1, D, device=dev)
    sess.beam_advance(beam, next_tok, None, wte, 0, tok[1], tok[0], x)
    total, n = 0.0, 0
    for step in range(1, entry):
        rm = sess.row_map[:, : sess.pos].view(S, beam, sess.pos).sort(dim=1).values
        total += float((rm[:, 1:] != rm[:, :-1]).sum() + S * sess.pos + R)      # distinct old rows + the R new keys
        n += 1
        logits = sess.forward(x, partials=True, group=beam)
        next_tok, src = beam_step(logits, S, beam, 1.0, False, 50256, scores, seq_lengths, has_stopped, bufs, sess.lpart)
        sess.beam_advance(beam, next_tok, src, wte, step, tok[(step - 1) & 1], tok[step & 1], x)
    return total / max(1, n)


def sample_bench(args, device):
    """nucleus-sampling decode (top_p 0.8), GPT-2-medium, KV cache + cc_sample_step, 320 prefixes per step (the row
    count of the beam bench: 64 x 5).  A "step" = prefill of the 10-row prefix + 67 sampled tokens per row (no early stop with
    random-init weights; rows that sample EOS keep running to the common length)."""
    from types import SimpleNamespace
    from clipcap_amd.inference.base import sample_tokens
    from clipcap_amd.model.gpt2 import GPT2LM
    torch.manual_seed(1234)
    lm = GPT2LM(n_embd=1024, n_layer=24, n_head=16, vocab_size=50257, n_positions=1024).to(device)
    model = SimpleNamespace(language_model=lm)
    R, L, entry = args.batch or 320, 10, 67
    prefix = torch.randn(R, L, 1024, device=device) * 0.5
    gen = torch.Generator(device=device).manual_seed(7)
    for _ in range(max(1, args.warmup)):
        sample_tokens(model, prefix, entry, 50256, mode=0, top_p=0.8, generator=gen)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for _ in range(args.steps):
        toks, stop_pos = sample_tokens(model, prefix, entry, 50256, mode=0, top_p=0.8, generator=gen)
        n += int(toks.shape[0] * toks.shape[1])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if getattr(args, "dump_outputs", None):
        dump_outputs(args.dump_outputs, {"tokens": toks.double(), "stop_pos": stop_pos.double()})
    return {"metric": "sampling decode tok/s (nucleus top_p=0.8, GPT-2-medium, KV cache)", "value": round(n / dt, 1), "unit": "tokens/s",
            "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 2), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
            "config": {"workload": "nucleus sampling decode, GPT-2-medium random init, 320 prefixes x 10 rows, 67 new tokens", "rows": R,
                       "entry_length": entry}}


def mapper_bench(args, device):
    """north_star sub-target: mapping-transformer forward+backward alone at batch 256 as a fraction of the bf16 MFMA peak
    (algorithmic FLOPs: 3 x 1.5276 GFLOP per sample)."""
    c = dict(CONFIGS[args.config])
    if args.batch:
        c["B"] = args.batch
    me, ge, eng = init_engines(c, device)
    B = c["B"]
    gen = torch.Generator(device=device).manual_seed(1234)
    emb = torch.randn(B, c["E"], generator=gen, device=device)
    dout = torch.randn(B, c["L"], c["D"], generator=gen, device=device) * 1e-3

    def it():
        me.arena.grads().zero_()
        out = me.forward(emb, save=True)
        me.backward(dout)
        return out

    for _ in range(max(1, args.warmup)):
        it()
    torch.cuda.synchronize()
    each = []
    for k in region_sizes(args.steps, max(1, int(getattr(args, "regions", 3) or 3))):   # median of the timed regions, min / max beside it
        t0 = time.perf_counter()
        for _ in range(k):
            prefix = it()
        torch.cuda.synchronize()
        each.append((time.perf_counter() - t0) / k)
    if getattr(args, "dump_outputs", None):
        dump_outputs(args.dump_outputs, {"prefix": dump_sample(prefix, 300), "mapper_grads": dump_sample(me.arena.grads(), 100)})
    dt = sorted(each)[len(each) // 2]
    tf = 3 * mapper_flops_fwd(c) * B / dt / 1e12
    return {"metric": "mapping-transformer fwd+bwd (batch 256)", "value": round(B / dt, 1), "unit": "samples/s", "n_gpus": 1, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(dt * 1e3, 3), "ms_per_step_min": round(min(each) * 1e3, 3),
            "ms_per_step_max": round(max(each) * 1e3, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "bf16", "data": "synthetic", "config": {"workload": f"mapper of {c['name']}", "per_gpu_batch": B},
            "roofline": {"bound": "mfma", "kernel": "whole mapper fwd+bwd chain", "achieved": round(tf, 1), "peak": PEAK_BF16_TFLOPS,
                         "unit": "TFLOP/s", "frac": round(tf / PEAK_BF16_TFLOPS, 4), "traffic": None}}


def train_sub_bench(key, device, steps=12, warmup=3, repeats=3):
    """One-GPU training step of another BASELINE configuration (configs[2]: full finetune of GPT-2-small, configs[3]: CLAP 1024-d ->
    GPT-2-medium full finetune; GPT-2 train-mode dropout on, as the reference runs them) so that the driver's line times them too."""
    from clipcap_amd.model.optim import linear_warmup_decay
    c = dict(CONFIGS[key])
    me, ge, eng = init_engines(c, device)
    gen = torch.Generator(device=device).manual_seed(4321)
    embeds = torch.randn(c["B"], c["E"], generator=gen, device=device)
    tokens = torch.randint(1, c["V"], (c["B"], c["cap"]), generator=gen, device=device)
    sched = linear_warmup_decay(2, 4 * (steps * repeats + warmup) + 64)

    def one(i):
        eng.zero_grad()
        loss = eng.forward_backward(tokens, embeds, dropout=(0.1, 0.1, 0.1, 1000003 * (i + 1)) if c["train_lm"] else None)
        eng.optimizer_step(2e-5 * sched(i), i + 1)
        return loss

    for i in range(warmup):
        loss = one(i)
    torch.cuda.synchronize()
    each, i0 = [], warmup
    for _ in range(repeats):
        t0 = time.perf_counter()
        for i in range(i0, i0 + steps):
            loss = one(i)
        torch.cuda.synchronize()
        each.append((time.perf_counter() - t0) / steps * 1e3)
        i0 += steps
    ms = sorted(each)[len(each) // 2]
    tf = step_flops(c) * c["B"] / (ms * 1e-3) / 1e12
    out = {"workload": f"BASELINE configs[{int(key) - 1}]: {c['name']}", "per_gpu_batch": c["B"], "gpt2_dropout": 0.1 if c["train_lm"] else 0.0,
           "ms_per_step": round(ms, 3), "ms_per_step_min": round(min(each), 3), "ms_per_step_max": round(max(each), 3), "regions": repeats,
           "steps_per_region": steps, "samples_per_s": round(c["B"] / ms * 1e3, 1), "step_algorithmic_tflops": round(tf, 1),
           "step_frac_of_bf16_peak": round(tf / PEAK_BF16_TFLOPS, 4), "final_loss": round(float(loss.item()), 4)}
    del me, ge, eng
    torch.cuda.empty_cache()
    return out


class _BpeTokenizer:
    """A real byte-level BPE tokenizer object (the `tokenizers` Rust library, trained on the synthetic captions: no vocabulary file can be
    downloaded here) behind the three members the input path uses (clipcap/train/dataloader.py:56: batch_encode_plus)."""
    eos_token = "<|endoftext|>"

    def __init__(self, captions, vocab_size=8000):
        from tokenizers import Tokenizer, decoders, models, pre_tokenizers, trainers
        t = Tokenizer(models.BPE())
        t.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
        t.decoder = decoders.ByteLevel()
        t.train_from_iterator(captions, trainers.BpeTrainer(vocab_size=vocab_size, special_tokens=[self.eos_token],
                                                            initial_alphabet=pre_tokenizers.ByteLevel.alphabet(), show_progress=False))
        self.t = t

    def encode(self, s):
        return self.t.encode(s).ids

    def batch_encode_plus(self, captions):
        return {"input_ids": [e.ids for e in self.t.encode_batch(captions)]}

    def decode(self, ids):
        return self.t.decode([int(i) for i in ids])


def _write_e2e_dataset(root, rows, E, shards=4, seed=77, words_lo=44, words_hi=60):
    """The reference's on-disk layout (clipcap/preprocess/writer.py:49-75): embeddings/*.npy, captions/*.parquet, encoder_config.yaml.
    Captions: words_lo..words_hi words drawn from 3000 synthetic words.  Every word is at least one token, so a caption of >= 44 words is
    cut to the headline's 40 tokens by max_token_length (dataloader.py:41-63) and every batch has the headline shape [B, 40] — the reader
    tokenises MORE text than a 40-token caption holds (round 5 wrote 4..25 words: batches trimmed to 24 columns)."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    import yaml
    os.makedirs(os.path.join(root, "embeddings"))
    os.makedirs(os.path.join(root, "captions"))
    rng = np.random.default_rng(seed)
    letters = np.array(list("abcdefghijklmnopqrstuvwxyz"))
    words = ["".join(rng.choice(letters, size=int(rng.integers(2, 9)))) for _ in range(3000)]
    freq = 1.0 / np.arange(1, len(words) + 1)
    freq /= freq.sum()
    sample = None
    for s in range(shards):
        n = rows // shards
        np.save(os.path.join(root, "embeddings", f"img_emb_{s:04d}.npy"), rng.standard_normal((n, E), dtype=np.float32))
        lens = rng.integers(words_lo, words_hi + 1, n)
        idx = rng.choice(len(words), size=int(lens.sum()), p=freq)
        caps, at = [], 0
        for ln in lens:
            caps.append(" ".join(words[i] for i in idx[at:at + ln]) + ".")
            at += ln
        pq.write_table(pa.table({"caption": caps}), os.path.join(root, "captions", f"metadata_{s:04d}.parquet"))
        if sample is None:
            sample = caps[:20000]
    from clipcap_amd.encoders.config import EncoderConfig
    import dataclasses
    ec = EncoderConfig()
    d = dataclasses.asdict(ec) if dataclasses.is_dataclass(ec) else dict(vars(ec))
    with open(os.path.join(root, "encoder_config.yaml"), "w") as f:
        yaml.safe_dump(d, f)
    return sample


def e2e_bench(args, device, max_tokens=None):
    """The REAL train() loop (clipcap_amd/train/train.py; reference clipcap/train/train.py:17-93 over dataloader.py:11-66) on a synthetic dataset
    in the reference's on-disk layout: >= 200 k rows, npy embedding shards + parquet captions, a real BPE tokenizer, BASELINE configs[1]'s
    model.  Timed from step `warm` to the last step of the epoch through train()'s step hook (the loop itself is untouched); right after the
    last step the hook replays ONE device-resident batch of the same shape through the same model: the synthetic step rate the input path
    has to keep up with.  idle = the share of an end-to-end step in which the GPU had nothing to do."""
    import argparse
    import tempfile
    from clipcap_amd.model import add_model_args
    from clipcap_amd.model.gpt2 import GPT2LM
    from clipcap_amd.train import add_training_args, train
    c = dict(CONFIGS["2"])
    B = args.batch or c["B"]
    if args.steps > 0:
        # --mode e2e: exactly --steps timed steps after a warm-up of up to 50 (the four shards hold whole batches: steps in all % 4 == 0)
        warm = min(50, max(1, args.steps // 4))
        warm += -(args.steps + warm) % 4
        rows = (args.steps + warm) * B
    else:
        # the --full line's sub-benchmark: one epoch over >= 200 k rows, timed after 50 steps
        rows = max(204800, 60 * B) // (4 * B) * (4 * B)
        warm = None
    out = {}
    with tempfile.TemporaryDirectory(prefix="clipcap_e2e_") as tmp:
        t0 = time.perf_counter()
        max_tokens = int(max_tokens or c["cap"])        # 40 = the headline; 64 = the reference's default padding (--max-token-length, no trimming possible)
        sample = _write_e2e_dataset(os.path.join(tmp, "ds"), rows, c["E"], words_lo=max_tokens + 4, words_hi=max_tokens + 20)
        tok = _BpeTokenizer(sample)
        out["dataset"] = {"rows": rows, "embedding_shards": 4, "E": c["E"], "write_and_tokenizer_train_s": round(time.perf_counter() - t0, 1),
                          "tokenizer": f"byte-level BPE ({tok.t.get_vocab_size()} tokens, tokenizers library), captions {max_tokens + 4}..{max_tokens + 20} words cut to {max_tokens} tokens"}
        torch.manual_seed(1234)
        lm = GPT2LM(n_embd=c["D"], n_layer=c["n_layer"], n_head=c["n_head"], vocab_size=c["V"], n_positions=c["npos"])
        a = add_model_args(add_training_args(argparse.ArgumentParser())).parse_args([
            "--input-dataset", os.path.join(tmp, "ds"), "--output-folder", os.path.join(tmp, "out"), "--language-model", "gpt2", "--batch-size", str(B),
            "--epochs", "1", "--fp-precision", "bf16", "--prefix-length", str(c["L"]), "--projection-length", str(c["P"]),
            "--transformer-layers", str(c["N"]), "--transformer-attention-heads", str(c["H"]), "--logging-frequency", "1000000",
            "--checkpoint-filename-prefix", "e2e", "--reader-parallel-pieces", str(args.reader_parallel_pieces),
            "--reader-max-piece-size", "50", "--device", str(device.index or 0)])
        a.max_token_length = max_tokens
        n_steps = rows // B
        if warm is None:
            warm = min(50, n_steps // 4)
        st = {}

        def hook(step, model):
            if step == warm:
                torch.cuda.synchronize()
                st["t0"] = time.perf_counter()
            elif step == n_steps:
                torch.cuda.synchronize()
                st["t1"] = time.perf_counter()
                # the same model on ONE device-resident batch of the shape the loop just ran: nothing but launches between steps
                batch = st["batch"]
                for _ in range(5):
                    model.fused_step(batch, lr=1e-6, reducer=None)
                torch.cuda.synchronize()
                r0 = time.perf_counter()
                for _ in range(100):
                    model.fused_step(batch, lr=1e-6, reducer=None)
                torch.cuda.synchronize()
                st["replay_ms"] = (time.perf_counter() - r0) * 10.0
                st["shape"] = [list(t.shape) for t in batch]

        # the hook needs the last batch: wrap the prefetcher's output through the model's own entry point
        import clipcap_amd.model.model as mm
        orig = mm.ClipCapModel.fused_step

        def spy(self, batch, *aa, **kw):
            st["batch"] = batch
            return orig(self, batch, *aa, **kw)

        mm.ClipCapModel.fused_step = spy
        try:
            train(a, tokenizer=tok, language_model=lm, step_hook=hook)
        finally:
            mm.ClipCapModel.fused_step = orig
    e2e_ms = (st["t1"] - st["t0"]) * 1e3 / (n_steps - warm)
    out.update({"steps_timed": n_steps - warm, "ms_per_step": round(e2e_ms, 3), "samples_per_s": round(B / e2e_ms * 1e3, 1),
                "device_resident_replay_ms_per_step": round(st["replay_ms"], 3), "device_resident_samples_per_s": round(B / st["replay_ms"] * 1e3, 1),
                "ratio_to_device_resident": round(st["replay_ms"] / e2e_ms, 4), "gpu_idle_fraction": round(max(0.0, 1.0 - st["replay_ms"] / e2e_ms), 4),
                "batch_shapes_tokens_embeds": st["shape"], "reader_parallel_pieces": args.reader_parallel_pieces,
                "what": "real train() (clipcap_amd/train/train.py) over embeddings/*.npy + captions/*.parquet with background piece readers, "
                        "pinned double-buffered staging and a side-stream H2D copy; device_resident = the same model replaying one batch of the same shape"})
    return out


def executed_step_flops(c):
    """FLOPs the kernels actually run per sample: lm_head forward + dgrad (+wgrad) on the 40 caption rows the loss reads instead of
    all T = 50 (SURVEY.md 8d asks for the reduced figure to be stated next to the algorithmic one)."""
    skipped_rows = c["L"]
    head = 2 * c["D"] * c["V"] * skipped_rows
    return step_flops(c) - (3 if c["train_lm"] else 2) * head


def profile_sites(lib, one_step, sync, n_steps, site, per_step, first_step):
    """n_steps extra steps with HIP events (recorded on the launch stream by the library) around one call site's launches."""
    from clipcap_amd import _lib
    lib.cc_prof_start(_lib.SITES[site], per_step * n_steps)
    sync()
    for i in range(first_step, first_step + n_steps):
        one_step(i)
    sync()
    n = C.c_int32(per_step * n_steps)
    ms = (C.c_float * n.value)()
    fl = (C.c_double * n.value)()
    lib.cc_prof_stop(ms, fl, C.byref(n))
    return [ms[i] for i in range(n.value)], [fl[i] for i in range(n.value)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="train", choices=["train", "decode", "mapper", "sample", "e2e"])
    ap.add_argument("--reader-parallel-pieces", type=int, default=10, help="--mode e2e: background reader workers (0 = read and tokenise on the training thread)")
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200, help="timed steps in all (split over --regions)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--regions", type=int, default=5,
                    help="the --steps timed steps are split into this many back-to-back regions of near-equal length (each bracketed by barrier + "
                         "synchronize, max over ranks); ms_per_step / value are the MEDIAN region's, min / max are reported beside it")
    ap.add_argument("--config", default="2", choices=sorted(CONFIGS))
    ap.add_argument("--batch", type=int, default=0, help="per-GPU batch override")
    ap.add_argument("--site", default="lmhead_fwd", help="single GEMM call site timed for the roofline_lmhead object")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "16", "32"],
                    help="operand mode: bf16 (default, BASELINE's configuration), 16 = fp16 + loss scaling, 32 = split-bf16 operands (the "
                         "reference's fp32 default precision: 3 MFMA terms per product, the parity mode)")
    ap.add_argument("--comm", default="torch", choices=["torch", "cabi"],
                    help="N>1 collectives: torch.distributed (backend nccl = RCCL) or the library's own C-ABI RCCL communicator")
    ap.add_argument("--grad-wire", default="auto", choices=["auto", "fp32", "bf16"],
                    help="N>1: dtype of the gradient slices on the wire (bf16 halves the all-reduce bytes; the fp32 arena stays the accumulator). "
                         "auto = bf16 for frozen-LM bf16 / fp16 runs (41.7 M mapper gradients that only the short mapper backward can hide; "
                         "tests/test_ddp_gloo.py: 8e-3 on the gradients, loss trajectories equal to 2e-3 over 20 steps), fp32 for a full finetune "
                         "and for the fp32-parity mode (--precision 32)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline steps, also run the extras of the line: the N>1 pass without the gradient all-reduce "
                         "(allreduce_exposed_ms), the event-bracketed roofline passes, the N=1 sub-benches and the CPU baselines (minutes); "
                         "without it the run times the --steps steps and prints the headline line only")
    ap.add_argument("--no-roofline-pass", action="store_true",
                    help="--full: skip the 25 extra event-bracketed steps (use under rocprofv3 --pmc, where every dispatch is serialised)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baselines")
    ap.add_argument("--no-sub-benches", action="store_true", help="--full: skip the mapper / decode / configs[2,3] sub-objects of the N=1 line")
    ap.add_argument("--no-dropout", action="store_true", help="configs 3/4: run the full finetune without GPT-2 dropout")
    ap.add_argument("--dry-run", action="store_true",
                    help="no GPU: every rank walks THIS file's control flow (warm-up, timed regions, max-over-ranks, process-group teardown; "
                         "with --full also the no-all-reduce pass, the event-bracketed passes, rank 0's sub-benches and CPU baseline) with a stub "
                         "workload over gloo — what tests/test_ddp_gloo.py runs at 8 ranks to show that no rank is left waiting in a collective")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path computed in its last step as DIR/<name>.npy (float32 / float64, "
                         "seeded samples of large tensors, <= 64 MB in all); the inputs are seeded, so two builds can be compared output for output")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs and args.mode == "e2e":
        ap.error("--dump-outputs is not supported with --mode e2e")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # launched bare (`python bench.py --gpus 8`): start the N ranks ourselves exactly as the driver's torchrun line does, and never
        # print a 1-rank line for an N-GPU request
        import socket
        import subprocess
        have = torch.cuda.device_count() if not args.dry_run else args.gpus      # (a dry run never opens the GPU)
        if have < args.gpus and "CC_BENCH_DEVICE" not in os.environ:
            sys.exit(f"bench.py: --gpus {args.gpus} requested but {have} GPU(s) visible; refusing to report a smaller run")
        with socket.socket() as sock:
            sock.bind(("127.0.0.1", 0))
            port = sock.getsockname()[1]
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.run(cmd, env=env).returncode)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    dry = args.dry_run
    # test hooks (single-GPU boxes): CC_BENCH_DEVICE pins every rank to one device, CC_BENCH_BACKEND=gloo replaces RCCL, so the
    # whole multi-rank flow of this file can be exercised where only one GPU exists.  Never set by the driver.
    if dry:
        device = torch.device("cpu")
    else:
        dev_index = int(os.environ.get("CC_BENCH_DEVICE", local))
        torch.cuda.set_device(dev_index)
        device = torch.device("cuda", dev_index)
    backend = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        backend = "gloo" if dry else os.environ.get("CC_BENCH_BACKEND", "nccl")   # "nccl" is RCCL on ROCm
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(backend)
    if args.mode in ("decode", "mapper", "sample", "e2e"):
        if rank == 0:
            fn = {"decode": decode_bench, "mapper": mapper_bench, "sample": sample_bench, "e2e": e2e_bench}[args.mode]
            print(json.dumps(fn(args, device)))
        return
    c = dict(CONFIGS[args.config])
    if args.batch:
        c["B"] = args.batch
    B, cap = c["B"], c["cap"]
    if args.grad_wire == "auto":      # clipcap_amd.train.train.grad_wire_dtype: fp32 in the fp32-parity mode and for a full finetune
        args.grad_wire = "fp32" if (c["train_lm"] or args.precision == "32") else "bf16"

    total_steps = args.steps + args.warmup
    base_lr, warm = 2e-5, 2
    comm = None
    if dry:
        # stub workload: the same collectives in the same order as the real step (one gradient all-reduce per step when reducing), nothing else
        arenas, lib, me, ge, eng = [], None, None, None, None
        grad = torch.ones(1024)

        def one_step(i, reduce=True):
            if world > 1 and reduce:
                torch.distributed.all_reduce(grad)
                grad.div_(world)
            return torch.tensor(1.0)

        def sync():
            # a CPU all-reduce as the barrier: barrier() probes for an accelerator, which would open the GPU in every rank of a dry run
            if world > 1:
                torch.distributed.all_reduce(torch.zeros(1))

        def profile(n_steps, site, per_step, first_step):
            for i in range(first_step, first_step + n_steps):
                one_step(i)
            sync()
            return [1.0] * (per_step * n_steps), [1e9] * (per_step * n_steps)
    else:
        from clipcap_amd import _lib
        from clipcap_amd.train.ddp import GradReducer
        from clipcap_amd.model.optim import linear_warmup_decay
        me, ge, eng = init_engines(c, device)
        if args.precision != "bf16":
            me.set_precision(int(args.precision))
            ge.set_precision(int(args.precision))
        gen = torch.Generator(device=device).manual_seed(1234 + rank)
        embeds = torch.randn(B, c["E"], generator=gen, device=device)
        tokens = torch.randint(1, c["V"], (B, cap), generator=gen, device=device)
        arenas = eng.arenas()
        if world > 1 and args.comm == "cabi":
            from clipcap_amd.train.ddp import CAbiComm
            comm = CAbiComm.from_process_group(device)
        reducer = GradReducer([a.grads() for a in arenas], comm=comm,
                              wire_dtype=torch.bfloat16 if args.grad_wire == "bf16" else torch.float32) if world > 1 else None
        sched = linear_warmup_decay(warm, 4 * total_steps + 64)
        lib = _lib.lib()

        def one_step(i, reduce=True):
            eng.zero_grad()
            # full finetune: GPT-2 train-mode dropout (p = 0.1 on embeddings, attention probabilities and both residual branches, the
            # GPT2Config defaults the reference runs with), a new mask seed per step and rank
            drop = (0.1, 0.1, 0.1, 1000003 * (i + 1) + rank) if (c["train_lm"] and not args.no_dropout) else None
            if reducer and reduce:   # all-reduce of each layer slice starts as soon as its backward kernels are enqueued
                reducer.begin()
                loss = eng.forward_backward(tokens, embeds, reduce_stats=reducer.reduce_stats, on_grads_ready=reducer.on_grads_ready, dropout=drop)
                reducer.finish()
            else:
                loss = eng.forward_backward(tokens, embeds, dropout=drop)
            eng.optimizer_step(base_lr * sched(i), i + 1)
            return loss

        def sync():
            if world > 1:
                torch.distributed.barrier()
            torch.cuda.synchronize()

        def profile(n_steps, site, per_step, first_step):
            return profile_sites(lib, one_step, sync, n_steps, site, per_step, first_step)

    def max_over_ranks(x):
        if world == 1:
            return x
        t = torch.tensor([x], device=device, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        return float(t.item())

    for i in range(args.warmup):
        loss = one_step(i)
    nxt = args.warmup
    sizes = region_sizes(args.steps, args.regions)
    region_ms = []
    for k in sizes:
        # one timed region: k of the --steps timed steps between barrier + synchronize on both sides, max over ranks
        sync()
        t0 = time.perf_counter()
        for i in range(nxt, nxt + k):
            loss = one_step(i)
        sync()
        region_ms.append(max_over_ranks(time.perf_counter() - t0) / k * 1e3)
        nxt += k
    ms_per_step = sorted(region_ms)[len(region_ms) // 2]
    if args.dump_outputs and rank == 0:     # the last timed step's outputs, before any untimed step below changes the arenas
        dump_outputs(args.dump_outputs, train_step_outputs(loss, eng))
    exposed_ms = None
    if world > 1 and args.full:
        # the same steps with the gradient all-reduce left out (timing only): the difference is the all-reduce time that backward
        # did not hide
        k2 = max(5, args.steps // 8)
        sync()
        t1 = time.perf_counter()
        for i in range(nxt, nxt + k2):
            one_step(i, reduce=False)
        sync()
        exposed_ms = max(0.0, ms_per_step - max_over_ranks((time.perf_counter() - t1) / k2) * 1e3)
        nxt += k2
    T, D, Mc, M = c["L"] + cap, c["D"], B * cap, B * (c["L"] + cap)
    S = c["P"] + c["L"]
    roof = {}
    if args.full and not args.no_roofline_pass:   # every rank runs the profiled extra steps (their collectives must match); rank 0 reports
        # ---- roofline of the dominant kernel family: every MFMA GEMM launch of the step (forward, dgrad, wgrad, lm_head), bracketed
        # with HIP events on the launch stream during 5 extra steps; achieved = sum of 2MNK / sum of launch durations ----
        n_prof = 5
        default_cfg = args.config == "2" and not args.batch and args.precision == "bf16"
        per_step_cap = 64 + 24 * c["N"] + 16 * c["n_layer"]
        ms, fl = profile(n_prof, "all_gemms", per_step_cap, nxt)
        nxt += n_prof
        gemm_ms, gemm_fl = sum(ms), sum(fl)
        fam = gemm_fl / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0
        tr = pmc_constant("train_gemm_bytes_per_step") if default_cfg else {"bytes": None, "source": None, "stale": "offline pass is for the default configuration"}
        alg = gemm_family_algorithmic_bytes(c)
        roof["roofline"] = {"bound": "mfma", "kernel": "bf16 MFMA GEMM family (gemm.hip.h: every NT / TT / lm_head launch of the step)",
                           "achieved": round(fam, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(fam / PEAK_BF16_TFLOPS, 4),
                           "launches_per_step": len(ms) // n_prof, "avg_launch_ms": round(gemm_ms / max(1, len(ms)), 4),
                           "time_share_of_step": round(gemm_ms / n_prof / ms_per_step, 3),
                           "flops_per_step": gemm_fl / n_prof,
                           "algorithmic_bytes": alg["total"], "algorithmic_bytes_by_part": {k: v for k, v in alg.items() if k != "total"},
                           "traffic": tr["bytes"], "traffic_source": tr.get("source"), "traffic_stale": tr.get("stale"),
                           "traffic_over_algorithmic": round(tr["bytes"] / alg["total"], 2) if tr["bytes"] else None,
                           "traffic_note": "HBM bytes of all GEMM launches of one step (per step, not per launch)"}
        mb = mfma_busy_constant("x3_train" if args.precision == "32" else "train") if (args.config == "2" and not args.batch and args.precision != "16") \
            else {"value": None, "source": None, "stale": "offline pass is for the default configuration"}
        roof["roofline"].update({"mfma_busy": mb["value"], "mfma_busy_source": mb["source"], "mfma_busy_stale": mb["stale"],
                                 "mfma_busy_note": "fraction of the GEMM launches' active cycles in which a SIMD's matrix pipe was executing (hardware counters, offline pass)"})
        # ---- second entry: the largest single launch (lm_head forward) at its own call site, 20 extra steps ----
        per_step = {"lmhead_fwd": 1, "lmhead_dgrad": 1, "gpt2_fc_fwd": c["n_layer"], "gpt2_proj2_fwd": c["n_layer"], "gpt2_fc_dgrad": c["n_layer"],
                    "mapper_fc1_fwd": c["N"], "mapper_qkv_fwd": c["N"], "mapper_wgrad_fc2": c["N"]}[args.site]
        ms, _ = profile(20, args.site, per_step, nxt)
        nxt += 20
        avg_ms = sum(ms) / max(1, len(ms))
        site_flops = {"lmhead_fwd": 2.0 * Mc * c["V"] * D, "lmhead_dgrad": 2.0 * Mc * c["V"] * D, "gpt2_fc_fwd": 2.0 * M * D * 4 * D,
                      "gpt2_proj2_fwd": 2.0 * M * D * 4 * D, "gpt2_fc_dgrad": 2.0 * M * D * 4 * D, "mapper_fc1_fwd": 2.0 * B * S * D * 2 * D,
                      "mapper_qkv_fwd": 2.0 * B * S * D * 3 * D, "mapper_wgrad_fc2": 2.0 * B * S * D * 2 * D}[args.site]
        ach = site_flops / (avg_ms * 1e-3) / 1e12 if avg_ms > 0 else 0.0
        default_site = args.site == "lmhead_fwd" and args.config == "2" and not args.batch
        trl = pmc_constant("lmhead_fwd_bytes_per_launch") if default_site else {"bytes": None, "source": None, "stale": "offline pass is for the default call site"}
        roof["roofline_lmhead" if args.site == "lmhead_fwd" else "roofline_site"] = {
            "bound": "mfma", "kernel": ("gemm_nt_stag256_kernel<EpiLMHeadExp,4,false,10> (320x256 tiles, exponential-form epilogue)" if args.site == "lmhead_fwd" else "NT GEMM") + f" @ {args.site}",
            "achieved": round(ach, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / PEAK_BF16_TFLOPS, 4),
            "avg_launch_ms": round(avg_ms, 4), "launches": len(ms), "time_share_of_step": round(avg_ms * per_step / ms_per_step, 3),
            "traffic": trl["bytes"], "traffic_source": trl.get("source"), "traffic_stale": trl.get("stale"),
            "mfma_busy": mfma_busy_constant("train", "EpiLMHead")["value"] if default_site and args.precision == "bf16" else None,
            "algorithmic_bytes": int(2 * (Mc * D + c["V"] * D + Mc * ((c["V"] + 127) // 128 * 128)) + 8 * Mc * ((c["V"] + 127) // 128 * 2))
            if args.site == "lmhead_fwd" else None}
    # every collective of the run is behind us: all ranks leave the process group NOW, so that rank 0's single-rank extras (sub-benches,
    # the CPU baseline: minutes) cannot leave the others waiting in a collective or a teardown barrier
    rccl_ranks = None
    if world > 1:
        rccl_ranks = (comm.count() if comm is not None else torch.distributed.get_world_size()) if backend == "nccl" else 0
        torch.distributed.destroy_process_group()
        sys.stderr.write(f"[bench rank {rank}] left the process group\n")      # one write: eight ranks share the pipe
        sys.stderr.flush()
    if rank != 0:
        return
    value = B * world / (ms_per_step * 1e-3)
    step_tflops = step_flops(c) * B * world / (ms_per_step * 1e-3) / 1e12
    exec_tflops = executed_step_flops(c) * B * world / (ms_per_step * 1e-3) / 1e12
    out = {
        "metric": "train samples/sec (512-d prefix, 40-tok caption)", "value": round(value, 2), "unit": "samples/s", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": {"bf16": "bf16", "16": "f16", "32": "bf16x3"}[args.precision], "data": "synthetic",
        "config": {"workload": f"BASELINE configs[{int(args.config) - 1}]: {c['name']}", "per_gpu_batch": B, "global_batch": B * world,
                   "caption_tokens": cap, "encoder_dim": c["E"], "train_language_model": c["train_lm"],
                   "parallelism": f"dp{world}", "final_loss": round(float(loss.item()), 4)},
        "timed_regions": {"regions": len(sizes), "steps_per_region": sizes, "statistic": "median region (ms_per_step, value)",
                          "ms_per_step_each": [round(r, 3) for r in region_ms],
                          "ms_per_step_min": round(min(region_ms), 3), "ms_per_step_max": round(max(region_ms), 3)},
        "step_algorithmic_tflops": round(step_tflops, 1),
        "step_executed_tflops": round(exec_tflops, 1),
        "step_frac_of_bf16_peak": round(step_tflops / (PEAK_BF16_TFLOPS * world), 4),
        "step_executed_frac_of_bf16_peak": round(exec_tflops / (PEAK_BF16_TFLOPS * world), 4),
    }
    if dry:
        out["dry_run"] = True
        out["data"] = "none (dry run: stub workload, control flow only)"
    if world > 1:
        out["rccl_ranks"] = rccl_ranks
        out["collective_backend"] = "rccl (C ABI cc_allreduce_bucket)" if comm is not None else ("rccl" if backend == "nccl" else backend)
        if exposed_ms is not None:                                      # --full
            out["allreduce_exposed_ms"] = round(exposed_ms, 3)
            out["exposed_allreduce_ms"] = out["allreduce_exposed_ms"]  # (the name VERDICT r4 item 9 uses)
        out["gradient_wire_dtype"] = args.grad_wire
        out["zero_stage"] = 0                                           # bench.py replicates the optimizer state (train() shards it under --deepspeed-strategy)
        out["allreduce_bytes_per_step_per_rank"] = int(sum(a.n for a in arenas) * (2 if args.grad_wire == "bf16" else 4))
        out["gradient_payload_bytes"] = int(sum(a.n for a in arenas) * (2 if args.grad_wire == "bf16" else 4))
        out["gradient_wire_dtype"] = args.grad_wire
    out.update(roof)
    if not args.full:
        # a plain run ends with its headline line: the extras below (minutes of sub-benches and CPU baselines) are --full's
        print(json.dumps(out))
        return
    if dry:
        # rank 0's single-rank extras, stubbed to a pause of the same order as the collectives' timeouts would need to survive
        time.sleep(float(os.environ.get("CC_BENCH_DRY_EXTRAS_S", "2.0")))
        out["cpu_baseline"] = {"value": None, "unit": "samples/s", "cores": torch.get_num_threads(), "kind": "port", "sample": "dry run"}
        print(json.dumps(out))
        return
    if world == 1 and not args.no_sub_benches:
        # north_star sub-targets in the same line: mapping-transformer fwd+bwd alone (target >= 40 % of the bf16 peak at batch 256), the
        # same at 4x / 16x the batch (is the limiter the problem size or the kernels?), and KV-cached beam decode (BASELINE configs[4])
        key = args.config if args.config in ("2", "3", "4") else "2"
        sub = argparse.Namespace(config=key, batch=0, steps=150, warmup=5, regions=3)
        mb = mapper_bench(sub, device)
        out["mapper"] = {"ms_fwd_bwd": mb["ms_per_step"], "ms_fwd_bwd_min": mb["ms_per_step_min"], "ms_fwd_bwd_max": mb["ms_per_step_max"], "samples_per_s": mb["value"], "tflops": mb["roofline"]["achieved"],
                         "frac_of_bf16_peak": mb["roofline"]["frac"], "target_frac": 0.40, "batch": CONFIGS[key]["B"], "batch_sweep": []}
        for bsz, st_ in ((1024, 30), (4096, 10)):
            mbs = mapper_bench(argparse.Namespace(config=key, batch=bsz, steps=st_, warmup=3, regions=1), device)
            out["mapper"]["batch_sweep"].append({"batch": bsz, "ms_fwd_bwd": mbs["ms_per_step"], "tflops": mbs["roofline"]["achieved"],
                                                 "frac_of_bf16_peak": mbs["roofline"]["frac"]})
            del mbs
            torch.cuda.empty_cache()
        del mb
        torch.cuda.empty_cache()
        db = decode_bench(argparse.Namespace(batch=0, steps=9, warmup=1, regions=3), device)
        out["decode"] = {"metric": db["metric"], "tokens_per_s": db["value"], "beam_tokens_per_s": db["beam_tokens_per_s"],
                         "ms_per_batch": db["ms_per_step"], "timed_regions": db["timed_regions"], "config": db["config"]["workload"],
                         "roofline": db["roofline"]}
        del db
        torch.cuda.empty_cache()
        if args.config == "2" and not args.batch and args.precision == "bf16":
            # the other single-GPU-sized BASELINE training configurations, timed by the same run
            out["config3_full_finetune_small"] = train_sub_bench("3", device)
            out["config4_clap_gpt2_medium"] = train_sub_bench("4", device)
    if world == 1 and not args.no_sub_benches and args.config == "2" and not args.batch and args.precision == "bf16":
        # the input path: the real train() loop over an on-disk dataset in the reference's layout against the same model replaying one
        # device-resident batch (the headline trains on a resident synthetic batch)
        torch.cuda.empty_cache()
        try:
            out["e2e_train"] = e2e_bench(argparse.Namespace(batch=0, steps=0, reader_parallel_pieces=10), device)
            # the same loop at the reference's 64-column padding (captions longer than 64 tokens: nothing to trim)
            p64 = e2e_bench(argparse.Namespace(batch=0, steps=0, reader_parallel_pieces=10), device, max_tokens=64)
            out["e2e_train_pad64"] = {k: p64[k] for k in ("ms_per_step", "samples_per_s", "device_resident_replay_ms_per_step", "ratio_to_device_resident",
                                                          "gpu_idle_fraction", "batch_shapes_tokens_embeds", "steps_timed")}
        except Exception as e:      # never lose the headline line to the extra
            out["e2e_train"] = {"error": f"{type(e).__name__}: {e}"}
        torch.cuda.empty_cache()
    if world == 1 and not args.no_sub_benches and args.precision == "bf16":
        # the same step in the parity mode (--fp-precision 32, the reference's default: split-bf16 operands, logits within 1e-3 of
        # the fp32 reference at full depth) next to the bf16 headline
        torch.cuda.empty_cache()
        me.set_precision(32)
        ge.set_precision(32)
        for i in range(nxt, nxt + 3):
            one_step(i)
        sync()
        t0 = time.perf_counter()
        k3 = 20
        for i in range(nxt + 3, nxt + 3 + k3):
            loss3 = one_step(i)
        sync()
        ms3 = (time.perf_counter() - t0) / k3 * 1e3
        out["fp32_parity_mode"] = {"operands": "split bf16 (hi*hi + hi*lo + lo*hi), fp32 activations", "flag": "--fp-precision 32",
                                   "ms_per_step": round(ms3, 3), "samples_per_s": round(B / ms3 * 1e3, 1), "steps": k3,
                                   "slowdown_vs_bf16": round(ms3 / ms_per_step, 2), "final_loss": round(float(loss3.item()), 4)}
        # and with IEEE fp16 operands (--fp-precision 16, the reference's AMP mode; device-side dynamic loss scaling inside the step): the
        # middle point of the precision / throughput curve — full-depth logits 2.0e-3 from the reference (bf16 1.5e-2, split bf16 4e-5;
        # tests/test_gpu_fp16.py, tests/test_gpu_x3.py assert these)
        try:
            me.set_precision(16)
            ge.set_precision(16)
            for i in range(nxt + 3 + k3, nxt + 6 + k3):
                one_step(i)
            sync()
            t0 = time.perf_counter()
            for i in range(nxt + 6 + k3, nxt + 6 + 2 * k3):
                loss16 = one_step(i)
            sync()
            ms16 = (time.perf_counter() - t0) / k3 * 1e3
            out["fp16_mode"] = {"operands": "IEEE fp16, dynamic loss scaling on the device", "flag": "--fp-precision 16", "ms_per_step": round(ms16, 3),
                                "samples_per_s": round(B / ms16 * 1e3, 1), "steps": k3, "slowdown_vs_bf16": round(ms16 / ms_per_step, 2),
                                "final_loss": round(float(loss16.item()), 4),
                                "logits_vs_reference": {"bf16": 1.5e-2, "fp16": 2.0e-3, "split_bf16": 4e-5, "bar": 1e-3,
                                                        "source": "full-depth configs[1] fixtures of the reference, asserted in tests/test_gpu_configs.py / test_gpu_fp16.py / test_gpu_x3.py"}}
        except Exception as e:      # never lose the headline line to the extra
            out["fp16_mode"] = {"error": f"{type(e).__name__}: {e}"}
        me.set_precision("bf16")
        ge.set_precision("bf16")
    if not args.no_cpu_baseline:
        # rank 0, after the process group is gone (N > 1) — the other ranks have exited
        out["cpu_baseline"] = cpu_baseline(c)
        if world == 1 and not args.no_sub_benches:
            out["cpu_decode_baseline"] = cpu_decode_baseline()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
