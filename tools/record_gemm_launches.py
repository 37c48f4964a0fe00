#!/usr/bin/env python3
"""Record what the GEMM host launchers launch, as tests/golden/gemm_launches.json.gz.  No GPU: the programs have no device image.

    tools/record_gemm_launches.py [--tree .] [--out tests/golden/gemm_launches.json.gz] [--coverage | --compare]

Per operand build (CC_OP 0 / 1 / 2), product and lab (-DCC_EXPERIMENTS), the tree's clipcap_amd/csrc/gemm_inst_*.hip are compiled with
`hipcc --cuda-host-only` together with the driver tools/gemm_launch_recorder.hip, tools/gemm_launch_hook.h force-included in front of each
unit: hipLaunchKernelGGL records (kernel stub address, grid, block, LDS bytes, every GemmShape field, the integer arguments) instead of
launching, and the other HIP runtime calls of the launchers return constants (256 CUs).  The stub address is resolved to the full kernel
instantiation name with `nm -C`.  Run it on the commit BEFORE a change to the dispatch rules (gemm_plan.h); tests/test_gemm_launches.py
then asserts that the current tree reproduces every recorded case.  To see what a changed rule moves, run it with --compare: it prints every
case the tree now launches otherwise than the table records; record the new table with the rule.

Runs: every program runs the full case list under the default mode globals and the core list under each other setting of them; the
lab programs then run the core list once per lab switch at a non-default value.  File layout (gzipped JSON, `zcat` shows one stored case per
line): {"kernels": [names], "ids": [case ids], "runs": [{"op", "lab", "env", "modes", "base", "n", "cases": [[id index, status, [[kernel
index, [grid], [block], LDS bytes, [GemmShape fields ...], [integer arguments ...]], ...]], ...]}]}; a run stores only the cases that differ
from its base run's (pack / unpack below).
"""
import argparse
import gzip
import json
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
UNITS = ("gemm_inst_bf16", "gemm_inst_resid", "gemm_inst_f32", "gemm_inst_dact", "gemm_inst_lmhead")
# every lab switch of the GEMM dispatch at a value that is not its default
LAB_SWITCHES = (("CC_GROUP_M", "4"), ("CC_GEMM_STAGGER", "3"), ("CC_GEMM_S160", "0"), ("CC_GEMM_Q4", "0"), ("CC_Q4_LAST", "0"), ("CC_X3_FUSED", "0"),
                ("CC_WGRAD_TAIL", "0"), ("CC_WGRAD_TILE", "128"), ("CC_WGRAD_TILE", "256"), ("CC_WGRAD_KS", "3"), ("CC_SKINNY_SINGLE", "20"),
                ("CC_SKINNY_80", "0"), ("CC_DEEPK", "0"), ("CC_DEEPK", "3"), ("CC_EPI_SPEC", "0"), ("CC_EPI_PLAIN", "0"), ("CC_PRE_NT", "1"),
                ("CC_RESID_INIT", "0"))


def build(tree, outdir, op, lab):
    """compile the five units and the driver host-only and link them without a device image; returns the program's path"""
    src = os.path.join(tree, "clipcap_amd", "csrc")
    tag = f"op{op}{'_lab' if lab else ''}"
    flags = ["-O1", "-std=c++17", "-Wno-unused-result", "-Wno-unused-value", f"-DCC_OP={op}", "--cuda-host-only", "-x", "hip", "-I", src, "-include",
             os.path.join(ROOT, "tools", "gemm_launch_hook.h")]
    flags += ["-DCC_EXPERIMENTS"] if lab else []
    jobs = [(os.path.join(src, u + ".hip"), os.path.join(outdir, f"{tag}_{u}.o")) for u in UNITS]
    jobs.append((os.path.join(ROOT, "tools", "gemm_launch_recorder.hip"), os.path.join(outdir, f"{tag}_driver.o")))

    def cc(job):
        subprocess.run([HIPCC, *flags, "-c", job[0], "-o", job[1]], check=True, capture_output=True, text=True)
        return job[1]

    with ThreadPoolExecutor(max_workers=min(6, os.cpu_count() or 1)) as ex:
        objs = list(ex.map(cc, jobs))
    exe = os.path.join(outdir, f"rec_{tag}")
    subprocess.run([HIPCC, "--cuda-host-only", "-Wl,--unresolved-symbols=ignore-all", "-o", exe, *objs], check=True, capture_output=True, text=True)
    return exe


def symbols(exe):
    """address -> kernel name (`k<T...>`, namespace and parameter list dropped) or plain symbol name; and the names of all kernel stubs"""
    out = subprocess.run(["nm", "-C", exe], check=True, capture_output=True, text=True).stdout
    by_addr = {}
    for line in out.splitlines():
        m = re.match(r"([0-9a-f]+) \w (.*)", line)
        if m and "__device_stub__" not in m.group(2):
            by_addr.setdefault(int(m.group(1), 16), kernel_name(m.group(2)))
    stubs = {kernel_name(l.split(None, 2)[2]) for l in out.splitlines() if "__device_stub__" in l}
    return by_addr, stubs


def kernel_name(sym):
    """`void ns::__device_stub__k<T...>(params)` -> `k<T...>`"""
    s = re.sub(r"cc_(bf16|f16|x3)::|__device_stub__|^void ", "", sym)
    depth = 0
    for i, ch in enumerate(s):
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            return s[:i]
    return s


def run(exe, case_set, env=None):
    """one run of a recorder program: {modes: {case id: [status, [[kernel name, grid, block, lds, shapes, ints], ...]]}}"""
    e = {k: v for k, v in os.environ.items() if not k.startswith("CC_")}
    e.update(env or {})
    out = subprocess.run([exe, case_set], check=True, capture_output=True, text=True, env=e).stdout.splitlines()
    by_addr, _ = symbols(exe)
    anchor = next(a for a, n in by_addr.items() if n == "cc_rec_anchor")
    passes = {}
    for line in out:
        r = json.loads(line)
        if "modes" in r:
            cur = passes.setdefault(r["modes"], {})
        else:
            assert r["id"] not in cur, r["id"]
            cur[r["id"]] = [r["rc"], [[by_addr[anchor + l["k"]], l["g"], l["b"], l["lds"], l["s"], l["i"]] for l in r["L"]]]
    return passes


def record(tree, outdir):
    """Every run of `tree`, in file order: {"op", "lab", "env", "modes", "cases"}, and the kernel stubs of each program.

    Per operand build: the product program runs the full case list under the default mode globals and the core list under each other
    setting of them; the lab program does the same with no switch set, then runs the core list once per lab switch at a non-default value."""
    os.makedirs(outdir, exist_ok=True)
    runs, stubs = [], {}
    for op in (0, 1, 2):
        prod, lab = build(tree, outdir, op, False), build(tree, outdir, op, True)
        stubs[(op, False)], stubs[(op, True)] = symbols(prod)[1], symbols(lab)[1]
        for modes, cases in run(prod, "full").items():
            runs.append({"op": op, "lab": False, "env": {}, "modes": modes, "cases": cases})
        for modes, cases in run(lab, "full").items():
            runs.append({"op": op, "lab": True, "env": {}, "modes": modes, "cases": cases})
        for k, v in LAB_SWITCHES:
            runs.append({"op": op, "lab": True, "env": {k: v}, "modes": "", "cases": run(lab, "core", {k: v})[""]})
    return runs, stubs


def pack(runs):
    """The file's form.  Kernel names and case ids are indices into two tables.  A run is stored against a base, the earlier run it
    shares most records with: it keeps only the cases whose record differs from the base's or that the base does not have; "n" is the
    run's case count.  What a run stores beside its base is therefore what its build, mode or switch moves."""
    names = sorted({l[0] for r in runs for c in r["cases"].values() for l in c[1]})
    ids = list(dict.fromkeys(i for r in runs for i in r["cases"]))
    kidx, cidx = {n: i for i, n in enumerate(names)}, {n: i for i, n in enumerate(ids)}
    out = []
    for k, r in enumerate(runs):
        differ = [sum(1 for i, c in r["cases"].items() if b["cases"].get(i) != c) for b in runs[:k]]
        base = min(range(k), key=lambda j: differ[j]) if k else None
        keep = {i: c for i, c in r["cases"].items() if base is None or runs[base]["cases"].get(i) != c}
        out.append(dict(r, base=base, n=len(r["cases"]), cases=[[cidx[i], c[0], [[kidx[l[0]], *l[1:]] for l in c[1]]] for i, c in keep.items()]))
    return {"kernels": names, "ids": ids, "runs": out}


def unpack(doc, ids):
    """the runs of a file with every case spelled out; ids[k] = the case ids of run k (the driver's, the same for every tree)"""
    names, table, runs = doc["kernels"], doc["ids"], []
    for k, r in enumerate(doc["runs"]):
        own = {table[c[0]]: [c[1], [[names[l[0]], *l[1:]] for l in c[2]]] for c in r["cases"]}
        base = runs[r["base"]]["cases"] if r["base"] is not None else {}
        runs.append(dict(r, cases={i: own[i] if i in own else base[i] for i in ids[k]}))
    return runs


def coverage(runs, stubs):
    """stubs never launched per program, and the share of refusals / fallbacks"""
    launched = {}
    for r in runs:
        launched.setdefault((r["op"], r["lab"]), set()).update(l[0] for c in r["cases"].values() for l in c[1])
    missing = {k: sorted(stubs[k] - launched.get(k, set())) for k in stubs}
    cases = [c for r in runs for c in r["cases"].values()]
    # a refusal: a non-zero status; a fallback: the register-staged kernel, which takes what no DMA-staged form accepts
    refused = sum(1 for c in cases if c[0] != 0 or any(l[0].startswith("gemm_bf16_kernel") for l in c[1]))
    return missing, refused, len(cases)


def dump(doc, path):
    """the file: gzip (no timestamp: the same table gives the same bytes) of JSON text with one stored case per line"""
    text = '{"kernels":' + json.dumps(doc["kernels"], indent=0) + ',\n"ids":' + json.dumps(doc["ids"], indent=0) + ',\n"runs":[\n'
    for i, r in enumerate(doc["runs"]):
        head = json.dumps({k: v for k, v in r.items() if k != "cases"}, separators=(",", ":"))[:-1]
        text += head + ',"cases":[\n' + ",\n".join(json.dumps(c, separators=(",", ":")) for c in r["cases"]) + "\n]}" + (",\n" if i + 1 < len(doc["runs"]) else "\n")
    text += "]}\n"
    with open(path, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
        f.write(text.encode())


def load(path):
    with gzip.open(path, "rt") as f:
        return json.load(f)


def differences(runs, then):
    """(run key, case id, recorded, now) of every case of `runs` that the unpacked table `then` records otherwise"""
    out = []
    for now, old in zip(runs, then):
        key = {k: now[k] for k in ("op", "lab", "env", "modes")}
        out += [(key, cid, old["cases"].get(cid), rec) for cid, rec in now["cases"].items() if old["cases"].get(cid) != rec]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "gemm_launches.json.gz"))
    ap.add_argument("--build-dir", default=None)
    ap.add_argument("--coverage", action="store_true", help="print the kernel stubs no case launches and the share of refusals and fallbacks")
    ap.add_argument("--compare", action="store_true", help="write nothing: print every case the tree launches otherwise than --out records")
    a = ap.parse_args()
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        runs, stubs = record(a.tree, a.build_dir or tmp)
    if a.compare:
        diffs = differences(runs, unpack(load(a.out), [list(r["cases"]) for r in runs]))
        for key, cid, old, new in diffs:
            print(f"{key} {cid}\n    recorded: {old}\n    now:      {new}")
        print(f"{len(diffs)} of {sum(len(r['cases']) for r in runs)} cases differ from {a.out}")
        return 1 if diffs else 0
    doc = pack(runs)
    dump(doc, a.out)
    n = sum(len(r["cases"]) for r in runs)
    stored = sum(len(r["cases"]) for r in doc["runs"])
    print(f"{a.out}: {len(runs)} runs, {n} cases ({stored} stored), {len(doc['kernels'])} kernel instantiations, {os.path.getsize(a.out)} bytes")
    if a.coverage:
        missing, refused, total = coverage(runs, stubs)
        print(f"refusals and fallbacks: {refused} of {total} cases ({100.0 * refused / total:.1f} %)")
        for k, names in sorted(missing.items()):
            print(f"op {k[0]}{' lab' if k[1] else ''}: {len(stubs[k])} stubs, {len(names)} never launched")
            for nm in names:
                print("    " + nm)
    return 0


if __name__ == "__main__":
    sys.exit(main())
