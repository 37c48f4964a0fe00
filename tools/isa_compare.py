#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel, from their assembly listings.

    hipcc <Makefile flags> -DCC_OP=<n> --cuda-device-only -S x.hip -o a/x.s      (once per tree)
    tools/isa_compare.py a/x.s b/x.s [more pairs: a/y.s b/y.s ...]   or   tools/isa_compare.py a/ b/   (every *.s of both directories)
    tools/isa_compare.py a/x.s b/x.s+b/y.s      (a side may be several listings joined with '+': kernels that moved to another unit)

For every kernel symbol it compares the resource figures (each .amdhsa_* directive of the kernel descriptor and each numeric field of the
kernel's metadata record: register counts, scratch, LDS, spills) and the histogram of instruction mnemonics.  It prints one line per file
and the details of every kernel that differs; exit status 1 if anything differs.  A refactor that only moves code between functions is
expected to print no difference at all (a compare and its branch may swap polarity together; the histogram delta shows that as +1 / -1 pairs).
"""
import collections
import os
import re
import sys


def parse(path):
    """-> {kernel: (resources dict, Counter of mnemonics)}"""
    kernels = {}
    body = {}
    cur = None          # function being read
    desc = None         # kernel descriptor being read
    meta = None         # metadata record being read
    meta_fields = {}
    in_meta = False
    label = re.compile(r"^([A-Za-z_$][\w$.]*):")
    with open(path) as f:
        for line in f:
            if "__hip_cuid_" in line:
                continue
            s = line.strip()
            if not s or s.startswith(";") or s.startswith("//"):
                continue
            if s.startswith(".amdgpu_metadata"):
                in_meta = True
                continue
            if s.startswith(".end_amdgpu_metadata"):
                in_meta = False
                continue
            if in_meta:
                m = re.match(r"^-?\s*\.(\w+):\s*(.*)$", s)
                if not m:
                    continue
                if s.startswith("- .") and m.group(1) in ("agpr_count", "args"):   # first key of a kernel record
                    meta = {}
                    meta_fields[id(meta)] = meta
                if meta is not None:
                    if m.group(1) == "name":
                        meta["__name"] = m.group(2).strip()
                    elif re.fullmatch(r"-?\d+", m.group(2).strip()) and not m.group(1).startswith(("offset", "size", "address")):
                        meta["meta." + m.group(1)] = m.group(2).strip()
                continue
            if s.startswith(".amdhsa_kernel"):
                desc = s.split()[1]
                kernels.setdefault(desc, ({}, collections.Counter()))
                continue
            if s.startswith(".end_amdhsa_kernel"):
                desc = None
                continue
            if desc is not None:
                k, _, v = s.partition(" ")
                kernels[desc][0][k] = v.strip()
                continue
            m = label.match(s)
            if m and not line[0].isspace():
                cur = m.group(1)
                body.setdefault(cur, collections.Counter())
                continue
            if s.startswith(".Lfunc_end"):
                cur = None
                continue
            if s.startswith(".") or cur is None or label.match(s):
                continue
            body[cur][s.split()[0]] += 1
    for k in kernels:
        kernels[k][1].update(body.get(k, {}))
    for rec in meta_fields.values():
        name = rec.pop("__name", None)
        if name in kernels:
            kernels[name][0].update(rec)
    return kernels


def parse_side(spec):
    """one listing, or several joined with '+' whose kernel tables are merged"""
    kernels = {}
    for path in spec.split("+"):
        kernels.update(parse(path))
    return kernels


def compare(pa, pb):
    a, b = parse_side(pa), parse_side(pb)
    bad = 0
    for k in sorted(set(a) ^ set(b)):
        print(f"  symbol only in {'first' if k in a else 'second'}: {k}")
        bad += 1
    for k in sorted(set(a) & set(b)):
        ra, ha = a[k]
        rb, hb = b[k]
        lines = [f"    {key}: {ra.get(key)} -> {rb.get(key)}" for key in sorted(set(ra) | set(rb)) if ra.get(key) != rb.get(key)]
        lines += [f"    {mn}: {ha.get(mn, 0)} -> {hb.get(mn, 0)}" for mn in sorted(set(ha) | set(hb)) if ha.get(mn, 0) != hb.get(mn, 0)]
        if lines:
            bad += 1
            print(f"  {k}  ({sum(ha.values())} instructions)")
            print("\n".join(lines))
    n_ins = sum(sum(h.values()) for _, h in a.values())
    print(f"{os.path.basename(pa)}: {len(a)} kernels, {n_ins} instructions, {bad} differ")
    return bad


def main(argv):
    if len(argv) == 2 and os.path.isdir(argv[0]) and os.path.isdir(argv[1]):
        names = sorted(n for n in os.listdir(argv[0]) if n.endswith(".s"))
        pairs = [(os.path.join(argv[0], n), os.path.join(argv[1], n)) for n in names]
    elif argv and len(argv) % 2 == 0:
        pairs = list(zip(argv[0::2], argv[1::2]))
    else:
        sys.exit(__doc__)
    return 1 if sum(compare(x, y) for x, y in pairs) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
