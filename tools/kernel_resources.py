#!/usr/bin/env python3
"""Per-kernel resources of two builds of one HIP file, from the device assembly.

    hipcc <the Makefile's FLAGS> --save-temps -c vibevoice_amd/csrc/gemm.hip -o /tmp/a/gemm.o
        (once per tree, from a scratch directory: the temporaries land in the
         working directory; the device assembly is gemm-hip-amdgcn-amd-amdhsa-gfx950.s)
    python tools/kernel_resources.py BEFORE.s AFTER.s [--all]

Reads only the `amdhsa.kernels` metadata at the end of each file: per kernel
.vgpr_count, .agpr_count, .sgpr_count, .private_segment_fixed_size (scratch)
and .group_segment_fixed_size (static LDS).  Prints a summary per file, the
kernels present in only one file, and every kernel whose row differs, with the
waves per SIMD (512 / (VGPRs + AGPRs rounded up to 8), at most 8) on both
sides.  --all prints every kernel's row.  Exit status 1 if a kernel's scratch,
static LDS or waves per SIMD differ, or a kernel is missing on one side.
"""
import re
import subprocess
import sys

FIELDS = [".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size"]
SHORT = ["vgpr", "agpr", "sgpr", "scratch", "lds"]


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        d = out.split("\n")[:len(names)]
        return dict(zip(names, d)) if len(d) == len(names) else {n: n for n in names}
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def kernels(path):
    """{mangled name: (vgpr, agpr, sgpr, scratch, lds)} from the amdhsa.kernels metadata."""
    text = open(path).read()
    at = text.rfind("amdhsa.kernels:")
    if at < 0:
        sys.exit(f"{path}: no amdhsa.kernels metadata")
    res, cur = {}, {}
    for line in text[at:].splitlines()[1:]:
        if line.startswith("amdhsa.") or line.startswith(".end_amdgpu_metadata"):
            break
        m = re.match(r"(  - |    )(\.[a-z_]+):\s*(.*)$", line)   # a kernel's own keys (its arguments' sit deeper)
        if not m:
            continue
        if m.group(1) == "  - ":   # a new kernel entry
            if ".name" in cur:
                res[cur[".name"]] = cur
            cur = {}
        if m.group(2) in FIELDS or m.group(2) == ".name":
            cur[m.group(2)] = m.group(3).strip()
    if ".name" in cur:
        res[cur[".name"]] = cur
    return {k: tuple(int(v.get(f, 0)) for f in FIELDS) for k, v in res.items()}


def waves(row):
    return min(8, 512 // max(8, (row[0] + row[1] + 7) // 8 * 8))


def summary(tag, ks, names):
    g1 = [r for k, r in ks.items() if names[k].startswith("void k_gemv1<") or names[k].startswith("k_gemv1<")]
    line = f"# {tag}: {len(ks)} kernels, {sum(1 for r in ks.values() if r[3])} with scratch"
    if g1:
        line += f"; {len(g1)} k_gemv1, VGPRs {min(r[0] for r in g1)} .. {max(r[0] for r in g1)}"
    print(line)


def main():
    args = [a for a in sys.argv[1:] if a != "--all"]
    if len(args) != 2:
        sys.exit(__doc__)
    a, b = kernels(args[0]), kernels(args[1])
    names = demangle(sorted(set(a) | set(b)))
    summary("before", a, names)
    summary("after", b, names)
    bad = 0
    for k in sorted(set(a) ^ set(b)):
        print(f"only {'before' if k in a else 'after'}: {names[k]}")
        bad = 1
    fmt = lambda r: " ".join(f"{s} {v}" for s, v in zip(SHORT, r)) + f" waves {waves(r)}"
    ndiff = 0
    for k in sorted(set(a) & set(b), key=lambda k: names[k]):
        if a[k] != b[k]:
            ndiff += 1
            print(f"differs: {names[k]}\n  before {fmt(a[k])}\n  after  {fmt(b[k])}")
            if a[k][3:] != b[k][3:] or waves(a[k]) != waves(b[k]):
                bad = 1
        elif "--all" in sys.argv:
            print(f"{names[k]}: {fmt(a[k])}")
    print(f"# {ndiff} of {len(set(a) & set(b))} kernels differ" + ("; scratch, LDS or waves per SIMD moved" if bad else ""))
    return bad


if __name__ == "__main__":
    sys.exit(main())
