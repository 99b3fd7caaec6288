#!/usr/bin/env python3
"""Compare two builds' device assembly function by function.

    isa_diff.py --a parent/*.s --b result/*.s

Each side is one or more gfx950 `.s` files (hipcc -save-temps, `make asm`).  Every function (kernels
and the device functions they call) is matched by name; its `.amdhsa_*` resource directives and its
instruction stream are compared, with local labels (.LBB*, .Ltmp*, ...) masked, so that a function
may move between translation units.  A function that one side has in several units is compared in
each, against the other side's copy in the unit of the same name where there is one.  Prints one line per function (resources and instruction count, a / b) and exits 1 if any
differs or is missing."""
import argparse
import re
import subprocess
import sys

LABEL = re.compile(r"\.L[A-Za-z_]*\d+(_\d+)?")
RES = ("next_free_sgpr", "next_free_vgpr", "private_segment_fixed_size", "group_segment_fixed_size", "accum_offset")


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return dict(zip(names, out.split("\n")))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def parse(path):
    """{name: {"ins": [...], "res": {...}}} of one .s file."""
    funcs, cur, kern = {}, None, None
    for raw in open(path, errors="replace"):
        line = raw.split(";", 1)[0].strip()
        if not line:
            continue
        m = re.match(r"\.type\s+(\S+),@function", line)
        if m:
            cur = m.group(1)
            funcs[cur] = {"ins": [], "res": {}}
            continue
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", line)
        if m:
            kern = m.group(1)
            continue
        if line == ".end_amdhsa_kernel":
            kern = None
            continue
        if kern is not None:
            if line.startswith(".amdhsa_") and kern in funcs:
                k, _, v = line.partition(" ")
                funcs[kern]["res"][k[len(".amdhsa_"):]] = v.strip()
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
        elif not line.startswith(".") and not line.endswith(":"):
            funcs[cur]["ins"].append(LABEL.sub(".L", " ".join(line.split())))
    return funcs


def side(paths):
    out = {}
    for p in paths:
        for name, f in parse(p).items():
            out.setdefault(name, []).append((p, f))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--a", nargs="+", required=True)
    ap.add_argument("--b", nargs="+", required=True)
    ap.add_argument("--only", default="", help="substring of the (mangled or demangled) names to keep")
    args = ap.parse_args()
    A, B = side(args.a), side(args.b)
    names = sorted(set(A) | set(B))
    pretty = demangle(names)
    bad = 0
    print(f"{'function':86s} {'kind':6s} {'SGPR':>9s} {'VGPR':>9s} {'scratch':>9s} {'LDS':>13s} {'instructions':>13s}  verdict")
    for n in names:
        if args.only and args.only not in n and args.only not in pretty[n]:
            continue
        fa, fb = A.get(n, []), B.get(n, [])
        if not fa or not fb:
            bad += 1
            print(f"{pretty[n][:86]:86s} only in {'a' if fa else 'b'}")
            continue
        unit_a = {pa.rsplit("/", 1)[-1]: a for pa, a in fa}
        for pb, b in fb:
            # a function both sides have in the same unit is compared there: a __noinline__ callee is
            # specialised to the callers of its unit, so its copies differ between units of one build
            a = unit_a.get(pb.rsplit("/", 1)[-1], fa[0][1])
            same_res, same_ins = a["res"] == b["res"], a["ins"] == b["ins"]
            cell = [f"{a['res'].get(k, '-')}/{b['res'].get(k, '-')}" for k in RES[:4]]
            verdict = "identical" if same_res and same_ins else ("RESOURCES DIFFER" if not same_res else "code differs")
            bad += verdict != "identical"
            kind = "kernel" if a["res"] else "func"
            where = "" if len(fb) == 1 else f"  [{pb.rsplit('/', 1)[-1]}]"
            print(f"{pretty[n][:86]:86s} {kind:6s} {cell[0]:>9s} {cell[1]:>9s} {cell[2]:>9s} {cell[3]:>13s} "
                  f"{len(a['ins']):>6d}/{len(b['ins']):<6d}  {verdict}{where}")
    print(f"{len(names)} functions, {bad} differ or are missing")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
