#!/usr/bin/env python3
"""Compare the compiled kernels of two source trees, kernel by kernel.  Needs no GPU.

    python tools/kernel_streams.py PARENT_TREE THIS_TREE [--markdown]

Every `.hip` under `segdino3d_amd/csrc` (and `csrc/experimental`) of both trees is compiled with the Makefile's flags plus
`--cuda-device-only -S` into a temporary directory.  Kernels are matched by mangled name across files (a kernel may change
file), and one row per kernel is printed: instruction count parent / this tree, VGPR / AGPR / scratch / LDS / occupancy of
both (the `.amdhsa_kernel` block and the resource comment the compiler writes after it), and `identical` or the nature of
the difference.  Comments and the names of local labels are ignored.  Exit status 1 when a kernel of the parent is missing
or any kernel differs in instruction count or resources.
"""
import argparse
import collections
import concurrent.futures
import difflib
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join("segdino3d_amd", "csrc")
Kernel = collections.namedtuple("Kernel", "file insts res")
RES_KEYS = ("vgpr", "agpr", "scratch", "lds", "occupancy")


def make_flags(csrc):
    """HIPCC, CXXFLAGS of the tree's Makefile, with $(ARCH) filled in."""
    text = open(os.path.join(csrc, "Makefile")).read()
    var = lambda name: re.search(r"^%s\s*[:?]?=\s*(.*)$" % name, text, re.M).group(1).strip()  # noqa: E731
    flags = var("CXXFLAGS").replace("$(ARCH)", var("ARCH")).split()
    return os.environ.get("HIPCC", var("HIPCC")), flags


def compile_tree(tree, out_dir, jobs, only):
    csrc = os.path.join(os.path.abspath(tree), CSRC)
    hipcc, flags = make_flags(csrc)
    srcs = sorted(os.path.join(d, f) for d in (csrc, os.path.join(csrc, "experimental")) if os.path.isdir(d)
                  for f in os.listdir(d) if f.endswith(".hip") and (not only or f in only))

    def one(src):
        out = os.path.join(out_dir, os.path.relpath(src, csrc).replace(os.sep, "_")[:-4] + ".s")
        subprocess.run([hipcc, *flags, "-Wno-unused-command-line-argument", "--cuda-device-only", "-S", src, "-o", out],
                       check=True, cwd=os.path.dirname(src))
        return os.path.relpath(src, csrc), out

    with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        return list(pool.map(one, srcs))


LABEL = re.compile(r"\.L[A-Za-z_]*\d+(_\d+)?")


def parse(rel, path, kernels):
    """kernels[mangled name] = Kernel(file, [instruction lines], {resource: value})"""
    lines = open(path).read().split("\n")
    names = [m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m]
    starts = {n + ":" for n in names}
    i = 0
    while i < len(lines):
        head = lines[i].split(";")[0].strip()
        if head not in starts:
            i += 1
            continue
        name, insts, labels, res = head[:-1], [], {}, {}
        i += 1
        while not lines[i].startswith(".Lfunc_end"):
            l = lines[i].split(";")[0].strip()
            i += 1
            if not l or l.startswith(".") and not l.endswith(":"):
                m = re.match(r"\.amdhsa_(\w+)\s+(\d+)", l)
                if m:
                    res[m.group(1)] = int(m.group(2))
                continue
            l = LABEL.sub(lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), l)
            if not l.endswith(":"):
                insts.append(re.sub(r"\s+", " ", l))
        out = {"scratch": res["private_segment_fixed_size"], "lds": res["group_segment_fixed_size"]}
        while i < len(lines) and not lines[i].startswith("; Occupancy"):
            m = re.match(r"; (NumVgprs|NumAgprs): (\d+)", lines[i])
            if m:
                out["vgpr" if m.group(1) == "NumVgprs" else "agpr"] = int(m.group(2))
            i += 1
        out["occupancy"] = int(lines[i].split(":")[1])
        assert name not in kernels, "kernel %s is defined in %s and %s" % (name, kernels[name].file, rel)
        kernels[name] = Kernel(rel, insts, out)


def nature(a, b):
    if a == b:
        return "identical"
    if len(a) != len(b):
        return "instruction count differs"
    diff = [(x, y) for x, y in zip(a, b) if x != y]
    split = lambda l: (l.split(" ", 1)[0], sorted(l.replace(",", " ").split()[1:]))  # noqa: E731
    if all(split(x) == split(y) for x, y in diff):
        ops = collections.Counter(x.split(" ", 1)[0] for x, _ in diff)
        return "operand order: " + ", ".join("%d x %s" % (n, op) for op, n in sorted(ops.items()))
    if sorted(a) == sorted(b):
        return "same instructions, %d lines in another order" % len(diff)
    if sorted(l.split(" ", 1)[0] for l in a) == sorted(l.split(" ", 1)[0] for l in b):
        return "same opcodes, %d lines differ (registers or order)" % len(diff)
    return "%d lines differ" % len(diff)


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return {n: re.sub(r"\(.*", "", re.sub(r"^void ", "", d)) for n, d in zip(names, out)}
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent_tree")
    ap.add_argument("this_tree")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--markdown", action="store_true", help="print a markdown table")
    ap.add_argument("--files", nargs="+", default=[], metavar="NAME.hip", help="compile only these sources (of either tree)")
    ap.add_argument("--diff", default="", metavar="TEXT", help="also print the unified diff of the kernels whose name contains TEXT")
    args = ap.parse_args()
    trees = []
    with tempfile.TemporaryDirectory(prefix="kernel_streams_") as tmp:
        for tag, tree in (("parent", args.parent_tree), ("this", args.this_tree)):
            out_dir = os.path.join(tmp, tag)
            os.mkdir(out_dir)
            kernels = {}
            for rel, s in compile_tree(tree, out_dir, args.jobs, args.files):
                parse(rel, s, kernels)
            trees.append(kernels)
    parent, this = trees
    short = demangle(sorted(set(parent) | set(this)))
    fmt = (lambda c: "| " + " | ".join(c) + " |") if args.markdown else (lambda c: "  ".join(c))
    print(fmt(["kernel", "file (parent -> this tree)", "instructions", "VGPR/AGPR/scratch/LDS/occupancy parent", "this tree", "stream"]))
    if args.markdown:
        print("|---|---|---|---|---|---|")
    counts = collections.Counter()
    for name in sorted(set(parent) | set(this), key=lambda n: ((parent.get(n) or this[n]).file, short[n])):
        p, t = parent.get(name), this.get(name)
        if p is None or t is None:
            verdict = "MISSING in this tree" if t is None else "new in this tree"
            k = p or t
            print(fmt(["`%s`" % short[name], k.file, str(len(k.insts)), "", "", verdict]))
            counts[verdict] += 1
            continue
        res = lambda k: " / ".join(str(k.res[x]) for x in RES_KEYS)  # noqa: E731
        verdict = nature(p.insts, t.insts)
        if p.res != t.res:
            verdict = "RESOURCES DIFFER; " + verdict
        counts[verdict.split(":")[0].split(",")[0] if not verdict[0].isdigit() else "lines differ"] += 1
        print(fmt(["`%s`" % short[name], p.file if p.file == t.file else "%s -> %s" % (p.file, t.file),
                   "%d / %d" % (len(p.insts), len(t.insts)), res(p), res(t), verdict]))
        if args.diff and args.diff in short[name] and p.insts != t.insts:
            print("\n".join(difflib.unified_diff(p.insts, t.insts, "parent", "this tree", n=2, lineterm="")))
    print()
    print("%d kernels in the parent, %d in this tree: " % (len(parent), len(this)) + ", ".join("%d %s" % (n, v) for v, n in counts.most_common()))
    bad = sum(n for v, n in counts.items() if v.startswith(("MISSING", "RESOURCES", "instruction count")))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
