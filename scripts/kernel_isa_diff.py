#!/usr/bin/env python3
"""Compare the gfx950 code of every kernel of some source files between a
base revision and the working tree, without a GPU.

    python scripts/kernel_isa_diff.py BASE_REV [--files F.hip ...]
                                      [--pair OLD=NEW ...] [--diff]
                                      [--keep DIR]

The sources under geomx_amd/csrc are taken from BASE_REV with `git show`
into a temporary directory; the files (default: conv.hip and convwrw2.hip)
of both sides are compiled to device-only assembly with the flags of
setup.py. --pair names a kernel of the base and the one that replaced it,
as the table prints them (`k<A, 4>=k<B, 4>`), so that a renamed template
instantiation is compared with its predecessor instead of being listed
twice as missing. Per kernel the script compares

  * the instruction stream: comments, directives and blank lines dropped,
    local labels and referenced data symbols renamed in order of first
    appearance (their numbering and names carry no code), and
  * the metadata the code object records: VGPR, AGPR, SGPR counts, LDS
    and scratch bytes, spill counts, and the occupancy the compiler
    reports

and prints one table row per kernel. --diff adds the unified diff of the
two streams for every kernel whose stream differs. It only compares two
builds: it knows nothing about particular instructions. Exit status 0
when every kernel's stream and metadata are identical, 1 otherwise."""
import argparse
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "geomx_amd/csrc"
FILES = ["conv.hip", "convwrw2.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only",
         "-S", "-Wno-unused-command-line-argument"]
META = [("vgpr", "vgpr_count"), ("agpr", "agpr_count"),
        ("sgpr", "sgpr_count"), ("lds", "group_segment_fixed_size"),
        ("scratch", "private_segment_fixed_size"),
        ("vspill", "vgpr_spill_count"), ("sspill", "sgpr_spill_count"),
        ("occ", "occupancy")]


def hipcc():
    for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    sys.exit("hipcc not found")


def base_tree(rev, dst):
    """csrc/ of `rev`, headers included, so the base builds on its own."""
    names = subprocess.run(
        ["git", "ls-tree", "--name-only", rev, CSRC + "/"], cwd=ROOT,
        check=True, capture_output=True, text=True).stdout.split()
    for n in names:
        blob = subprocess.run(["git", "show", f"{rev}:{n}"], cwd=ROOT,
                              check=True, capture_output=True).stdout
        with open(os.path.join(dst, os.path.basename(n)), "wb") as f:
            f.write(blob)


def compile_asm(cc, files, src_dir, out_dir):
    procs = []
    for f in files:
        out = os.path.join(out_dir, f + ".s")
        procs.append((out, subprocess.Popen(
            [cc, *FLAGS, "-I", src_dir, "-o", out,
             os.path.join(src_dir, f)])))
    for out, p in procs:
        if p.wait() != 0:
            sys.exit(f"compiling {out} failed")
    return [o for o, _ in procs]


def parse(path):
    """{kernel: (stream lines, metadata dict)} of one assembly file."""
    lines = open(path).read().splitlines()
    kernels = {m.group(1) for l in lines
               if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l))}
    streams, cur, occ, last = {}, None, {}, None
    for l in lines:
        code = l.split(";", 1)[0].strip()
        if not code:
            m = re.match(r"\s*;\s*Occupancy:\s*(\d+)", l)
            if m and last:
                occ[last] = m.group(1)
            continue
        if cur is None:
            if code.endswith(":") and code[:-1] in kernels:
                last = code[:-1]
                cur = streams.setdefault(last, [])
            continue
        if code.startswith(".Lfunc_end"):
            cur = None
        elif code.endswith(":") or not code.startswith("."):
            cur.append(re.sub(r"\s+", " ", code))
    meta, name, cur_m = {}, None, None
    for l in lines:
        if re.match(r"  - \.", l):              # next entry of amdhsa.kernels
            cur_m = {}
        m = re.match(r"  (?:- | {2})\.(\w+):\s+(\S+)", l)
        if m and cur_m is not None:
            if m.group(1) == "name":
                meta[m.group(2).strip("'\"")] = cur_m
            else:
                cur_m[m.group(1)] = m.group(2)
    for k in streams:
        meta.setdefault(k, {})["occupancy"] = occ.get(k, "?")
    return {k: (normalise(streams[k]), meta[k]) for k in streams}


def normalise(stream):
    labels, syms = {}, {}
    for l in stream:
        if l.endswith(":"):
            labels.setdefault(l[:-1], f"L{len(labels)}")

    def sub_label(m):
        return labels.get(m.group(0), m.group(0))

    def sub_sym(m):
        return syms.setdefault(m.group(1), f"SYM{len(syms)}") + m.group(2)

    out = []
    for l in stream:
        if l.endswith(":"):
            out.append(labels[l[:-1]] + ":")
            continue
        l = re.sub(r"\.L[\w$.]+", sub_label, l)
        l = re.sub(r"([\w$.]+)(@(?:rel32|gotpcrel32)@(?:lo|hi))", sub_sym, l)
        out.append(l)
    return out


def n_instr(stream):
    return sum(1 for l in stream if not l.endswith(":"))


def demangle(names):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if filt:
        out = subprocess.run([filt, *names], check=True, capture_output=True,
                             text=True).stdout.split("\n")
        return dict(zip(names, out))

    def plain(n):  # no demangler: name and integral template arguments
        m = re.match(r"_Z(\d+)", n)
        if not m:
            return n
        beg = m.end()
        name, rest = n[beg:beg + int(m.group(1))], n[beg + int(m.group(1)):]
        targs = re.match(r"I((?:L[ib]\d+E|[ft])+)E", rest)
        if not targs:
            return name
        return name + "<" + ", ".join(
            {"f": "float", "t": "unsigned short"}.get(ty) or
            (v if t == "i" else ("false", "true")[int(v)])
            for t, v, ty in re.findall(r"L([ib])(\d+)E|([ft])",
                                       targs.group(1))) + ">"
    return {n: plain(n) for n in names}


def short(name):
    """`void k<1, 2>(args...)` -> `k<1, 2>`"""
    name = re.sub(r"^void ", "", name)
    depth = 0
    for i, c in enumerate(name):
        depth += c == "<"
        depth -= c == ">"
        if c == "(" and depth == 0:
            return name[:i]
    return name


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("base_rev")
    ap.add_argument("--files", nargs="+", default=FILES, metavar="F.hip",
                    help="sources under %s to compare (default: %s)"
                    % (CSRC, " ".join(FILES)))
    ap.add_argument("--pair", action="append", default=[],
                    metavar="OLD=NEW",
                    help="compare base kernel OLD with new kernel NEW")
    ap.add_argument("--diff", action="store_true",
                    help="print the stream diff of every kernel that differs")
    ap.add_argument("--keep", metavar="DIR",
                    help="leave sources and assembly of both sides in DIR")
    args = ap.parse_args()
    cc = hipcc()
    tmp = args.keep or tempfile.mkdtemp(prefix="isa_diff_")
    try:
        sides = {}
        for side in ("base", "new"):
            d = os.path.join(tmp, side)
            os.makedirs(d, exist_ok=True)
            src = os.path.join(ROOT, CSRC)
            if side == "base":
                src = os.path.join(d, "src")
                os.makedirs(src, exist_ok=True)
                base_tree(args.base_rev, src)
            sides[side] = {}
            for s in compile_asm(cc, args.files, src, d):
                sides[side].update(parse(s))
    finally:
        if not args.keep:
            shutil.rmtree(tmp, ignore_errors=True)

    base, new = sides["base"], sides["new"]
    names = demangle(sorted(set(base) | set(new)))
    by_short = {short(v): k for k, v in names.items()}
    for pair in args.pair:
        old, _, repl = pair.partition("=")
        if by_short.get(old) not in base or by_short.get(repl) not in new:
            sys.exit(f"--pair {pair}: no such kernel on that side")
        base[by_short[repl]] = base.pop(by_short[old])
        del names[by_short[old]]
    head = ["kernel", "instr base/new", "same"] + [h for h, _ in META]
    rows, diffs, all_same = [], [], True
    for k in sorted(names, key=lambda k: short(names[k])):
        if k not in base or k not in new:
            rows.append([short(names[k]),
                         "only in " + ("base" if k in base else "new"), "no"])
            all_same = False
            continue
        (sb, mb), (sn, mn) = base[k], new[k]
        same = sb == sn
        row = [short(names[k]), f"{n_instr(sb)}/{n_instr(sn)}",
               "yes" if same else "no"]
        for _, key in META:
            b, n = mb.get(key, "0"), mn.get(key, "0")
            row.append(b if b == n else f"{b}->{n}")
            all_same &= b == n
        all_same &= same
        rows.append(row)
        if not same:
            diffs.append((short(names[k]), list(difflib.unified_diff(
                sb, sn, "base", "new", lineterm="", n=2))))
    rows = [r + [""] * (len(head) - len(r)) for r in rows]
    width = [max(len(r[i]) for r in [head] + rows) for i in range(len(head))]
    for r in [head, ["-" * w for w in width]] + rows:
        print("| " + " | ".join(c.ljust(w) for c, w in zip(r, width)) + " |")
    if args.diff:
        for name, d in diffs:
            print(f"\n=== {name}")
            print("\n".join(d))
    return 0 if all_same else 1


if __name__ == "__main__":
    sys.exit(main())
