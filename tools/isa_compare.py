#!/usr/bin/env python3
"""Compare the device code of two builds, function by function.

    hipcc --offload-arch=gfx950 <the Makefile's flags> --offload-device-only -S unit.hip -o unit.s
    tools/isa_compare.py before/unit.s after/unit.s        (or two directories of *.s with the same names)

Every function present in both files is classified as
    identical     the same instructions and labels, line for line
    same opcodes  the same multiset of opcodes (registers renamed, instructions reordered)
    different     anything else; the instruction counts are printed
after directives, comments and the translation unit's hash symbol are dropped and the function's number is
taken out of its local labels (it changes when another function of the unit comes or goes).  For a function
that is not identical, the register, scratch, spill and LDS figures of the kernel metadata are printed where
they differ.  Functions in only one file are listed.  --pair OLD=NEW compares a function that was renamed
(substrings of the mangled names).  The exit status is 1 when any function is different.
"""
import argparse
import collections
import os
import re
import sys

FIGURES = [("vgpr", "vgpr_count"), ("agpr", "agpr_count"), ("sgpr", "sgpr_count"),
           ("scratch", "private_segment_fixed_size"), ("vgpr_spill", "vgpr_spill_count"),
           ("sgpr_spill", "sgpr_spill_count"), ("lds", "group_segment_fixed_size")]
LONG_NAME = 100  # longer mangled names are listed only with -v
LOCAL_LABEL = re.compile(r"\.L([A-Za-z_]+)\d+(_\d+)?")


def functions(text):
    """name -> normalised body lines (labels and instructions)"""
    names = set(re.findall(r"^\s*\.type\s+([^\s,]+),@function", text, re.M))
    out, cur = {}, None
    for raw in text.splitlines():
        line = raw.split(";", 1)[0].strip()
        if not line:
            continue
        if cur is None:
            if line.endswith(":") and line[:-1] in names:
                cur = line[:-1]
                out[cur] = []
            continue
        if re.match(r"\.Lfunc_end\d+:", line):
            cur = None
            continue
        if line.startswith(".") and not line.endswith(":"):
            continue  # a directive
        if "__hip_cuid_" in line:
            continue
        out[cur].append(LOCAL_LABEL.sub(lambda m: ".L" + m.group(1) + (m.group(2) or ""), line))
    return out


def metadata(text):
    """kernel name -> {figure: value} from the amdhsa.kernels notes"""
    out, cur = {}, None
    m = re.search(r"^amdhsa\.kernels:\s*$", text, re.M)
    if not m:
        return out
    for line in text[m.end():].splitlines():
        if line.startswith("amdhsa."):
            break
        if line.startswith("  - "):
            cur = {}
            line = "    " + line[4:]
        k = re.match(r"    \.(\w+):\s+(\S+)\s*$", line)
        if k and cur is not None:
            cur[k.group(1)] = k.group(2)
            if k.group(1) == "name":
                out[k.group(2)] = cur
    return out


def opcodes(body):
    return collections.Counter(l.split()[0] for l in body if not l.endswith(":"))


def classify(a, b):
    if a == b:
        return "identical"
    return "same opcodes" if opcodes(a) == opcodes(b) else "different"


def compare(path_a, path_b, pairs, verbose):
    ta, tb = open(path_a).read(), open(path_b).read()
    fa, fb, ma, mb = functions(ta), functions(tb), metadata(ta), metadata(tb)
    match = {n: n for n in fa if n in fb}
    for old, new in pairs:
        ca = [n for n in fa if old in n and n not in match]
        cb = [n for n in fb if new in n and n not in match.values()]
        if len(ca) == 1 and len(cb) == 1:
            match[ca[0]] = cb[0]
    tally = collections.Counter()
    for na in sorted(match):
        nb = match[na]
        kind = classify(fa[na], fb[nb])
        tally[kind] += 1
        if kind == "identical" and not verbose and na == nb:
            continue
        note = "" if na == nb else f"  (as {nb})"
        if kind == "different":
            note += f"  instructions {sum(opcodes(fa[na]).values())} -> {sum(opcodes(fb[nb]).values())}"
        print(f"  {kind:12s} {na}{note}")
        if kind != "identical":
            x, y = ma.get(na, {}), mb.get(nb, {})
            diff = [f"{s} {x.get(k, '?')} -> {y.get(k, '?')}" for s, k in FIGURES if x.get(k) != y.get(k)]
            if diff:
                print("               " + ", ".join(diff))
    for side, names in (("only before", set(fa) - set(match)), ("only after", set(fb) - set(match.values()))):
        tally[side] += len(names)
        shown = sorted(n for n in names if verbose or len(n) <= LONG_NAME)
        for n in shown:
            print(f"  {side:12s} {n}")
        if len(shown) < len(names):
            print(f"  {side:12s} ... and {len(names) - len(shown)} template instantiations with longer names (-v)")
    return +tally


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--pair", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("-v", "--verbose", action="store_true", help="list identical functions too")
    args = ap.parse_args()
    pairs = [tuple(p.split("=", 1)) for p in args.pair]
    if os.path.isdir(args.before):
        names = sorted(n for n in set(os.listdir(args.before)) | set(os.listdir(args.after)) if n.endswith(".s"))
        files = [(n, os.path.join(args.before, n), os.path.join(args.after, n)) for n in names]
    else:
        files = [(os.path.basename(args.after), args.before, args.after)]
    total = collections.Counter()
    for name, a, b in files:
        if not (os.path.exists(a) and os.path.exists(b)):
            print(f"{name}: only {'before' if os.path.exists(a) else 'after'}")
            continue
        print(f"{name}:")
        t = compare(a, b, pairs, args.verbose)
        print("  " + (", ".join(f"{v} {k}" for k, v in sorted(t.items())) or "no functions"))
        total.update(t)
    print("total: " + ", ".join(f"{v} {k}" for k, v in sorted(total.items())))
    return 1 if total["different"] else 0


if __name__ == "__main__":
    sys.exit(main())
