#!/usr/bin/env python3
"""Compares two gfx950 assembly listings (hipcc ... --cuda-device-only -S) kernel by kernel: instruction count before / after and whether
the instruction streams are identical. Comments and directives are stripped and block labels lose their function index; nothing else is
normalised, so a changed register, offset or order is a difference. Compares two .s files and nothing else.

    python tools/compare_isa.py before.s after.s [--map REGEX=REPLACEMENT ...] [--only REGEX] [--demangler c++filt]

--map rewrites the demangled kernel names of `before` (a renamed or re-parameterised kernel); --only restricts the per-kernel lines
that are printed (the totals always cover every kernel). For a kernel that differs the register, scratch and LDS figures of both
listings are printed too. Exit status 1 when a kernel differs or exists on one side only."""
import argparse
import re
import subprocess
import sys

META = {"vgpr": r"\.vgpr_count:\s*(\d+)", "sgpr": r"\.sgpr_count:\s*(\d+)", "scratch": r"\.private_segment_fixed_size:\s*(\d+)",
        "lds": r"\.group_segment_fixed_size:\s*(\d+)"}


def kernels(path, demangler):
    """demangled name (no parameter list) -> (instruction lines, labels kept in place, resource figures)"""
    text = open(path).read()
    funcs = re.findall(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M)
    names = subprocess.run([demangler], input="\n".join(f[0] for f in funcs), capture_output=True, text=True, check=True).stdout.split("\n")
    meta = {}
    for block in text.split("amdhsa.kernels:")[-1].split("\n  - .agpr_count")[1:]:
        sym = re.search(r"\.symbol:\s*(\w+)\.kd", block)
        if sym:
            meta[sym.group(1)] = {k: int(re.search(p, block).group(1)) for k, p in META.items() if re.search(p, block)}
    out = {}
    for (mangled, body), name in zip(funcs, names):
        name = name.replace("(anonymous namespace)::", "").replace("void ", "", 1).split("(")[0].strip()
        lines = []
        for ln in body.split("\n"):
            ln = ln.split(";")[0].strip()
            if not ln or (ln.startswith(".") and not ln.endswith(":")):
                continue
            lines.append(re.sub(r"\.LBB\d+_", ".LBB_", ln))
        out[name] = (lines, meta.get(mangled, {}))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--map", action="append", default=[], metavar="REGEX=REPLACEMENT")
    ap.add_argument("--only", default=None)
    ap.add_argument("--demangler", default="c++filt")
    a = ap.parse_args()
    before, after = kernels(a.before, a.demangler), kernels(a.after, a.demangler)
    for m in a.map:
        pat, rep = m.split("=", 1)
        before = {re.sub(pat, rep, k): v for k, v in before.items()}
    n_inst = lambda lines: sum(1 for ln in lines if not ln.endswith(":"))
    bad = 0
    print(f"{'kernel':72s} {'before':>7s} {'after':>7s}  identical")
    for k in sorted(set(before) | set(after)):
        b, c = before.get(k), after.get(k)
        same = b is not None and c is not None and b[0] == c[0]
        bad += not same
        if a.only and not re.search(a.only, k) and same:
            continue
        print(f"{k:72s} {n_inst(b[0]) if b else '-':>7} {n_inst(c[0]) if c else '-':>7}  {'yes' if same else 'NO'}")
        if not same and b and c:
            print(f"    before {b[1]}\n    after  {c[1]}")
    print(f"{len(set(before) | set(after))} kernels, {bad} differ or are on one side only")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
