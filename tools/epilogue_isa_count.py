#!/usr/bin/env python3
"""Instruction counts of the epilogues of the three GEMM kernels with a generated main loop (csrc/gemm_asm_tiles.inc).

Compiles csrc/gemm.hip for gfx950 with -S (device code only; no GPU needed) and, per kernel, counts what follows the main loop: the
main loop is the longest inline-assembly block of the kernel (;;#ASMSTART .. ;;#ASMEND in the listing), the accumulator dumps are the
short ones behind it. Printed per kernel, and per basic block of the epilogue that issues at least eight stores to global memory (a specialised group
body is one block; the generic body branches inside a step, and its blocks are summed in one line):

  valu      v_* instructions (v_accvgpr_* of the dumps included)
  trans     of these, v_exp_f32 / v_rcp_f32
  imul      of these, integer multiplies (v_mul_lo / v_mul_hi / v_mad_u64_u32 / v_mad_i64_i32 / 24-bit forms)
  cvt_pk    v_cvt_pk_bf16_f32
  lds       ds_*
  store     global_store_* / buffer_store_*
  load      global_load_* / buffer_load_*
  sbranch   s_cbranch_* / s_branch
  salu      every other s_* instruction (waits and nops excluded)

A basic block is labelled gelu if it holds a v_exp_f32 and bf16 / f32 by the stores it issues; `steps` is its number of 4-element
steps (bf16: 8-byte stores, f32: 16-byte stores). The counts are static: a kernel holds every epilogue variant, a launch runs one.

    python tools/epilogue_isa_count.py [--csrc DIR] [--asm FILE] [--label TEXT]

--csrc compiles another checkout's csrc directory (the parent's, for a before / after table); --asm reads a listing made earlier."""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("gemm_bf16_kernel_dtl", "gemm_bf16_kernel_qkv", "gemm_bf16_kernel_tall")
IMUL = re.compile(r"v_(mul_lo_|mul_hi_|mad_u64_u32|mad_i64_i32|mul_u32_u24|mul_i32_i24|mad_u32_u24|mad_i32_i24)")
COLS = ("valu", "trans", "imul", "cvt_pk", "lds", "store", "load", "sbranch", "salu")


def listing(csrc):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "gemm.s")
        subprocess.run([hipcc, "-O3", "-std=c++17", "-Wno-unused-function", "-Wno-unused-variable", "-Wno-unused-command-line-argument",
                        "--offload-arch=gfx950", "--cuda-device-only", "-S", "-x", "hip", "gemm.hip", "-o", out], check=True, cwd=csrc)
        with open(out) as f:
            return f.read().splitlines()


def kernel_body(lines, name):
    """the lines of the kernel whose mangled symbol holds `name`, from its label to its s_endpgm-terminated end"""
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w*%s\w*:" % name, l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start + 1:end]


def after_main_loop(body):
    blocks, begin = [], None
    for i, l in enumerate(body):
        if "#ASMSTART" in l:
            begin = i
        elif "#ASMEND" in l and begin is not None:
            blocks.append((i - begin, i))
            begin = None
    return body[max(blocks)[1] + 1:]


def classify(op, c):
    if op.startswith("v_"):
        c["valu"] += 1
        if op.startswith(("v_exp_f32", "v_rcp_f32")):
            c["trans"] += 1
        if IMUL.match(op):
            c["imul"] += 1
        if op.startswith("v_cvt_pk_bf16_f32"):
            c["cvt_pk"] += 1
    elif op.startswith("ds_"):
        c["lds"] += 1
    elif op.startswith(("global_store", "buffer_store")):
        c["store"] += 1
        c["store16" if op.endswith("dwordx4") else "store8" if op.endswith("dwordx2") else "store_other"] += 1
    elif op.startswith(("global_load", "buffer_load")):
        c["load"] += 1
    elif op.startswith(("s_cbranch", "s_branch")):
        c["sbranch"] += 1
    elif op.startswith("s_") and not op.startswith(("s_waitcnt", "s_nop", "s_endpgm", "s_barrier")):
        c["salu"] += 1


def count(tail):
    """(totals, [(label, counts)] of the basic blocks that store)"""
    total, blocks = collections.Counter(), []
    label, cur = "entry", collections.Counter()
    for l in tail:
        t = l.split(";")[0].strip()
        if not t or t.startswith("."):
            m = re.match(r"^(\.LBB\w+):", t)
            if m:
                blocks.append((label, cur))
                label, cur = m.group(1), collections.Counter()
            continue
        op = t.split()[0]
        classify(op, cur)
        classify(op, total)
    blocks.append((label, cur))
    return total, [(lb, c) for lb, c in blocks if c["store"]]


def row(name, c, extra=""):
    return f"  {name:<34}" + "".join(f"{c[k]:>8}" for k in COLS) + extra


def report(lines, label):
    out = [f"== {label}", "  " + " " * 34 + "".join(f"{k:>8}" for k in COLS)]
    for k in KERNELS:
        total, blocks = count(after_main_loop(kernel_body(lines, k)))
        out.append(row(k + " (all variants)", total))
        small = collections.Counter()
        for lb, c in blocks:
            steps = max(c["store16"], c["store8"], c["store_other"])
            if steps < 8:  # the generic body: a step is spread over several basic blocks
                small.update(c)
                small["blocks"] += 1
                continue
            kind = ("gelu " if c["trans"] else "") + "+".join(n for n, key in (("f32", "store16"), ("bf16", "store8"), ("other", "store_other")) if c[key])
            out.append(row(f"  {lb} [{kind}]", c, f"   {steps} steps, {c['valu'] / steps:.1f} valu / step"))
        if small["blocks"]:
            out.append(row(f"  {small['blocks']} blocks with < 8 stores", small))
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--csrc", default=os.path.join(ROOT, "ltx-video-swift-mlx_amd", "csrc"))
    ap.add_argument("--asm")
    ap.add_argument("--label", default="working tree")
    a = ap.parse_args()
    if a.asm:
        with open(a.asm) as f:
            lines = f.read().splitlines()
    else:
        lines = listing(a.csrc)
    print(report(lines, a.label))


if __name__ == "__main__":
    sys.exit(main())
