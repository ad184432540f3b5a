#!/usr/bin/env python3
"""Micro-benchmark of the fused q|k + V projection (gemm_bf16_kernel_qkv, one launch of 192 x 384 tiles) against the two launches it
replaces, through ltx_op_qkv_projection, in one process with interleaved rounds and HBM-cold weights (every launch takes the next of
> 640 MB of distinct weight sets, as a DiT block does: tools/bench_gemm.py --cold).
    python tools/bench_qkv.py [--rows 1536,3072,6144,9984] [--rounds 7] [--D 4096]"""
import argparse
import importlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ltx = importlib.import_module("ltx-video-swift-mlx_amd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1536,3072,6144,9984")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--D", type=int, default=4096)
    a = ap.parse_args()
    D = K = a.D
    ctx = ltx.Context(0)
    nset = max(2, (640 * 2 ** 20) // (3 * D * K * 2))
    Ws = [((torch.randn(2 * D, K, device="cuda") / K ** 0.5).to(torch.bfloat16), (torch.randn(D, K, device="cuda") / K ** 0.5).to(torch.bfloat16))
          for _ in range(nset)]
    bqk, bv = torch.randn(2 * D, device="cuda"), torch.randn(D, device="cuda")
    for rows in (int(r) for r in a.rows.split(",")):
        X = torch.randn(rows, K, device="cuda").to(torch.bfloat16)
        ldvt = (rows + 63) // 64 * 64
        qk = torch.empty((rows, 2 * D), dtype=torch.bfloat16, device="cuda")
        vt = torch.empty((D, ldvt), dtype=torch.bfloat16, device="cuda")
        out, times, it = {}, {0: [], 1: []}, 0
        for fused in (0, 1):
            ctx.op_qkv_projection(X, Ws[0][0], bqk, Ws[0][1], bv, qk, vt, rows=rows, fused=fused)
            torch.cuda.synchronize()
            out[fused] = (qk.clone(), vt[:, :rows].clone())
        same = torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
        for r in range(a.rounds + 1):
            for fused in (0, 1):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(5):
                    Wqk, Wv = Ws[it % nset]
                    it += 1
                    ctx.op_qkv_projection(X, Wqk, bqk, Wv, bv, qk, vt, rows=rows, fused=fused)
                e1.record()
                torch.cuda.synchronize()
                if r > 0:
                    times[fused].append(e0.elapsed_time(e1) / 5 * 1e3)
        med = {f: sorted(t)[len(t) // 2] for f, t in times.items()}
        fl = 2.0 * rows * 3 * D * K
        print(f"rows {rows:5d}  N = {2 * D} + {D}  K = {K}: two launches " + " ".join(f"{t:.1f}" for t in times[0]) + f" (median {med[0]:.1f} us, "
              f"{fl / med[0] / 1e6:.0f} TFLOP/s) | fused " + " ".join(f"{t:.1f}" for t in times[1]) + f" (median {med[1]:.1f} us, {fl / med[1] / 1e6:.0f} TFLOP/s)"
              f" | fused - two = {med[1] - med[0]:+.1f} us | bit-equal: {same}", flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
