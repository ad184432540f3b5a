#!/usr/bin/env python3
"""Times the head-dim-64 attention kernel (ltx_op_attention_hd, 32 heads x 64) at the four launch shapes of the dual video + audio
block - audio self, audio text cross (masked), a2v, v2a - at T_v = 1536 video tokens and T_a = ltx_audio_latent_frames(25, 24) and 126
audio tokens, next to torch.nn.functional.scaled_dot_product_attention in bf16 on the same inputs in the same process.

Each sample is `--batch` back-to-back launches between two HIP events (one launch is a few microseconds: shorter than an event pair
resolves), the two implementations alternate sample by sample, and the median over `--iters` samples after `--warmup` is reported per
launch, with the fraction of the dense bf16 MFMA peak that the launch's 4 * B * H * Tq * Tk * 64 FLOP amount to. Run by hand:

    python tools/bench_attn64.py [--iters 30] [--warmup 5] [--batch 50] [--out profiles/attn_d64_bench.txt]
"""
import argparse
import importlib
import os
import socket
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_BF16 = 2.5e15  # dense bf16 MFMA peak of one MI355X, FLOP/s
H, T_V, T_TEXT = 32, 1536, 1024


def sample(fn, batch, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(batch):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / batch  # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F

    ltx = importlib.import_module("ltx-video-swift-mlx_amd")
    assert torch.cuda.is_available(), "this benchmark needs the GPU: there is no CPU path"
    ctx = ltx.Context(0)
    D = H * 64
    lines = [f"head-dim-64 attention, B = 1, H = {H}: ltx_op_attention_hd vs torch SDPA (bf16), us per launch, median of {args.iters} samples of "
             f"{args.batch} launches after {args.warmup} warm-up samples; host {socket.gethostname()}, torch {torch.__version__}",
             f"{'launch':<18}{'Tq':>6}{'Tk':>6}{'q/wg':>6}{'ours us':>10}{'min':>8}{'sdpa us':>10}{'min':>8}{'ours/sdpa':>11}{'% peak':>8}{'max|diff|':>11}"]
    for T_a in (ltx.audio_latent_frames(25, 24.0), 126):
        for name, Tq, Tk, masked in (("audio self", T_a, T_a, False), ("audio text cross", T_a, T_TEXT, True), ("a2v", T_V, T_a, False),
                                     ("v2a", T_a, T_V, False)):
            g = torch.Generator(device="cuda").manual_seed(Tq * 7 + Tk)
            q = torch.randn((1, Tq, D), device="cuda", generator=g).to(torch.bfloat16)
            k = torch.randn((1, Tk, D), device="cuda", generator=g).to(torch.bfloat16)
            v = torch.randn((1, Tk, D), device="cuda", generator=g).to(torch.bfloat16)
            ldvt = (Tk + 63) // 64 * 64
            vt = torch.zeros((1, D, ldvt), device="cuda", dtype=torch.bfloat16)
            vt[:, :, :Tk] = v.transpose(1, 2)
            bias = None
            if masked:
                bias = torch.zeros((1, Tk), device="cuda")
                bias[:, Tk - Tk // 3:] = -10000.0
            o = torch.empty((1, Tq, D), device="cuda", dtype=torch.bfloat16)
            qh, kh, vh = (t.view(1, -1, H, 64).transpose(1, 2) for t in (q, k, v))  # SDPA's [B, H, T, 64] views of the same memory
            mask = None if bias is None else bias.to(torch.bfloat16).view(1, 1, 1, Tk)
            ours = lambda: ctx.op_attention_hd(q, k, vt, bias, H, o, 64, 0.125)  # noqa: E731
            sdpa = lambda: F.scaled_dot_product_attention(qh, kh, vh, attn_mask=mask, scale=0.125)  # noqa: E731
            ours()
            diff = (o.float() - sdpa().transpose(1, 2).reshape(1, Tq, D).float()).abs().max().item()
            t_o, t_s = [], []
            for i in range(args.warmup + args.iters):
                a, b = sample(ours, args.batch, torch), sample(sdpa, args.batch, torch)
                if i >= args.warmup:
                    t_o.append(a)
                    t_s.append(b)
            mo, ms = statistics.median(t_o), statistics.median(t_s)
            flop = 4.0 * H * Tq * Tk * 64
            lines.append(f"{name:<18}{Tq:>6}{Tk:>6}{ctx.attention_hd_workgroup_queries(1, H, Tq):>6}{mo:>10.2f}{min(t_o):>8.2f}{ms:>10.2f}{min(t_s):>8.2f}"
                         f"{mo / ms:>11.2f}{100.0 * flop / (mo * 1e-6) / PEAK_BF16:>8.2f}{diff:>11.4f}")
    lines.append("ours/sdpa < 1: the library's launch is faster. Each launch is issued from Python - ctypes and the library's launcher on one side, torch's "
                 "dispatcher on the other - and a kernel of a few microseconds is shorter than either dispatch: where a time sits near the floor of its column "
                 "it is the host's issue rate, not the kernel, and the ratio compares the two dispatch paths. % peak = 4 * H * Tq * Tk * 64 FLOP over the "
                 "library's time over 2.5 PFLOP/s (MFMA bound); launches this small are bounded by launch latency and grid fill, not by the matrix pipe.")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
