#!/usr/bin/env python3
"""Times the Gemma-3 text encoder (ltx_gemma_encode_dev) on the 48-layer synthetic model at T = 1024, B = 1 and 2: the whole encode,
the causal head-dim-256 attention launch alone, and the three row passes (norm + residual + norm, q/k-norm + RoPE, GeGLU), next to the
same graph composed in torch bf16 (F.linear, F.scaled_dot_product_attention under the causal AND padding mask, F.gelu) on weights of the
same shapes in the same process. The two implementations alternate sample by sample; medians and minima over `--iters` samples after
`--warmup`. B = 2 pads its second element by 200 positions. The per-launch figures of the attention and the row passes are taken from
20 back-to-back launches on the same buffers, whose inputs therefore sit in the L2 / Infinity Cache: they are cache-warm LOWER bounds, and
so are the shares of the encode derived from them (inside the encode each pass reads what a GEMM just wrote, mostly from the same caches,
but nothing here measures that). Run by hand:

    python tools/bench_gemma.py [--iters 10] [--warmup 2] [--out profiles/gemma_encode_bench.txt]
"""
import argparse
import importlib
import math
import os
import socket
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
T, L, HID, INTER, HQ, HKV = 1024, 48, 3840, 15360, 16, 8


def timed(fn, torch, reps=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps  # ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F

    ltx = importlib.import_module("ltx-video-swift-mlx_amd")
    assert torch.cuda.is_available(), "this benchmark needs the GPU: there is no CPU path"
    ctx = ltx.Context(0)
    ctx.gemma_init_synthetic(ltx.gemma_config(), 1)
    bf = dict(device="cuda", dtype=torch.bfloat16)
    g = torch.Generator(device="cuda").manual_seed(0)

    def rnd(*shape, s=0.02):
        return (torch.randn(shape, device="cuda", generator=g) * s).to(torch.bfloat16)

    # the torch graph's own weights, same shapes (one layer's set per layer: the same HBM traffic as the library's)
    tw = [dict(qkv=rnd((HQ + 2 * HKV) * 256, HID), o=rnd(HID, HQ * 256), gu=rnd(2 * INTER, HID), down=rnd(HID, INTER),
               n=[1 + rnd(HID) for _ in range(4)], qn=1 + rnd(256), kn=1 + rnd(256)) for _ in range(L)]
    emb, fn_w = rnd(4096, HID, s=1.0), 1 + rnd(HID)

    def rms(x, w):
        xf = x.float()
        return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-6)).to(torch.bfloat16) * w

    def rope(x, cos, sin):
        return x * cos + torch.cat([-x[..., 128:], x[..., :128]], -1) * sin

    def torch_encode(ids, add_mask, tabs):
        B = ids.shape[0]
        x = emb[ids % 4096] * 62.0
        states = [x]
        for i, w in enumerate(tw):
            xn = rms(x, w["n"][0])
            qkv = F.linear(xn, w["qkv"]).view(B, T, HQ + 2 * HKV, 256).transpose(1, 2)
            cos, sin = tabs[(i + 1) % 6 == 0]
            q, k, v = rope(rms(qkv[:, :HQ], w["qn"]), cos, sin), rope(rms(qkv[:, HQ:HQ + HKV], w["kn"]), cos, sin), qkv[:, HQ + HKV:]
            o = F.scaled_dot_product_attention(q, k, v, attn_mask=add_mask, scale=1.0 / 16.0, enable_gqa=True)
            h = x + rms(F.linear(o.transpose(1, 2).reshape(B, T, HQ * 256), w["o"]), w["n"][1])
            gu = F.linear(rms(h, w["n"][2]), w["gu"])
            x = h + rms(F.linear(F.gelu(gu[..., :INTER], approximate="tanh") * gu[..., INTER:], w["down"]), w["n"][3])
            states.append(x)
        states[-1] = rms(x, fn_w)
        return states

    tabs = {}
    for glob, base in ((False, 1e4), (True, 1e6)):
        ang = torch.arange(T, device="cuda", dtype=torch.float64)[:, None] * base ** (-torch.arange(128, device="cuda", dtype=torch.float64) / 128)
        tabs[glob] = (torch.cat([ang.cos(), ang.cos()], -1).to(torch.bfloat16), torch.cat([ang.sin(), ang.sin()], -1).to(torch.bfloat16))

    lines = [f"Gemma-3 text encoder, 48 layers, T = {T}: ltx_gemma_encode_dev vs the same graph in torch bf16 (SDPA, causal + padding mask); median "
             f"(min) of {args.iters} alternating samples after {args.warmup}; host {socket.gethostname()}, torch {torch.__version__}",
             "per-launch lines: 20 back-to-back launches on the same buffers, i.e. cache-warm lower bounds (and so are their shares of the encode)"]
    for B in (1, 2):
        ids = torch.randint(0, 262208, (B, T), device="cuda", generator=g, dtype=torch.int32)
        mask = torch.ones((B, T), device="cuda", dtype=torch.int32)
        if B == 2:
            mask[1, :200] = 0
        ks = (T - mask.sum(1)).to(torch.int32)
        allowed = torch.tril(torch.ones(T, T, device="cuda", dtype=torch.bool))[None, None] & mask.bool()[:, None, None, :]
        add = torch.where(allowed, 0.0, torch.finfo(torch.bfloat16).min).to(torch.bfloat16)
        hid = torch.empty((L + 1, B, T, HID), **bf)
        idl = ids.long()
        ours = lambda: ctx.gemma_encode_dev(ids, mask, hid)  # noqa: E731
        ref = lambda: torch_encode(idl, add, tabs)  # noqa: E731
        t_o, t_r = [], []
        for i in range(args.warmup + args.iters):
            a, b = timed(ours, torch), timed(ref, torch)
            if i >= args.warmup:
                t_o.append(a)
                t_r.append(b)
        rows = B * T
        q, k = rnd(B, T, HQ * 256, s=1.0), rnd(B, T, HKV * 256, s=1.0)
        vt, o = rnd(B, HKV * 256, T, s=1.0), torch.empty((B, T, HQ * 256), **bf)
        r, x, h, n = rnd(rows, HID, s=1.0), rnd(rows, HID, s=1.0), torch.empty((rows, HID), **bf), torch.empty((rows, HID), **bf)
        w1, w2, wq = torch.zeros(HID, device="cuda"), torch.zeros(HID, device="cuda"), torch.zeros(256, device="cuda")
        qk, gu, ff = rnd(rows, (HQ + HKV) * 256, s=1.0), rnd(rows, 2 * INTER, s=1.0), torch.empty((rows, INTER), **bf)
        cos = torch.ones((T, 128), device="cuda")
        sin = torch.zeros((T, 128), device="cuda")
        parts = {"attention (16/8 heads x 256, causal)": lambda: ctx.op_attention_causal(q, k, vt, o, 1.0 / 16.0, ks),
                 "norm + residual + norm": lambda: ctx.op_gemma_norm(r, w1, h=h, x=x, w2=w2, n=n),
                 "q/k-norm + RoPE": lambda: ctx.op_gemma_qknorm_rope(qk, wq, wq, HQ, HKV, cos, sin, T),
                 "GeGLU": lambda: ctx.op_geglu(gu, ff)}
        mo, mr = statistics.median(t_o), statistics.median(t_r)
        flop = 2.0 * rows * L * (HID * (HQ + 2 * HKV) * 256 + HQ * 256 * HID + 3 * HID * INTER)
        lines.append(f"B = {B}: encode {mo:8.2f} ms (min {min(t_o):.2f})   torch {mr:8.2f} ms (min {min(t_r):.2f})   ours/torch {mo / mr:.2f}   "
                     f"GEMM work {flop / 1e12:.1f} TFLOP = {flop / mo / 1e9:.0f} TFLOP/s over the whole encode")
        for name, fn in parts.items():
            fn()
            ts = [timed(fn, torch, 20) * 1000.0 for _ in range(args.warmup + args.iters)][args.warmup:]
            per_layer = {"attention (16/8 heads x 256, causal)": 1, "norm + residual + norm": 2, "q/k-norm + RoPE": 1, "GeGLU": 1}[name]
            us = statistics.median(ts)
            lines.append(f"    {name:<40}{us:9.1f} us (min {min(ts):.1f}) per launch, x {per_layer * L} launches = {us * per_layer * L / 1000.0:6.2f} ms = "
                         f"{100.0 * us * per_layer * L / 1000.0 / mo:4.1f} % of the encode")
        if B == 1:
            af = 2.0 * HQ * T * T * 256 * L  # causal: half of 4 * H * T * T * 256
            lines.append(f"    attention FLOP share of the encode: {100.0 * af / (af + flop):.1f} %")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    ctx.gemma_unload()
    ctx.close()


if __name__ == "__main__":
    main()
