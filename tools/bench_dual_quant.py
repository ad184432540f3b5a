#!/usr/bin/env python3
"""Times the quantised dual video + audio model (ltx_dual_model_quantize; video 32 x 128 = 4096, audio 32 x 64 = 2048, caption_channels
3840, L = 1) against the bf16 model and writes profiles/dual_quant_bench.txt. Three contexts of one process hold the same synthetic
model as bf16, 8-bit and 4-bit; the variants of a table alternate sample by sample.

  1. the timestep path alone (ltx_dual_model_embed_dev) at B = 1 and 2: bf16 weights (three launch_gemv_group launches), 8- and 4-bit
     codes (three launch_gemv_group_q launches; option "gemvq_sb" 0 and 1: how the scale / bias pair reaches the 8 lanes of a group),
     and the composed alternative the codes kernel replaces (per Linear launch_dequant into the scratch matrix + launch_gemv_f32, 18 of
     each). Gate: the grouped codes path is faster than the composed one by more than both spreads, at both bit widths;
  2. one cached forward (text_cache = 1) at T_v = 1536 = (4, 16, 24), T_a = 126, S = 1024, B = 1 and 2 on the bf16, the 8-bit (option
     "qb_off" 0 and 1) and the 4-bit model;
  3. ltx_dual_model_memory_info of the L = 1 model before and after quantising.

Each sample is `--batch` back-to-back calls between two HIP events; median and minimum over `--iters` samples after `--warmup`;
spread = (p90 - p10) / median. Run by hand:

    python tools/bench_dual_quant.py [--iters 20] [--warmup 3] [--batch 10] [--out profiles/dual_quant_bench.txt]
"""
import argparse
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_dual_model import CAPTION, COPY_RATE, DA, DV, FHW, S, T_A, T_V, measure, stats  # noqa: E402


def embed_params():
    """Linear parameters of the six embedders: per stream 3 x 256 x D + 3 x D^2 + (6 + 4 + 1) x D^2."""
    return sum(3 * 256 * D + 14 * D * D for D in (DV, DA))


def weight_bytes(n, bits):
    return 2 * n if bits == 16 else n * bits // 8 + n // 64 * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    ltx = importlib.import_module("ltx-video-swift-mlx_amd")
    assert torch.cuda.is_available(), "this benchmark needs the GPU: there is no CPU path"
    g = torch.Generator(device="cuda").manual_seed(1)
    rn = lambda *s: torch.randn(s, device="cuda", generator=g)  # noqa: E731
    lines = [f"quantised dual video + audio model, full width: Dv {DV}, Da {DA}, caption_channels {CAPTION}, one block; us per call, median / min of "
             f"{args.iters} samples of {args.batch} calls after {args.warmup} warm-up samples; spread = (p90 - p10) / median; variants alternate "
             f"sample by sample; torch {torch.__version__}"]
    head = f"{'row':<58}{'median us':>12}{'min us':>12}{'spread':>9}"
    row = lambda name, ts: lines.append("{:<58}{:>12.1f}{:>12.1f}{:>8.1f}%".format(name, stats(ts)[0], stats(ts)[1], 100 * stats(ts)[2]))  # noqa: E731

    ctxs, mem = {}, {}
    for bits in (16, 8, 4):
        c = ltx.Context(0)
        c.dual_model_init_synthetic(ltx.default_dual_model_config(num_layers=1), seed=9)
        mem[bits] = [c.dual_model_memory_info()]
        if bits != 16:
            c.dual_model_quantize(bits)
            mem[bits].append(c.dual_model_memory_info())
        ctxs[bits] = c
    opt = ctxs[16].set_option  # the option table is process-wide

    # 1. the timestep path
    n = embed_params()
    lines.append(f"1. timestep path: six embedders, {n / 1e6:.1f} M Linear parameters = " + ", ".join(
        f"{weight_bytes(n, b) / 1e6:.1f} MB at {b} bits (floor {weight_bytes(n, b) / COPY_RATE * 1e6:.1f} us at {COPY_RATE / 1e12:.2f} TB/s)" for b in (16, 8, 4)))
    lines.append(head)
    gate = []
    for B in (1, 2):
        ts_v, ts_a = torch.rand(B, device="cuda", generator=g), torch.rand(B, device="cuda", generator=g)
        mk = lambda: [torch.empty(s, device="cuda") for s in ((B, 6, DV), (B, 6, DA), (B, 5, DV), (B, 5, DA), (B, DV), (B, DA))]  # noqa: E731
        outs = {}

        def variant(bits, mode, sb):
            o = outs.setdefault((bits, mode, sb), mk())

            def fn():
                opt("gemvq_sb", sb)
                ctxs[bits].dual_model_embed_dev(ts_v, ts_a, *o, ungrouped=mode)
            return fn

        names = [("bf16 grouped (5 launches)", 16, 0, 0), ("8-bit codes grouped, own scale/bias loads", 8, 0, 0), ("8-bit codes grouped, cross-lane scale/bias (default)", 8, 0, 1),
                 ("8-bit composed: 18 x (dequant + gemv)", 8, 2, 0), ("4-bit codes grouped, own scale/bias loads", 4, 0, 0),
                 ("4-bit codes grouped, cross-lane scale/bias (default)", 4, 0, 1), ("4-bit composed: 18 x (dequant + gemv)", 4, 2, 0)]
        fns = [variant(b, m, s) for _, b, m, s in names]
        for f in fns:
            f()
        torch.cuda.synchronize()
        same = {b: all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for s in (0, 1) for x, y in zip(outs[(b, 0, s)], outs[(b, 2, 0)])) for b in (8, 4)}
        res = dict(zip([(b, m, s) for _, b, m, s in names], measure(fns, args, torch)))
        opt("gemvq_sb", 1)
        for (name, b, m, s) in names:
            row(f"B={B} {name}", res[(b, m, s)])
        base = stats(res[(16, 0, 0)])[0]
        for b in (8, 4):
            mg, mc = stats(res[(b, 0, 1)]), stats(res[(b, 2, 0)])  # the default route: cross-lane scale / bias
            ok = mg[0] * (1 + max(mg[2], mc[2])) < mc[0]
            gate.append(ok)
            lines.append(f"B={B} {b} bits: grouped codes / composed = {mg[0] / mc[0]:.3f} ({'faster beyond both spreads' if ok else 'NOT faster beyond both spreads'}); "
                         f"grouped codes / bf16 = {mg[0] / base:.3f} (bytes {weight_bytes(n, b) / weight_bytes(n, 16):.3f}); streams "
                         f"{weight_bytes(n, b) / (mg[0] * 1e-6) / 1e12:.2f} TB/s = {100 * weight_bytes(n, b) / (mg[0] * 1e-6) / COPY_RATE:.0f}% of the copy rate "
                         f"(bf16 {100 * weight_bytes(n, 16) / (base * 1e-6) / COPY_RATE:.0f}%); cross-lane / own loads = "
                         f"{mg[0] / stats(res[(b, 0, 0)])[0]:.3f}; grouped, cross-lane and composed outputs bit-equal: {same[b]}")
    lines.append("gate: " + ("the grouped codes path stays the route of quantised models" if all(gate) else
                             "FAILED - embed_launches must take the composed route for quantised models"))

    # 2. one cached forward
    lines.append(f"2. one cached forward (text_cache = 1), L = 1, T_v = {T_V}, T_a = {T_A}, S = {S}")
    lines.append(head)
    bf = torch.bfloat16
    for B in (1, 2):
        lat_v, lat_a = rn(B, T_V, 128).to(bf), rn(B, T_A, 128).to(bf)
        ctx_v, ctx_a = (4 * rn(B, S, CAPTION)).to(bf), (4 * rn(B, S, CAPTION)).to(bf)
        mask = torch.ones((B, S), device="cuda", dtype=torch.int32)
        mask[:, S - S // 3:] = 0
        ts_v, ts_a = torch.full((B,), 0.875, device="cuda"), torch.full((B,), 0.25, device="cuda")
        vel = {}
        for c in ctxs.values():
            c.dual_model_prepare_text(ctx_v, ctx_a, mask, mask)

        def fwd(bits, qb_off):
            vv, va = vel.setdefault((bits, qb_off), (torch.empty((B, T_V, 128), device="cuda"), torch.empty((B, T_A, 128), device="cuda")))

            def fn():
                opt("qb_off", qb_off)
                ctxs[bits].dual_model_forward_dev(lat_v, lat_a, None, None, ts_v, ts_a, vv, va, *FHW, text_cache=1, S=S)
            return fn

        names = [("bf16", 16, 0), ("8 bits (codes in the few-row GEMMs)", 8, 0), ("8 bits, qb_off = 1 (every GEMM through the scratch)", 8, 1), ("4 bits", 4, 0)]
        fns = [fwd(b, q) for _, b, q in names]
        for f in fns:
            f()
        torch.cuda.synchronize()
        finite = all(bool(torch.isfinite(t).all()) for pair in vel.values() for t in pair)
        res = measure(fns, args, torch)
        opt("qb_off", 0)
        for (name, _, _), ts in zip(names, res):
            row(f"B={B} {name}", ts)
        base = stats(res[0])[0]
        lines.append(f"B={B}: against bf16 " + ", ".join(f"{name.split(' (')[0]} {stats(ts)[0] / base:.3f}" for (name, _, _), ts in list(zip(names, res))[1:])
                     + f"; outputs finite: {finite}")

    # 3. memory
    lines.append("3. ltx_dual_model_memory_info of the L = 1 model, bytes (the text cache of section 2 is not in these: taken before it was filled)")
    lines.append(f"bf16: {mem[16][0]}")
    for b in (8, 4):
        lines.append(f"{b} bits: {mem[b][1]}; resident weights + scratch / bf16 weights = "
                     f"{(mem[b][1]['quantised_weights'] + mem[b][1]['scratch']) / mem[b][0]['bf16_weights']:.3f}")
    lines.append("Not measured: a 48-block model; the kernels' own times under a profiler (every row is event time around launches issued from Python "
                 "through ctypes, so rows of a few launches include the host's issue rate).")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    for c in ctxs.values():
        c.dual_model_unload()
        c.close()


if __name__ == "__main__":
    main()
