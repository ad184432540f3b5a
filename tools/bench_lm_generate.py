#!/usr/bin/env python3
"""Times Gemma-3 token generation on a KV cache (csrc/gemma_generate.cpp) on the 48-layer synthetic model at the reference's size:
prompt 700 tokens, 64 new tokens, greedy. Reports the prefill, the time per cached step and its ratio to the weight-streaming floor
(resident weight bytes over the 6.3 TB/s measured copy rate), each kernel of the step on its own, and two baselines from the same
process: the same step with every Linear sent through the few-row GEMM at M = 1 (option "lm_gemm"), and one ltx_gemma_encode of the
whole prefix per token. Device events around work on the context's stream; medians (minima) of `--iters` samples after `--warmup`.

The per-kernel lines rotate each launch through copies of the weight matrix in a 2 GB pool, so that no launch finds its weights in
the 256 MB Infinity Cache (the logits matrix is the pool itself); the decode attention and the pick re-read the same buffers and are
cache-warm lower bounds. Run by hand:

    python tools/bench_lm_generate.py [--iters 5] [--warmup 1] [--out profiles/lm_generate_bench.txt]
"""
import argparse
import importlib
import os
import socket
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PROMPT, NEW, CAP = 700, 64, 1536
HID, INTER, HQ, HKV, VOCAB, L = 3840, 15360, 16, 8, 262208, 48
COPY_RATE = 6.3e12  # bytes / s, the measured copy rate of the MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    ltx = importlib.import_module("ltx-video-swift-mlx_amd")
    assert torch.cuda.is_available(), "this benchmark needs the GPU: there is no CPU path"
    ctx = ltx.Context(0)
    ctx.gemma_init_synthetic(ltx.gemma_config(), 1)
    weight_bytes = ctx.gemma_memory_info()["weights"]
    floor_ms = weight_bytes / COPY_RATE * 1e3
    g = torch.Generator(device="cuda").manual_seed(0)
    ids = torch.randint(0, VOCAB, (PROMPT + NEW,), device="cuda", generator=g, dtype=torch.int32)

    def timed(fn, reps=1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(reps):
            fn(i)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps  # ms

    def samples(fn, reps=1):
        ts = [timed(fn, reps) for _ in range(args.warmup + args.iters)][args.warmup:]
        return statistics.median(ts), min(ts)

    lines = [f"Gemma-3 token generation, 48 layers, prompt {PROMPT}, {NEW} new tokens, greedy, cache of {CAP} positions; median (min) of {args.iters} "
             f"samples after {args.warmup}; host {socket.gethostname()}, torch {torch.__version__}",
             f"weights resident: {weight_bytes / 1e9:.2f} GB; floor = weights / 6.3 TB/s = {floor_ms:.2f} ms per token"]
    ctx.lm_begin(CAP)
    info = ctx.lm_memory_info()
    lines.append(f"session: KV cache {info['cache'] / 1e6:.0f} MB ({info['cache'] / CAP / 1e3:.0f} KB per position), workspace {info['workspace'] / 1e6:.1f} MB")

    pre = samples(lambda i: ctx.lm_prefill_dev(ids[:PROMPT]))
    lines.append(f"prefill of {PROMPT} tokens (the encoder's launches into the cache + logits of the last row): {pre[0]:8.2f} ms (min {pre[1]:.2f})")

    def steps(i):  # teacher-forced: 64 cached steps behind one prefill; the prefill is outside the timed window
        for t in range(NEW):
            ctx.lm_step_dev(ids[PROMPT + t:PROMPT + t + 1])

    def step_time():
        out = []
        for s in range(args.warmup + args.iters):
            ctx.lm_prefill_dev(ids[:PROMPT])
            out.append(timed(steps) / NEW)
        out = out[args.warmup:]
        return statistics.median(out), min(out)

    st = step_time()
    lines.append(f"cached step, positions {PROMPT} .. {PROMPT + NEW - 1}: {st[0]:8.3f} ms per token (min {st[1]:.3f}) = {st[0] / floor_ms:.2f} x the floor, "
                 f"{weight_bytes / st[0] / 1e9:.2f} TB/s of weights = {100.0 * floor_ms / st[0]:.0f} % of the copy rate; {10 * L + 3} launches")

    # the whole loop as a user runs it: prefill + 64 x (pick, 4-byte read-back, step), host clock around calls that end in a synchronise
    host_ids = ids[:PROMPT].cpu().numpy()

    def gen_ms(**kw):
        out = []
        for s in range(args.warmup + args.iters):
            t0 = time.perf_counter()
            n = len(ctx.lm_generate(host_ids, ltx.lm_params(max_new_tokens=NEW, eos_ids=[], **kw)))
            out.append((time.perf_counter() - t0) * 1e3)
            assert n == NEW
        out = out[args.warmup:]
        return statistics.median(out), min(out)

    gg = gen_ms(temperature=0.0)
    gs = gen_ms(temperature=0.7, seed=1)
    lines.append(f"ltx_lm_generate greedy:  {gg[0]:8.2f} ms (min {gg[1]:.2f}) for prefill + {NEW} tokens = {(gg[0] - pre[0]) / NEW:.3f} ms per token behind the prefill")
    lines.append(f"ltx_lm_generate sampled: {gs[0]:8.2f} ms (min {gs[1]:.2f}): the host sampler (1 MB of logits to the host, penalty, f64 softmax, partial sort) "
                 f"adds {(gs[0] - gg[0]) / NEW:.3f} ms per token - its worst case: the synthetic model's logits are nearly flat, so the 0.95 nucleus is most "
                 f"of the vocabulary and the partial sort becomes a full one")

    # baselines from the parent's own code, same process
    ctx.set_option("lm_gemm", 1)
    sg = step_time()
    ctx.set_option("lm_gemm", 0)
    lines.append(f"baseline, every Linear of the step through the few-row GEMM at M = 1 (lm_gemm = 1): {sg[0]:8.3f} ms per token (min {sg[1]:.3f}) = "
                 f"{sg[0] / st[0]:.2f} x the gemv step")
    Tfull = PROMPT + NEW
    hid = torch.empty((L + 1, 1, Tfull, HID), device="cuda", dtype=torch.bfloat16)
    full_ids, ones = ids[None, :Tfull].contiguous(), torch.ones((1, Tfull), device="cuda", dtype=torch.int32)
    en = samples(lambda i: ctx.gemma_encode_dev(full_ids, ones, hid))
    lines.append(f"baseline, one ltx_gemma_encode of the whole prefix per token, at {Tfull} tokens: {en[0]:8.2f} ms (min {en[1]:.2f}) = {en[0] / st[0]:.1f} x the gemv step")
    del hid
    ctx.lm_end()

    # each kernel of the step on its own
    lines.append("per kernel (20 launches per sample; gemv weights rotate through a 2 GB pool: HBM-cold; attention and pick: cache-warm):")
    pool = torch.empty(VOCAB * HID, device="cuda", dtype=torch.bfloat16)
    pool.view(torch.int16).random_(0, 0x3F80, generator=g)  # bf16 patterns of [0, 1): finite
    x = (torch.randn(INTER, device="cuda", generator=g)).to(torch.bfloat16)
    ob = torch.empty(INTER * 64, device="cuda", dtype=torch.bfloat16)
    of = torch.empty(VOCAB, device="cuda")
    shapes = [("q|k   6144 x 3840", 6144, HID, 0, 1), ("v     2048 x 3840, strided store", 2048, HID, 0, 64), ("o     3840 x 4096", HID, HQ * 256, 0, 1),
              ("gate|up GeGLU 2 x 15360 x 3840", INTER, HID, 2, 1), ("down  3840 x 15360", HID, INTER, 0, 1), ("logits 262208 x 3840, f32 store", VOCAB, HID, 1, 1)]
    total = 0.0
    for name, N, K, epi, stride in shapes:
        rows = N * (2 if epi == 2 else 1)
        slots = max(1, pool.numel() // (rows * K))
        mats = [pool[s * rows * K:(s + 1) * rows * K].view(rows, K) for s in range(slots)]
        fn = lambda i: ctx.op_gemv_bf16(x, mats[i % slots], N, K, epilogue=epi, out_bf16=ob, out_stride=stride, out_f32=of)  # noqa: E731
        fn(0)
        us, mn = (v * 1e3 for v in samples(fn, 20))
        byts = rows * K * 2
        per_step = L if N != VOCAB else 1
        total += us * per_step
        lines.append(f"    gemv {name:<36}{us:9.1f} us (min {mn:.1f}) = {byts / us / 1e6:6.2f} TB/s = {100.0 * byts / us / 1e6 / 6.3:3.0f} % of the copy rate, "
                     f"x {per_step} = {us * per_step / 1e3:.3f} ms")
    q = torch.randn(HQ * 256, device="cuda", generator=g).to(torch.bfloat16)
    kc = torch.randn((CAP, HKV * 256), device="cuda", generator=g).to(torch.bfloat16)
    vt = torch.randn((HKV * 256, CAP), device="cuda", generator=g).to(torch.bfloat16)
    o = torch.empty(HQ * 256, device="cuda", dtype=torch.bfloat16)
    for n in (700, 1500):
        fn = lambda i: ctx.op_attention_decode(q, kc, vt, o, HQ, HKV, n, 1.0 / 16.0)  # noqa: E731
        fn(0)
        us, mn = (v * 1e3 for v in samples(fn, 20))
        byts = 2 * n * HKV * 256 * 2
        lines.append(f"    decode attention + combine, {n:4d} keys {us:9.1f} us (min {mn:.1f}) for {byts / 1e6:.1f} MB of K / V = {byts / us / 1e6:.2f} TB/s, "
                     f"x {L} = {us * L / 1e3:.3f} ms")
        if n == 700:
            total += us * L
    lg = torch.randn(VOCAB, device="cuda", generator=g)
    hist = torch.randint(0, VOCAB, (128,), device="cuda", generator=g, dtype=torch.int32)
    tok = torch.zeros(1, device="cuda", dtype=torch.int32)
    fn = lambda i: ctx.op_lm_pick(lg, tok, hist=hist, n_gen=64, context=64, penalty=1.1)  # noqa: E731
    fn(0)
    us, mn = (v * 1e3 for v in samples(fn, 20))
    lines.append(f"    pick (penalty over 64 tokens + argmax of {VOCAB}) {us:9.1f} us (min {mn:.1f})")
    lines.append(f"    sum of the gemv and attention lines over a step: {total / 1e3:.3f} ms; the rest of the {st[0]:.3f} ms step is the {3 * L + 2} row-pass launches and "
                 f"the gaps between {10 * L + 3} launches (not measured separately)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    ctx.gemma_unload()
    ctx.close()


if __name__ == "__main__":
    main()
