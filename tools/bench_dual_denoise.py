#!/usr/bin/env python3
"""Times the joint video + audio denoise loop and its per-prompt text cache (ltx_dual_denoise_dev, ltx_dual_model_prepare_text_dev,
ltx_op_dual_step) and writes profiles/dual_denoise_bench.txt. Full width (video 32 x 128 = 4096, audio 32 x 64 = 2048,
caption_channels 3840), L = 1, T_v = 1536 = (4, 16, 24), T_a = 126, S = 1024, a third of the keys masked; at B = 1 (no CFG) and B = 2
(CFG, contexts [negative, positive]):

  * one forward with the text cache against one without (= the forward before the cache existed), alternating sample by sample;
  * ltx_dual_model_prepare_text_dev alone: what the cache costs once per prompt;
  * ltx_op_dual_step alone at the loop's sizes: the one launch per step for CFG, both Euler steps and the next tokens;
  * an 8-step loop with and without the cache (the cached loop pays prepare_text inside every call);
  * image-to-video next to those rows: the cached forward with two timestep groups (frame-0 tokens at 0, the rest at sigma:
    ltx_dual_model_forward_groups_dev), the step with a frozen, re-noised prefix of one frame, and the 8-step loop with cond_latent,
    without and with re-noising. Reported as differences, with no gate on them.

The method is tools/bench_dual_model.py's: each sample is `--batch` back-to-back calls between two HIP events in one process; median
and minimum over `--iters` samples after `--warmup`; the spread of a row is (p90 - p10) / median. Gate: the cached forward must not be
slower than the uncached one beyond the larger of the two spreads, at B 1 and at B 2; otherwise text_cache must default to 0 in the
loop. Run by hand:

    python tools/bench_dual_denoise.py [--iters 20] [--warmup 3] [--batch 5] [--out profiles/dual_denoise_bench.txt]
"""
import argparse
import importlib
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DV, DA = 32 * 128, 32 * 64
FHW, T_A, S, CAPTION, L = (4, 16, 24), 126, 1024, 3840, 1
T_V = FHW[0] * FHW[1] * FHW[2]
STEPS = 8


def sample(fn, batch, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(batch):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / batch  # us per call


def stats(ts):
    ts = sorted(ts)
    med = statistics.median(ts)
    p10, p90 = ts[int(0.1 * (len(ts) - 1))], ts[int(math.ceil(0.9 * (len(ts) - 1)))]
    return med, ts[0], (p90 - p10) / med


def measure(fns, args, torch, batch=None):
    """Alternates the callables sample by sample; returns one list of samples per callable."""
    out = [[] for _ in fns]
    for i in range(args.warmup + args.iters):
        for k, fn in enumerate(fns):
            t = sample(fn, batch or args.batch, torch)
            if i >= args.warmup:
                out[k].append(t)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    ltx = importlib.import_module("ltx-video-swift-mlx_amd")
    assert torch.cuda.is_available(), "this benchmark needs the GPU: there is no CPU path"
    ctx = ltx.Context(0)
    ctx.dual_model_init_synthetic(ltx.default_dual_model_config(num_layers=L), seed=9)
    g = torch.Generator(device="cuda").manual_seed(1)
    rn = lambda *s: torch.randn(s, device="cuda", generator=g)  # noqa: E731
    bf = torch.bfloat16
    ceil64 = (S + 63) // 64 * 64
    lines = [f"joint video + audio loop, full width: Dv {DV}, Da {DA}, caption_channels {CAPTION}, L = {L}, T_v {T_V} = {FHW}, T_a {T_A}, S {S}, a third "
             f"of the keys masked; us per call, median / min of {args.iters} samples of {args.batch} calls (loops: 1 call) after {args.warmup} warm-up "
             f"samples; spread = (p90 - p10) / median; torch {torch.__version__}",
             f"{'row':<52}{'median us':>12}{'min us':>12}{'spread':>9}"]
    row = lambda name, ts: lines.append("{:<52}{:>12.1f}{:>12.1f}{:>8.1f}%".format(name, stats(ts)[0], stats(ts)[1], 100 * stats(ts)[2]))  # noqa: E731

    verdicts = []
    for B in (1, 2):
        lat_v, lat_a = rn(B, T_V, 128).to(bf), rn(B, T_A, 128).to(bf)
        ctx_v, ctx_a = (4 * rn(B, S, CAPTION)).to(bf), (4 * rn(B, S, CAPTION)).to(bf)
        mask = torch.ones((B, S), device="cuda", dtype=torch.int32)
        mask[:, S - S // 3:] = 0
        ts = torch.full((B,), 0.875, device="cuda")
        out_c = (torch.empty((B, T_V, 128), device="cuda"), torch.empty((B, T_A, 128), device="cuda"))
        out_u = (torch.empty((B, T_V, 128), device="cuda"), torch.empty((B, T_A, 128), device="cuda"))
        prepare = lambda: ctx.dual_model_prepare_text(ctx_v, ctx_a, mask, mask)  # noqa: E731
        cached = lambda: ctx.dual_model_forward_dev(lat_v, lat_a, None, None, ts, ts, *out_c, *FHW, text_cache=1, S=S)  # noqa: E731
        uncached = lambda: ctx.dual_model_forward_dev(lat_v, lat_a, ctx_v, ctx_a, ts, ts, *out_u, *FHW, video_mask=mask, audio_mask=mask)  # noqa: E731
        prepare()
        cached()
        uncached()
        torch.cuda.synchronize()
        equal = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out_c, out_u))
        info = ctx.dual_model_text_cache_info()
        # image-to-video: two timestep groups per batch element, {sigma, 0}; the tokens of frame 0 in group 1 (launch_i2v_rowmap's layout)
        hw = FHW[1] * FHW[2]
        ts_g = torch.tensor([[0.875, 0.0]] * B, device="cuda")
        rmap = (torch.arange(T_V, device="cuda") < hw).to(torch.int32).repeat(B, 1) + 2 * torch.arange(B, device="cuda", dtype=torch.int32)[:, None]
        rmap = rmap.reshape(-1).contiguous()
        out_g = (torch.empty((B, T_V, 128), device="cuda"), torch.empty((B, T_A, 128), device="cuda"))
        groups = lambda: ctx.dual_model_forward_groups_dev(lat_v, lat_a, None, None, ts_g, ts, *out_g, *FHW, 2, rmap, text_cache=1, S=S)  # noqa: E731
        groups()
        tc, tu, tg = measure([cached, uncached, groups], args, torch)
        (tp,) = measure([prepare], args, torch)
        row(f"forward B={B} text cache", tc)
        row(f"forward B={B} text cache, image-to-video (2 groups)", tg)
        row(f"forward B={B} no cache (the forward before the cache)", tu)
        row(f"prepare_text B={B} (once per prompt)", tp)
        mc, mu, mp = stats(tc), stats(tu), stats(tp)
        keep = mc[0] <= mu[0] * (1 + max(mc[2], mu[2]))
        verdicts.append(keep)
        lines.append(f"B={B}: cached / uncached = {mc[0] / mu[0]:.3f}, {mu[0] - mc[0]:.1f} us saved per forward and block; velocities bit-equal: {equal}; "
                     f"cache {info['bytes'] / 1e6:.1f} MB = L * B * (S + {ceil64}) * (Dv + Da) * 2; prepare_text pays for itself after "
                     f"{mp[0] / max(mu[0] - mc[0], 1e-9):.1f} forwards; "
                     + ("cached is not slower beyond the spread" if keep else "cached is SLOWER beyond the spread"))

        # the step alone, at the loop's sizes: B = 2 is the CFG step (an unconditional velocity, two token copies)
        nv, na = T_V * 128, T_A * 128
        job = lambda n, form: dict(latent=rn(n), v_cond=rn(n), v_uncond=rn(n) if B == 2 else None, cfg_scale=3.0 if B == 2 else 1.0,  # noqa: E731
                                   form=form, tokens=torch.empty(B * n, device="cuda", dtype=bf), copies=B)
        jv, ja = job(nv, 0), job(na, 1)
        step = lambda: ctx.op_dual_step(jv, ja, 0.725, 0.7)  # noqa: E731
        (tst,) = measure([step], args, torch, batch=50)
        row(f"dual_step B={B} ({nv} + {na} elements, 1 launch)", tst)
        nk = hw * 128
        jk = dict(job(nv, 0), n_keep=nk, keep_src=rn(nk), keep_noise=rn(nk), keep_scale=0.15)
        step_keep = lambda: ctx.op_dual_step(jk, ja, 0.725, 0.7)  # noqa: E731
        (tsk,) = measure([step_keep], args, torch, batch=50)
        row(f"dual_step B={B} image-to-video ({nk} frozen, re-noised)", tsk)
        lines.append(f"B={B}: image-to-video forward - text-to-video forward = {stats(tg)[0] - mc[0]:+.1f} us (three more gemv launches, mapped "
                     f"modulation rows and gates); step with a prefix - step without = {stats(tsk)[0] - stats(tst)[0]:+.2f} us")
        nbytes = (nv + na) * (4 + 4 + (4 if B == 2 else 0) + 4 + 2 * B)
        lines.append(f"B={B}: the step moves {nbytes / 1e6:.2f} MB; it stands for " + ("2 CFG + " if B == 2 else "") +
                     "2 Euler + 2 cast" + (" + 2 copy" if B == 2 else "") + " launches of separate kernels, and in token layout the loop "
                     "needs none of denoise()'s per-step patchify / unpatchify passes")

        # the loop: 8 steps from sigma 1 to 0
        sig = [1.0 - i / STEPS for i in range(STEPS + 1)]
        lc = ctx_v if B == 2 else ctx_v[:1]
        vl, al = rn(1, 128, *FHW), rn(1, 8, T_A, 16)
        loop = lambda tcache: (lambda: ctx.dual_denoise_dev(vl.clone(), al.clone(), sig, lc, *FHW, mask=mask, cfg_scale=3.0 if B == 2 else 1.0,  # noqa: E731
                                                             text_cache=tcache))
        loop(1)()
        torch.cuda.synchronize()
        tl1, tl0 = measure([loop(1), loop(0)], args, torch, batch=1)
        cond, cnoise = rn(1, 128, 1, *FHW[1:]), rn(STEPS, 128, 1, *FHW[1:])
        i2v = lambda scale: (lambda: ctx.dual_denoise_dev(vl.clone(), al.clone(), sig, lc, *FHW, mask=mask, cfg_scale=3.0 if B == 2 else 1.0,  # noqa: E731
                                                           cond_latent=cond, image_cond_noise_scale=scale, cond_noise=cnoise if scale > 0 else None))
        i2v(0.15)()
        torch.cuda.synchronize()
        tl1, tl0, ti0, ti1 = measure([loop(1), loop(0), i2v(0.0), i2v(0.15)], args, torch, batch=1)
        row(f"loop {STEPS} steps B={B} text cache (prepare inside)", tl1)
        row(f"loop {STEPS} steps B={B} no cache", tl0)
        row(f"loop {STEPS} steps B={B} image-to-video, text cache", ti0)
        row(f"loop {STEPS} steps B={B} image-to-video, re-noised (0.15)", ti1)
        lines.append(f"B={B}: cached loop / uncached loop = {stats(tl1)[0] / stats(tl0)[0]:.3f}; image-to-video loop - text-to-video loop = "
                     f"{stats(ti0)[0] - stats(tl1)[0]:+.1f} us without re-noising, {stats(ti1)[0] - stats(tl1)[0]:+.1f} us with it "
                     f"({STEPS} forwards with groups, one set_frame0, one row map and up to two transposes at entry)")
    lines.append("default of ltx_dual_denoise_args.text_cache: " + ("1 (the gate holds at B 1 and B 2)" if all(verdicts) else
                                                                   "must become 0: the cached forward is slower beyond the spread"))
    lines.append("Not measured: a 48-block model or loop, and the per-block split of the cached saving (k GEMM, k norm, V^T GEMMs).")
    lines.append("Each call is issued from Python through ctypes: rows of a few microseconds sit at the host's issue rate, not at the kernel's time.")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    ctx.dual_model_unload()
    ctx.close()


if __name__ == "__main__":
    main()
