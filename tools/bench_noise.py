#!/usr/bin/env python3
"""Times the noise of a video + audio generation and writes profiles/noise_bench.txt. Two routes to the same draws (the plan of
ltx_dual_noise_plan, in the reference's order):

  * device: every draw of the plan in ONE ltx_op_mlx_normal_group launch (csrc/noise.hip), as ltx_dual_generate_dev makes them. Each
    sample is `--batch` back-to-back launches between two HIP events;
  * host: what the parent commit offers - ltx_mlx_random_normal per draw on one host thread, the scale as a numpy multiply, then the
    upload (torch.from_numpy(...).cuda()), wall clock with a final synchronisation.

Sizes: the headline shape 768x512x25 (VIDEO1 49 152 values at half resolution, 196 608 at full, AUDIO1 for 25 frames) and config 5's
768x512x201, each for the text-to-video and the image-to-video + re-noise two-stage plan (8 + 3 steps). Median and minimum over `--iters`
samples after `--warmup`, the two routes alternating in one process; spread = (p90 - p10) / median. No ratio is gated: both times and
their spreads are the record. `--share-file` / `--wall-file` append what the GPU tests measured (the share of device normals bit-equal
to the host generator, tests/test_mlx_normal_gpu.py; the wall time of each new GPU test file). Run by hand:

    python tools/bench_noise.py [--iters 20] [--warmup 3] [--batch 50] [--out profiles/noise_bench.txt]
"""
import argparse
import importlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 42
SHAPES = {"768x512x25 (headline)": (768, 512, 25), "768x512x201 (config 5)": (768, 512, 201)}


def stats(xs):
    xs = sorted(xs)
    med = statistics.median(xs)
    p10, p90 = xs[int(0.1 * (len(xs) - 1))], xs[int(round(0.9 * (len(xs) - 1)))]
    return med, xs[0], (p90 - p10) / med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noise_bench.txt"))
    ap.add_argument("--share-file")
    ap.add_argument("--wall-file")
    a = ap.parse_args()
    import numpy as np
    import torch

    assert torch.cuda.is_available(), "bench_noise needs a GPU: a CPU run says nothing about the device route"
    ltx = importlib.import_module("ltx-video-swift-mlx_amd")
    ctx = ltx.Context(0)
    lines = [f"noise of a video + audio generation: one grouped device launch against host draws + upload ({torch.cuda.get_device_name(0)})",
             f"iters {a.iters}, warmup {a.warmup}, device batch {a.batch}; us per whole plan; spread = (p90 - p10) / median", ""]
    for label, (w, h, frames) in SHAPES.items():
        F, H, W = ltx.latent_shape(w // 2, h // 2, frames)
        T_a = ltx.audio_latent_frames(frames, 24.0)
        for kind, i2v in (("t2v two-stage", False), ("i2v+renoise two-stage", True)):
            cond = np.zeros(1, np.float32)
            args = ltx.dual_generate_args(SEED, F, H, W, T_a, 1024, ltx.sigmas(True, 8), two_stage=True, cond_latent1=cond if i2v else None,
                                          cond_latent2=cond if i2v else None, image_cond_noise_scale=0.15 if i2v else 0.0)
            plan, total = ltx.dual_noise_plan(args)
            values = sum(d["numel"] for d in plan)
            ws = torch.empty(total, device="cuda")
            audio = torch.empty(128 * T_a, device="cuda")
            jobs = [dict(key=ltx.mlx_draw_key(SEED, d["draw_index"]), dst=ws[d["offset"]:d["offset"] + d["numel"]] if d["offset"] >= 0 else audio,
                         n=d["numel"], scale=d["scale"]) for d in plan]

            def device():
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
                for _ in range(a.batch):
                    ctx.op_mlx_normal_group(jobs)
                ev1.record()
                ev1.synchronize()
                return ev0.elapsed_time(ev1) * 1000.0 / a.batch

            def host():
                torch.cuda.synchronize()
                t = time.perf_counter()
                keep = [torch.from_numpy(np.float32(d["scale"]) * ltx.mlx_random_normal(SEED, (d["numel"],), d["draw_index"])).cuda() for d in plan]
                torch.cuda.synchronize()
                del keep
                return (time.perf_counter() - t) * 1e6

            dev_us, host_us = [], []
            for i in range(a.warmup + a.iters):  # alternating, in one process
                d_, h_ = device(), host()
                if i >= a.warmup:
                    dev_us.append(d_)
                    host_us.append(h_)
            (dm, dmin, ds), (hm, hmin, hs) = stats(dev_us), stats(host_us)
            lines.append(f"{label}, {kind}: {len(plan)} draws, {values} values, workspace {total} floats")
            lines.append(f"    device, one launch    median {dm:10.1f} us  min {dmin:10.1f} us  spread {100 * ds:5.1f} %   "
                         f"({values * 4 / dm / 1e3:.1f} GB/s of f32 written)")
            lines.append(f"    host draws + upload   median {hm:10.1f} us  min {hmin:10.1f} us  spread {100 * hs:5.1f} %   (host / device = {hm / dm:.0f})")
    if a.share_file and os.path.exists(a.share_file):
        eq, tot, share = open(a.share_file).read().split()
        lines += ["", f"device normals bit-equal to the host generator (tests/test_mlx_normal_gpu.py, not asserted): {eq} of {tot} = {100 * float(share):.3f} %; "
                  "the rest are within rtol 2e-6 / atol 1e-7 (the last place of logf)"]
    if a.wall_file and os.path.exists(a.wall_file):
        lines += ["", "wall time of each new GPU test file (pytest process, imports included):"] + ["    " + ln.strip() for ln in open(a.wall_file) if ln.strip()]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)
    ctx.close()


if __name__ == "__main__":
    main()
