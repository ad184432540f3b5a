#!/usr/bin/env python3
"""Times the dual video + audio model above its blocks (ltx_dual_model_*; video 32 x 128 = 4096, audio 32 x 64 = 2048,
caption_channels 3840, L = 1) and writes profiles/dual_model_bench.txt:

  * the timestep path alone through ltx_dual_model_embed_dev, grouped (three launch_gemv_group launches of six jobs) against ungrouped
    (the 18 launch_gemv_f32 launches it replaces: the baseline), at B = 1 and B = 2, alternating sample by sample in one process; the
    grouped path's bytes per second are the bf16 weights it must stream (computed from the shapes below) over its median time,
    against the 6.29 TB/s copy rate of the MI355X. The weights (0.6 GB) exceed every cache, so each call streams them from HBM;
  * one whole forward at L = 1 with T_v = 1536 = (4, 16, 24), T_a = 126, S = 1024, B = 1, grouped and ungrouped.

Each sample is `--batch` back-to-back calls between two HIP events; the median and the minimum over `--iters` samples after `--warmup`
are reported, and the run-to-run spread of a row is (p90 - p10) / median of its samples. The grouped path stays the default only if
its median is not above the ungrouped median by more than the larger of the two spreads. Run by hand:

    python tools/bench_dual_model.py [--iters 20] [--warmup 3] [--batch 10] [--out profiles/dual_model_bench.txt]
"""
import argparse
import importlib
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HV = HA = 32
DV, DA = HV * 128, HA * 64
FHW, T_A, S, CAPTION = (4, 16, 24), 126, 1024, 3840
T_V = FHW[0] * FHW[1] * FHW[2]
COPY_RATE = 6.29e12  # bytes / s, the device copy rate of the MI355X


def embed_weight_bytes():
    """bf16 weight bytes of the six embedders: per stream 3 x 256 x D (first Linears) + (1 + 1 + 1) x D^2 (second) + (6 + 4 + 1) x D^2."""
    return sum(2 * (3 * 256 * D + 14 * D * D) for D in (DV, DA))


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


def measure(fns, args, torch):
    """Alternates the callables sample by sample; returns one list of samples per callable."""
    out = [[] for _ in fns]
    for i in range(args.warmup + args.iters):
        for k, fn in enumerate(fns):
            t = sample(fn, args.batch, torch)
            if i >= args.warmup:
                out[k].append(t)
    return out


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
    ctx = ltx.Context(0)
    ctx.dual_model_init_synthetic(ltx.default_dual_model_config(num_layers=1), seed=9)
    g = torch.Generator(device="cuda").manual_seed(1)
    rn = lambda *s: torch.randn(s, device="cuda", generator=g)  # noqa: E731
    wbytes = embed_weight_bytes()
    lines = [f"dual video + audio model, full width: Dv {DV} (32 x 128), Da {DA} (32 x 64), caption_channels {CAPTION}, one block; us per call, "
             f"median / min of {args.iters} samples of {args.batch} calls after {args.warmup} warm-up samples; spread = (p90 - p10) / median; "
             f"torch {torch.__version__}",
             f"timestep path: six embedders, {wbytes / 1e9:.3f} GB of bf16 weights per call; floor at {COPY_RATE / 1e12:.2f} TB/s = {wbytes / COPY_RATE * 1e6:.1f} us",
             f"{'row':<44}{'median us':>12}{'min us':>12}{'spread':>9}"]
    row = lambda name, ts: lines.append("{:<44}{:>12.1f}{:>12.1f}{:>8.1f}%".format(name, stats(ts)[0], stats(ts)[1], 100 * stats(ts)[2]))  # noqa: E731

    verdicts = []
    for B in (1, 2):
        ts_v, ts_a = torch.rand(B, device="cuda", generator=g), torch.rand(B, device="cuda", generator=g)
        mk = lambda: [torch.empty(s, device="cuda") for s in ((B, 6, DV), (B, 6, DA), (B, 5, DV), (B, 5, DA), (B, DV), (B, DA))]  # noqa: E731
        og, ou = mk(), mk()
        grouped = lambda: ctx.dual_model_embed_dev(ts_v, ts_a, *og, ungrouped=False)  # noqa: E731
        ungrouped = lambda: ctx.dual_model_embed_dev(ts_v, ts_a, *ou, ungrouped=True)  # noqa: E731
        grouped()
        ungrouped()
        torch.cuda.synchronize()
        equal = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(og, ou))
        tg, tu = measure([grouped, ungrouped], args, torch)
        row(f"timestep path B={B} grouped (5 launches)", tg)
        row(f"timestep path B={B} ungrouped (20 launches)", tu)
        mg, mu = stats(tg), stats(tu)
        keep = mg[0] <= mu[0] * (1 + max(mg[2], mu[2]))
        verdicts.append(keep)
        lines.append(f"B={B}: grouped / ungrouped = {mg[0] / mu[0]:.3f}; outputs bit-equal: {equal}; grouped streams {wbytes / (mg[0] * 1e-6) / 1e12:.2f} TB/s = "
                     f"{100 * wbytes / (mg[0] * 1e-6) / COPY_RATE:.0f}% of the copy rate (ungrouped {wbytes / (mu[0] * 1e-6) / 1e12:.2f} TB/s); "
                     + ("grouped is not slower beyond the spread" if keep else "grouped is SLOWER beyond the spread"))
    lines.append("default: " + ("grouped (three launch_gemv_group launches)" if all(verdicts) else
                                "UNGROUPED must become the default of dual_model_forward; the grouped kernel stays behind the seam"))

    # one whole forward at L = 1, the shape of DESIGN.md section 6c
    bf = torch.bfloat16
    lat_v, lat_a = rn(1, T_V, 128).to(bf), rn(1, T_A, 128).to(bf)
    ctx_v, ctx_a = (4 * rn(1, S, CAPTION)).to(bf), (4 * rn(1, S, CAPTION)).to(bf)
    mask = torch.ones((1, S), device="cuda", dtype=torch.int32)
    mask[:, S - S // 3:] = 0
    ts_v, ts_a = torch.tensor([0.875], device="cuda"), torch.tensor([0.25], device="cuda")
    vv, va = torch.empty((1, T_V, 128), device="cuda"), torch.empty((1, T_A, 128), device="cuda")
    fwd = lambda u: (lambda: ctx.dual_model_forward_dev(lat_v, lat_a, ctx_v, ctx_a, ts_v, ts_a, vv, va, *FHW, video_mask=mask, audio_mask=mask,  # noqa: E731
                                                        ungrouped=u))
    fwd(False)()
    torch.cuda.synchronize()
    finite = bool(torch.isfinite(vv).all() and torch.isfinite(va).all())
    fg, fu = measure([fwd(False), fwd(True)], args, torch)
    row(f"forward L=1 T_v={T_V} T_a={T_A} S={S} grouped", fg)
    row("the same, ungrouped timestep path", fu)
    lines.append(f"forward outputs finite: {finite}. Not measured: a 48-block model, B > 1 at full width for the whole forward.")
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
