#!/usr/bin/env python3
"""Times the two-stage video + audio path (ltx_dual_two_stage_dev) and the one launch between its stages (ltx_op_dual_restage) and writes
profiles/dual_two_stage_bench.txt. Full width (video 32 x 128 = 4096, audio 32 x 64 = 2048, caption_channels 3840), L = 1, stage 1 at
(4, 8, 12) = 384 tokens, stage 2 at (4, 16, 24) = 1536 tokens, T_a = 126, S = 1024, a third of the keys masked, image-to-video with
re-noising; the upscaler at mid = 1024 from a synthetic bf16 file written to a temporary directory. Rows:

  * the restage launch (statistics given, so the row is the one launch);
  * the same bridge composed from nine launches: ltx_adain_filter_latent_dev (two launch_mean_var + launch_adain), ltx_renoise_dev on
    the video and on the audio latent, then frame 0, the transpose to token layout and the two bf16 casts. The library has no hook for
    those last four (launch_set_frame0, launch_unpatchify_f32, launch_cast_f32_bf16 x 2), so they are timed as the torch kernels of the
    same traffic (a strided copy, transpose + contiguous, two dtype casts);
  * ltx_upscale_latent_dev;
  * the whole two-stage call, 8 + 3 steps, wall clock with a final synchronisation;
  * the same work through the existing host-glued route, wall clock: ltx_dual_denoise (host pointers) for stage 1, ltx_upscale_latent,
    ltx_adain_filter_latent, the re-noise as a numpy expression, ltx_dual_denoise for stage 2. That route cannot step stage 2's video by
    the plain form; its time is what is compared, not its bits.

The method is tools/bench_dual_denoise.py's: each sample is `--batch` back-to-back calls between two HIP events (the last two rows: one
call, wall clock); median and minimum over `--iters` samples after `--warmup`, variants alternating in one process; spread = (p90 - p10)
/ median. Gate: the restage launch must be faster than the composed bridge by more than both spreads. Run by hand:

    python tools/bench_dual_two_stage.py [--iters 20] [--warmup 3] [--batch 50] [--out profiles/dual_two_stage_bench.txt]
"""
import argparse
import importlib
import math
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
FHW1, T_A, S, CAPTION, L, MID, C = (4, 8, 12), 126, 1024, 3840, 1, 1024, 128
FHW2 = (FHW1[0], 2 * FHW1[1], 2 * FHW1[2])
T1, T2, HW2 = FHW1[0] * FHW1[1] * FHW1[2], FHW2[0] * FHW2[1] * FHW2[2], FHW2[1] * FHW2[2]
STEPS1 = 8
S_NOISE, COND_SCALE = 0.909375, 0.15


def sample(fn, batch, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(batch):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / batch  # us per call


def wall(fn, batch, torch):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e6


def stats(ts):
    ts = sorted(ts)
    med = statistics.median(ts)
    p10, p90 = ts[int(0.1 * (len(ts) - 1))], ts[int(math.ceil(0.9 * (len(ts) - 1)))]
    return med, ts[0], (p90 - p10) / med


def measure(fns, args, torch, batch=None, timer=sample):
    """Alternates the callables sample by sample; returns one list of samples per callable."""
    out = [[] for _ in fns]
    for i in range(args.warmup + args.iters):
        for k, fn in enumerate(fns):
            t = timer(fn, batch or args.batch, torch)
            if i >= args.warmup:
                out[k].append(t)
    return out


def write_upscaler(path, torch):
    """A synthetic upscaler file at mid = MID: the oracle's parameter shapes, N(0, 1 / fan-in) weights drawn on the device, stored as bf16."""
    import ltx_oracle as oracle
    from safetensors.torch import save_file

    g = torch.Generator(device="cuda").manual_seed(4)
    w = {}
    for k, shp in oracle.upscaler_param_shapes(MID).items():
        t = torch.randn(tuple(shp), device="cuda", generator=g)
        if "norm" in k and k.endswith(".weight"):
            t = 1.0 + 0.1 * t
        elif k.endswith(".bias"):
            t = 0.05 * t
        else:
            t = t / math.sqrt(float(math.prod(shp[1:])))
        w[k] = t.to(torch.bfloat16).cpu().contiguous()
    save_file(w, path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from safetensors.numpy import save_file as save_np

    ltx = importlib.import_module("ltx-video-swift-mlx_amd")
    assert torch.cuda.is_available(), "this benchmark needs the GPU: there is no CPU path"
    ctx = ltx.Context(0)
    ctx.dual_model_init_synthetic(ltx.default_dual_model_config(num_layers=L), seed=9)
    with tempfile.TemporaryDirectory() as d:
        write_upscaler(os.path.join(d, "up.safetensors"), torch)
        ctx.upscaler_load(os.path.join(d, "up.safetensors"))
        rng = np.random.default_rng(0)
        save_np({"latents_mean": (0.2 * rng.standard_normal(C)).astype(np.float32), "latents_std": (1.0 + 0.3 * rng.random(C)).astype(np.float32)},
                os.path.join(d, "vae.safetensors"))
        ctx.vae_load(os.path.join(d, "vae.safetensors"))
    g = torch.Generator(device="cuda").manual_seed(1)
    rn = lambda *s: torch.randn(s, device="cuda", generator=g)  # noqa: E731
    bf = torch.bfloat16
    lines = [f"two-stage video + audio path, full width, L = {L}: stage 1 {FHW1} = {T1} tokens, stage 2 {FHW2} = {T2} tokens, T_a {T_A}, S {S}, a third of "
             f"the keys masked, image-to-video with re-noising, upscaler mid {MID}; us per call, median / min of {args.iters} samples of {args.batch} "
             f"calls (whole path: 1 call, wall clock) after {args.warmup} warm-up samples; spread = (p90 - p10) / median; torch {torch.__version__}",
             f"{'row':<64}{'median us':>12}{'min us':>12}{'spread':>9}"]
    row = lambda name, ts: lines.append("{:<64}{:>12.1f}{:>12.1f}{:>8.1f}%".format(name, stats(ts)[0], stats(ts)[1], 100 * stats(ts)[2]))  # noqa: E731

    # ---- the bridge ----
    nv, na = T2 * C, T_A * C
    x, ref, noise = 1.5 * rn(C, T2) + 0.3, rn(C, T1), rn(C, T2)
    cond, cnoise = rn(C, HW2), rn(C, HW2)
    xa, anoise = rn(T_A, C), rn(T_A, C)
    st = torch.stack([x.mean(1), x.var(1, unbiased=False)], 1).contiguous()
    sr = torch.stack([ref.mean(1), ref.var(1, unbiased=False)], 1).contiguous()
    lat, tok = torch.empty((T2, C), device="cuda"), torch.empty((T2, C), device="cuda", dtype=bf)
    xa_w, atok = xa.clone(), torch.empty((T_A, C), device="cuda", dtype=bf)
    s2 = float(np.float32(S_NOISE) * np.float32(S_NOISE))
    vj = dict(x=x, latent=lat, tokens=tok, stats=st, stats_ref=sr, noise=noise, noise_scale=S_NOISE, cond=cond, cond_noise=cnoise,
              cond_scale=COND_SCALE, cond_sigma2=s2)
    aj = dict(latent=xa_w, tokens=atok, noise=anoise, noise_scale=S_NOISE)
    restage = lambda: ctx.op_dual_restage(vj, aj)  # noqa: E731
    xw, frame0 = x.clone(), (cond + (COND_SCALE * cnoise) * s2).contiguous()
    lat9, tok9, atok9 = torch.empty((T2, C), device="cuda"), torch.empty((T2, C), device="cuda", dtype=bf), torch.empty((T_A, C), device="cuda", dtype=bf)
    lib = ltx.lib

    def composed():
        ctx._ck(lib.ltx_adain_filter_latent_dev(ctx._h, xw.data_ptr(), T2, ref.data_ptr(), T1, C, 1.0))  # 3 launches
        ctx._ck(lib.ltx_renoise_dev(ctx._h, xw.data_ptr(), noise.data_ptr(), S_NOISE, nv))
        ctx._ck(lib.ltx_renoise_dev(ctx._h, xa_w.data_ptr(), anoise.data_ptr(), S_NOISE, na))
        xw[:, :HW2].copy_(frame0)            # for launch_set_frame0
        lat9.copy_(xw.t())                   # for launch_unpatchify_f32
        tok9.copy_(lat9)                     # for launch_cast_f32_bf16
        atok9.copy_(xa_w)                    # for launch_cast_f32_bf16
    restage()  # the context launches on torch's current stream, so the torch kernels are ordered with the library's
    composed()
    torch.cuda.synchronize()
    t_r, t_c = measure([restage, composed], args, torch)
    row("restage: 1 launch (ltx_op_dual_restage)", t_r)
    row("the same bridge from 9 launches (5 library + 4 torch)", t_c)
    mr, mc = stats(t_r), stats(t_c)
    gate = mr[0] < mc[0] * (1 - max(mr[2], mc[2]))
    lines.append(f"restage / composed = {mr[0] / mc[0]:.3f}; video job: reads 2 * nv * 4 = {2 * nv * 4 / 1e6:.2f} MB, writes nv * 6 = {nv * 6 / 1e6:.2f} MB "
                 f"(+ audio {na * 14 / 1e6:.2f} MB); the composed bridge moves about 11 * nv * 4 = {11 * nv * 4 / 1e6:.2f} MB. Gate (faster by more "
                 f"than both spreads): " + ("holds" if gate else "DOES NOT HOLD"))

    # ---- the upscaler ----
    v1, up = rn(1, C, *FHW1), torch.empty((1, C, *FHW2), device="cuda")
    upscale = lambda: ctx.upscale_latent_dev(v1, up)  # noqa: E731
    upscale()
    torch.cuda.synchronize()
    (t_u,) = measure([upscale], args, torch, batch=5)
    row(f"upscaler_forward {FHW1} -> {FHW2}, mid {MID}", t_u)

    # ---- the whole path ----
    sig1 = [1.0 - i / STEPS1 for i in range(STEPS1 + 1)]
    sig2 = list(ltx.stage2_sigmas())
    ctx_v = (4 * rn(1, S, CAPTION)).to(bf)
    mask = torch.ones((1, S), device="cuda", dtype=torch.int32)
    mask[:, S - S // 3:] = 0
    vl, al = rn(1, C, *FHW1), rn(1, 8, T_A, 16)
    vn2, an2 = rn(1, C, *FHW2), rn(T_A, C)
    c1, c2 = rn(1, C, 1, *FHW1[1:]), rn(1, C, 1, *FHW2[1:])
    n1, n2 = rn(STEPS1, C, 1, *FHW1[1:]), rn(len(sig2) - 1, C, 1, *FHW2[1:])
    out = torch.empty((1, C, *FHW2), device="cuda")
    whole = lambda: ctx.dual_two_stage_dev(vl, out, al.clone(), sig1, vn2, an2, ctx_v, *FHW1, mask=mask, cond_latent1=c1, cond_latent2=c2,  # noqa: E731
                                           image_cond_noise_scale=COND_SCALE, cond_noise1=n1, cond_noise2=n2)
    h = {k: t.cpu().numpy() for k, t in dict(vl=vl, al=al, vn2=vn2, an2=an2, c1=c1, c2=c2, n1=n1, n2=n2, mask=mask).items()}
    h_ctx = ctx_v.view(torch.int16).cpu().numpy().view(np.uint16)

    def glued():
        v, a = ctx.dual_denoise(h["vl"], h["al"], sig1, h_ctx, *FHW1, mask=h["mask"], cond_latent=h["c1"], image_cond_noise_scale=COND_SCALE,
                                cond_noise=h["n1"])
        u = ctx.adain_filter_latent(ctx.upscale_latent(v), v)
        s = np.float32(sig2[0])
        u = (s * h["vn2"] + (np.float32(1.0) - s) * u).astype(np.float32)
        a = (s * h["an2"].reshape(T_A, 8, 16).transpose(1, 0, 2)[None] + (np.float32(1.0) - s) * a).astype(np.float32)
        ctx.dual_denoise(u, a, sig2, h_ctx, *FHW2, mask=h["mask"], cond_latent=h["c2"], image_cond_noise_scale=COND_SCALE, cond_noise=h["n2"])
    whole()
    glued()
    t_w, t_g = measure([whole, glued], args, torch, batch=1, timer=wall)
    row(f"two-stage call, {STEPS1} + {len(sig2) - 1} steps (ltx_dual_two_stage_dev)", t_w)
    row("the same through the host-glued route (5 host-pointer calls)", t_g)
    lines.append(f"two-stage call / host-glued route = {stats(t_w)[0] / stats(t_g)[0]:.3f}; the call holds both latents on the device, fills the text "
                 f"cache once (the glued route twice) and crosses to host memory at no stage boundary (the glued route at four)")
    lines.append("Not measured: a 48-block model. The four torch stand-ins of the composed bridge are not the library's kernels; their traffic is the same.")
    lines.append("Each call is issued from Python through ctypes: rows of a few microseconds sit at the host's issue rate, not at the kernel's time.")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
