#!/usr/bin/env python3
"""Times the audio decode leg (audio VAE decoder + vocoder) at the headline clip, T = 126 audio-latent frames -> 120 240 samples per
channel, with HIP events after warm-up, next to the SAME graph run by torch-ROCm in bf16 in the same process (tests/helpers/audio_ref.py
moved to the GPU; imported here only, never by the library). Also prints the library's per-family kernel time and the convolutions'
fraction of the MFMA peak (ltx_prof_*).

    python tools/bench_audio.py [--T 126] [--iters 20] [--warmup 5] [--out profiles/audio_decode_bench.txt]
"""
import argparse
import importlib
import os
import socket
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
PEAK_BF16 = 2.5e15  # dense bf16 MFMA peak of one MI355X, FLOP/s


def timed(fn, iters, warmup, torch):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=126)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from safetensors.torch import save_file

    import audio_ref as R

    ltx = importlib.import_module("ltx-video-swift-mlx_amd")
    ctx = ltx.Context(0)
    T, Tm = args.T, max(4 * args.T - 3, 1)
    wv, wg = R.build_audio_vae_weights(128), R.build_vocoder_weights(1024)
    with tempfile.TemporaryDirectory() as d:
        save_file(wv, os.path.join(d, "v.safetensors"))
        save_file(wg, os.path.join(d, "g.safetensors"))
        ctx.audio_vae_load(os.path.join(d, "v.safetensors"))
        ctx.vocoder_load(os.path.join(d, "g.safetensors"))
    lat = torch.randn((8, T, 16), generator=R._gen(7)).cuda()
    mel = torch.empty((2, Tm, 64), device="cuda")
    wav = torch.empty((2, 240 * Tm), device="cuda")
    lines = [f"audio decode bench: T={T} mel={Tm} samples={240 * Tm}  device={torch.cuda.get_device_name(0)}  host={socket.gethostname()}  "
             f"torch={torch.__version__}  iters={args.iters} warmup={args.warmup} (median / min, ms, HIP events)"]
    native = {}
    for name, fn in (("audio_vae_decode_dev", lambda: ctx.audio_vae_decode_dev(lat, mel)),
                     ("vocoder_forward_dev", lambda: ctx.vocoder_forward_dev(mel, wav)),
                     ("audio_decode_dev", lambda: ctx.audio_decode_dev(lat, wav))):
        native[name] = timed(fn, args.iters, args.warmup, torch)
        lines.append(f"native  {name:24s} {native[name][0]:9.3f} {native[name][1]:9.3f}")
    # per-family kernel time of one chained decode
    for name, fn in (("audio_vae", lambda: ctx.audio_vae_decode_dev(lat, mel)), ("vocoder", lambda: ctx.vocoder_forward_dev(mel, wav))):
        ctx.prof_enable(True)
        ctx.prof_collect(3, reset=True)
        fn()
        conv = ctx.prof_collect(2)
        elem = ctx.prof_collect(3, reset=True)  # reset clears every kind
        ctx.prof_enable(False)
        lines.append(f"stages  {name:10s} conv: {conv}  row passes: {elem}")
        try:
            ms, flops = conv["ms"], conv["work"]
            lines.append(f"        {name:10s} conv {flops / 1e12:.3f} TFLOP in {ms:.3f} ms = {flops / ms / 1e9:.1f} TFLOP/s = {flops / ms * 1e3 / PEAK_BF16:.3f} of the bf16 MFMA peak")
        except Exception:
            pass
    # the yardstick: the same graph in torch, bf16, on the same device
    bf = torch.bfloat16
    wv_b, wg_b = R.to(wv, "cuda", bf), R.to(wg, "cuda", bf)
    lat_b = lat.to(bf)
    with torch.no_grad():
        mel_b = R.audio_vae_decode(wv_b, lat_b).contiguous()
        yard = {}
        for name, fn in (("audio_vae_decode_dev", lambda: R.audio_vae_decode(wv_b, lat_b)),
                         ("vocoder_forward_dev", lambda: R.vocoder_forward(wg_b, mel_b)),
                         ("audio_decode_dev", lambda: R.audio_decode(wv_b, wg_b, lat_b))):
            yard[name] = timed(fn, args.iters, args.warmup, torch)
            lines.append(f"torch   {name:24s} {yard[name][0]:9.3f} {yard[name][1]:9.3f}")
    for name in native:
        lines.append(f"ratio   {name:24s} native / torch-bf16 = {native[name][0] / yard[name][0]:.3f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
