"""`ltx-video generate --audio [--two-stage]`: a clip with sound from a seed alone (host/ltx_video_cli.cpp over
LTXPipeline::generateVideoWithAudio / generateVideoWithAudioTwoStage, host/LTXVideo.hpp). CPU: validation and the missing-weights
messages. GPU: a narrow dual checkpoint exported from a synthetic model (as tests/test_dual_two_stage_gpu.py makes one), the synthetic
upscaler, a synthetic video VAE and narrow audio models, 9 frames at 64 x 64: frames and a WAV exist, the WAV holds
ltx_audio_sample_count(T_a) samples per channel, the same seed gives the same files and another seed other files."""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "ltx-video-swift-mlx_amd", "csrc", "build", "ltx-video")
LAYERS, HV, HA, CAPTION, S = 2, 4, 4, 256, 24
FRAMES, SIDE = 9, 64


def run(*args):
    p = subprocess.run([CLI, *args], capture_output=True, text=True, timeout=600)
    return p.returncode, p.stdout, p.stderr


def test_audio_dry_run_validates(ltx):
    rc, out, _ = run("generate", "rain on a tin roof", "--audio", "--dry-run")
    assert rc == 0 and "Audio: enabled" in out and out.strip().endswith("Validation passed (dry run mode)")
    rc, out, _ = run("generate", "x", "--audio", "--two-stage", "-w", "128", "-h", "64", "-f", "9", "--audio-gain", "0.5", "--audio-heads", "4",
                     "--audio-vae-weights", "a.safetensors", "--vocoder-weights", "v.safetensors", "--dry-run")
    assert rc == 0 and "Two-stage pipeline: 64x32 -> upscale 2x -> 128x64" in out
    rc, _, err = run("generate", "x", "--audio", "--two-stage", "-w", "96", "--dry-run")
    assert rc == 64 and "Two-stage requires width and height divisible by 64" in err


def test_missing_weights_errors_name_the_audio_files(ltx):
    rc, _, err = run("generate", "x", "--audio")
    assert rc == 64 and "--audio-vae-weights" in err and "--vocoder-weights" in err
    rc, _, err = run("generate", "x", "--audio", "--audio-vae-weights", "a.safetensors")
    assert rc == 64 and "--vocoder-weights" in err
    rc, _, err = run("generate", "x", "--audio", "--two-stage", "--audio-vae-weights", "a.safetensors", "--vocoder-weights", "v.safetensors")
    assert rc == 64 and "--upscaler-weights" in err
    rc, _, err = run("generate", "x", "--audio", "--audio-vae-weights", "a.safetensors", "--vocoder-weights", "v.safetensors")
    assert rc == 64 and "--ltx-weights" in err and "--vae-weights" in err
    # what stays refused
    rc, _, err = run("generate", "x", "--audio", "--image", "cat.png")
    assert rc == 64 and "--image-tensor" in err
    rc, _, err = run("generate", "x", "--enhance-prompt")
    assert rc == 64 and "--enhance-prompt" in err


@pytest.fixture(scope="module")
def weights(ltx, oracle, tmp_path_factory):
    """Every file the command reads, written once."""
    import torch
    from safetensors.numpy import save_file
    from safetensors.torch import save_file as save_torch

    import audio_ref
    import dual_model_ref as ref

    d = tmp_path_factory.mktemp("cli_generate_audio")
    ctx = ltx.Context(0)
    try:
        cfg = ltx.default_dual_model_config(num_layers=LAYERS, video_heads=HV, audio_heads=HA, caption_channels=CAPTION)
        ctx.dual_model_init_synthetic(cfg, seed=81)
        shapes = ref.param_shapes(LAYERS, HV, HA, caption_channels=CAPTION)
        w = {k: ctx.dual_model_export_param(k).reshape(s) for k, s in shapes.items()}
    finally:
        ctx.close()
    save_file({ref.checkpoint_spelling(k): np.ascontiguousarray(v, dtype=np.float32) for k, v in w.items()}, str(d / "dual.safetensors"))
    wu = oracle.synth_upscaler_weights(mid=64, seed=4)
    save_file({k: np.ascontiguousarray(v, dtype=np.float32) for k, v in wu.items()}, str(d / "up.safetensors"))
    wv = oracle.synth_vae_weights(seed=5)
    save_torch({k: torch.from_numpy(np.ascontiguousarray(v)).to(torch.bfloat16 if v.ndim == 5 else torch.float32)
                for k, v in oracle.vae_file_keys(wv).items()}, str(d / "vae.safetensors"))
    (d / "config.json").write_text(json.dumps({"timestep_conditioning": False}))
    save_torch(audio_ref.build_audio_vae_weights(32), str(d / "audio_vae.safetensors"))
    save_torch(audio_ref.build_vocoder_weights(128), str(d / "vocoder.safetensors"))
    rng = np.random.default_rng(0)
    save_file({"prompt_embeddings": rng.standard_normal((1, S, CAPTION)).astype(np.float32), "prompt_mask": np.ones((1, S), np.int32)},
              str(d / "emb.safetensors"))
    return d


def generate(d, out, seed, two_stage):
    side = 2 * SIDE if two_stage else SIDE  # two-stage: stage 1 at 64 x 64, the smallest the validators allow for it
    args = ["generate", "a bell", "--audio", "-w", str(side), "-h", str(side), "-f", str(FRAMES), "--seed", str(seed), "-o", str(out),
            "--ltx-weights", str(d / "dual.safetensors"), "--vae-weights", str(d / "vae.safetensors"),
            "--audio-vae-weights", str(d / "audio_vae.safetensors"), "--vocoder-weights", str(d / "vocoder.safetensors"),
            "--embeddings", str(d / "emb.safetensors"), "--num-layers", str(LAYERS), "--num-heads", str(HV), "--audio-heads", str(HA),
            "--caption-channels", str(CAPTION)]
    if two_stage:
        args += ["--two-stage", "--upscaler-weights", str(d / "up.safetensors")]
    rc, so, se = run(*args)
    assert rc == 0, se
    return so, side


@pytest.mark.gpu
@pytest.mark.parametrize("two_stage", [False, True], ids=["one-stage", "two-stage"])
def test_generate_audio_writes_frames_and_a_wav_from_a_seed(ltx, weights, tmp_path, two_stage):
    outs = [tmp_path / "a.raw", tmp_path / "b.raw", tmp_path / "c.raw"]
    so, side = generate(weights, outs[0], 7, two_stage)
    generate(weights, outs[1], 7, two_stage)
    generate(weights, outs[2], 8, two_stage)
    steps = 8 + 3 if two_stage else 8
    assert f"Step {steps}/{steps}" in so and f"Generated {FRAMES} frames ({side}x{side})" in so
    T_a = ltx.audio_latent_frames(FRAMES, 24)
    n = ltx.audio_sample_count(T_a)
    assert f"{n} samples/channel" in so
    meta = json.loads(open(str(outs[0]) + ".json").read())
    assert meta == {"frames": FRAMES, "height": side, "width": side, "channels": 3, "dtype": "float32", "range": [0, 1], "seed": 7}
    frames = np.fromfile(outs[0], np.float32).reshape(FRAMES, side, side, 3)
    assert np.isfinite(frames).all() and frames.min() >= 0 and frames.max() <= 1 and frames.std() > 0
    with wave.open(str(outs[0]) + ".wav", "rb") as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (2, 2, ltx.audio_sample_rate(), n)
        assert any(f.readframes(n)), "silent output"
    same = lambda a, b, ext: open(str(a) + ext, "rb").read() == open(str(b) + ext, "rb").read()  # noqa: E731
    assert same(outs[0], outs[1], "") and same(outs[0], outs[1], ".wav")  # a seed is a clip
    assert not same(outs[0], outs[2], "") and not same(outs[0], outs[2], ".wav")
