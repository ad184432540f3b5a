"""`ltx-video decode-audio --synthetic` writes a WAV whose header and length match the frame-count helpers."""
import os
import struct
import subprocess
import wave

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "ltx-video-swift-mlx_amd", "csrc", "build", "ltx-video")


def test_decode_audio_usage_errors(ltx):
    """No GPU needed: argument validation happens before the pipeline is created."""
    r = subprocess.run([CLI, "decode-audio"], capture_output=True, text=True)
    assert r.returncode == 64 and "--latent" in r.stderr and "--synthetic" in r.stderr
    r = subprocess.run([CLI, "decode-audio", "--latent", "x.safetensors"], capture_output=True, text=True)
    assert r.returncode == 64 and "--vocoder-weights" in r.stderr


@pytest.mark.gpu
def test_decode_audio_synthetic_writes_wav(ltx, tmp_path):
    out = tmp_path / "a.wav"
    frames = 25
    r = subprocess.run([CLI, "decode-audio", "--synthetic", "--frames", str(frames), "--audio-gain", "0.5", "-o", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    T = ltx.audio_latent_frames(frames, 24)
    assert T == 26
    n = ltx.audio_sample_count(T)
    raw = open(out, "rb").read()
    assert len(raw) == 44 + n * 4
    assert raw[:4] == b"RIFF" and raw[8:16] == b"WAVEfmt " and struct.unpack("<I", raw[40:44])[0] == n * 4
    with wave.open(str(out), "rb") as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (2, 2, ltx.audio_sample_rate(), n)
        pcm = f.readframes(n)
    assert any(pcm), "silent output"
    assert f"{n} samples/channel" in r.stdout
