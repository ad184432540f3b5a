"""Audio decode leg, host side: frame-count helpers, the WAV writer, the conditions that keep the torch restatement
(tests/helpers/audio_ref.py) a meaningful reference, and the loaders' reporting (the last needs a device to load onto)."""
import os
import struct
import sys
import wave

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))


def test_audio_frame_counts(ltx):
    """computeAudioLatentFrames (LTXPipeline.swift:530-534) known answers; mel = max(4T-3, 1); samples = 240 mel; 24 kHz."""
    for n, want in ((9, 9), (25, 26), (121, 126), (241, 251)):
        assert ltx.audio_latent_frames(n, 24) == want, n
    for T in (1, 2, 5, 126, 251):
        assert ltx.audio_mel_frames(T) == max(4 * T - 3, 1)
        assert ltx.audio_sample_count(T) == 240 * max(4 * T - 3, 1)
    assert ltx.audio_mel_frames(126) == 501 and ltx.audio_sample_count(126) == 120240
    assert ltx.audio_sample_rate() == 24000


@pytest.mark.parametrize("gain", [0.5, 1.0])
def test_write_wav_bytes(ltx, tmp_path, gain):
    """ltx_write_wav is byte-identical to a file assembled here (AudioExporter.swift:19-92) and readable by the stdlib."""
    left = np.array([1.0, -1.0, 0.99999, -0.99999, 1.5, -0.00002, 0.25, -1.5], np.float32)
    right = left[::-1].copy()
    wav = np.stack([left, right])
    path = tmp_path / "a.wav"
    ltx.write_wav(path, wav, 24000, gain)
    n = wav.shape[1]
    g = wav * np.float32(gain) if gain != 1.0 else wav
    scaled = np.clip(g, np.float32(-1), np.float32(1)).astype(np.float32) * np.float32(32767.0)
    pcm = np.trunc(scaled).astype("<i2")  # truncation toward zero
    data = pcm.T.tobytes()  # interleaved L0 R0 L1 R1 ...
    hdr = b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 1, 2, 24000, 24000 * 4, 4, 16)
    hdr += b"data" + struct.pack("<I", len(data))
    assert len(hdr) == 44
    got = open(path, "rb").read()
    assert got == hdr + data
    if gain == 1.0:
        assert list(pcm[0][:6]) == [32767, -32767, 32766, -32766, 32767, 0]
    with wave.open(str(path), "rb") as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (2, 2, 24000, n)
        assert f.readframes(n) == data


def test_reference_conditions():
    """The reference alone, narrow model: stage stds in [0.1, 10], pre-tanh std in [0.1, 1.0], < 1 % of pre-tanh samples beyond 3."""
    import torch

    import audio_ref as R

    wv, wg = R.build_audio_vae_weights(32), R.build_vocoder_weights(128)
    for T in (5, 30):
        lat = torch.randn((8, T, 16), generator=R._gen(3))
        stages, pre = [], []
        mel = R.audio_vae_decode(wv, lat, stages)
        assert mel.shape == (2, max(4 * T - 3, 1), 64)
        wav = R.vocoder_forward(wg, mel, stages, pre)
        assert wav.shape == (2, 240 * mel.shape[1])
        assert len(stages) == 4 + 5
        for s in stages + [mel]:
            assert 0.1 <= float(s.std()) <= 10.0, float(s.std())
        p = pre[0]
        assert 0.1 <= float(p.std()) <= 1.0, float(p.std())
        assert float((p.abs() > 3).float().mean()) < 0.01


@pytest.mark.gpu
def test_audio_loaders_report(ltx, gpu_ctx, tmp_path):
    """Foreign keys, encoder keys and a wrong-rank tensor are dropped or reported through ltx_load_report, never silently applied."""
    import torch
    from safetensors.torch import save_file

    import audio_ref as R

    wv = R.build_audio_vae_weights(32, with_encoder_keys=True)
    n_dec = sum(1 for k in wv if k.startswith("decoder.")) + 2
    p = str(tmp_path / "vae.safetensors")
    save_file(wv, p)
    gpu_ctx.audio_vae_load(p)
    assert gpu_ctx.load_report() == {'loaded': n_dec, 'missing': 0, 'unmatched': 0}  # encoder.* filtered before matching (ModelDownloader.swift:1120-1126)
    bad = dict(wv)
    bad["decoder.bogus.conv.weight"] = torch.zeros(4, 4)          # kept by the filter, no such parameter
    bad["decoder.conv_out.conv.bias"] = torch.zeros(2, 1)         # wrong rank: not applied, the bias counts as missing
    bad["foreign.weight"] = torch.zeros(3)
    del bad["latents_std"]
    save_file(bad, p)
    gpu_ctx.audio_vae_load(p)
    assert gpu_ctx.load_report() == {'loaded': n_dec - 2, 'missing': 2, 'unmatched': 2}
    broken = dict(wv)
    broken["decoder.mid.block_1.conv1.conv.weight"] = torch.zeros(8, 8)  # wrong rank on a convolution: the load fails loudly
    save_file(broken, p)
    with pytest.raises(ltx.LTXError) as e:
        gpu_ctx.audio_vae_load(p)
    assert e.value.case == "weightLoadingFailed"
    with pytest.raises(ltx.LTXError) as e:
        gpu_ctx.audio_vae_decode(np.zeros((8, 2, 16), np.float32))
    assert e.value.case == "modelNotLoaded"

    wg = R.build_vocoder_weights(128)
    q = str(tmp_path / "voc.safetensors")
    save_file(wg, q)
    gpu_ctx.vocoder_load(q)
    assert gpu_ctx.load_report() == {'loaded': len(wg), 'missing': 0, 'unmatched': 0}
    bad = dict(wg)
    bad["discriminator.0.weight"] = torch.zeros(2, 2, 2)
    bad["resnets.3.convs1.0.bias"] = torch.zeros(1, 1)
    save_file(bad, q)
    gpu_ctx.vocoder_load(q)
    assert gpu_ctx.load_report() == {'loaded': len(wg) - 1, 'missing': 1, 'unmatched': 2}
    gpu_ctx.vocoder_unload()
    gpu_ctx.audio_vae_unload()


@pytest.mark.gpu
@pytest.mark.parametrize("k,s,p", [(16, 6, 5), (15, 5, 5), (8, 2, 3), (4, 2, 1)])
def test_conv_transpose1d_phase_slabs_read_back(gpu_ctx, k, s, p):
    """The [Cout][taps][Cin] phase slabs, read back element by element: unit impulses, one input channel per row block, make the
    output of ltx_op_conv_transpose1d a copy of the weights in the order the phases placed them, and every weight is distinct from
    its neighbours in all three indices. Same reference and same exact comparison as tests/test_audio_gpu.py
    (torch conv_transpose1d, torch.equal). The hook builds its slabs with convt_phase_slab, the function the vocoder loader calls,
    so this comparison and those of test_audio_gpu.py cover the loader's reorder too (needs a device to launch on)."""
    import torch
    import torch.nn.functional as F

    cin, cout, gap = 64, 32, 8  # gap rows between impulses >= the k / s rows one impulse reaches
    c, o, j = torch.meshgrid(torch.arange(cin), torch.arange(cout), torch.arange(k), indexing="ij")
    w = ((c * 31 + o * 7 + j * 3) % 201 - 100).float()  # torch layout (in, out, k); integers, exact in bf16
    x = torch.zeros((cin * gap, cin))
    x[torch.arange(cin) * gap + 3, torch.arange(cin)] = 1.0
    L = x.shape[0]
    ref = F.conv_transpose1d(x.t()[None].double(), w.double(), None, stride=s, padding=p)[0].t().float()
    assert ref.shape == (s * L, cout) and len(torch.unique(ref)) > 150
    out = torch.full((s * L, cout), float("nan"), device="cuda")
    gpu_ctx.op_conv_transpose1d(x.to(torch.bfloat16).cuda().contiguous(), w.to(torch.bfloat16).cuda().contiguous(), None, s, p, out_f32=out)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), ref)
