"""Audio decode leg on the GPU: the three convolution forms integer-exact against torch, each fused epilogue against its unfused
composition, and the two models (narrow and full width, T = 5 and the headline T = 126) against the f32 torch restatement of
tests/helpers/audio_ref.py.

Model bound: rel-L2 <= 3e-2 and cosine >= 0.999 on the mel and on the waveform - the project's bound for about 30 bf16 convolutions in a
row over an f32 residual stream (tests/test_vae_encoder_gpu.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

pytestmark = pytest.mark.gpu

REL_L2, COSINE = 3e-2, 0.999
UPS = [(16, 6, 5), (15, 5, 5), (8, 2, 3), (4, 2, 1), (4, 2, 1)]  # the vocoder's five (k, stride, padding)


def _ints(torch, shape, lo, hi, seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _bits(t):
    """f32 tensor holding bf16-exact values -> device bf16 tensor (the ABI's uint16 operands)."""
    import torch

    return t.to(torch.bfloat16).cuda().contiguous()


# ---------------------------------------------------------------------------------------------------------------
# operators, integer-exact
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout", [(128, 1024), (512, 512), (256, 256), (128, 128), (64, 64), (32, 32), (32, 2)])
def test_conv1d_integer_exact(gpu_ctx, cin, cout):
    """k in {3, 7, 11} x dilation in {1, 3, 5}; L = 203 is no multiple of any tile, L = 7 is shorter than the receptive field."""
    import torch
    import torch.nn.functional as F

    seed = cin * 7 + cout
    for k in (3, 7, 11):
        w = _ints(torch, (cout, cin, k), -2, 2, seed + k)  # torch layout (out, in, k)
        b = _ints(torch, (cout,), -8, 8, seed + 1)
        w_dev = _bits(w.permute(0, 2, 1))  # [Cout][k][Cin]
        for dil in (1, 3, 5):
            for L in (203, 7):
                x = _ints(torch, (L, cin), -3, 3, seed + L + dil)
                ref = F.conv1d(x.t()[None].double(), w.double(), b.double(), padding=dil * (k - 1) // 2, dilation=dil)[0].t().float()
                out = torch.full((L, cout), float("nan"), device="cuda")
                gpu_ctx.op_conv1d(_bits(x), w_dev, b.cuda(), dilation=dil, out_f32=out)
                torch.cuda.synchronize()
                assert torch.equal(out.cpu(), ref), (k, dil, L)
    # every instance on this shape
    k, dil, L = 7, 3, 203
    w = _ints(torch, (cout, cin, k), -2, 2, seed)
    x = _ints(torch, (L, cin), -3, 3, seed + 5)
    ref = F.conv1d(x.t()[None].double(), w.double(), None, padding=dil * (k - 1) // 2, dilation=dil)[0].t().float()
    for tile in (128, 64, 32):
        out = torch.full((L, cout), float("nan"), device="cuda")
        gpu_ctx.op_conv1d(_bits(x), _bits(w.permute(0, 2, 1)), None, dilation=dil, tile=tile, out_f32=out)
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), ref), tile


@pytest.mark.parametrize("stage", range(5))
def test_conv_transpose1d_integer_exact(gpu_ctx, stage):
    """The vocoder's five (k, s, p), at the stage's own channel counts; the output has exactly s * L rows."""
    import torch
    import torch.nn.functional as F

    k, s, p = UPS[stage]
    cin = 1024 >> stage
    cout = cin // 2
    for L in (37, 3):
        x = _ints(torch, (L, cin), -3, 3, stage + L)
        w = _ints(torch, (cin, cout, k), -2, 2, stage + 11)  # torch layout (in, out, k)
        b = _ints(torch, (cout,), -8, 8, stage + 12)
        ref = F.conv_transpose1d(x.t()[None].double(), w.double(), b.double(), stride=s, padding=p)[0].t().float()
        assert ref.shape == (s * L, cout)
        out = torch.full((s * L, cout), float("nan"), device="cuda")
        gpu_ctx.op_conv_transpose1d(_bits(x), _bits(w), b.cuda(), s, p, out_f32=out)
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), ref), L


@pytest.mark.parametrize("width", [16, 32, 64])
@pytest.mark.parametrize("ksize", [3, 1])
def test_conv2d_causal_integer_exact(gpu_ctx, width, ksize):
    """Bit-equal including the first rows, where causality shows: all of the height padding is on top."""
    import torch
    import torch.nn.functional as F

    for H in (1, 2, 7):
        for cin, cout in ((32, 64), (128, 128), (64, 2)):
            seed = width + H * 3 + cin
            x = _ints(torch, (H, width, cin), -3, 3, seed)
            w = _ints(torch, (cout, cin, ksize, ksize), -2, 2, seed + 1)
            b = _ints(torch, (cout,), -8, 8, seed + 2)
            pad = ksize - 1
            xp = F.pad(x.permute(2, 0, 1)[None].double(), (pad // 2, pad - pad // 2, pad, 0))
            ref = F.conv2d(xp, w.double(), b.double())[0].permute(1, 2, 0).float()
            out = torch.full((H, width, cout), float("nan"), device="cuda")
            gpu_ctx.op_conv2d_causal(_bits(x), _bits(w.permute(0, 2, 3, 1).reshape(cout, ksize * ksize, cin)), b.cuda(), ksize=ksize,
                                     out_f32=out)
            torch.cuda.synchronize()
            assert torch.equal(out.cpu(), ref), (H, cin, cout)
            # the same through the transposed store the models' last convolutions use
            out_t = torch.full((cout, H * width), float("nan"), device="cuda")
            gpu_ctx.op_conv2d_causal(_bits(x), _bits(w.permute(0, 2, 3, 1).reshape(cout, ksize * ksize, cin)), b.cuda(), ksize=ksize,
                                     transposed=True, out_f32=out_t)
            torch.cuda.synchronize()
            assert torch.equal(out_t.cpu(), ref.reshape(H * width, cout).t())


@pytest.mark.parametrize("cout", [64, 2])
def test_fused_epilogues_match_unfused(gpu_ctx, cout):
    """bias / f32 residual / LeakyReLU-to-bf16 / tanh / transposed store, each against the plain launch followed by torch."""
    import torch

    g = torch.Generator(device="cpu")
    g.manual_seed(5 + cout)
    L, cin, k = 301, 64, 7
    x = torch.randn((L, cin), generator=g).to(torch.bfloat16)
    w = (torch.randn((cout, k, cin), generator=g) * 0.05).to(torch.bfloat16)
    b = torch.randn((cout,), generator=g)
    resid = torch.randn((L, cout), generator=g).cuda()
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    nobias = torch.empty((L, cout), device="cuda")
    plain = torch.empty((L, cout), device="cuda")
    gpu_ctx.op_conv1d(xd, wd, None, out_f32=nobias)
    gpu_ctx.op_conv1d(xd, wd, bd, out_f32=plain)
    assert torch.equal(plain, nobias + bd)
    for slope in (0.1, 0.01):
        fused = torch.empty((L, cout), device="cuda")
        act = torch.zeros((L, cout), device="cuda", dtype=torch.bfloat16)
        gpu_ctx.op_conv1d(xd, wd, bd, resid=resid, out_f32=fused, bf16_act=1, slope=slope, out_bf16=act)
        want = plain + resid
        assert torch.equal(fused, want)
        assert torch.equal(act, torch.where(want >= 0, want, want * np.float32(slope)).to(torch.bfloat16))
    only_bf16 = torch.zeros((L, cout), device="cuda", dtype=torch.bfloat16)
    gpu_ctx.op_conv1d(xd, wd, bd, bf16_act=0, out_bf16=only_bf16)
    assert torch.equal(only_bf16, plain.to(torch.bfloat16))
    th = torch.empty((cout, L), device="cuda")
    gpu_ctx.op_conv1d(xd, wd, bd, f32_act=2, transposed=True, out_f32=th)
    torch.cuda.synchronize()
    assert float((th - torch.tanh(plain).t()).abs().max()) <= 2e-6
    assert float(th.abs().max()) <= 1.0


def test_unsupported_shapes_throw(ltx, gpu_ctx):
    """Shapes the launchers do not take raise invalidConfiguration before anything is launched."""
    import torch

    def raises(fn):
        with pytest.raises(ltx.LTXError) as e:
            fn()
        assert e.value.case == "invalidConfiguration", e.value

    bf = torch.bfloat16
    out = torch.zeros((16, 32), device="cuda")
    x32 = torch.zeros((16, 32), device="cuda", dtype=bf)
    w3 = torch.zeros((32, 3, 32), device="cuda", dtype=bf)
    raises(lambda: gpu_ctx.op_conv1d(torch.zeros((16, 48), device="cuda", dtype=bf), torch.zeros((32, 3, 48), device="cuda", dtype=bf), None,
                                     out_f32=out))                                             # Cin not a multiple of 32
    raises(lambda: gpu_ctx.op_conv1d(x32, w3, None, tile=16, out_f32=out))                      # no such instance
    raises(lambda: gpu_ctx.op_conv1d(x32, w3, None))                                            # no output
    raises(lambda: gpu_ctx.op_conv1d(x32, torch.zeros((32, 4, 32), device="cuda", dtype=bf), None, out_f32=out))  # even kernel
    raises(lambda: gpu_ctx.op_conv1d(x32, torch.zeros((32, 11, 32), device="cuda", dtype=bf), None, dilation=7, out_f32=out))  # past the halo
    raises(lambda: gpu_ctx.op_conv1d(x32, w3, None, f32_act=1, out_f32=out))                    # LeakyReLU is a bf16-side activation
    raises(lambda: gpu_ctx.op_conv_transpose1d(x32, torch.zeros((32, 32, 4), device="cuda", dtype=bf), None, 2, 0, out_f32=out))  # padding
    raises(lambda: gpu_ctx.op_conv2d_causal(torch.zeros((2, 8, 32), device="cuda", dtype=bf),
                                            torch.zeros((32, 4, 32), device="cuda", dtype=bf), None, ksize=2, out_f32=out))
    assert float(out.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------
# model parity
# ---------------------------------------------------------------------------------------------------------------
def _metrics(got, ref):
    import torch

    g, r = got.double().flatten().cpu(), ref.double().flatten().cpu()
    rel = float(torch.linalg.norm(g - r) / torch.linalg.norm(r))
    cos = float(torch.dot(g, r) / (torch.linalg.norm(g) * torch.linalg.norm(r)))
    return rel, cos


@pytest.fixture(scope="session", params=["narrow", "full"])
def audio_models(request, tmp_path_factory):
    """One set of weight files and one f32 reference per size and T for the whole session (the reference runs on the GPU through
    torch's native convolutions, f32 end to end)."""
    import torch
    from safetensors.torch import save_file

    import audio_ref as R

    base, hidden = (32, 128) if request.param == "narrow" else (128, 1024)
    wv, wg = R.build_audio_vae_weights(base), R.build_vocoder_weights(hidden)
    d = tmp_path_factory.mktemp("audio_" + request.param)
    pv, pg = str(d / "audio_vae.safetensors"), str(d / "vocoder.safetensors")
    save_file(wv, pv)
    save_file(wg, pg)
    wv_d, wg_d = R.to(wv, "cuda"), R.to(wg, "cuda")
    refs = {}
    with torch.no_grad(), torch.backends.cudnn.flags(enabled=False):
        for T in (1, 5, 126):
            lat = torch.randn((8, T, 16), generator=R._gen(100 + T))
            stages, pre = [], []
            mel = R.audio_vae_decode(wv_d, lat.cuda(), stages)
            wav = R.vocoder_forward(wg_d, mel, stages, pre)
            # the conditions of audio_ref hold for THIS model and input too: the comparisons below are not vacuous. (Not asked of T = 1:
            # one latent frame between zero padding is a handful of samples per stage, no population to take a std of.)
            if T > 1:
                for s in stages + [mel]:
                    assert 0.1 <= float(s.std()) <= 10.0, (request.param, T, float(s.std()))
                assert 0.1 <= float(pre[0].std()) <= 1.0, (request.param, T, float(pre[0].std()))
            assert float((pre[0].abs() > 3).float().mean()) < 0.01
            refs[T] = (lat, mel.contiguous(), wav.contiguous())
    torch.cuda.synchronize()
    return {"name": request.param, "vae": pv, "voc": pg, "refs": refs}


@pytest.mark.parametrize("T", [5, 126])
def test_audio_model_parity(gpu_ctx, audio_models, T):
    import torch

    gpu_ctx.audio_vae_load(audio_models["vae"])
    gpu_ctx.vocoder_load(audio_models["voc"])
    lat, ref_mel, ref_wav = audio_models["refs"][T]
    Tm = max(4 * T - 3, 1)
    lat_d = lat.cuda()
    mel = torch.empty((2, Tm, 64), device="cuda")
    gpu_ctx.audio_vae_decode_dev(lat_d, mel)
    wav_from_ref_mel = torch.empty((2, 240 * Tm), device="cuda")
    gpu_ctx.vocoder_forward_dev(ref_mel, wav_from_ref_mel)
    wav = torch.empty((2, 240 * Tm), device="cuda")
    gpu_ctx.audio_decode_dev(lat_d, wav)
    torch.cuda.synchronize()
    if T == 126:
        assert tuple(wav.shape) == (2, 120240)
    for what, got, ref in (("mel", mel, ref_mel), ("vocoder", wav_from_ref_mel, ref_wav), ("chained", wav, ref_wav)):
        assert bool(torch.isfinite(got).all())
        rel, cos = _metrics(got, ref)
        print(f"audio parity {audio_models['name']} T={T} {what}: rel-L2 {rel:.3e} cosine {cos:.6f}")
        assert rel <= REL_L2 and cos >= COSINE, (what, rel, cos)
    # two runs agree bit for bit; the host-pointer entry points agree with the device ones bit for bit
    wav2 = torch.empty_like(wav)
    gpu_ctx.audio_decode_dev(lat_d, wav2)
    torch.cuda.synchronize()
    assert torch.equal(wav, wav2)
    assert np.array_equal(gpu_ctx.audio_decode(lat.numpy()), wav.cpu().numpy())
    assert np.array_equal(gpu_ctx.audio_vae_decode(lat.numpy()), mel.cpu().numpy())
    assert np.array_equal(gpu_ctx.vocoder_forward(ref_mel.cpu().numpy()), wav_from_ref_mel.cpu().numpy())


def test_audio_single_frame(gpu_ctx, audio_models):
    """T = 1 decodes: one mel frame, 240 samples."""
    gpu_ctx.audio_vae_load(audio_models["vae"])
    gpu_ctx.vocoder_load(audio_models["voc"])
    lat, ref_mel, ref_wav = audio_models["refs"][1]
    mel = gpu_ctx.audio_vae_decode(lat.numpy())
    wav = gpu_ctx.audio_decode(lat.numpy())
    assert mel.shape == (2, 1, 64) and wav.shape == (2, 240)
    import torch

    for got, ref in ((mel, ref_mel), (wav, ref_wav)):
        rel, cos = _metrics(torch.from_numpy(got), ref)
        print(f"audio parity {audio_models['name']} T=1: rel-L2 {rel:.3e} cosine {cos:.6f}")
        assert rel <= REL_L2 and cos >= COSINE, (rel, cos)


def test_audio_synthetic_models_run(gpu_ctx):
    """The on-library synthetic initialisers give a finite, unsaturated waveform (what the CLI's --synthetic and the bench tool use)."""
    gpu_ctx.audio_vae_init_synthetic(32, 1)
    gpu_ctx.vocoder_init_synthetic(128, 2)
    rng = np.random.default_rng(0)
    wav = gpu_ctx.audio_decode(rng.standard_normal((8, 9, 16)).astype(np.float32))
    assert wav.shape == (2, 240 * 33) and np.isfinite(wav).all()
    assert 0.01 < float(wav.std()) < 0.9 and float(np.abs(wav).max()) < 1.0
    gpu_ctx.audio_vae_unload()
    gpu_ctx.vocoder_unload()
