"""Image-to-video in the joint video + audio denoise loop (csrc/dual_denoise.cpp, reference LTXPipeline.swift:1261-1399) through
ltx_dual_denoise_dev and ltx_dual_denoise with cond_latent / image_cond_noise_scale / cond_noise, on the narrow model of
tests/test_dual_denoise_gpu.py (4 x 128 / 4 x 64, L 2, caption 256, (F, H, W) = (2, 6, 8), T_a 26, S 70, boosted).

Exact: the loop against the same loop composed here, in the REFERENCE's order (frame 0 re-noised at the start of a step), from the
library's own uncached groups forward and the numpy float32 step of tests/helpers/dual_i2v_ref.py - final latents bit-equal in the
caller's layouts, although the library re-noises frame 0 inside the step launch of the step before; frame 0 of the result; text-to-video
through the grown struct against the old struct_size; host pointers against device pointers; the refusal.

Parity with the f32 reference loop at the setting tests/test_dual_i2v_host.py shows every piece visible at (distilled, 3 steps ending at
sigma 0, image_cond_noise_scale 0.5): rel-L2 of each final latent <= min(2 x the CPU rounding-point replay's, 3e-2)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import dual_denoise_ref as dd  # noqa: E402
import dual_i2v_ref as iv  # noqa: E402
import dual_model_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
NARROW = dict(Hv=4, Ha=4, F=2, H=6, W=8, T_a=26, S=70, caption_channels=256)
L_NARROW = 2
DISTILLED = [1.0, 0.725, 0.25, 0.0]   # 3 steps ending at sigma 0
CFG_SIGMAS = [1.0, 0.6, 0.25]         # 2 steps
NOISE_SCALE = 0.5                     # the setting of tests/test_dual_i2v_host.py


def dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda().to(dtype)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def run_dev(ctx, case, sigmas, cond=None, noise=None, scale=0.0, **kw):
    """ltx_dual_denoise_dev on fresh device copies; returns (video latent [C][F][H][W], audio latent [8][T_a][16])."""
    v, a = dev(case["video_latent"][None]), dev(case["audio_latent"][None])
    ctx.dual_denoise_dev(v, a, sigmas, dev(case["video_context"], torch.bfloat16), case["F"], case["H"], case["W"],
                         audio_context=None if case["audio_context"] is None else dev(case["audio_context"], torch.bfloat16),
                         mask=None if case["mask"] is None else dev(case["mask"], torch.int32),
                         cond_latent=None if cond is None else dev(cond[None]), image_cond_noise_scale=scale,
                         cond_noise=None if noise is None else dev(noise), **kw)
    torch.cuda.synchronize()
    return v[0].cpu().numpy(), a[0].cpu().numpy()


def gpu_forward(ctx):
    """The library's uncached groups forward as dual_i2v_ref.loop's forward, in the loop's own group layout ({sigma, 0}, frame 0 in group 1)."""
    def fwd(inp):
        B, F, H, W = inp["B"], inp["F"], inp["H"], inp["W"]
        Tv = F * H * W
        vv, va = torch.empty((B, Tv, 128), device="cuda"), torch.empty((B, inp["T_a"], 128), device="cuda")
        ts = np.zeros((B, 2), np.float32)
        ts[:, 0] = inp["sigma"]
        rm = np.zeros((B, Tv), np.int32)
        rm[:, :H * W] = 1
        rm += 2 * np.arange(B, dtype=np.int32)[:, None]
        assert np.array_equal(ts.reshape(-1)[rm], inp["video_token_timesteps"])
        mv = None if inp["null_mask"] else dev(inp["video_mask"], torch.int32)
        ma = None if inp["null_mask"] else dev(inp["audio_mask"], torch.int32)
        ctx.dual_model_forward_groups_dev(dev(inp["video_latent"], torch.bfloat16), dev(inp["audio_latent"], torch.bfloat16),
                                          dev(inp["video_context"], torch.bfloat16), dev(inp["audio_context"], torch.bfloat16), dev(ts),
                                          dev(inp["audio_timesteps"]), vv, va, F, H, W, 2, dev(rm.reshape(-1), torch.int32), video_mask=mv, audio_mask=ma)
        torch.cuda.synchronize()
        return vv.cpu().numpy(), va.cpu().numpy()
    return fwd


@pytest.fixture(scope="module")
def model(gpu_ctx, ltx, tmp_path_factory):
    from safetensors.numpy import save_file

    cfg = ltx.default_dual_model_config(num_layers=L_NARROW, video_heads=NARROW["Hv"], audio_heads=NARROW["Ha"],
                                        caption_channels=NARROW["caption_channels"])
    path = tmp_path_factory.mktemp("dual_i2v_denoise") / "boosted.safetensors"
    gpu_ctx.dual_model_init_synthetic(cfg, seed=81)
    shapes = ref.param_shapes(L_NARROW, NARROW["Hv"], NARROW["Ha"], caption_channels=NARROW["caption_channels"])
    w = ref.boost({k: gpu_ctx.dual_model_export_param(k).reshape(s) for k, s in shapes.items()}, NARROW["Hv"], NARROW["Ha"])
    save_file({ref.checkpoint_spelling(k): np.ascontiguousarray(v, dtype=np.float32) for k, v in w.items()}, str(path))
    gpu_ctx.dual_model_load(path, cfg)
    yield {"w": w}
    gpu_ctx.dual_model_unload()


@pytest.fixture(scope="module")
def cases():
    """Inputs, shared and left unchanged: distilled (the audio context defaults to the video context) and CFG (an audio context of its
    own), both masked; the image latent and four re-noising draws."""
    c = {"distilled": dd.make_case(cfg=False, seed=1, **NARROW), "cfg": dd.make_case(cfg=True, seed=2, audio_context=True, **NARROW)}
    c["cond"], c["noise"] = iv.make_cond(c["distilled"], 3)
    return c


SETTINGS = {"distilled": ("distilled", DISTILLED, {}, False), "distilled_noise": ("distilled", DISTILLED, {}, True),
            "cfg": ("cfg", CFG_SIGMAS, {"cfg_scale": 3.0}, False), "cfg_noise": ("cfg", CFG_SIGMAS, {"cfg_scale": 3.0}, True)}


@pytest.fixture(scope="module")
def composed(gpu_ctx, model, cases):
    """The image-to-video loop composed from the uncached groups forward and the numpy step, once per setting."""
    fwd = gpu_forward(gpu_ctx)
    out = {}
    for name, (case, sigmas, kw, noised) in SETTINGS.items():
        noise = cases["noise"][:len(sigmas) - 1] if noised else None
        out[name] = iv.loop(fwd, cases[case], sigmas, cases["cond"], noise=noise, noise_scale=NOISE_SCALE if noised else 0.0, **kw)
    return out


def run_setting(ctx, cases, name, **extra):
    case, sigmas, kw, noised = SETTINGS[name]
    noise = cases["noise"][:len(sigmas) - 1] if noised else None
    return run_dev(ctx, cases[case], sigmas, cases["cond"], noise, NOISE_SCALE if noised else 0.0, **dict(kw, **extra))


@pytest.mark.parametrize("name", list(SETTINGS))
def test_the_loop_equals_the_composed_loop_bit_for_bit(gpu_ctx, cases, composed, name):
    """Distilled, 3 steps ending at sigma 0, and CFG 3.0, 2 steps; each without and with re-noising (scale 0.5)."""
    gv, ga = run_setting(gpu_ctx, cases, name)
    wv, wa = composed[name]
    assert gv.shape == (128, 2, 6, 8) and ga.shape == (8, 26, 16) and np.isfinite(gv).all() and np.isfinite(ga).all()
    assert same_bits(gv, wv), float(np.abs(gv - wv).max())
    assert same_bits(ga, wa), float(np.abs(ga - wa).max())
    plain = run_setting(gpu_ctx, cases, name, text_cache=0)  # the text cache changes no bit
    assert same_bits(plain[0], gv) and same_bits(plain[1], ga)


@pytest.mark.parametrize("name", list(SETTINGS))
def test_frame_zero_of_the_result(gpu_ctx, cases, composed, name):
    """Without noise frame 0 is the image latent, bit for bit; with it, cond + (scale * noise[last]) * sigma_last^2 with the LAST STEP's
    sigma and draw. The other frames moved."""
    case, sigmas, _, noised = SETTINGS[name]
    gv, _ = run_setting(gpu_ctx, cases, name)
    if noised:
        s = np.float32(sigmas[-2])
        want = iv.noised(cases["cond"], cases["noise"][len(sigmas) - 2], NOISE_SCALE, np.float32(s * s))
        assert not same_bits(want, cases["cond"])
    else:
        want = cases["cond"]
    assert same_bits(gv[:, 0:1], want)
    assert not same_bits(gv[:, 1:], cases[case]["video_latent"][:, 1:])


def test_the_conditioning_reaches_the_audio_latent(gpu_ctx, cases, composed):
    """Text-to-video on the same inputs ends at another audio latent: frame 0 reaches the audio stream through v2a."""
    c = cases["distilled"]
    tv, ta = run_dev(gpu_ctx, c, DISTILLED)
    iv_, ia = composed["distilled"]
    moved = dd.rel_l2(ia, ta)
    print(f"audio latent, image-to-video against text-to-video: rel-L2 {moved:.3e}")
    assert moved > 1e-2 and not same_bits(tv[:, 1:], iv_[:, 1:])


def test_text_to_video_through_the_new_struct_equals_the_old_struct_size(gpu_ctx, ltx, cases):
    """cond_latent NULL is text-to-video, launch for launch: the same bits as a call whose struct_size ends at step_stats."""
    from importlib import import_module

    lib_mod = import_module("ltx-video-swift-mlx_amd._lib")
    old = lib_mod.DualDenoiseArgs.step_stats.offset + ctypes.sizeof(ctypes.c_void_p)
    assert old < ctypes.sizeof(lib_mod.DualDenoiseArgs)
    for case, sigmas, kw in (("distilled", DISTILLED, {}), ("cfg", CFG_SIGMAS, {"cfg_scale": 3.0})):
        new = run_dev(gpu_ctx, cases[case], sigmas, **kw)
        short = run_dev(gpu_ctx, cases[case], sigmas, struct_size=old, **kw)
        assert same_bits(new[0], short[0]) and same_bits(new[1], short[1])
    # a short struct does not read the fields it does not cover: cond_latent is ignored, not an error
    short = run_dev(gpu_ctx, cases["distilled"], DISTILLED, cases["cond"], struct_size=old)
    plain = run_dev(gpu_ctx, cases["distilled"], DISTILLED)
    assert same_bits(short[0], plain[0])


@pytest.mark.parametrize("name", ["distilled_noise", "cfg"])
def test_host_entry_equals_device_entry(gpu_ctx, ltx, cases, composed, name):
    case, sigmas, kw, noised = SETTINGS[name]
    c = cases[case]
    hv, ha = gpu_ctx.dual_denoise(c["video_latent"][None], c["audio_latent"][None], sigmas, ltx.f32_to_bf16_bits(c["video_context"]),
                                  c["F"], c["H"], c["W"],
                                  audio_context_bf16=None if c["audio_context"] is None else ltx.f32_to_bf16_bits(c["audio_context"]),
                                  mask=c["mask"], cond_latent=cases["cond"][None], image_cond_noise_scale=NOISE_SCALE if noised else 0.0,
                                  cond_noise=cases["noise"][:len(sigmas) - 1] if noised else None, **kw)
    assert same_bits(hv[0], composed[name][0]) and same_bits(ha[0], composed[name][1])


def test_one_latent_frame_with_cond_latent_is_refused(gpu_ctx, ltx, cases):
    one = dict(NARROW, F=1)
    c = dd.make_case(cfg=False, seed=4, **one)
    v, a = dev(c["video_latent"][None]), dev(c["audio_latent"][None])
    v0, a0 = v.clone(), a.clone()
    cond = dev(cases["cond"][None])
    with pytest.raises(ltx.LTXError, match="two latent frames") as e:
        gpu_ctx.dual_denoise_dev(v, a, DISTILLED, dev(c["video_context"], torch.bfloat16), 1, 6, 8, mask=dev(c["mask"], torch.int32), cond_latent=cond)
    assert e.value.case == "invalidConfiguration"
    torch.cuda.synchronize()
    assert torch.equal(v, v0) and torch.equal(a, a0), "a refused call wrote"
    hv, ha = c["video_latent"][None].copy(), c["audio_latent"][None].copy()
    with pytest.raises(ltx.LTXError, match="two latent frames"):  # the host entry refuses before it stages
        gpu_ctx.dual_denoise(hv, ha, DISTILLED, ltx.f32_to_bf16_bits(c["video_context"]), 1, 6, 8, mask=c["mask"], cond_latent=cases["cond"][None])
    gpu_ctx.dual_denoise_dev(v, a, DISTILLED, dev(c["video_context"], torch.bfloat16), 1, 6, 8, mask=dev(c["mask"], torch.int32))  # text-to-video may
    torch.cuda.synchronize()
    assert not torch.equal(v, v0)


def test_parity_with_the_f32_reference_loop(gpu_ctx, model, cases):
    """Distilled, 3 steps ending at sigma 0, re-noising at scale 0.5, masked, the audio context defaulting to the video context. MI355X:
    video 5.94e-4 (replay 5.88e-4, bound 1.18e-3), audio 5.08e-4 (replay 5.03e-4, bound 1.01e-3); DESIGN.md section 6f."""
    c, noise = cases["distilled"], cases["noise"]
    kw = dict(noise=noise, noise_scale=NOISE_SCALE)
    fv, fa = iv.loop(iv.ref_forward(model["w"], L_NARROW), c, DISTILLED, cases["cond"], **kw)
    rv, ra = iv.loop(iv.ref_forward(model["w"], L_NARROW, replay=True), c, DISTILLED, cases["cond"], **kw)
    gv, ga = run_dev(gpu_ctx, c, DISTILLED, cases["cond"], noise, NOISE_SCALE)
    for name, g, f, r in (("video", gv, fv, rv), ("audio", ga, fa, ra)):
        rel, rep = dd.rel_l2(g, f), dd.rel_l2(r, f)
        bound = dd.update_bound(rep)
        print(f"{name} latent after 3 image-to-video steps: rel-L2 GPU {rel:.3e}; CPU replay {rep:.3e}, bound {bound:.3e}")
        assert np.isfinite(g).all()
        assert rel <= bound, (name, rel, bound)
