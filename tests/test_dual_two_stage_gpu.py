"""The two-stage video + audio path (csrc/dual_two_stage.cpp, reference LTXPipeline.swift:1613-1817) through ltx_dual_two_stage_dev and
ltx_dual_two_stage, on the narrow model of the dual tests (4 x 128 / 4 x 64, L 2, caption 256, T_a 26, S 70, a third of the keys masked,
boosted): stage 1 at (F, H, W) = (2, 3, 4), stage 2 at (2, 6, 8), the synthetic upscaler (mid 64) and VAE statistics of
tests/test_two_stage_gpu.py, sigmas1 = [1, 0.725, 0.25, 0], sigmas2 = ltx_stage2_sigmas.

Exact: (a) the final latents against the composition of public pieces - ltx_dual_denoise_dev, ltx_upscale_latent_dev,
ltx_op_dual_restage and a stage-2 loop of the library's uncached forward with the numpy float32 step, form 1 on BOTH streams -
text-to-video, image-to-video, image-to-video with re-noising; (b) the same composition with the video stepped by form 0 in stage 2 is
NOT equal: the only guard for the form (tests/test_dual_two_stage_host.py shows the two forms a last place apart); (c) one text-cache
fill per call; (d) stage1_out against ltx_dual_denoise_dev; (e) host entry against device entry; (f) frame 0; (g) the progress sequence;
(h) the refusals. (i) Parity with the f32 reference path: rel-L2 of each final latent <= min(2 x (CPU rounding-point replay + the
upscaler's own error as it enters stage 2), 5e-2)."""
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
import dual_two_stage_ref as ts  # noqa: E402
import ltx_oracle as oracle  # noqa: E402

pytestmark = pytest.mark.gpu
N = ts.NARROW
F, H, W = N["F"], N["H"], N["W"]
SETTINGS = {"t2v": dict(i2v=False, renoise=False), "i2v": dict(i2v=True, renoise=False), "i2v_noise": dict(i2v=True, renoise=True)}


def dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda().to(dtype)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.fixture(scope="module")
def env(ltx, tmp_path_factory):
    """A context of its own with the three models the path needs: the boosted narrow dual model, the synthetic upscaler, VAE statistics."""
    from safetensors.numpy import save_file

    d = tmp_path_factory.mktemp("dual_two_stage")
    ctx = ltx.Context(0)
    cfg = ltx.default_dual_model_config(num_layers=ts.L_NARROW, video_heads=N["Hv"], audio_heads=N["Ha"], caption_channels=N["caption_channels"])
    ctx.dual_model_init_synthetic(cfg, seed=81)
    shapes = ref.param_shapes(ts.L_NARROW, N["Hv"], N["Ha"], caption_channels=N["caption_channels"])
    w = ref.boost({k: ctx.dual_model_export_param(k).reshape(s) for k, s in shapes.items()}, N["Hv"], N["Ha"])
    save_file({ref.checkpoint_spelling(k): np.ascontiguousarray(v, dtype=np.float32) for k, v in w.items()}, str(d / "boosted.safetensors"))
    ctx.dual_model_load(d / "boosted.safetensors", cfg)
    wu = oracle.synth_upscaler_weights(mid=ts.UPSCALER_MID, seed=ts.UPSCALER_SEED)
    save_file({k: np.ascontiguousarray(v, dtype=np.float32) for k, v in wu.items()}, str(d / "up.safetensors"))
    ctx.upscaler_load(d / "up.safetensors")
    mean, std = ts.vae_stats()
    save_file({"latents_mean": mean, "latents_std": std}, str(d / "vae.safetensors"))
    ctx.vae_load(d / "vae.safetensors")
    case = ts.make_case(steps1=len(ts.SIGMAS1) - 1, steps2=len(ts.SIGMAS2) - 1, seed=1, **N)
    yield {"ctx": ctx, "w": w, "wu": wu, "mean": mean, "std": std, "case": case, "cfg": cfg, "dir": d}
    ctx.close()


def call_args(case, i2v, renoise):
    """Fresh device tensors of one call, by keyword of Context.dual_two_stage_dev."""
    a = dict(video_latent_in=dev(case["video_latent"][None]), video_latent_out=torch.full((1, 128, F, 2 * H, 2 * W), 9.0, device="cuda"),
             audio_latent=dev(case["audio_latent"][None]), sigmas1=ts.SIGMAS1, video_noise2=dev(case["video_noise2"][None]),
             audio_noise2=dev(case["audio_noise2"]), video_context=dev(case["video_context"], torch.bfloat16), F=F, H=H, W=W,
             mask=dev(case["mask"], torch.int32), stage1_out=torch.zeros((1, 128, F, H, W), device="cuda"))
    if i2v:
        a.update(cond_latent1=dev(case["cond1"][None]), cond_latent2=dev(case["cond2"][None]))
    if renoise:
        a.update(image_cond_noise_scale=ts.NOISE_SCALE, cond_noise1=dev(case["cnoise1"]), cond_noise2=dev(case["cnoise2"]))
    return a


def run_dev(ctx, case, i2v=False, renoise=False, **kw):
    a = call_args(case, i2v, renoise)
    a.update(kw)
    ctx.dual_two_stage_dev(**a)
    torch.cuda.synchronize()
    return {"video": a["video_latent_out"][0].cpu().numpy(), "audio": a["audio_latent"][0].cpu().numpy(), "stage1": a["stage1_out"][0].cpu().numpy()}


def gpu_forward(ctx):
    """The library's uncached forward as dual_two_stage_ref.stage's forward: plain for text-to-video, two timestep groups ({sigma, 0},
    frame 0 in group 1) for image-to-video."""
    def fwd(inp):
        Fi, Hi, Wi = inp["F"], inp["H"], inp["W"]
        Tv = Fi * Hi * Wi
        vv, va = torch.empty((1, Tv, 128), device="cuda"), torch.empty((1, inp["T_a"], 128), device="cuda")
        args = [dev(inp["video_latent"], torch.bfloat16), dev(inp["audio_latent"], torch.bfloat16), dev(inp["video_context"], torch.bfloat16),
                dev(inp["audio_context"], torch.bfloat16)]
        masks = dict(video_mask=dev(inp["video_mask"], torch.int32), audio_mask=dev(inp["audio_mask"], torch.int32))
        if inp["i2v"]:
            tsv = np.asarray([[inp["sigma"], 0.0]], np.float32)
            rm = np.zeros(Tv, np.int32)
            rm[:Hi * Wi] = 1
            assert np.array_equal(tsv.reshape(-1)[rm][None], inp["video_token_timesteps"])
            ctx.dual_model_forward_groups_dev(*args, dev(tsv), dev(inp["audio_timesteps"]), vv, va, Fi, Hi, Wi, 2, dev(rm, torch.int32), **masks)
        else:
            ctx.dual_model_forward_dev(*args, dev(inp["video_timesteps"]), dev(inp["audio_timesteps"]), vv, va, Fi, Hi, Wi, **masks)
        torch.cuda.synchronize()
        return vv.cpu().numpy(), va.cpu().numpy()
    return fwd


def compose(ctx, case, i2v, renoise, video_form2=1):
    """The path from public pieces: ltx_dual_denoise_dev, ltx_upscale_latent_dev, ltx_op_dual_restage, then stage 2 as the numpy loop
    around the library's uncached forward."""
    C, T1, T2, HW2 = 128, F * H * W, 4 * F * H * W, 4 * H * W
    v1, a1 = dev(case["video_latent"][None]), dev(case["audio_latent"][None])
    ctx.dual_denoise_dev(v1, a1, ts.SIGMAS1, dev(case["video_context"], torch.bfloat16), F, H, W, mask=dev(case["mask"], torch.int32),
                         cond_latent=dev(case["cond1"][None]) if i2v else None, image_cond_noise_scale=ts.NOISE_SCALE if renoise else 0.0,
                         cond_noise=dev(case["cnoise1"]) if renoise else None)
    up = torch.empty((1, C, F, 2 * H, 2 * W), device="cuda")
    ctx.upscale_latent_dev(v1, up)
    torch.cuda.synchronize()
    s = np.float32(ts.SIGMAS2[0])
    lat, tok = torch.empty((T2, C), device="cuda"), torch.empty((T2, C), device="cuda", dtype=torch.bfloat16)
    xa, atok = dev(dd.pack_audio(a1[0].cpu().numpy())), torch.empty((N["T_a"], C), device="cuda", dtype=torch.bfloat16)
    vj = dict(x=up[0].reshape(C, T2), ref=v1[0].reshape(C, T1), latent=lat, tokens=tok, noise=dev(case["video_noise2"].reshape(C, T2)), noise_scale=float(s))
    if i2v:
        vj["cond"] = dev(case["cond2"].reshape(C, HW2))
    if renoise:
        vj.update(cond_noise=dev(case["cnoise2"][0].reshape(C, HW2)), cond_scale=ts.NOISE_SCALE, cond_sigma2=float(np.float32(s * s)))
    ctx.op_dual_restage(vj, dict(latent=xa, tokens=atok, noise=dev(case["audio_noise2"]), noise_scale=float(s)))
    torch.cuda.synchronize()
    dims = {k: case[k] for k in ("Hv", "Ha", "F", "T_a", "S")}
    dims["H"], dims["W"] = 2 * H, 2 * W
    z = dd.unpack_video(lat.cpu().numpy(), F, 2 * H, 2 * W)
    v, a = ts.stage(gpu_forward(ctx), dims, z, xa.cpu().numpy(), case, ts.SIGMAS2, video_form2, case["cond2"] if i2v else None,
                    case["cnoise2"] if renoise else None, ts.NOISE_SCALE if renoise else 0.0)
    return {"video": v, "audio": dd.unpack_audio(a), "stage1": v1[0].cpu().numpy(), "z0": z}


@pytest.fixture(scope="module")
def results(env):
    """The device entry and the composition, once per setting; shared and left unchanged."""
    out = {}
    for name, kw in SETTINGS.items():
        before = env["ctx"].dual_model_text_cache_info()["builds"]
        got = run_dev(env["ctx"], env["case"], **kw)
        fills = env["ctx"].dual_model_text_cache_info()["builds"] - before
        out[name] = {"got": got, "fills": fills, "want": compose(env["ctx"], env["case"], **kw)}
    return out


@pytest.mark.parametrize("name", list(SETTINGS))
def test_a_the_path_equals_its_composition_from_public_pieces(results, name):
    got, want = results[name]["got"], results[name]["want"]
    assert got["video"].shape == (128, F, 2 * H, 2 * W) and got["audio"].shape == (8, N["T_a"], 16)
    assert np.isfinite(got["video"]).all() and np.isfinite(got["audio"]).all()
    assert same_bits(got["video"], want["video"]), float(np.abs(got["video"] - want["video"]).max())
    assert same_bits(got["audio"], want["audio"]), float(np.abs(got["audio"] - want["audio"]).max())


@pytest.mark.parametrize("name", ["t2v", "i2v_noise"])
def test_b_stage_two_steps_the_video_by_the_plain_form(env, results, name):
    """Form 0 for the video in stage 2 - what reusing ltx_dual_denoise for stage 2 would do - gives other bits."""
    other = compose(env["ctx"], env["case"], video_form2=0, **SETTINGS[name])
    got = results[name]["got"]
    assert same_bits(other["z0"], results[name]["want"]["z0"])  # the same start
    assert not same_bits(other["video"], got["video"])
    print(f"{name}: form 0 against the library's stage 2: {100 * np.mean(other['video'] != got['video']):.1f} % of the f32 results differ, "
          f"rel-L2 {dd.rel_l2(other['video'], got['video']):.3e}")


@pytest.mark.parametrize("name", list(SETTINGS))
def test_c_one_text_cache_fill_per_call(results, name):
    assert results[name]["fills"] == 1


@pytest.mark.parametrize("name", list(SETTINGS))
def test_d_stage1_out_is_the_joint_loop(results, name):
    assert same_bits(results[name]["got"]["stage1"], results[name]["want"]["stage1"])


@pytest.mark.parametrize("name", ["t2v", "i2v_noise"])
def test_e_host_entry_equals_device_entry(env, ltx, results, name):
    c, kw = env["case"], SETTINGS[name]
    extra = {}
    if kw["i2v"]:
        extra.update(cond_latent1=c["cond1"][None], cond_latent2=c["cond2"][None])
    if kw["renoise"]:
        extra.update(image_cond_noise_scale=ts.NOISE_SCALE, cond_noise1=c["cnoise1"], cond_noise2=c["cnoise2"])
    audio_in = c["audio_latent"][None].copy()
    v, a, s1 = env["ctx"].dual_two_stage(c["video_latent"][None], audio_in, ts.SIGMAS1, c["video_noise2"][None], c["audio_noise2"],
                                         ltx.f32_to_bf16_bits(c["video_context"]), sigmas2=ts.SIGMAS2, mask=c["mask"], stage1_out=True, **extra)
    got = results[name]["got"]
    assert same_bits(v[0], got["video"]) and same_bits(a[0], got["audio"]) and same_bits(s1[0], got["stage1"])
    assert same_bits(audio_in, c["audio_latent"][None])  # the binding works on copies


def test_f_frame_zero_of_the_result(env, results):
    c = env["case"]
    assert same_bits(results["i2v"]["got"]["video"][:, 0:1], c["cond2"])
    s = np.float32(ts.SIGMAS2[-2])
    want = iv.noised(c["cond2"], c["cnoise2"][-1], ts.NOISE_SCALE, np.float32(s * s))
    assert not same_bits(want, c["cond2"]) and same_bits(results["i2v_noise"]["got"]["video"][:, 0:1], want)
    assert same_bits(results["i2v"]["got"]["stage1"][:, 0:1], c["cond1"])
    assert not same_bits(results["t2v"]["got"]["video"][:, 1:], results["i2v"]["got"]["video"][:, 1:])


def test_g_the_progress_callback_sequence(env, results):
    """Also without stage1_out: the stage-1 latent then lives in the context's own buffer, and the result is the same."""
    seen = []
    a = call_args(env["case"], False, False)
    a.update(stage1_out=None, on_progress=lambda step, total, sigma, user: seen.append((step, total, np.float32(sigma))))
    env["ctx"].dual_two_stage_dev(**a)
    torch.cuda.synchronize()
    assert same_bits(a["video_latent_out"][0].cpu().numpy(), results["t2v"]["got"]["video"])
    assert same_bits(a["audio_latent"][0].cpu().numpy(), results["t2v"]["got"]["audio"])
    n1, n2 = len(ts.SIGMAS1) - 1, len(ts.SIGMAS2) - 1
    want = [(i, n1, np.float32(ts.SIGMAS1[i])) for i in range(n1)] + [(n1 + i, n1 + n2, np.float32(ts.SIGMAS2[i])) for i in range(n2)]
    assert seen == want


def test_h_refusals_leave_the_latents_untouched(env, ltx):
    from importlib import import_module

    ctx, c = env["ctx"], env["case"]
    lib_mod = import_module("ltx-video-swift-mlx_amd._lib")

    def refused(case_name, match=None, i2v=False, renoise=False, use=None, **kw):
        a = call_args(c, i2v, renoise)
        a.update(kw)
        keep = {k: a[k].clone() for k in ("video_latent_out", "audio_latent", "stage1_out", "video_latent_in") if a[k] is not None}
        with pytest.raises(ltx.LTXError, match=match) as e:
            (use or ctx).dual_two_stage_dev(**a)
        assert e.value.case == case_name, (kw, str(e.value))
        torch.cuda.synchronize()
        for k, t in keep.items():
            assert torch.equal(a[k], t), (k, kw)

    refused("invalidConfiguration", "struct_size", struct_size=ctypes.sizeof(lib_mod.DualTwoStageArgs) - 8)
    refused("invalidConfiguration", "null", video_noise2=None)
    refused("invalidConfiguration", "null", audio_noise2=None)
    refused("invalidConfiguration", "both resolutions", cond_latent1=dev(c["cond1"][None]))
    refused("invalidConfiguration", "both resolutions", cond_latent2=dev(c["cond2"][None]))
    refused("invalidConfiguration", "positive", sigmas1=[1.0, 0.0, 0.25, 0.0])
    refused("invalidConfiguration", "positive", sigmas2=[0.9, -0.1, 0.0])
    refused("invalidConfiguration", "at least 2", sigmas1=[1.0])
    one = ts.make_case(steps1=3, steps2=3, seed=5, **dict(N, F=1))
    a = dict(video_latent_in=dev(one["video_latent"][None]), video_latent_out=torch.zeros((1, 128, 1, 2 * H, 2 * W), device="cuda"),
             audio_latent=dev(one["audio_latent"][None]), video_noise2=dev(one["video_noise2"][None]), stage1_out=None, F=1)
    refused("invalidConfiguration", "two latent frames", i2v=True, **a)
    # the host entry refuses before it stages
    with pytest.raises(ltx.LTXError, match="both resolutions"):
        ctx.dual_two_stage(c["video_latent"][None], c["audio_latent"][None], ts.SIGMAS1, c["video_noise2"][None], c["audio_noise2"],
                           ltx.f32_to_bf16_bits(c["video_context"]), cond_latent1=c["cond1"][None])
    # a missing model: the dual model, then the upscaler, then the VAE
    bare = ltx.Context(0)
    try:
        refused("modelNotLoaded", "dual transformer", use=bare)
        bare.dual_model_init_synthetic(env["cfg"], seed=81)
        refused("modelNotLoaded", "upscaler", use=bare)
        bare.upscaler_load(env["dir"] / "up.safetensors")
        refused("modelNotLoaded", "vaeDecoder", use=bare)
    finally:
        bare.close()


def test_i_parity_with_the_f32_reference_path(env, results):
    """Image-to-video with re-noising at scale 0.5 in both stages, masked. Bound per latent: min(2 x (replay + allowance), 5e-2), where
    replay is the CPU rounding-point replay (replay=True forwards, the f32 upscaler) and allowance the upscaler's own error e_up, measured
    here on the stage-1 reference latent (<= 3e-2), times (1 - s) |y| / |z0| from the reference arrays. MI355X: e_up 6.26e-3, allowance
    6.30e-4; video 7.75e-4 (replay 5.60e-4, bound 2.38e-3), audio 5.25e-4 (replay 5.33e-4, bound 2.33e-3); DESIGN.md section 6g."""
    ctx, c = env["ctx"], env["case"]
    kw = dict(i2v=True, renoise=True, noise_scale=ts.NOISE_SCALE)
    up = lambda lat: oracle.upsample_latents(env["wu"], lat, env["mean"], env["std"])  # noqa: E731
    f = ts.two_stage(iv.ref_forward(env["w"], ts.L_NARROW), c, ts.SIGMAS1, ts.SIGMAS2, up, **kw)
    r = ts.two_stage(iv.ref_forward(env["w"], ts.L_NARROW, replay=True), c, ts.SIGMAS1, ts.SIGMAS2, up, **kw)
    e_up = dd.rel_l2(ctx.upscale_latent(f["stage1"][None]), up(f["stage1"][None]))
    print(f"upscaler on the stage-1 reference latent: rel-L2 {e_up:.3e} (bound {ts.UPSCALER_BOUND:.0e})")
    assert e_up <= ts.UPSCALER_BOUND
    got = results["i2v_noise"]["got"]
    for k in ("video", "audio"):
        rel, rep = dd.rel_l2(got[k], f[k]), dd.rel_l2(r[k], f[k])
        bound, allowance = ts.parity_bound(rep, e_up, f["y"], f["z0"], ts.SIGMAS2[0])
        print(f"{k} latent after both stages: rel-L2 GPU {rel:.3e}; CPU replay {rep:.3e}, upscaler allowance {allowance:.3e}, bound {bound:.3e}")
        assert np.isfinite(got[k]).all()
        assert rel <= bound, (k, rel, bound)
