"""A video + audio generation from a seed (csrc/dual_generate.cpp) through ltx_dual_generate_dev and ltx_dual_generate, on the narrow
model, the synthetic upscaler and the VAE statistics of tests/helpers/dual_two_stage_ref.py: stage 1 at (F, H, W) = (2, 3, 4), T_a 26,
S 70, {one-stage, two-stage} x {text-to-video, image-to-video, image-to-video with re-noising}, and one-stage with CFG.

The driver adds no numerics, so the check is exact: with a caller's workspace the final latents are those of the existing loop
(ltx_dual_denoise_dev / ltx_dual_two_stage_dev) called by the test with pointers into that same workspace at the plan's offsets, and
with the two in-place draws made by ltx_mlx_random_normal_dev. The draws themselves are compared with the host generator at the
tolerance of tests/test_mlx_normal_gpu.py. One noise launch per call: the workspace is complete at the first progress callback and is
not written again."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import dual_denoise_ref as dd  # noqa: E402
import dual_two_stage_ref as ts  # noqa: E402
import ltx_oracle as oracle  # noqa: E402

pytestmark = pytest.mark.gpu
N = ts.NARROW
F, H, W, T_A, S = N["F"], N["H"], N["W"], N["T_a"], N["S"]
C = 128
SEED = 2**40 + 5
RTOL, ATOL = 2e-6, 1e-7
V1, A1, K1, V2, A2, K2 = range(6)
CASES = {
    "one t2v": dict(two_stage=False), "one i2v": dict(two_stage=False, i2v=True), "one i2v_noise": dict(two_stage=False, i2v=True, renoise=True),
    "one cfg": dict(two_stage=False, cfg=True),
    "two t2v": dict(two_stage=True), "two i2v": dict(two_stage=True, i2v=True), "two i2v_noise": dict(two_stage=True, i2v=True, renoise=True),
}


def dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda().to(dtype)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.fixture(scope="module")
def env(ltx, tmp_path_factory):
    from safetensors.numpy import save_file

    d = tmp_path_factory.mktemp("dual_generate")
    ctx = ltx.Context(0)
    cfg = ltx.default_dual_model_config(num_layers=ts.L_NARROW, video_heads=N["Hv"], audio_heads=N["Ha"], caption_channels=N["caption_channels"])
    ctx.dual_model_init_synthetic(cfg, seed=81)
    wu = oracle.synth_upscaler_weights(mid=ts.UPSCALER_MID, seed=ts.UPSCALER_SEED)
    save_file({k: np.ascontiguousarray(v, dtype=np.float32) for k, v in wu.items()}, str(d / "up.safetensors"))
    ctx.upscaler_load(d / "up.safetensors")
    mean, std = ts.vae_stats()
    save_file({"latents_mean": mean, "latents_std": std}, str(d / "vae.safetensors"))
    ctx.vae_load(d / "vae.safetensors")
    cases = {cfg_on: dd.make_case(cfg=cfg_on, seed=3, audio_context=True, **N) for cfg_on in (False, True)}
    rng = np.random.default_rng(17)
    cond = {"cond1": rng.standard_normal((1, C, 1, H, W)).astype(np.float32), "cond2": rng.standard_normal((1, C, 1, 2 * H, 2 * W)).astype(np.float32)}
    yield {"ctx": ctx, "cfg": cfg, "cases": cases, "cond": cond, "dir": d}
    ctx.close()


def inputs(env, two_stage, i2v=False, renoise=False, cfg=False, host=False):
    """Keyword arguments of ltx.dual_generate_args for one case, on device tensors (or host arrays) made afresh."""
    c = env["cases"][cfg]
    put = (lambda x, dt=torch.float32: np.ascontiguousarray(x)) if host else dev
    up = 2 if two_stage else 1
    ctx_v, ctx_a = c["video_context"], c["audio_context"]
    if host:
        ctx_v, ctx_a = oracle.f32_to_bf16_bits(ctx_v), oracle.f32_to_bf16_bits(ctx_a)
    kw = dict(seed=SEED, F=F, H=H, W=W, T_a=T_A, S=S, sigmas1=ts.SIGMAS1, two_stage=two_stage, sigmas2=ts.SIGMAS2 if two_stage else None,
              video_latent=put(np.full((1, C, F, up * H, up * W), 9.0, np.float32)), audio_latent=put(np.full((1, 8, T_A, 16), 9.0, np.float32)),
              video_context=put(ctx_v, torch.bfloat16), audio_context=put(ctx_a, torch.bfloat16), mask=put(c["mask"], torch.int32))
    if cfg:
        kw.update(cfg_scale=3.0, guidance_rescale=0.7)
    if i2v:
        kw["cond_latent1"] = put(env["cond"]["cond1"])
        if two_stage:
            kw["cond_latent2"] = put(env["cond"]["cond2"])
    if renoise:
        kw["image_cond_noise_scale"] = ts.NOISE_SCALE
    return kw


def slot(ws, d):
    return ws[d["offset"]:d["offset"] + d["numel"]]


def by_existing_driver(ctx, kw, plan, ws):
    """The loop this driver wraps, called with pointers into `ws` at the plan's offsets; the in-place draws by ltx_mlx_random_normal_dev."""
    role = lambda r: [d for d in plan if d["role"] == r]  # noqa: E731
    first = lambda r: slot(ws, role(r)[0]) if role(r) else None  # noqa: E731
    audio = torch.empty((1, 8, T_A, 16), device="cuda")
    ctx.mlx_random_normal_dev(SEED, audio, draw_index=1, scale=ts.SIGMAS1[0])
    common = dict(audio_context=kw["audio_context"], mask=kw["mask"], image_cond_noise_scale=kw.get("image_cond_noise_scale", 0.0), T_a=T_A, S=S)
    if kw["two_stage"]:
        out = torch.empty((1, C, F, 2 * H, 2 * W), device="cuda")
        ctx.dual_two_stage_dev(first(V1), out, audio, ts.SIGMAS1, first(V2), first(A2), kw["video_context"], F, H, W, sigmas2=ts.SIGMAS2,
                               cond_latent1=kw.get("cond_latent1"), cond_latent2=kw.get("cond_latent2"), cond_noise1=first(K1),
                               cond_noise2=first(K2), **common)
    else:
        out = torch.empty((1, C, F, H, W), device="cuda")
        ctx.mlx_random_normal_dev(SEED, out, draw_index=0, scale=ts.SIGMAS1[0])
        ctx.dual_denoise_dev(out, audio, ts.SIGMAS1, kw["video_context"], F, H, W, cfg_scale=kw.get("cfg_scale", 1.0),
                             guidance_rescale=kw.get("guidance_rescale", 0.0), cond_latent=kw.get("cond_latent1"), cond_noise=first(K1), **common)
    torch.cuda.synchronize()
    return out.cpu().numpy(), audio.cpu().numpy()


@pytest.fixture(scope="module")
def results(env, ltx):
    """Every case once: the driver on a caller's workspace, what the first progress callback saw, and the existing loop on that workspace."""
    out = {}
    for name, case in CASES.items():
        kw = inputs(env, **case)
        plan, total = ltx.dual_noise_plan(ltx.dual_generate_args(**kw))
        ws = torch.full((total + 64,), 7.0, device="cuda")  # 64 guard floats behind it
        seen = []

        def on_progress(step, n, sigma, user, ws=ws, seen=seen):
            if not seen:
                torch.cuda.synchronize()
                seen.append(ws.clone())

        env["ctx"].dual_generate_dev(ltx.dual_generate_args(noise_workspace=ws, **kw), on_progress)
        torch.cuda.synchronize()
        got = (kw["video_latent"].cpu().numpy(), kw["audio_latent"].cpu().numpy())
        want = by_existing_driver(env["ctx"], kw, plan, ws)
        out[name] = dict(kw=kw, plan=plan, total=total, ws=ws.cpu().numpy(), at_first_step=seen[0].cpu().numpy(), got=got, want=want)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_a_the_latents_are_the_wrapped_loops_on_the_same_draws(results, name):
    r = results[name]
    (v, a), (wv, wa) = r["got"], r["want"]
    assert np.isfinite(v).all() and np.isfinite(a).all() and not (v == 9.0).any() and not (a == 9.0).any()
    assert same_bits(v, wv), float(np.abs(v - wv).max())
    assert same_bits(a, wa), float(np.abs(a - wa).max())


@pytest.mark.parametrize("name", list(CASES))
def test_b_every_workspace_draw_is_the_host_draw_of_its_index(results, ltx, name):
    r = results[name]
    covered = np.zeros(r["total"] + 64, bool)
    for d in r["plan"]:
        if d["offset"] < 0:
            continue
        want = np.float32(d["scale"]) * ltx.mlx_random_normal(SEED, (d["numel"],), d["draw_index"])
        np.testing.assert_allclose(slot(r["ws"], d), want, rtol=RTOL, atol=ATOL, err_msg=str(d))
        covered[d["offset"]:d["offset"] + d["numel"]] = True
    assert (r["ws"][~covered] == 7.0).all()  # the padding between slots and the guard behind the workspace


@pytest.mark.parametrize("name", list(CASES))
def test_c_one_noise_launch_fills_the_workspace_before_the_first_step(results, name):
    r = results[name]
    assert same_bits(r["at_first_step"], r["ws"])
    if r["total"]:
        assert not (r["ws"][:r["total"]] == 7.0).all()


def test_d_the_in_place_audio_draw_is_the_scaled_host_draw(env, ltx):
    """A schedule of one step whose last sigma equals its first: the audio stream's plain form leaves x + 0 * v, the draw itself (draw 1,
    times sigmas[0], shape [1][8][T_a][16]). The video stream's form is not the identity there; its in-place draw is covered by test_a,
    whose reference makes it with ltx_mlx_random_normal_dev."""
    kw = inputs(env, two_stage=False)
    kw["sigmas1"] = [0.75, 0.75]
    env["ctx"].dual_generate_dev(ltx.dual_generate_args(**kw))
    torch.cuda.synchronize()
    want = np.float32(0.75) * ltx.mlx_random_normal(SEED, (1, 8, T_A, 16), 1)
    np.testing.assert_allclose(kw["audio_latent"].cpu().numpy(), want, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("name", ["one i2v_noise", "one cfg", "two i2v_noise"])
def test_e_host_entry_equals_device_entry(env, results, ltx, name):
    r = results[name]
    kw = inputs(env, host=True, **CASES[name])
    ws = np.full(r["total"], 7.0, np.float32)
    env["ctx"].dual_generate(ltx.dual_generate_args(noise_workspace=ws, **kw))
    assert same_bits(kw["video_latent"], r["got"][0]) and same_bits(kw["audio_latent"], r["got"][1])
    assert same_bits(ws, r["ws"][:r["total"]])  # the host entry hands the draws back
    kw = inputs(env, host=True, **CASES[name])  # and without a workspace
    env["ctx"].dual_generate(ltx.dual_generate_args(**kw))
    assert same_bits(kw["video_latent"], r["got"][0]) and same_bits(kw["audio_latent"], r["got"][1])


def test_f_the_librarys_own_workspace_and_another_seed(env, results, ltx):
    kw = inputs(env, **CASES["two i2v_noise"])
    env["ctx"].dual_generate_dev(ltx.dual_generate_args(**kw))
    torch.cuda.synchronize()
    r = results["two i2v_noise"]
    assert same_bits(kw["video_latent"].cpu().numpy(), r["got"][0]) and same_bits(kw["audio_latent"].cpu().numpy(), r["got"][1])
    kw = inputs(env, **CASES["two i2v_noise"])
    kw["seed"] = SEED + 1
    env["ctx"].dual_generate_dev(ltx.dual_generate_args(**kw))
    torch.cuda.synchronize()
    assert not same_bits(kw["video_latent"].cpu().numpy(), r["got"][0]) and not same_bits(kw["audio_latent"].cpu().numpy(), r["got"][1])


def test_g_a_refused_call_leaves_outputs_and_workspace_untouched(env, ltx):
    from importlib import import_module

    lib_mod = import_module("ltx-video-swift-mlx_amd._lib")

    def refused(case_name, match, base, use=None, **change):
        kw = inputs(env, **base)
        kw.update(change)
        _, total = ltx.dual_noise_plan(ltx.dual_generate_args(**inputs(env, **base)))
        ws = torch.full((max(total, 64),), 7.0, device="cuda")
        with pytest.raises(ltx.LTXError, match=match) as e:
            (use or env["ctx"]).dual_generate_dev(ltx.dual_generate_args(noise_workspace=ws, **kw))
        assert e.value.case == case_name, (change, str(e.value))
        torch.cuda.synchronize()
        for t in (kw["video_latent"], kw["audio_latent"]):
            assert t is None or (t == 9.0).all(), change
        assert (ws == 7.0).all(), change

    one, two = CASES["one i2v_noise"], CASES["two i2v_noise"]
    refused("invalidConfiguration", "struct_size", one, struct_size=ctypes.sizeof(lib_mod.DualGenerateArgs) - 16)
    refused("invalidConfiguration", "channels", one, channels=64)
    refused("invalidConfiguration", "null", one, video_latent=None)
    refused("invalidConfiguration", "null", two, video_context=None)
    refused("invalidConfiguration", "positive", one, sigmas1=[1.0, 0.0, 0.25, 0.0])
    refused("invalidConfiguration", "positive", two, sigmas2=[0.9, -0.1, 0.0])
    refused("invalidConfiguration", "at least 2", two, sigmas1=[1.0])
    refused("invalidConfiguration", "guidance_rescale", one, guidance_rescale=0.5)
    refused("invalidConfiguration", "distilled", two, cfg_scale=3.0)
    refused("invalidConfiguration", "both resolutions", two, cond_latent2=None)
    refused("invalidConfiguration", "two latent frames", one, F=1)
    # the host entry refuses before it stages
    kw = inputs(env, host=True, **two)
    kw["cond_latent2"] = None
    with pytest.raises(ltx.LTXError, match="both resolutions"):
        env["ctx"].dual_generate(ltx.dual_generate_args(**kw))
    assert (kw["video_latent"] == 9.0).all() and (kw["audio_latent"] == 9.0).all()
    # a missing model: the dual model, then (two-stage) the upscaler, then the VAE
    bare = ltx.Context(0)
    try:
        refused("modelNotLoaded", "dual transformer", one, use=bare)
        bare.dual_model_init_synthetic(env["cfg"], seed=81)
        refused("modelNotLoaded", "upscaler", two, use=bare)
        bare.upscaler_load(env["dir"] / "up.safetensors")
        refused("modelNotLoaded", "vaeDecoder", two, use=bare)
    finally:
        bare.close()
