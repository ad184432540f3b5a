"""The joint video + audio denoise loop (csrc/dual_denoise.cpp, reference LTXPipeline.swift:1276-1417) through ltx_dual_denoise_dev and
ltx_dual_denoise on the narrow model of tests/test_dual_model_gpu.py (4 x 128 / 4 x 64, L 2, caption 256, (F, H, W) = (2, 6, 8), T_a 26,
S 70), loaded from a boosted checkpoint as there.

(a) - (e) are exact: the loop against the same loop composed here from the library's own uncached forward and the numpy float32 step of
tests/helpers/dual_denoise_ref.py (final latents torch.equal, in the caller's layouts: both layout round trips are in it), the text
cache against none, host pointers against device pointers, the progress callback, the refusals.

(f) guidance rescale and (g) the step statistics differ from the composition (variances and means in float64) by the f32 reductions of
launch_mean_var and the last-place rounding of launch_cfg_combine / launch_guidance_rescale, whose multiply-adds may fuse. Measured on
an MI355X: (f) max |x' - x'_ref| / max |x'_ref - x| = MEASURED_F over one step; (g) |statistic - numpy| / std of
its tensor at most MEASURED_G. The bounds are 10 x those, capped at 1e-4.

(h) parity with the f32 reference loop over 3 steps at CFG 12, rescale 1.0 (the setting at which tests/test_dual_denoise_host.py shows
every piece of the loop visible): rel-L2 of each final latent <= min(2 x the CPU rounding-point replay's, 3e-2), the project's bound."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import dual_denoise_ref as dd  # noqa: E402
import dual_model_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
NARROW = dict(Hv=4, Ha=4, F=2, H=6, W=8, T_a=26, S=70, caption_channels=256)
L_NARROW = 2
DISTILLED = [1.0, 0.725, 0.25, 0.0]   # 3 steps ending at sigma 0
CFG_SIGMAS = [1.0, 0.6, 0.25]         # 2 steps
MEASURED_F = 2.9e-7                   # MI355X, test (f)
MEASURED_G = 8.9e-8                   # MI355X, test (g)
BOUND_F = min(10 * MEASURED_F, 1e-4)
BOUND_G = min(10 * MEASURED_G, 1e-4)
NOT_LOADED = "dual transformer model not loaded"


def dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda().to(dtype)


def case_tensors(case):
    t = {"video_latent": dev(case["video_latent"][None]), "audio_latent": dev(case["audio_latent"][None]),
         "video_context": dev(case["video_context"], torch.bfloat16),
         "audio_context": None if case["audio_context"] is None else dev(case["audio_context"], torch.bfloat16),
         "mask": None if case["mask"] is None else dev(case["mask"], torch.int32)}
    return t


def run_dev(ctx, case, sigmas, **kw):
    """ltx_dual_denoise_dev on fresh device copies; returns (video latent [C][F][H][W], audio latent [8][T_a][16], stats or None)."""
    t = case_tensors(case)
    stats = ctx.dual_denoise_dev(t["video_latent"], t["audio_latent"], sigmas, t["video_context"], case["F"], case["H"], case["W"],
                                 audio_context=t["audio_context"], mask=t["mask"], **kw)
    torch.cuda.synchronize()
    return t["video_latent"][0].cpu().numpy(), t["audio_latent"][0].cpu().numpy(), stats


def gpu_forward(ctx):
    """The library's uncached forward as dual_denoise_ref.loop's forward."""
    def fwd(inp):
        B, Tv = inp["B"], inp["F"] * inp["H"] * inp["W"]
        vv, va = torch.empty((B, Tv, 128), device="cuda"), torch.empty((B, inp["T_a"], 128), device="cuda")
        mv = None if inp["null_mask"] else dev(inp["video_mask"], torch.int32)
        ma = None if inp["null_mask"] else dev(inp["audio_mask"], torch.int32)
        ctx.dual_model_forward_dev(dev(inp["video_latent"], torch.bfloat16), dev(inp["audio_latent"], torch.bfloat16),
                                   dev(inp["video_context"], torch.bfloat16), dev(inp["audio_context"], torch.bfloat16),
                                   dev(inp["video_timesteps"]), dev(inp["audio_timesteps"]), vv, va, inp["F"], inp["H"], inp["W"],
                                   video_mask=mv, audio_mask=ma)
        torch.cuda.synchronize()
        return vv.cpu().numpy(), va.cpu().numpy()
    return fwd


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.fixture(scope="module")
def model(gpu_ctx, ltx, tmp_path_factory):
    """The narrow model: random init -> exported -> dual_model_ref.boost -> a checkpoint-spelling file -> loaded."""
    from safetensors.numpy import save_file

    cfg = ltx.default_dual_model_config(num_layers=L_NARROW, video_heads=NARROW["Hv"], audio_heads=NARROW["Ha"],
                                        caption_channels=NARROW["caption_channels"])
    path = tmp_path_factory.mktemp("dual_denoise") / "boosted.safetensors"
    gpu_ctx.dual_model_init_synthetic(cfg, seed=61)
    shapes = ref.param_shapes(L_NARROW, NARROW["Hv"], NARROW["Ha"], caption_channels=NARROW["caption_channels"])
    w = ref.boost({k: gpu_ctx.dual_model_export_param(k).reshape(s) for k, s in shapes.items()}, NARROW["Hv"], NARROW["Ha"])
    save_file({ref.checkpoint_spelling(k): np.ascontiguousarray(v, dtype=np.float32) for k, v in w.items()}, str(path))
    load = lambda: gpu_ctx.dual_model_load(path, cfg)  # noqa: E731
    load()
    yield {"w": w, "load": load}
    gpu_ctx.dual_model_unload()


@pytest.fixture(scope="module")
def cases():
    """Inputs, shared and left unchanged: distilled (one context, the audio context defaults to it), CFG (own audio context), both masked."""
    return {"distilled": dd.make_case(cfg=False, seed=1, **NARROW), "cfg": dd.make_case(cfg=True, seed=2, audio_context=True, **NARROW),
            "cfg_shared": dd.make_case(cfg=True, seed=1, **NARROW), "null_mask": dd.make_case(cfg=False, seed=3, masked=False, **NARROW)}


@pytest.fixture(scope="module")
def composed(gpu_ctx, model, cases):
    """The loop composed from the uncached forward and the numpy step, once per setting."""
    fwd = gpu_forward(gpu_ctx)
    return {"distilled": dd.loop(fwd, cases["distilled"], DISTILLED), "cfg": dd.loop(fwd, cases["cfg"], CFG_SIGMAS, cfg_scale=3.0),
            "null_mask": dd.loop(fwd, cases["null_mask"], DISTILLED[1:])}


@pytest.mark.parametrize("name,sigmas,kw", [("distilled", DISTILLED, {}), ("cfg", CFG_SIGMAS, {"cfg_scale": 3.0}),
                                            ("null_mask", DISTILLED[1:], {})])
def test_a_loop_equals_the_composed_loop_bit_for_bit(gpu_ctx, cases, composed, name, sigmas, kw):
    """(a): distilled, 3 steps ending at sigma 0; CFG 3.0, 2 steps, an audio context of its own; a NULL mask."""
    gv, ga, _ = run_dev(gpu_ctx, cases[name], sigmas, **kw)
    wv, wa, _ = composed[name]
    assert gv.shape == (128, 2, 6, 8) and ga.shape == (8, 26, 16) and np.isfinite(gv).all() and np.isfinite(ga).all()
    assert not same_bits(gv, cases[name]["video_latent"]) and not same_bits(ga, cases[name]["audio_latent"])
    assert same_bits(gv, wv), float(np.abs(gv - wv).max())
    assert same_bits(ga, wa), float(np.abs(ga - wa).max())


def test_b_text_cache_on_and_off_give_the_same_bits_and_one_build(gpu_ctx, cases, composed):
    before = gpu_ctx.dual_model_text_cache_info()["builds"]
    cached = run_dev(gpu_ctx, cases["distilled"], DISTILLED, text_cache=1)
    after = gpu_ctx.dual_model_text_cache_info()
    assert after["builds"] == before + 1 and (after["B"], after["S"]) == (1, 70)
    plain = run_dev(gpu_ctx, cases["distilled"], DISTILLED, text_cache=0)
    assert gpu_ctx.dual_model_text_cache_info()["builds"] == before + 1
    for c, p, w in zip(cached[:2], plain[:2], composed["distilled"][:2]):
        assert same_bits(c, p) and same_bits(c, w)
    cfg_plain = run_dev(gpu_ctx, cases["cfg"], CFG_SIGMAS, cfg_scale=3.0, text_cache=0)
    for p, w in zip(cfg_plain[:2], composed["cfg"][:2]):
        assert same_bits(p, w)


def test_c_host_pointers_equal_device_pointers(gpu_ctx, ltx, cases, composed):
    c = cases["cfg"]
    hv, ha = gpu_ctx.dual_denoise(c["video_latent"][None], c["audio_latent"][None], CFG_SIGMAS, ltx.f32_to_bf16_bits(c["video_context"]),
                                  c["F"], c["H"], c["W"], audio_context_bf16=ltx.f32_to_bf16_bits(c["audio_context"]), mask=c["mask"],
                                  cfg_scale=3.0)
    assert same_bits(hv[0], composed["cfg"][0]) and same_bits(ha[0], composed["cfg"][1])
    d = cases["distilled"]  # NULL audio context and the statistics through the host entry
    hv, ha, st = gpu_ctx.dual_denoise(d["video_latent"][None], d["audio_latent"][None], DISTILLED, ltx.f32_to_bf16_bits(d["video_context"]),
                                      d["F"], d["H"], d["W"], mask=d["mask"], step_stats=True)
    assert same_bits(hv[0], composed["distilled"][0]) and same_bits(ha[0], composed["distilled"][1]) and st.shape == (3, 8)


def test_d_progress_is_called_before_each_forward(gpu_ctx, cases):
    """(d): `steps` calls, in order, with (step, steps, sigma of that step); the callback runs on the host before the step's forward is
    queued, so the count it has seen when it is called is the number of forwards queued so far."""
    seen = []
    run_dev(gpu_ctx, cases["distilled"], DISTILLED, on_progress=lambda step, total, sigma, user: seen.append((step, total, sigma, len(seen))))
    assert [(s[0], s[1], s[3]) for s in seen] == [(0, 3, 0), (1, 3, 1), (2, 3, 2)]
    assert np.array_equal(np.asarray([s[2] for s in seen], np.float32), np.asarray(DISTILLED[:3], np.float32))


def test_e_every_refusal_leaves_both_latents_untouched(gpu_ctx, ltx, model, cases):
    c = cases["cfg"]
    t = case_tensors(c)
    v0, a0 = t["video_latent"].clone(), t["audio_latent"].clone()

    def refused(case="invalidConfiguration", match=None, sigmas=CFG_SIGMAS, **kw):
        args = dict(dict(video_latent=t["video_latent"], audio_latent=t["audio_latent"], video_context=t["video_context"], F=2, H=6, W=8,
                         T_a=26, S=70, audio_context=t["audio_context"], mask=t["mask"], cfg_scale=3.0), **kw)
        with pytest.raises(ltx.LTXError, match=match) as e:
            gpu_ctx.dual_denoise_dev(args.pop("video_latent"), args.pop("audio_latent"), sigmas, args.pop("video_context"), args.pop("F"),
                                     args.pop("H"), args.pop("W"), **args)
        assert e.value.case == case, (kw, e.value)

    try:
        gpu_ctx.dual_model_unload()
        refused("modelNotLoaded", NOT_LOADED)
        model["load"]()
        refused(match="struct_size", struct_size=88)           # ends before step_stats
        refused(sigmas=[1.0])                                    # n_sigmas < 2
        refused(sigmas=[])
        for dim in ("F", "H", "W", "T_a", "S"):
            refused(**{dim: 0})
        refused(video_latent=None)
        refused(audio_latent=None)
        refused(video_context=None)
        refused(match="guidance_rescale", cfg_scale=1.0, guidance_rescale=0.7)
        refused(sigmas=[1.0, 0.0, 0.5])                          # a step from sigma 0
        torch.cuda.synchronize()
        assert torch.equal(t["video_latent"], v0) and torch.equal(t["audio_latent"], a0), "a refused call wrote"
        hv, ha = c["video_latent"][None].copy(), c["audio_latent"][None].copy()
        with pytest.raises(ltx.LTXError, match="guidance_rescale"):  # the host entry refuses before it stages
            gpu_ctx.dual_denoise(hv, ha, CFG_SIGMAS, ltx.f32_to_bf16_bits(c["video_context"][:1]), 2, 6, 8, guidance_rescale=0.7)
        assert ltx.lib.ltx_dual_denoise(gpu_ctx._h, None, ltx.PROGRESS_CB(lambda *a: None), None) == 2
    finally:
        model["load"]()


def test_f_guidance_rescale_one_step(gpu_ctx, cases):
    """(f): ONE step, CFG 3.0, phi 0.7 against the composition with its two variances in float64. MI355X: video deviation / max |x' - x|
    = MEASURED_F (see the constant); the audio latent is bit-equal to the run without rescale."""
    fwd = gpu_forward(gpu_ctx)
    c, sig = cases["cfg"], CFG_SIGMAS[:2]
    wv, wa, _ = dd.loop(fwd, c, sig, cfg_scale=3.0, rescale=0.7)
    nv, na, _ = dd.loop(fwd, c, sig, cfg_scale=3.0)
    gv, ga, _ = run_dev(gpu_ctx, c, sig, cfg_scale=3.0, guidance_rescale=0.7)
    moved = float(np.abs(wv - c["video_latent"]).max())
    dev_ = float(np.abs(gv - wv).max()) / moved
    print(f"(f) video: max |x' - x'_ref| / max |x'_ref - x| = {dev_:.3e} (bound {BOUND_F:.1e}); rescale moved the reference by "
          f"{float(np.abs(wv - nv).max()) / moved:.3e} of that")
    assert same_bits(ga, na) and same_bits(ga, wa), "rescale touched the audio stream"
    assert float(np.abs(wv - nv).max()) / moved > 100 * BOUND_F  # the rescale itself is far outside the bound
    assert dev_ <= BOUND_F, dev_


def test_g_step_statistics_against_numpy(gpu_ctx, cases, composed):
    """(g): mean and std of the video velocity, the video latent, the audio velocity and the audio latent per step, against float64
    numpy on the composed loop's tensors; each within BOUND_G of its tensor's std. The latents are unchanged by asking for them."""
    for name, sigmas, kw in (("distilled", DISTILLED, {}), ("cfg", CFG_SIGMAS, {"cfg_scale": 3.0})):
        gv, ga, st = run_dev(gpu_ctx, cases[name], sigmas, step_stats=True, **kw)
        wv, wa, want = composed[name]
        assert same_bits(gv, wv) and same_bits(ga, wa) and st.shape == want.shape
        worst = 0.0
        for i in range(len(sigmas) - 1):
            for k in range(4):
                std = want[i, 2 * k + 1]
                worst = max(worst, abs(st[i, 2 * k] - want[i, 2 * k]) / std, abs(st[i, 2 * k + 1] - std) / std)
        print(f"(g) {name}: worst |statistic - numpy| / std = {worst:.3e} (bound {BOUND_G:.1e})")
        assert worst <= BOUND_G, (name, worst)


def test_h_parity_with_the_f32_reference_loop(gpu_ctx, model, cases):
    """(h): 3 steps, CFG 12, rescale 1.0, masked, the audio context defaulting to the video context. MI355X: video 3.97e-3 (replay
    4.05e-3, bound 8.1e-3), audio 6.24e-3 (replay 6.21e-3, bound 1.24e-2); DESIGN.md section 6e."""
    c, sig, kw = cases["cfg_shared"], DISTILLED, dict(cfg_scale=12.0, rescale=1.0)
    fv, fa, _ = dd.loop(dd.ref_forward(model["w"], L_NARROW), c, sig, **kw)
    rv, ra, _ = dd.loop(dd.ref_forward(model["w"], L_NARROW, replay=True), c, sig, **kw)
    gv, ga, _ = run_dev(gpu_ctx, c, sig, cfg_scale=12.0, guidance_rescale=1.0)
    for name, g, f, r in (("video", gv, fv, rv), ("audio", ga, fa, ra)):
        rel, rep = dd.rel_l2(g, f), dd.rel_l2(r, f)
        bound = dd.update_bound(rep)
        print(f"(h) {name} latent after 3 steps: rel-L2 GPU {rel:.3e}; CPU replay {rep:.3e}, bound {bound:.3e}")
        assert np.isfinite(g).all()
        assert rel <= bound, (name, rel, bound)
