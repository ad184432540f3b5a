"""The dual video + audio model with timestep GROUPS on the video stream (ltx_dual_model_forward_groups_dev: csrc/dual_model.cpp,
csrc/dual_block.cpp; reference LTX2Transformer.swift:285-312, where the adaLN rows, both cross-modal embedders and the head read
per-token video timesteps) against the per-token f32 reference of tests/helpers/dual_i2v_ref.py on the library's own exported weights.

The narrow model is that of tests/test_dual_model_gpu.py (4 x 128 / 4 x 64, L 2, caption 256, (F, H, W) = (2, 6, 8), T_a 26, S 70,
boosted): frame 0 is 48 of 96 tokens, so the group boundary falls inside one GEMM tile, and inside a B = 2 tile.
tests/test_dual_i2v_host.py shows that at these inputs a forward whose frame-0 tokens run at sigma, whose cross-modal rows are per
batch element or whose head is per batch element leaves the bounds below by a factor of 10 or more.

Bounds: the project's module bound, rel-L2 <= 1e-2 and cosine >= 0.9995 against the f32 reference, and rel-L2 within twice that of the
CPU rounding-point replay at the same shape, never above 3e-2 (dual_block_ref.update_bound)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import dual_i2v_ref as iv  # noqa: E402
import dual_model_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
NARROW = dict(Hv=4, Ha=4, F=2, H=6, W=8, T_a=26, S=70, caption_channels=256)
L_NARROW = 2
CANARY = 7.0


def dev(x, bf16=False):
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    return t.to(torch.bfloat16) if bf16 else t


def idev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).cuda()


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def i2v_groups(B, F, H, W, sigma):
    """The loop's own layout: ts[b] = {sigma_b, 0}, frame-0 tokens in group 1 (launch_i2v_rowmap)."""
    ts = np.zeros((B, 2), np.float32)
    ts[:, 0] = np.asarray(sigma, np.float32)
    rm = np.zeros((B, F * H * W), np.int32)
    rm[:, :H * W] = 1
    return ts, (rm + 2 * np.arange(B, dtype=np.int32)[:, None]).reshape(-1)


def run(ctx, inp, ts, row_map, n_groups=None, out=None, text_cache=0, masks=True):
    """One groups forward; returns (video_velocity, audio_velocity) as numpy."""
    B, Tv = inp["B"], inp["F"] * inp["H"] * inp["W"]
    vv = torch.empty((B, Tv, 128), device="cuda") if out is None else out[0]
    va = torch.empty((B, inp["T_a"], 128), device="cuda") if out is None else out[1]
    G = ts.shape[1] if n_groups is None else n_groups
    mask = lambda k: idev(inp[k]) if masks else None  # noqa: E731
    ctx.dual_model_forward_groups_dev(dev(inp["video_latent"], True), dev(inp["audio_latent"], True), dev(inp["video_context"], True),
                                      dev(inp["audio_context"], True), dev(ts), dev(inp["audio_timesteps"]), vv, va, inp["F"], inp["H"], inp["W"],
                                      G, None if row_map is None else idev(row_map), video_mask=mask("video_mask"), audio_mask=mask("audio_mask"),
                                      text_cache=text_cache)
    torch.cuda.synchronize()
    return vv.cpu().numpy(), va.cpu().numpy()


def check(name, got, want, replay):
    rel, cos, rep = ref.rel_l2(got, want), ref.cosine(got, want), ref.rel_l2(replay, want)
    bound = ref.update_bound(rep)
    print(f"{name}: velocity rel-L2 GPU {rel:.3e} cosine {cos:.6f}; CPU replay {rep:.3e}, bound {bound:.3e}")
    assert np.isfinite(got).all()
    assert rel <= 1e-2, (name, rel)
    assert cos >= 0.9995, (name, cos)
    assert rel <= bound, (name, rel, bound)


def narrow_cfg(ltx):
    return ltx.default_dual_model_config(num_layers=L_NARROW, video_heads=NARROW["Hv"], audio_heads=NARROW["Ha"],
                                         caption_channels=NARROW["caption_channels"])


def export_weights(ctx, L, Hv, Ha, caption_channels):
    return {k: ctx.dual_model_export_param(k).reshape(shp) for k, shp in ref.param_shapes(L, Hv, Ha, caption_channels=caption_channels).items()}


@pytest.fixture(scope="module")
def model(gpu_ctx, ltx, tmp_path_factory):
    """Random init -> exported -> dual_model_ref.boost -> a checkpoint-spelling file -> loaded, as tests/test_dual_model_gpu.py does."""
    from safetensors.numpy import save_file

    path = tmp_path_factory.mktemp("dual_i2v_forward") / "boosted.safetensors"
    gpu_ctx.dual_model_init_synthetic(narrow_cfg(ltx), seed=71)
    w = ref.boost(export_weights(gpu_ctx, L_NARROW, NARROW["Hv"], NARROW["Ha"], NARROW["caption_channels"]), NARROW["Hv"], NARROW["Ha"])
    save_file({ref.checkpoint_spelling(k): np.ascontiguousarray(v, dtype=np.float32) for k, v in w.items()}, str(path))

    def reload():
        gpu_ctx.dual_model_load(path, narrow_cfg(ltx))
    reload()
    yield {"w": w, "reload": reload}
    gpu_ctx.dual_model_unload()


@pytest.fixture(scope="module")
def cases(gpu_ctx, model):
    """Inputs, the GPU result, the f32 reference and the replay, once; shared and left unchanged. "equal": frame 0 at 0, the rest at one
    sigma for every batch element, in the loop's own group layout; "unequal": another sigma per batch element (make_inputs'), grouped by
    ltx.timestep_groups, which numbers frame 0's group first."""
    out = {}
    for B in (1, 2):
        for name in ("equal", "unequal"):
            inp = ref.make_inputs(B, seed=10 + B, **NARROW)
            sigma = np.full(B, 0.725, np.float32) if name == "equal" else inp["video_timesteps"]
            inp["video_token_timesteps"] = iv.i2v_token_timesteps(B, NARROW["F"], NARROW["H"], NARROW["W"], sigma)
            out[B, name] = {"inp": inp, "sigma": sigma, "f32": iv.forward(model["w"], L_NARROW, inp), "replay": iv.forward(model["w"], L_NARROW, inp, replay=True)}
    return out


def groups_of(ltx, c, name):
    inp = c["inp"]
    if name == "equal":
        return i2v_groups(inp["B"], inp["F"], inp["H"], inp["W"], c["sigma"])
    ts, rm = ltx.timestep_groups(inp["video_token_timesteps"])
    assert ts.shape == (inp["B"], 2) and np.array_equal(ts[:, 0], np.zeros(inp["B"], np.float32))  # first appearance: frame 0
    return ts, rm


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("name", ["equal", "unequal"])
def test_narrow_groups_forward_against_the_per_token_reference(gpu_ctx, ltx, cases, B, name):
    """MI355X: video 2.60e-3 - 2.67e-3 (replay 2.61e-3 - 2.65e-3), audio 2.24e-3 - 2.38e-3 (replay 2.24e-3 -
    2.36e-3), cosine >= 0.999996; bounds twice the replay."""
    c = cases[B, name]
    ts, rm = groups_of(ltx, c, name)
    gv, ga = run(gpu_ctx, c["inp"], ts, rm)
    check(f"B={B} {name} video", gv, c["f32"][0], c["replay"][0])
    check(f"B={B} {name} audio", ga, c["f32"][1], c["replay"][1])
    # the groups are READ: the per-batch forward at sigma is far outside the bound (tests/test_dual_i2v_host.py: 20 x)
    plain = dict(c["inp"], video_timesteps=c["sigma"])
    pv, pa = run(gpu_ctx, plain, np.asarray(c["sigma"], np.float32).reshape(B, 1), None)
    assert ref.rel_l2(pv, c["f32"][0]) > 5 * ref.update_bound(ref.rel_l2(c["replay"][0], c["f32"][0]))
    assert ref.rel_l2(pa, c["f32"][1]) > 5 * ref.update_bound(ref.rel_l2(c["replay"][1], c["f32"][1]))


@pytest.mark.parametrize("B", [1, 2])
def test_one_group_without_a_map_is_the_plain_forward(gpu_ctx, cases, B):
    """n_groups = 1 with a NULL map is ltx_dual_model_forward_dev: the same bits."""
    c = cases[B, "unequal"]
    inp = dict(c["inp"], video_timesteps=c["sigma"])
    a = run(gpu_ctx, inp, np.asarray(c["sigma"], np.float32).reshape(B, 1), None)
    vv, va = torch.empty((B, 96, 128), device="cuda"), torch.empty((B, 26, 128), device="cuda")
    gpu_ctx.dual_model_forward_dev(dev(inp["video_latent"], True), dev(inp["audio_latent"], True), dev(inp["video_context"], True),
                                   dev(inp["audio_context"], True), dev(c["sigma"]), dev(inp["audio_timesteps"]), vv, va, 2, 6, 8,
                                   video_mask=idev(inp["video_mask"]), audio_mask=idev(inp["audio_mask"]))
    torch.cuda.synchronize()
    assert np.array_equal(bits(a[0]), bits(vv.cpu().numpy())) and np.array_equal(bits(a[1]), bits(va.cpu().numpy()))


@pytest.mark.parametrize("B", [1, 2])
def test_text_cache_on_and_off_give_the_same_bits(gpu_ctx, ltx, cases, B):
    c = cases[B, "unequal"]
    inp = c["inp"]
    ts, rm = groups_of(ltx, c, "unequal")
    plain = run(gpu_ctx, inp, ts, rm)
    gpu_ctx.dual_model_prepare_text(dev(inp["video_context"], True), dev(inp["audio_context"], True), idev(inp["video_mask"]), idev(inp["audio_mask"]))
    cached = run(gpu_ctx, inp, ts, rm, text_cache=1)
    for p, q in zip(plain, cached):
        assert torch.equal(torch.from_numpy(p), torch.from_numpy(q)) and np.array_equal(bits(p), bits(q))


@pytest.mark.parametrize("B", [1, 2])
def test_the_group_a_token_is_in_does_not_matter_when_the_groups_carry_one_sigma(gpu_ctx, cases, B):
    """G = 2, both groups at the batch element's sigma: every token in group 0, every token in group 1 and the image-to-video split give
    the same bits - a modulation row depends on its timestep, not on its place among the rows."""
    c = cases[B, "unequal"]
    inp = c["inp"]
    ts = np.repeat(np.asarray(c["sigma"], np.float32).reshape(B, 1), 2, axis=1)
    base = (2 * np.arange(B, dtype=np.int32))[:, None] + np.zeros((B, 96), np.int32)
    g0 = run(gpu_ctx, inp, ts, base.reshape(-1))
    g1 = run(gpu_ctx, inp, ts, (base + 1).reshape(-1))
    split = run(gpu_ctx, inp, ts, i2v_groups(B, 2, 6, 8, c["sigma"])[1])
    for a, b, s in zip(g0, g1, split):
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(s))
    assert np.isfinite(g0[0]).all() and np.isfinite(g0[1]).all()


def test_full_width_groups_forward(gpu_ctx, ltx, model):
    """32 x 128 / 32 x 64, L = 1, caption 3840, (F, H, W) = (2, 4, 8), T_a 26, S 70, B = 1, random init, as test_full_width_model of
    tests/test_dual_model_gpu.py does it: the two grouped launches per stage at K = 4096, norm_mod2's NV = 4 / 2 instances and the mapped
    gates at their real widths. Unloads and restores the narrow model."""
    shape = dict(Hv=32, Ha=32, F=2, H=4, W=8, T_a=26, S=70, caption_channels=3840)
    inp = ref.make_inputs(1, seed=7, **shape)
    inp["video_token_timesteps"] = iv.i2v_token_timesteps(1, 2, 4, 8, inp["video_timesteps"])
    ts, rm = i2v_groups(1, 2, 4, 8, inp["video_timesteps"])
    gpu_ctx.dual_model_init_synthetic(ltx.default_dual_model_config(num_layers=1), seed=72)
    try:
        gv, ga = run(gpu_ctx, inp, ts, rm)
        w = export_weights(gpu_ctx, 1, 32, 32, 3840)
    finally:
        gpu_ctx.dual_model_unload()
        model["reload"]()
    fv, fa = iv.forward(w, 1, inp)
    rv, ra = iv.forward(w, 1, inp, replay=True)
    check("full-width video", gv, fv, rv)
    check("full-width audio", ga, fa, ra)


def test_refusals_write_nothing(gpu_ctx, ltx, cases):
    """n_groups < 1, B * n_groups > 8, more than one group without a map: invalidConfiguration before the first launch."""
    c = cases[2, "equal"]
    inp = c["inp"]
    out = (torch.full((2, 96, 128), CANARY, device="cuda"), torch.full((2, 26, 128), CANARY, device="cuda"))
    ts, rm = i2v_groups(2, 2, 6, 8, c["sigma"])
    wide = np.zeros((2, 5), np.float32)
    for kw in (dict(ts=ts, row_map=rm, n_groups=0), dict(ts=ts, row_map=rm, n_groups=-1), dict(ts=wide, row_map=rm, n_groups=5),
               dict(ts=ts, row_map=None, n_groups=2)):
        with pytest.raises(ltx.LTXError, match="n_groups") as e:
            run(gpu_ctx, inp, kw["ts"], kw["row_map"], n_groups=kw["n_groups"], out=out)
        assert e.value.case == "invalidConfiguration", kw["n_groups"]
    torch.cuda.synchronize()
    assert (out[0] == CANARY).all() and (out[1] == CANARY).all(), "a refused call wrote"
    good = run(gpu_ctx, inp, np.zeros((2, 4), np.float32) + ts[:, :1], rm * 2)  # B * G = 8 passes (groups 0 and 2 of 4 used)
    assert np.isfinite(good[0]).all()
