"""The dual video + audio model (csrc/dual_model.cpp, reference LTX2Transformer.swift:254-392) through ltx_dual_model_forward_dev and
ltx_dual_model_embed_dev against the numpy reference of tests/helpers/dual_model_ref.py on the library's own exported weights.

The narrow model is loaded from a safetensors file in the checkpoint's spelling: random-init weights, exported, brought to a trained
checkpoint's modulation regime by dual_model_ref.boost (bf16-exact changes) and loaded back, because tests/test_dual_model_host.py shows
that with weights of the same distribution and boost (drawn from numpy's generator there, exported from the library here: other values)
and dual_model_ref.make_inputs every piece of the model is visible far outside the bound below.

Bounds. Timestep path: max abs error against float64 <= 1e-4 x the reference's max abs, per output (the gemv test's 1e-4 at unit
scale). Velocities: the project's module bound, rel-L2 <= 1e-2 and cosine >= 0.9995 against the f32 reference, and rel-L2 within twice
that of the CPU rounding-point replay at the same shape, never above 3e-2 (dual_block_ref.update_bound applied to the velocity)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import dual_block_ref as bref  # noqa: E402
import dual_model_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
NARROW = dict(Hv=4, Ha=4, F=2, H=6, W=8, T_a=26, S=70, caption_channels=256)  # 96 video tokens, 26 audio tokens, 70 text keys
L_NARROW = 2
NOT_LOADED = "dual transformer model not loaded"
EMBED_OUTS = ("temb_v", "temb_a", "cross_v", "cross_a", "embts_v", "embts_a")


def dev(x, bf16=False):
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    return t.to(torch.bfloat16) if bf16 else t


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def narrow_cfg(ltx, **kw):
    return ltx.default_dual_model_config(**dict(dict(num_layers=L_NARROW, video_heads=NARROW["Hv"], audio_heads=NARROW["Ha"],
                                                     caption_channels=NARROW["caption_channels"]), **kw))


def export_weights(ctx, L, Hv, Ha, caption_channels):
    return {k: ctx.dual_model_export_param(k).reshape(shp) for k, shp in ref.param_shapes(L, Hv, Ha, caption_channels=caption_channels).items()}


def write_checkpoint(path, w, extra=None):
    from safetensors.numpy import save_file

    t = {ref.checkpoint_spelling(k): np.ascontiguousarray(v, dtype=np.float32) for k, v in w.items()}
    t.update(extra or {})
    save_file(t, str(path))
    return t


def run(ctx, inp, masks=True, ones=False, T_a=None, out=None, **kw):
    """One forward; returns (video_velocity, audio_velocity) as numpy. `out`: caller tensors (the error-path tests pass canaries)."""
    Ta = inp["T_a"] if T_a is None else T_a
    B, Tv = inp["B"], inp["F"] * inp["H"] * inp["W"]
    vv = torch.empty((B, Tv, 128), device="cuda") if out is None else out[0]
    va = torch.empty((B, max(Ta, 1), 128), device="cuda") if out is None else out[1]

    def mask(name):
        if not masks:
            return None
        m = np.ones_like(inp[name]) if ones else inp[name]
        return torch.from_numpy(np.ascontiguousarray(m, dtype=np.int32)).cuda()

    ctx.dual_model_forward_dev(dev(inp["video_latent"], True), dev(inp["audio_latent"][:, :max(Ta, 1)], True), dev(inp["video_context"], True),
                               dev(inp["audio_context"], True), dev(inp["video_timesteps"]), dev(inp["audio_timesteps"]), vv, va,
                               inp["F"], inp["H"], inp["W"], video_mask=mask("video_mask"), audio_mask=mask("audio_mask"), T_a=Ta, **kw)
    torch.cuda.synchronize()
    return vv.cpu().numpy(), va.cpu().numpy()


def embed(ctx, inp, Dv, Da, ungrouped):
    B = inp["B"]
    shapes = {"temb_v": (B, 6, Dv), "temb_a": (B, 6, Da), "cross_v": (B, 5, Dv), "cross_a": (B, 5, Da), "embts_v": (B, Dv), "embts_a": (B, Da)}
    o = {k: torch.full(s, float("nan"), device="cuda") for k, s in shapes.items()}
    ctx.dual_model_embed_dev(dev(inp["video_timesteps"]), dev(inp["audio_timesteps"]), *(o[k] for k in EMBED_OUTS), ungrouped=ungrouped)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def check(name, got, want, replay):
    """Module bound and replay bound of one velocity; every figure is printed before it is asserted."""
    rel, cos, rep = ref.rel_l2(got, want), ref.cosine(got, want), ref.rel_l2(replay, want)
    bound = ref.update_bound(rep)
    print(f"{name}: velocity rel-L2 GPU {rel:.3e} cosine {cos:.6f}; CPU replay {rep:.3e}, bound {bound:.3e}")
    assert np.isfinite(got).all()
    assert rel <= 1e-2, (name, rel)
    assert cos >= 0.9995, (name, cos)
    assert rel <= bound, (name, rel, bound)


def check_embed(name, ctx, w, inp, Dv, Da):
    g, u = embed(ctx, inp, Dv, Da, False), embed(ctx, inp, Dv, Da, True)
    want = ref.embed(w, inp, dtype=np.float64)
    for k in EMBED_OUTS:
        scale = float(np.abs(want[k]).max())
        err = float(np.abs(g[k] - want[k]).max())
        print(f"{name} {k}: max abs error against float64 {err:.2e} = {err / scale:.2e} x the reference's max abs {scale:.3f}")
        assert np.isfinite(g[k]).all()
        assert err <= 1e-4 * scale, (k, err, scale)
        assert np.array_equal(bits(g[k]), bits(u[k])), f"{k}: grouped and ungrouped differ"


@pytest.fixture(scope="module")
def model(gpu_ctx, ltx, tmp_path_factory):
    """The narrow model under test: random init (seed 41) -> exported -> boosted -> a checkpoint-spelling file -> loaded. `reload`
    restores it after a test that replaced or unloaded the model."""
    path = tmp_path_factory.mktemp("dual_model") / "boosted.safetensors"
    gpu_ctx.dual_model_init_synthetic(narrow_cfg(ltx), seed=41)
    w = ref.boost(export_weights(gpu_ctx, L_NARROW, NARROW["Hv"], NARROW["Ha"], NARROW["caption_channels"]), NARROW["Hv"], NARROW["Ha"])
    write_checkpoint(path, w)

    def reload():
        gpu_ctx.dual_model_load(path, narrow_cfg(ltx))
    reload()
    yield {"w": w, "path": path, "reload": reload}
    gpu_ctx.dual_model_unload()


@pytest.fixture(scope="module")
def case(gpu_ctx, model):
    """GPU result, f32 reference and replay of the narrow forward at B = 1 and 2: computed once, shared, left unchanged."""
    out = {}
    for B in (1, 2):
        inp = ref.make_inputs(B, seed=B, **NARROW)
        out[B] = {"inp": inp, "gpu": run(gpu_ctx, inp), "f32": ref.forward(model["w"], L_NARROW, inp),
                  "replay": ref.forward(model["w"], L_NARROW, inp, replay=True)}
    return out


def test_the_loaded_model_holds_the_boosted_weights(gpu_ctx, model):
    for k in ("adaln_single.linear.bias", "av_ca_a2v_gate_adaln_single.linear.weight", "scale_shift_table", "caption_projection.linear_2.weight",
              "audio_patchify_proj.weight", "transformer_blocks.1.audio_attn1.to_q.weight"):
        assert np.array_equal(gpu_ctx.dual_model_export_param(k), model["w"][k].ravel()), k


@pytest.mark.parametrize("B", [1, 2])
def test_timestep_path_against_float64(gpu_ctx, model, B):
    """The embed seam with unequal video / audio sigmas: all six outputs against float64 on the exported weights; grouped == ungrouped."""
    check_embed(f"B={B}", gpu_ctx, model["w"], ref.make_inputs(B, seed=B, **NARROW), NARROW["Hv"] * 128, NARROW["Ha"] * 64)


@pytest.mark.parametrize("B", [1, 2])
def test_narrow_forward_against_the_f32_reference(case, B):
    """4 x 128 / 4 x 64, L = 2, caption_channels 256, (F, H, W) = (2, 6, 8), T_a = 26, S = 70, a third of the keys masked per stream."""
    c = case[B]
    check(f"B={B} video", c["gpu"][0], c["f32"][0], c["replay"][0])
    check(f"B={B} audio", c["gpu"][1], c["f32"][1], c["replay"][1])


def test_full_width_model(gpu_ctx, ltx, model):
    """32 x 128 / 32 x 64, L = 1, caption_channels 3840, (F, H, W) = (1, 4, 8), T_a = 26, S = 70, B = 1: the K = 4096 and N = 6 x 4096
    grouped launches and both heads at their real widths, on random-init weights (a boosted file would be gigabytes). Unloads."""
    shape = dict(Hv=32, Ha=32, F=1, H=4, W=8, T_a=26, S=70, caption_channels=3840)
    inp = ref.make_inputs(1, seed=7, **shape)
    gpu_ctx.dual_model_init_synthetic(ltx.default_dual_model_config(num_layers=1), seed=42)
    try:
        gv, ga = run(gpu_ctx, inp)
        w = export_weights(gpu_ctx, 1, 32, 32, 3840)
        check_embed("full width", gpu_ctx, w, inp, 4096, 2048)
    finally:
        gpu_ctx.dual_model_unload()
        model["reload"]()
    fv, fa = ref.forward(w, 1, inp)
    rv, ra = ref.forward(w, 1, inp, replay=True)
    check("full-width video", gv, fv, rv)
    check("full-width audio", ga, fa, ra)


def test_audio_stream_wider_than_the_video_stream(gpu_ctx, ltx, model, tmp_path):
    """1 x 128 / 4 x 64: audio_dim 256 > video_dim 128, which the configuration allows. Every scratch buffer the two streams share (the
    caption projections' hidden activation, the heads' operand) must be sized by the wider one. Boosted weights from a file, B = 2,
    L = 1, caption_channels 128, (F, H, W) = (1, 4, 4), T_a = 9, S = 40; the same bounds as the narrow model."""
    shape = dict(Hv=1, Ha=4, F=1, H=4, W=4, T_a=9, S=40, caption_channels=128)
    cfg = ltx.default_dual_model_config(num_layers=1, video_heads=1, audio_heads=4, caption_channels=128)
    inp = ref.make_inputs(2, seed=5, **shape)
    try:
        gpu_ctx.dual_model_init_synthetic(cfg, seed=46)
        w = ref.boost(export_weights(gpu_ctx, 1, 1, 4, 128), 1, 4)
        write_checkpoint(tmp_path / "wide_audio.safetensors", w)
        gpu_ctx.dual_model_load(tmp_path / "wide_audio.safetensors", cfg)
        gv, ga = run(gpu_ctx, inp)
        check_embed("audio wider", gpu_ctx, w, inp, 128, 256)
        again = run(gpu_ctx, inp, ungrouped=True)
    finally:
        model["reload"]()
    fv, fa = ref.forward(w, 1, inp)
    rv, ra = ref.forward(w, 1, inp, replay=True)
    check("audio-wider video", gv, fv, rv)
    check("audio-wider audio", ga, fa, ra)
    assert np.array_equal(bits(gv), bits(again[0])) and np.array_equal(bits(ga), bits(again[1]))


def test_two_forwards_give_the_same_bits_and_ungrouped_equals_grouped(gpu_ctx, case):
    for B in (1, 2):
        again, ungrouped = run(gpu_ctx, case[B]["inp"]), run(gpu_ctx, case[B]["inp"], ungrouped=True)
        for first, a, u in zip(case[B]["gpu"], again, ungrouped):
            assert np.array_equal(bits(first), bits(a))
            assert np.array_equal(bits(first), bits(u))


def test_equal_batch_elements_give_equal_rows(gpu_ctx, model):
    inp = ref.make_inputs(1, seed=1, **NARROW)
    two = dict(inp, B=2)
    for k in ("video_latent", "audio_latent", "video_context", "audio_context", "video_timesteps", "audio_timesteps", "video_mask", "audio_mask"):
        two[k] = np.concatenate([inp[k], inp[k]], axis=0)
    for v in run(gpu_ctx, two):
        assert np.array_equal(bits(v[0]), bits(v[1]))


def test_null_mask_equals_all_ones_mask_bit_for_bit(gpu_ctx, case):
    inp = case[2]["inp"]
    a, b = run(gpu_ctx, inp, masks=False), run(gpu_ctx, inp, ones=True)
    for x, y, z in zip(a, b, case[2]["gpu"]):
        assert np.array_equal(bits(x), bits(y))
        assert np.abs(x - z).max() > 1e-4  # the mask itself is not a no-op


def test_shape_change_and_back_reproduces_the_first_result(gpu_ctx, model, case):
    """(F, H, W, T_a) = (2, 6, 8, 26) -> (1, 4, 4, 9) -> back: scratch, tables and V^T layouts change and return."""
    small = dict(NARROW, F=1, H=4, W=4, T_a=9)
    inp2 = ref.make_inputs(1, seed=3, **small)
    gv, ga = run(gpu_ctx, inp2)
    fv, fa = ref.forward(model["w"], L_NARROW, inp2)
    assert gv.shape == (1, 16, 128) and ga.shape == (1, 9, 128)
    assert ref.rel_l2(gv, fv) <= 1e-2 and ref.rel_l2(ga, fa) <= 1e-2
    for first, again in zip(case[1]["gpu"], run(gpu_ctx, case[1]["inp"])):
        assert np.array_equal(bits(first), bits(again))


def test_safetensors_round_trip_in_the_checkpoint_spelling(gpu_ctx, ltx, model, tmp_path):
    """Random-init model -> exported -> a file in the checkpoint's spelling (proj_in., time_embed.emb.timestep_embedder., time_embed.linear.,
    .emb.timestep_embedder., to_out.0, ...) plus tensors that are no parameter -> ltx_dual_model_load: the load report, the file's values,
    the synthetic model's forward bits; a file lacking one tensor is weightLoadingFailed and leaves no model."""
    inp = ref.make_inputs(1, seed=1, **NARROW)
    try:
        gpu_ctx.dual_model_init_synthetic(narrow_cfg(ltx), seed=43)
        want = run(gpu_ctx, inp)
        w = export_weights(gpu_ctx, L_NARROW, NARROW["Hv"], NARROW["Ha"], NARROW["caption_channels"])
        extra = {"norm_out.weight": np.ones(512, np.float32), "transformer_blocks.0.norm1.weight": np.ones(512, np.float32),
                 "transformer_blocks.7.attn1.to_q.weight": np.zeros((512, 512), np.float32)}  # block 7 is outside the model: not counted
        tensors = write_checkpoint(tmp_path / "model.safetensors", w, extra)
        assert "time_embed.emb.timestep_embedder.linear_1.weight" in tensors and "proj_in.weight" in tensors
        assert "av_ca_v2a_gate_adaln_single.emb.timestep_embedder.linear_2.bias" in tensors and "adaln_single.linear.weight" not in tensors
        gpu_ctx.dual_model_load(tmp_path / "model.safetensors", narrow_cfg(ltx))
        assert gpu_ctx.load_report() == {"loaded": len(w), "missing": 0, "unmatched": 2}
        for k in ("adaln_single.emb.linear_1.weight", "audio_adaln_single.linear.bias", "av_ca_audio_scale_shift_adaln_single.emb.linear_2.weight",
                  "patchify_proj.bias", "audio_scale_shift_table", "audio_caption_projection.linear_1.weight", "proj_out.weight",
                  "transformer_blocks.1.audio_ff.project_out.weight", "transformer_blocks.0.scale_shift_table_a2v_ca_audio"):
            assert np.array_equal(gpu_ctx.dual_model_export_param(k), w[k].ravel()), k
        for x, y in zip(want, run(gpu_ctx, inp)):
            assert np.array_equal(bits(x), bits(y))
        for gone in ("av_ca_a2v_gate_adaln_single.linear.bias", "transformer_blocks.1.audio_attn2.to_out.bias"):
            lacking = {k: v for k, v in w.items() if k != gone}
            write_checkpoint(tmp_path / "lacking.safetensors", lacking)
            with pytest.raises(ltx.LTXError, match=gone.split("transformer_blocks.1.")[-1]) as e:
                gpu_ctx.dual_model_load(tmp_path / "lacking.safetensors", narrow_cfg(ltx))
            assert e.value.case == "weightLoadingFailed"
            out = (torch.full((1, 96, 128), 7.0, device="cuda"), torch.full((1, 26, 128), 7.0, device="cuda"))
            with pytest.raises(ltx.LTXError, match=NOT_LOADED) as e:
                run(gpu_ctx, inp, out=out)
            assert e.value.case == "modelNotLoaded"
            assert (out[0] == 7.0).all() and (out[1] == 7.0).all()
    finally:
        model["reload"]()


def test_error_paths_report_the_documented_case_and_write_nothing(gpu_ctx, ltx, model):
    inp = ref.make_inputs(1, seed=1, **NARROW)
    out = (torch.full((1, 96, 128), 7.0, device="cuda"), torch.full((1, 26, 128), 7.0, device="cuda"))
    emb = [torch.full((1, n), 7.0, device="cuda") for n in (6 * 512, 6 * 256, 5 * 512, 5 * 256, 512, 256)]
    ts = dev(inp["video_timesteps"])
    try:
        gpu_ctx.dual_model_unload()
        with pytest.raises(ltx.LTXError, match=NOT_LOADED) as e:   # forward before load
            run(gpu_ctx, inp, out=out)
        assert e.value.case == "modelNotLoaded"
        with pytest.raises(ltx.LTXError, match=NOT_LOADED):
            gpu_ctx.dual_model_embed_dev(ts, ts, *emb)
        with pytest.raises(ltx.LTXError, match=NOT_LOADED):
            gpu_ctx.dual_model_export_param("scale_shift_table")
        model["reload"]()
        with pytest.raises(ltx.LTXError, match="struct_size") as e:  # a struct that ends before audio_velocity
            run(gpu_ctx, inp, out=out, struct_size=96)
        assert e.value.case == "invalidConfiguration"
        with pytest.raises(ltx.LTXError, match="T_a=0") as e:
            run(gpu_ctx, inp, out=out, T_a=0)
        assert e.value.case == "invalidConfiguration"
        with pytest.raises(ltx.LTXError, match="null") as e:
            gpu_ctx.dual_model_forward_dev(dev(inp["video_latent"], True), dev(inp["audio_latent"], True), dev(inp["video_context"], True),
                                           dev(inp["audio_context"], True), ts, None, out[0], out[1], 2, 6, 8)
        assert e.value.case == "invalidConfiguration"
        for bad in (dict(B=0), dict(B=9)):
            with pytest.raises(ltx.LTXError, match="B=") as e:
                gpu_ctx.dual_model_embed_dev(ts, ts, *emb, **bad)
            assert e.value.case == "invalidConfiguration"
        with pytest.raises(ltx.LTXError, match="null") as e:
            gpu_ctx.dual_model_embed_dev(ts, ts, *emb[:5], None)
        assert e.value.case == "invalidConfiguration"
        with pytest.raises(ltx.LTXError, match="no parameter"):
            gpu_ctx.dual_model_export_param("norm_out.weight")
        torch.cuda.synchronize()
        assert (out[0] == 7.0).all() and (out[1] == 7.0).all() and all((t == 7.0).all() for t in emb), "a refused call wrote"
        # a configuration the model cannot have: refused, and (as every replace) the slot is empty afterwards
        for bad in (dict(video_dim=500), dict(video_context_dim=256), dict(caption_channels=100), dict(out_channels=0)):
            with pytest.raises(ltx.LTXError) as e:
                gpu_ctx.dual_model_init_synthetic(narrow_cfg(ltx, **bad), seed=1)
            assert e.value.case == "invalidConfiguration", bad
        with pytest.raises(ltx.LTXError, match=NOT_LOADED):
            run(gpu_ctx, inp, out=out)
        with pytest.raises(ltx.LTXError) as e:
            gpu_ctx.dual_model_load("/nonexistent/model.safetensors", narrow_cfg(ltx))
        assert e.value.case == "fileNotFound"
        assert (out[0] == 7.0).all() and (out[1] == 7.0).all()
    finally:
        model["reload"]()


def test_lifecycle(gpu_ctx, ltx, model, case):
    """load -> forward -> replace -> forward -> load back -> the first bits -> unload (twice) -> "not loaded"."""
    inp = case[1]["inp"]
    try:
        gpu_ctx.dual_model_init_synthetic(narrow_cfg(ltx), seed=44)   # replace: other weights, other result
        b = run(gpu_ctx, inp)
        assert np.isfinite(b[0]).all() and np.abs(b[0] - case[1]["gpu"][0]).max() > 1e-3 and np.abs(b[1] - case[1]["gpu"][1]).max() > 1e-3
        model["reload"]()
        for x, y in zip(case[1]["gpu"], run(gpu_ctx, inp)):
            assert np.array_equal(bits(x), bits(y))
        gpu_ctx.dual_model_unload()
        gpu_ctx.dual_model_unload()   # unloading an empty slot is LTX_OK
        with pytest.raises(ltx.LTXError, match=NOT_LOADED) as e:
            run(gpu_ctx, inp)
        assert e.value.case == "modelNotLoaded"
    finally:
        model["reload"]()


def test_the_model_and_the_block_stack_are_independent_slots(gpu_ctx, ltx, model, case):
    """ltx_dual_blocks_* holds a stack of its own: loading, replacing or unloading either leaves the other's bits alone."""
    shape = {k: NARROW[k] for k in ("Hv", "Ha", "F", "H", "W", "T_a", "S")}
    binp = bref.make_inputs(1, seed=1, **shape)

    def blocks_forward():
        xv, xa = dev(binp["x_video"]), dev(binp["x_audio"])
        gpu_ctx.dual_blocks_forward_dev(xv, xa, dev(binp["context_video"], True), dev(binp["context_audio"], True), dev(binp["temb_video"]),
                                        dev(binp["temb_audio"]), dev(binp["cross_video_ss"]), dev(binp["cross_audio_ss"]), 2, 6, 8)
        torch.cuda.synchronize()
        return xv.cpu().numpy(), xa.cpu().numpy()

    try:
        gpu_ctx.dual_blocks_init_synthetic(ltx.default_dual_block_config(num_layers=1, video_heads=4, audio_heads=4), seed=31)
        for x, y in zip(case[1]["gpu"], run(gpu_ctx, case[1]["inp"])):   # loading a stack did not touch the model
            assert np.array_equal(bits(x), bits(y))
        first = blocks_forward()
        gpu_ctx.dual_model_init_synthetic(narrow_cfg(ltx), seed=45)
        gpu_ctx.dual_model_unload()
        for x, y in zip(first, blocks_forward()):                         # replacing / unloading the model did not touch the stack
            assert np.array_equal(bits(x), bits(y))
        with pytest.raises(ltx.LTXError, match=NOT_LOADED):
            run(gpu_ctx, case[1]["inp"])
        model["reload"]()
        gpu_ctx.dual_blocks_unload()
        with pytest.raises(ltx.LTXError, match="dual transformer blocks not loaded"):
            blocks_forward()
        for x, y in zip(case[1]["gpu"], run(gpu_ctx, case[1]["inp"])):   # unloading the stack did not touch the model
            assert np.array_equal(bits(x), bits(y))
    finally:
        gpu_ctx.dual_blocks_unload()
        model["reload"]()
