"""The dual video + audio transformer block stack (csrc/dual_block.cpp, reference LTX2TransformerBlock.swift:174-297) through
ltx_dual_blocks_forward_dev against the f32 numpy reference of tests/helpers/dual_block_ref.py on the library's own exported weights.

Bounds. Full stream: the project's module bound, rel-L2 <= 1e-2 and cosine >= 0.9995 per stream against the f32 reference on the
unrounded inputs. The stream is dominated by its own input, so the UPDATE out - in is bounded as well: twice the rel-L2 of the CPU
rounding-point replay against the f32 reference at that shape, never above 3e-2 (dual_block_ref.update_bound). The inputs are those of
dual_block_ref.make_inputs, for which tests/test_dual_block_host.py shows that dropping any one of the eight phases, or taking normVCA
after the a2v update, lands far outside that bound."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import dual_block_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
NARROW = dict(Hv=4, Ha=4, F=2, H=6, W=8, T_a=26, S=70)  # 96 video tokens, 26 audio tokens, 70 text keys
L_NARROW = 2
NOT_LOADED = "dual transformer blocks not loaded"


def dev(x, bf16=False):
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    return t.to(torch.bfloat16) if bf16 else t


def narrow_cfg(ltx, **kw):
    return ltx.default_dual_block_config(num_layers=L_NARROW, video_heads=NARROW["Hv"], audio_heads=NARROW["Ha"], **kw)


def export_weights(ctx, L, Hv, Ha):
    return {k: ctx.dual_blocks_export_param(k).reshape(shp) for k, shp in ref.param_shapes(L, Hv, Ha).items()}


def run(ctx, inp, bias=True, zero_bias=False, T_a=None, **kw):
    """One forward on copies of the streams of `inp`; returns (x_video, x_audio) as numpy."""
    Ta = inp["T_a"] if T_a is None else T_a
    xv, xa = dev(inp["x_video"]), dev(inp["x_audio"][:, :Ta])
    bv = dev(np.zeros_like(inp["bias_video"]) if zero_bias else inp["bias_video"]) if bias else None
    ba = dev(np.zeros_like(inp["bias_audio"]) if zero_bias else inp["bias_audio"]) if bias else None
    ctx.dual_blocks_forward_dev(xv, xa, dev(inp["context_video"], True), dev(inp["context_audio"], True), dev(inp["temb_video"]),
                                dev(inp["temb_audio"]), dev(inp["cross_video_ss"]), dev(inp["cross_audio_ss"]), inp["F"], inp["H"], inp["W"],
                                key_bias_video=bv, key_bias_audio=ba, **kw)
    torch.cuda.synchronize()
    return xv.cpu().numpy(), xa.cpu().numpy()


def check(name, got, want, replay, x):
    """Stream bound and update bound; every figure is printed before it is asserted."""
    rel, cos = ref.rel_l2(got, want), ref.cosine(got, want)
    upd, rep = ref.rel_l2(got - x, want - x), ref.rel_l2(replay - x, want - x)
    bound = ref.update_bound(rep)
    print(f"{name}: stream rel-L2 {rel:.3e} cosine {cos:.6f}; update rel-L2 GPU {upd:.3e}, CPU replay {rep:.3e}, bound {bound:.3e}")
    assert np.isfinite(got).all()
    assert rel <= 1e-2, (name, rel)
    assert cos >= 0.9995, (name, cos)
    assert upd <= bound, (name, upd, bound)


@pytest.fixture(scope="module")
def stack(gpu_ctx, ltx):
    """The narrow stack (seed 31) and its exported weights; tests that replace the stack restore it through `reload`."""
    def reload():
        gpu_ctx.dual_blocks_init_synthetic(narrow_cfg(ltx), seed=31)
    reload()
    w = export_weights(gpu_ctx, L_NARROW, NARROW["Hv"], NARROW["Ha"])
    tabs = ref.tables(None, NARROW["F"], NARROW["H"], NARROW["W"], NARROW["T_a"], NARROW["Hv"], NARROW["Ha"])
    yield {"w": w, "tabs": tabs, "reload": reload}
    gpu_ctx.dual_blocks_unload()


@pytest.mark.parametrize("B", [1, 2])
def test_narrow_stack_against_the_f32_reference(gpu_ctx, stack, B):
    """video 4 x 128 = 512, audio 4 x 64 = 256, L = 2, (F, H, W) = (2, 6, 8), T_a = 26, S = 70 with a third of the keys masked
    (different masks per stream)."""
    inp = ref.make_inputs(B, seed=B, **NARROW)
    gv, ga = run(gpu_ctx, inp)
    fv, fa = ref.forward(stack["w"], L_NARROW, inp, stack["tabs"])
    rv, ra = ref.forward(stack["w"], L_NARROW, inp, stack["tabs"], replay=True)
    check(f"B={B} video", gv, fv, rv, inp["x_video"])
    check(f"B={B} audio", ga, fa, ra, inp["x_audio"])


def test_full_width_block(gpu_ctx, ltx, stack):
    """32 x 128 / 32 x 64, L = 1, (F, H, W) = (4, 6, 8) -> 192 video tokens, T_a = 26: the real GEMM shapes. Unloads afterwards."""
    shape = dict(Hv=32, Ha=32, F=4, H=6, W=8, T_a=26, S=70)
    gpu_ctx.dual_blocks_init_synthetic(ltx.default_dual_block_config(num_layers=1), seed=32)
    try:
        inp = ref.make_inputs(1, seed=7, **shape)
        gv, ga = run(gpu_ctx, inp)
        w = export_weights(gpu_ctx, 1, 32, 32)
    finally:
        gpu_ctx.dual_blocks_unload()
        stack["reload"]()
    tabs = ref.tables(None, 4, 6, 8, 26, 32, 32)
    fv, fa = ref.forward(w, 1, inp, tabs)
    rv, ra = ref.forward(w, 1, inp, tabs, replay=True)
    check("full-width video", gv, fv, rv, inp["x_video"])
    check("full-width audio", ga, fa, ra, inp["x_audio"])


def test_null_key_bias_equals_zero_bias_bit_for_bit(gpu_ctx, stack):
    inp = ref.make_inputs(2, seed=2, **NARROW)
    a = run(gpu_ctx, inp, bias=False)
    b = run(gpu_ctx, inp, zero_bias=True)
    c = run(gpu_ctx, inp)
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        assert np.abs(x - z).max() > 1e-4  # the mask itself is not a no-op


def test_shape_change_rebuilds_the_tables_and_reproduces_the_first_result(gpu_ctx, stack):
    """T_a 26 -> 9 -> 26: the audio and cross-modal tables and the V^T layouts change and come back; the bits of the first run return."""
    inp = ref.make_inputs(1, seed=1, **NARROW)
    first = run(gpu_ctx, inp)
    short = run(gpu_ctx, inp, T_a=9)
    again = run(gpu_ctx, inp)
    assert short[1].shape[1] == 9 and np.isfinite(short[0]).all() and np.isfinite(short[1]).all()
    assert np.abs(short[0] - first[0]).max() > 1e-4   # fewer audio keys change the video stream through a2v
    for x, y in zip(first, again):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    small = dict(NARROW, F=1, H=4, W=4)  # another (F, H, W): the video tables are rebuilt too
    inp2 = ref.make_inputs(1, seed=3, **small)
    gv, ga = run(gpu_ctx, inp2)
    tabs = ref.tables(None, 1, 4, 4, 26, NARROW["Hv"], NARROW["Ha"])
    fv, fa = ref.forward(stack["w"], L_NARROW, inp2, tabs)
    assert ref.rel_l2(gv, fv) <= 1e-2 and ref.rel_l2(ga, fa) <= 1e-2


def test_safetensors_round_trip_in_the_checkpoint_spelling(gpu_ctx, ltx, stack, tmp_path):
    """Exported weights -> a file under transformer_blocks.3. / .4. in the checkpoint's spelling (to_out.0, norm_q, ff.net.0.proj, ...)
    plus RMSNorm weights the stack has no use for and a block the load must ignore -> ltx_dual_blocks_load(first_block = 3): equal
    forward bits, the expected load report; a file lacking one tensor is weightLoadingFailed and leaves no stack."""
    from safetensors.numpy import save_file

    inp = ref.make_inputs(1, seed=1, **NARROW)
    want = run(gpu_ctx, inp)
    n_params = len(stack["w"])
    tensors = {}
    for k, v in stack["w"].items():
        i, rest = k[len("transformer_blocks."):].split(".", 1)
        tensors[ref.checkpoint_spelling(f"transformer_blocks.{int(i) + 3}.{rest}")] = np.ascontiguousarray(v, dtype=np.float32)
    extra = ["norm1", "audio_norm2", "audio_to_video_norm"]
    for n in extra:
        tensors[f"transformer_blocks.3.{n}.weight"] = np.ones(512 if "audio_norm" not in n else 256, np.float32)
    tensors["transformer_blocks.5.attn1.to_q.weight"] = np.zeros((512, 512), np.float32)  # outside [3, 5): not this stack's
    tensors["proj_out.weight"] = np.zeros((128, 512), np.float32)
    path = tmp_path / "dual.safetensors"
    save_file(tensors, str(path))
    try:
        gpu_ctx.dual_blocks_load(path, narrow_cfg(ltx), first_block=3)
        assert gpu_ctx.load_report() == {"loaded": n_params, "missing": 0, "unmatched": len(extra)}
        for k in ("transformer_blocks.1.audio_ff.project_out.weight", "transformer_blocks.0.scale_shift_table_a2v_ca_audio",
                  "transformer_blocks.1.attn1.to_k.bias", "transformer_blocks.0.video_to_audio_attn.k_norm.weight"):
            assert np.array_equal(gpu_ctx.dual_blocks_export_param(k), stack["w"][k].ravel()), k
        got = run(gpu_ctx, inp)
        for x, y in zip(want, got):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        # one tensor missing: the documented case, and the slot is empty afterwards
        lacking = dict(tensors)
        del lacking["transformer_blocks.4.audio_attn2.to_out.0.bias"]
        bad = tmp_path / "lacking.safetensors"
        save_file(lacking, str(bad))
        with pytest.raises(ltx.LTXError, match="audio_attn2.to_out.bias") as e:
            gpu_ctx.dual_blocks_load(bad, narrow_cfg(ltx), first_block=3)
        assert e.value.case == "weightLoadingFailed"
        xv = torch.full((1, 96, 512), 7.0, device="cuda")
        with pytest.raises(ltx.LTXError, match=NOT_LOADED) as e:
            run_raw(gpu_ctx, inp, xv)
        assert e.value.case == "modelNotLoaded"
        assert (xv == 7.0).all()
    finally:
        stack["reload"]()


def run_raw(ctx, inp, xv, xa=None, **kw):
    xa = torch.full((inp["B"], inp["T_a"], inp["Ha"] * 64), 7.0, device="cuda") if xa is None else xa
    ctx.dual_blocks_forward_dev(xv, xa, dev(inp["context_video"], True), dev(inp["context_audio"], True), dev(inp["temb_video"]),
                                dev(inp["temb_audio"]), dev(inp["cross_video_ss"]), dev(inp["cross_audio_ss"]), inp["F"], inp["H"], inp["W"], **kw)
    return xa


def test_error_paths_report_the_documented_case_and_write_nothing(gpu_ctx, ltx, stack):
    inp = ref.make_inputs(1, seed=1, **NARROW)
    xv = torch.full((1, 96, 512), 7.0, device="cuda")
    xa = torch.full((1, 26, 256), 7.0, device="cuda")
    try:
        gpu_ctx.dual_blocks_unload()
        with pytest.raises(ltx.LTXError, match=NOT_LOADED) as e:   # forward before load
            run_raw(gpu_ctx, inp, xv, xa)
        assert e.value.case == "modelNotLoaded"
        with pytest.raises(ltx.LTXError, match=NOT_LOADED):
            gpu_ctx.dual_blocks_export_param("transformer_blocks.0.scale_shift_table")
        stack["reload"]()
        with pytest.raises(ltx.LTXError, match="struct_size") as e:  # a struct that ends before cross_audio_ss
            run_raw(gpu_ctx, inp, xv, xa, struct_size=64)
        assert e.value.case == "invalidConfiguration"
        with pytest.raises(ltx.LTXError, match="T_a=0") as e:
            run_raw(gpu_ctx, inp, xv, xa, T_a=0)
        assert e.value.case == "invalidConfiguration"
        with pytest.raises(ltx.LTXError, match="phase_mask") as e:
            run_raw(gpu_ctx, inp, xv, xa, phase_mask=0x100)
        assert e.value.case == "invalidConfiguration"
        torch.cuda.synchronize()
        assert (xv == 7.0).all() and (xa == 7.0).all(), "a refused forward wrote a stream"
        # dims that are not heads x 128 / heads x 64: refused, and (as every replace) the slot is empty afterwards
        for bad in (dict(video_dim=500), dict(audio_dim=250), dict(video_context_dim=100)):
            with pytest.raises(ltx.LTXError) as e:
                gpu_ctx.dual_blocks_init_synthetic(narrow_cfg(ltx, **bad), seed=1)
            assert e.value.case == "invalidConfiguration", bad
        with pytest.raises(ltx.LTXError, match=NOT_LOADED):
            run_raw(gpu_ctx, inp, xv, xa)
        with pytest.raises(ltx.LTXError) as e:
            gpu_ctx.dual_blocks_load("/nonexistent/dual.safetensors", narrow_cfg(ltx))
        assert e.value.case == "fileNotFound"
        assert (xv == 7.0).all() and (xa == 7.0).all()
    finally:
        stack["reload"]()


def test_lifecycle(gpu_ctx, ltx, stack):
    """init -> forward -> replace -> forward -> unload -> "not loaded", as test_model_lifecycle_gpu.py does for the other slots."""
    inp = ref.make_inputs(1, seed=1, **NARROW)
    try:
        gpu_ctx.dual_blocks_init_synthetic(narrow_cfg(ltx), seed=31)
        a = run(gpu_ctx, inp)
        gpu_ctx.dual_blocks_init_synthetic(narrow_cfg(ltx), seed=33)   # replace: other weights, other result
        b = run(gpu_ctx, inp)
        assert np.isfinite(b[0]).all() and np.abs(a[0] - b[0]).max() > 1e-3 and np.abs(a[1] - b[1]).max() > 1e-3
        gpu_ctx.dual_blocks_init_synthetic(narrow_cfg(ltx), seed=31)   # and back: the first bits
        c = run(gpu_ctx, inp)
        for x, y in zip(a, c):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        gpu_ctx.dual_blocks_unload()
        gpu_ctx.dual_blocks_unload()   # unloading an empty slot is LTX_OK
        with pytest.raises(ltx.LTXError, match=NOT_LOADED) as e:
            run(gpu_ctx, inp)
        assert e.value.case == "modelNotLoaded"
    finally:
        stack["reload"]()


def test_phase_mask_runs_single_phases(gpu_ctx, stack):
    """The measurement seam: each phase alone touches only its own stream; all eight bits = no mask."""
    inp = ref.make_inputs(1, seed=1, **NARROW)
    full = run(gpu_ctx, inp)
    for x, y in zip(full, run(gpu_ctx, inp, phase_mask=0xff)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    for p, name in enumerate(ref.PHASES, 1):
        gv, ga = run(gpu_ctx, inp, phase_mask=1 << (p - 1))
        moved_v, moved_a = np.abs(gv - inp["x_video"]).max() > 0, np.abs(ga - inp["x_audio"]).max() > 0
        assert (moved_v, moved_a) == (name in ref.VIDEO_PHASES, name in ref.AUDIO_PHASES), name
