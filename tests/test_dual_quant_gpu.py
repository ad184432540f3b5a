"""The quantised dual video + audio model (dual_model_quantize, csrc/dual_model.cpp; reference quantize(model: ltx2, groupSize: 64,
bits: 8 | 4), LTXPipeline.swift:487-492) on the narrow model of tests/test_dual_model_gpu.py (4 x 128 / 4 x 64, L 2, caption 256,
(F, H, W) = (2, 6, 8), T_a 26, S 70), its weights exported, boosted and written with that file's helpers.

wq = the same weights with every 2-D `.weight` replaced by oracle.bf16_round(oracle.fake_quant(w, bits)): what a quantised Linear
computes with. (a) storage and the memory books; (b) with option "qb_off" = 1 (every GEMM through the scratch matrix) the quantised
model's forward and timestep path are BIT-EQUAL to a bf16 model loaded from a checkpoint of wq - one test for the quantisation rule,
every Linear, the fused q|k row views and the codes gemv inside the model; (c) default options at 8 bits (codes read inside the few-row
GEMMs) against the f32 reference on wq with the bf16 model's own bounds; (d) int4 is closer to the reference on wq than to the one on
the bf16 weights; (e) the joint loop; (f) lifecycle."""
import numpy as np
import pytest
import torch

from test_dual_model_gpu import EMBED_OUTS, L_NARROW, NARROW, bits as ubits, check, embed, export_weights, narrow_cfg, ref, run, write_checkpoint
from test_dual_denoise_gpu import DISTILLED, dd, run_dev, same_bits

pytestmark = pytest.mark.gpu
DV, DA = NARROW["Hv"] * 128, NARROW["Ha"] * 64
STORAGE_KEYS = ("transformer_blocks.1.attn1.to_q.weight", "transformer_blocks.1.attn1.to_k.weight", "transformer_blocks.0.audio_attn1.to_k.weight",
                "transformer_blocks.0.audio_to_video_attn.to_v.weight", "transformer_blocks.1.video_to_audio_attn.to_out.weight",
                "transformer_blocks.1.ff.project_out.weight", "transformer_blocks.0.audio_ff.project_in.proj.weight", "adaln_single.linear.weight",
                "av_ca_v2a_gate_adaln_single.emb.linear_1.weight", "caption_projection.linear_1.weight", "audio_proj_out.weight", "patchify_proj.weight")
F32_KEYS = ("adaln_single.linear.bias", "scale_shift_table", "transformer_blocks.1.attn1.q_norm.weight", "transformer_blocks.0.audio_ff.project_out.bias",
            "transformer_blocks.1.scale_shift_table_a2v_ca_audio", "transformer_blocks.0.attn1.to_k.bias")


def is_linear(k, v):
    return k.endswith(".weight") and v.ndim == 2


@pytest.fixture(scope="module")
def base(gpu_ctx, ltx, oracle, tmp_path_factory):
    """The boosted narrow weights w, wq at 8 and 4 bits, and a checkpoint of each. Computed once, shared, left unchanged."""
    d = tmp_path_factory.mktemp("dual_quant")
    cfg = narrow_cfg(ltx)
    gpu_ctx.dual_model_init_synthetic(cfg, seed=41)
    w = ref.boost(export_weights(gpu_ctx, L_NARROW, NARROW["Hv"], NARROW["Ha"], NARROW["caption_channels"]), NARROW["Hv"], NARROW["Ha"])
    write_checkpoint(d / "bf16.safetensors", w)
    wq = {}
    for b in (8, 4):
        wq[b] = {k: oracle.bf16_round(oracle.fake_quant(v, b)) if is_linear(k, v) else v for k, v in w.items()}
        write_checkpoint(d / f"wq{b}.safetensors", wq[b])
    yield {"w": w, "wq": wq, "cfg": cfg, "bf16": d / "bf16.safetensors", "wq_path": {b: d / f"wq{b}.safetensors" for b in (8, 4)},
           "inp": {B: ref.make_inputs(B, seed=B, **NARROW) for B in (1, 2)}}
    gpu_ctx.set_option("qb_off", 0)
    gpu_ctx.dual_model_unload()


@pytest.mark.parametrize("nbits", [8, 4])
def test_a_storage_and_memory_books(gpu_ctx, base, nbits):
    w, wq = base["w"], base["wq"][nbits]
    gpu_ctx.dual_model_load(base["bf16"], base["cfg"])
    mem0 = gpu_ctx.dual_model_memory_info()
    f32_before = {k: gpu_ctx.dual_model_export_param(k) for k in F32_KEYS}
    lin = {k: v for k, v in w.items() if is_linear(k, v)}
    n_weights = sum(v.size for v in lin.values())
    assert mem0["quantised_weights"] == 0 and mem0["scratch"] == 0 and mem0["bf16_weights"] >= 2 * n_weights and mem0["other"] > 0, mem0
    gpu_ctx.dual_model_quantize(nbits)
    mem1 = gpu_ctx.dual_model_memory_info()
    print(f"{nbits} bits: before {mem0}, after {mem1}")
    for k in STORAGE_KEYS:
        got = gpu_ctx.dual_model_export_param(k).reshape(wq[k].shape)
        assert np.array_equal(ubits(got), ubits(wq[k])), (k, float(np.abs(got - wq[k]).max()))
        assert not np.array_equal(got, w[k]), k  # and the quantisation is visible
    for k in F32_KEYS:
        assert np.array_equal(ubits(gpu_ctx.dual_model_export_param(k)), ubits(f32_before[k])), k
    counted = sum(v.size * nbits // 8 + v.size // 64 * 4 for v in lin.values())
    # a fused self-attention q|k matrix is ONE Linear of [2 inner][Dq]
    largest = max(max(v.size for v in lin.values()), 2 * DV * DV)
    assert mem1["bf16_weights"] == 0, mem1
    assert counted <= mem1["quantised_weights"] <= counted + 256 * 3 * len(lin), (mem1, counted)
    assert mem1["scratch"] == largest * 2, (mem1, largest)
    assert mem1["other"] == mem0["other"], (mem0, mem1)


@pytest.mark.parametrize("nbits", [8, 4])
def test_b_the_forward_is_the_dequantised_models_forward(gpu_ctx, base, nbits):
    """qb_off = 1: velocities at B = 1 and B = 2 (masked) and the six timestep-path outputs (grouped, ungrouped and the composed
    de-quantise + gemv route) are bit-equal to the bf16 model of wq."""
    gpu_ctx.dual_model_load(base["wq_path"][nbits], base["cfg"])
    want = {B: (run(gpu_ctx, base["inp"][B]), embed(gpu_ctx, base["inp"][B], DV, DA, False)) for B in (1, 2)}
    gpu_ctx.dual_model_load(base["bf16"], base["cfg"])
    gpu_ctx.dual_model_quantize(nbits)
    try:
        gpu_ctx.set_option("qb_off", 1)
        for B in (1, 2):
            got = run(gpu_ctx, base["inp"][B])
            for name, g, x in zip(("video", "audio"), got, want[B][0]):
                assert np.isfinite(g).all()
                assert np.array_equal(ubits(g), ubits(x)), (nbits, B, name, float(np.abs(g - x).max()))
            for name, g, x in zip(("video", "audio"), run(gpu_ctx, base["inp"][B], ungrouped=True), want[B][0]):
                assert np.array_equal(ubits(g), ubits(x)), (nbits, B, name, "ungrouped")
            for mode in (0, 1, 2):
                e = embed(gpu_ctx, base["inp"][B], DV, DA, mode)
                for k in EMBED_OUTS:
                    assert np.array_equal(ubits(e[k]), ubits(want[B][1][k])), (nbits, B, k, mode)
    finally:
        gpu_ctx.set_option("qb_off", 0)


@pytest.fixture(scope="module")
def refs8(base):
    """f32 reference and CPU rounding-point replay on wq (8 bits), B = 1 and 2: once."""
    wq = base["wq"][8]
    return {B: (ref.forward(wq, L_NARROW, base["inp"][B]), ref.forward(wq, L_NARROW, base["inp"][B], replay=True)) for B in (1, 2)}


def test_c_default_options_at_8_bits(gpu_ctx, base, refs8):
    """Codes read inside the few-row GEMMs: two forwards bit-identical, and the bf16 model's own check against the reference on wq."""
    gpu_ctx.dual_model_load(base["bf16"], base["cfg"], quant_bits=8)
    for B in (1, 2):
        got, again = run(gpu_ctx, base["inp"][B]), run(gpu_ctx, base["inp"][B])
        for g, a in zip(got, again):
            assert np.array_equal(ubits(g), ubits(a))
        (fv, fa), (rv, ra) = refs8[B]
        check(f"8 bits B={B} video", got[0], fv, rv)
        check(f"8 bits B={B} audio", got[1], fa, ra)


def test_c_video_through_the_scratch_and_audio_through_codes_in_one_forward(gpu_ctx, base):
    """(F, H, W) = (2, 12, 16): 384 video rows are beyond the few-row GEMM (256), 26 audio rows are inside it."""
    inp = ref.make_inputs(1, seed=9, **dict(NARROW, H=12, W=16))
    gpu_ctx.dual_model_load(base["bf16"], base["cfg"], quant_bits=8)
    gv, ga = run(gpu_ctx, inp)
    wq = base["wq"][8]
    fv, fa = ref.forward(wq, L_NARROW, inp)
    rv, ra = ref.forward(wq, L_NARROW, inp, replay=True)
    check("8 bits 384 tokens video", gv, fv, rv)
    check("8 bits 384 tokens audio", ga, fa, ra)


def test_d_int4_follows_the_quantised_weights(gpu_ctx, base):
    inp = base["inp"][1]
    gpu_ctx.dual_model_load(base["bf16"], base["cfg"], quant_bits=4)
    got = run(gpu_ctx, inp)
    on_wq, on_w = ref.forward(base["wq"][4], L_NARROW, inp), ref.forward(base["w"], L_NARROW, inp)
    for name, g, q, b in zip(("video", "audio"), got, on_wq, on_w):
        rq, rb = ref.rel_l2(g, q), ref.rel_l2(g, b)
        print(f"int4 {name}: rel-L2 against the reference on wq {rq:.3e}, on the bf16 weights {rb:.3e}")
        assert np.isfinite(g).all() and rq < rb, (name, rq, rb)


def test_e_the_joint_loop_runs_unchanged_on_a_quantised_model(gpu_ctx, base):
    """3 distilled steps, masked, text cache on: the quantised model (qb_off = 1) against the bf16 model of wq, one cache fill."""
    case = dd.make_case(cfg=False, seed=1, **NARROW)
    gpu_ctx.dual_model_load(base["wq_path"][8], base["cfg"])
    wv, wa, _ = run_dev(gpu_ctx, case, DISTILLED, text_cache=1)
    gpu_ctx.dual_model_load(base["bf16"], base["cfg"], quant_bits=8)
    try:
        gpu_ctx.set_option("qb_off", 1)
        before = gpu_ctx.dual_model_text_cache_info()["builds"]
        gv, ga, _ = run_dev(gpu_ctx, case, DISTILLED, text_cache=1)
        after = gpu_ctx.dual_model_text_cache_info()
    finally:
        gpu_ctx.set_option("qb_off", 0)
    assert after["builds"] == before + 1 and (after["B"], after["S"]) == (1, NARROW["S"])
    assert np.isfinite(gv).all() and not same_bits(gv, case["video_latent"])
    assert same_bits(gv, wv), float(np.abs(gv - wv).max())
    assert same_bits(ga, wa), float(np.abs(ga - wa).max())


def test_f_lifecycle(gpu_ctx, ltx, base):
    inp = base["inp"][1]
    ctxs = [torch.from_numpy(np.ascontiguousarray(inp[k], dtype=np.float32)).cuda().to(torch.bfloat16) for k in ("video_context", "audio_context")]
    gpu_ctx.dual_model_load(base["bf16"], base["cfg"])
    gpu_ctx.dual_model_prepare_text(*ctxs)
    assert gpu_ctx.dual_model_text_cache_info()["B"] == 1
    for bad, match in ((dict(bits=3), "3 bits"), (dict(bits=8, group_size=32), "group size 32")):
        with pytest.raises(ltx.LTXError, match=match) as e:
            gpu_ctx.dual_model_quantize(**bad)
        assert e.value.case == "invalidConfiguration"
    assert gpu_ctx.dual_model_memory_info()["quantised_weights"] == 0 and gpu_ctx.dual_model_text_cache_info()["B"] == 1  # a refusal changed nothing
    gpu_ctx.dual_model_quantize(8)
    info = gpu_ctx.dual_model_text_cache_info()
    assert (info["B"], info["S"]) == (0, 0), info  # quantising dropped the filled cache
    out = (torch.full((1, 96, 128), 7.0, device="cuda"), torch.full((1, 26, 128), 7.0, device="cuda"))
    with pytest.raises(ltx.LTXError, match="prepare_text") as e:
        run(gpu_ctx, inp, out=out, text_cache=1)
    assert e.value.case == "invalidConfiguration"
    torch.cuda.synchronize()
    assert (out[0] == 7.0).all() and (out[1] == 7.0).all(), "a refused forward wrote"
    with pytest.raises(ltx.LTXError, match="already quantised") as e:
        gpu_ctx.dual_model_quantize(8)
    assert e.value.case == "invalidConfiguration"
    first = run(gpu_ctx, inp)
    mem_q = gpu_ctx.dual_model_memory_info()
    # load(..., quant_bits=8) is load + quantise
    gpu_ctx.dual_model_load(base["bf16"], base["cfg"], quant_bits=8)
    assert gpu_ctx.dual_model_memory_info() == mem_q
    for x, y in zip(first, run(gpu_ctx, inp)):
        assert np.array_equal(ubits(x), ubits(y))
    # loading afterwards gives a bf16 model again
    gpu_ctx.dual_model_load(base["bf16"], base["cfg"])
    mem = gpu_ctx.dual_model_memory_info()
    assert mem["quantised_weights"] == 0 and mem["scratch"] == 0 and mem["bf16_weights"] > 0, mem
    k = "transformer_blocks.1.attn1.to_k.weight"
    assert np.array_equal(gpu_ctx.dual_model_export_param(k), base["w"][k].ravel())
    gpu_ctx.dual_model_quantize(4)
    gpu_ctx.dual_model_unload()
    assert gpu_ctx.dual_model_memory_info() == {"bf16_weights": 0, "quantised_weights": 0, "scratch": 0, "other": 0}
    with pytest.raises(ltx.LTXError, match="dual transformer model not loaded"):
        gpu_ctx.dual_model_quantize(8)
