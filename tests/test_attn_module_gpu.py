"""LTXAttention at head dim 64 as a loadable module (csrc/attn_module.cpp) against the numpy reference of tests/helpers/attn64_ref.py
on the module's own exported weights: the four uses the dual block makes of it (audio self, audio text cross, a2v, v2a), one
full-width case, the `kPe ?? pe` rule, a safetensors round trip and the error paths. Bound: the project's module-level bound,
rel-L2 <= 1e-2 and cosine >= 0.9995 against the f32 reference on the UNROUNDED f32 inputs."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import attn64_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
HEADS, INNER = 4, 256
VIDEO_FHW = (2, 6, 8)  # 96 video tokens
T_V, T_A = 96, 26


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def weights(ctx, index, heads, Dq, Dc):
    shapes = {"to_q.weight": (heads * 64, Dq), "to_k.weight": (heads * 64, Dc), "to_v.weight": (heads * 64, Dc), "to_out.weight": (Dq, heads * 64)}
    return {n: ctx.attn_module_export_param(index, n).reshape(shapes.get(n, (-1,))) for n in ref.PARAMS}


def check(got, want):
    g, w = got.astype(np.float64).ravel(), want.astype(np.float64).ravel()
    rel = np.linalg.norm(g - w) / np.linalg.norm(w)
    cos = float(g @ w / (np.linalg.norm(g) * np.linalg.norm(w)))
    print(f"rel-L2 {rel:.3e} cosine {cos:.6f}")
    assert np.isfinite(got).all()
    assert rel <= 1e-2, rel
    assert cos >= 0.9995, cos


@pytest.fixture(scope="module")
def tables(ltx):
    """(cos, sin) host and device tables of the audio positions and of the video tokens' temporal positions, at INNER = 256."""
    a = ltx.rope_tables_positions(ltx.audio_positions(T_A), INNER)
    v = ltx.rope_tables_positions(ltx.video_temporal_positions(*VIDEO_FHW), INNER)
    return {"audio": a, "video": v, "audio_dev": tuple(dev(t) for t in a), "video_dev": tuple(dev(t) for t in v)}


def run(ctx, index, x, context=None, q_tables=None, k_tables=None, bias=None, context_bf16=False):
    xd = dev(x)
    cd = None if context is None else (dev(context).to(torch.bfloat16) if context_bf16 else dev(context))
    bd = None if bias is None else dev(bias)
    out = torch.empty(x.shape, device="cuda", dtype=torch.float32)
    ctx.attn_module_forward_dev(index, xd, out, cd, q_tables, k_tables, bd)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_audio_self_attention(gpu_ctx, tables):
    gpu_ctx.attn_module_init_synthetic(0, 256, 0, HEADS, seed=11)
    rng = np.random.default_rng(1)
    x = rng.standard_normal((1, T_A, 256)).astype(np.float32)
    got = run(gpu_ctx, 0, x, q_tables=tables["audio_dev"])
    check(got, ref.module_forward(weights(gpu_ctx, 0, HEADS, 256, 256), x, HEADS, q_tables=tables["audio"]))


def test_audio_text_cross_attention(gpu_ctx, oracle):
    """bf16 context, a third of the keys masked, no RoPE; two batch elements."""
    gpu_ctx.attn_module_init_synthetic(1, 256, 256, HEADS, seed=12)
    rng = np.random.default_rng(2)
    B, Tk = 2, 70
    x = rng.standard_normal((B, T_A, 256)).astype(np.float32)
    context = oracle.bf16_round(rng.standard_normal((B, Tk, 256)).astype(np.float32))
    m = (rng.random((B, Tk)) >= 1.0 / 3.0).astype(np.float32)
    m[:, 0] = 1
    bias = ((1 - m) * np.float32(-10000.0)).astype(np.float32)
    got = run(gpu_ctx, 1, x, context=context, bias=bias, context_bf16=True)
    check(got, ref.module_forward(weights(gpu_ctx, 1, HEADS, 256, 256), x, HEADS, context=context, bias=bias, kv_bf16=True))


def test_a2v_cross_modal_attention(gpu_ctx, tables):
    """Video queries (512 wide) over audio keys: video-temporal tables on q, audio tables on k."""
    gpu_ctx.attn_module_init_synthetic(2, 512, 256, HEADS, seed=13)
    rng = np.random.default_rng(3)
    x = rng.standard_normal((1, T_V, 512)).astype(np.float32)
    context = rng.standard_normal((1, T_A, 256)).astype(np.float32)
    got = run(gpu_ctx, 2, x, context=context, q_tables=tables["video_dev"], k_tables=tables["audio_dev"])
    check(got, ref.module_forward(weights(gpu_ctx, 2, HEADS, 512, 256), x, HEADS, context=context, q_tables=tables["video"], k_tables=tables["audio"]))


def test_v2a_cross_modal_attention(gpu_ctx, tables):
    """Audio queries over video keys (512 wide): the same tables, swapped."""
    gpu_ctx.attn_module_init_synthetic(3, 256, 512, HEADS, seed=14)
    rng = np.random.default_rng(4)
    x = rng.standard_normal((1, T_A, 256)).astype(np.float32)
    context = rng.standard_normal((1, T_V, 512)).astype(np.float32)
    got = run(gpu_ctx, 3, x, context=context, q_tables=tables["audio_dev"], k_tables=tables["video_dev"])
    w = weights(gpu_ctx, 3, HEADS, 256, 512)
    want = ref.module_forward(w, x, HEADS, context=context, q_tables=tables["audio"], k_tables=tables["video"])
    check(got, want)


def test_full_width_a2v_routes_the_real_gemm_shapes(gpu_ctx, ltx):
    """32 heads, query_dim 4096, context_dim 2048 (LTXConfig.swift:134-135), 192 video tokens of (F, H, W) = (4, 6, 8) over 26 audio tokens."""
    heads, Dq, Dc, fhw = 32, 4096, 2048, (4, 6, 8)
    gpu_ctx.attn_module_init_synthetic(0, Dq, Dc, heads, seed=21)
    try:
        qt = ltx.rope_tables_positions(ltx.video_temporal_positions(*fhw), heads * 64)
        kt = ltx.rope_tables_positions(ltx.audio_positions(T_A), heads * 64)
        rng = np.random.default_rng(5)
        x = rng.standard_normal((1, 192, Dq)).astype(np.float32)
        context = rng.standard_normal((1, T_A, Dc)).astype(np.float32)
        got = run(gpu_ctx, 0, x, context=context, q_tables=tuple(dev(t) for t in qt), k_tables=tuple(dev(t) for t in kt))
        check(got, ref.module_forward(weights(gpu_ctx, 0, heads, Dq, Dc), x, heads, context=context, q_tables=qt, k_tables=kt))
    finally:
        gpu_ctx.attn_module_unload(0)


@pytest.mark.parametrize("fhw,instance", [((4, 10, 20), 256), ((2, 10, 20), 128)])
def test_full_width_cross_attention_on_the_larger_kernel_instances(gpu_ctx, ltx, fhw, instance):
    """800 and 400 video-side queries on 32 heads against 26 keys with a key bias: 4 x 32 workgroups of 256 queries, and 4 x 32 of
    128 - the two instances of the attention kernel that the cases above (at most 192 queries) do not launch from the module."""
    heads, Dq, Dc = 32, 4096, 2048
    Tq = fhw[0] * fhw[1] * fhw[2]
    assert gpu_ctx.attention_hd_workgroup_queries(1, heads, Tq) == instance
    gpu_ctx.attn_module_init_synthetic(0, Dq, Dc, heads, seed=22)
    try:
        qt = ltx.rope_tables_positions(ltx.video_temporal_positions(*fhw), heads * 64)
        kt = ltx.rope_tables_positions(ltx.audio_positions(T_A), heads * 64)
        rng = np.random.default_rng(8 + instance)
        x = rng.standard_normal((1, Tq, Dq)).astype(np.float32)
        context = rng.standard_normal((1, T_A, Dc)).astype(np.float32)
        m = (rng.random((1, T_A)) >= 1.0 / 3.0).astype(np.float32)
        m[:, 0] = 1
        bias = ((1 - m) * np.float32(-10000.0)).astype(np.float32)
        got = run(gpu_ctx, 0, x, context=context, q_tables=tuple(dev(t) for t in qt), k_tables=tuple(dev(t) for t in kt), bias=bias)
        check(got, ref.module_forward(weights(gpu_ctx, 0, heads, Dq, Dc), x, heads, context=context, q_tables=qt, k_tables=kt, bias=bias))
    finally:
        gpu_ctx.attn_module_unload(0)


def test_key_tables_default_to_the_query_tables(gpu_ctx, tables):
    """`kPe ?? pe`: only q tables = the same tables for q and k, bit for bit; different key tables change the result."""
    gpu_ctx.attn_module_init_synthetic(0, 256, 0, HEADS, seed=11)
    rng = np.random.default_rng(6)
    x = rng.standard_normal((2, T_A, 256)).astype(np.float32)
    a = run(gpu_ctx, 0, x, q_tables=tables["audio_dev"])
    b = run(gpu_ctx, 0, x, q_tables=tables["audio_dev"], k_tables=tables["audio_dev"])
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    c = run(gpu_ctx, 0, x, q_tables=tables["audio_dev"], k_tables=tuple(t[:T_A].contiguous() for t in tables["video_dev"]))
    assert np.abs(a - c).max() > 1e-4
    d = run(gpu_ctx, 0, x)
    assert np.abs(a - d).max() > 1e-4


def test_load_round_trip(gpu_ctx, ltx, tables, tmp_path):
    """Exported weights -> safetensors under a block-style prefix (the checkpoint's spelling: to_out.0, norm_q, norm_k) -> another
    index: the forward bits are equal."""
    from safetensors.numpy import save_file

    gpu_ctx.attn_module_init_synthetic(2, 512, 256, HEADS, seed=13)
    w = weights(gpu_ctx, 2, HEADS, 512, 256)
    prefix = "transformer_blocks.0.audio_to_video_attn."
    spell = {"to_out.weight": "to_out.0.weight", "to_out.bias": "to_out.0.bias", "q_norm.weight": "norm_q.weight", "k_norm.weight": "norm_k.weight"}
    path = tmp_path / "attn.safetensors"
    save_file({prefix + spell.get(n, n): np.ascontiguousarray(v, dtype=np.float32) for n, v in w.items()}, str(path))
    gpu_ctx.attn_module_load(1, path, prefix, HEADS)
    assert gpu_ctx.load_report() == {"loaded": 10, "missing": 0, "unmatched": 0}
    for n, v in w.items():
        assert np.array_equal(gpu_ctx.attn_module_export_param(1, n), v.ravel()), n
    rng = np.random.default_rng(7)
    x = rng.standard_normal((1, T_V, 512)).astype(np.float32)
    context = rng.standard_normal((1, T_A, 256)).astype(np.float32)
    a = run(gpu_ctx, 2, x, context=context, q_tables=tables["video_dev"], k_tables=tables["audio_dev"])
    b = run(gpu_ctx, 1, x, context=context, q_tables=tables["video_dev"], k_tables=tables["audio_dev"])
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # a head count whose inner dim does not match the file: refused, and the index stays as it was
    with pytest.raises(ltx.LTXError, match="inner dim 256") as e:
        gpu_ctx.attn_module_load(1, path, prefix, 8)
    assert e.value.case == "invalidConfiguration"
    with pytest.raises(ltx.LTXError) as e:
        gpu_ctx.attn_module_load(1, path, "transformer_blocks.1.audio_to_video_attn.", HEADS)
    assert e.value.case == "weightLoadingFailed"


def test_error_paths_report_before_any_launch(gpu_ctx, ltx, tables):
    gpu_ctx.attn_module_unload(3)
    x = torch.zeros((1, T_A, 256), device="cuda")
    out = torch.full((1, T_A, 256), 7.0, device="cuda")
    with pytest.raises(ltx.LTXError, match="attention module not loaded") as e:
        gpu_ctx.attn_module_forward_dev(3, x, out)
    assert e.value.case == "modelNotLoaded"
    with pytest.raises(ltx.LTXError, match="index 4") as e:
        gpu_ctx.attn_module_forward_dev(4, x, out)
    assert e.value.case == "invalidConfiguration"
    # key tables shorter than Tk: a v2a module given the audio tables (26 rows) for its 96 video keys
    gpu_ctx.attn_module_init_synthetic(3, 256, 512, HEADS, seed=14)
    context = torch.zeros((1, T_V, 512), device="cuda")
    with pytest.raises(ltx.LTXError, match="key RoPE tables have 26 rows for Tk = 96") as e:
        gpu_ctx.attn_module_forward_dev(3, x, out, context, tables["audio_dev"], tables["audio_dev"])
    assert e.value.case == "invalidConfiguration"
    with pytest.raises(ltx.LTXError, match="key RoPE tables have 26 rows for Tk = 96"):
        gpu_ctx.attn_module_forward_dev(3, x, out, context, tables["audio_dev"])  # `kPe ?? pe` needs Tk rows of q's tables
    with pytest.raises(ltx.LTXError, match="query RoPE tables have 26 rows for Tq = 27"):
        gpu_ctx.attn_module_forward_dev(3, torch.zeros((1, 27, 256), device="cuda"), torch.empty((1, 27, 256), device="cuda"), context,
                                        tables["audio_dev"], tables["video_dev"])
    torch.cuda.synchronize()
    assert (out == 7.0).all(), "a refused forward wrote its output"
    with pytest.raises(ltx.LTXError) as e:
        gpu_ctx.attn_module_init_synthetic(3, 250, 0, HEADS)
    assert e.value.case == "invalidConfiguration"
    for i in range(4):
        gpu_ctx.attn_module_unload(i)
