"""The outputs of the three GEMM kernels with a generated gfx950 main loop (csrc/gemm_asm_tiles.inc: 192 x 256, 192 x 384 q|k|v,
384 x 256), as one sha256 per case. tests/test_gemm_asm_family_gpu.py compares them with tests/golden/gemm_asm_family_digests.json,
which tests/golden/make_golden.py --gemm-asm-family-digests records. The rest of the suite compares these kernels with each other
(384 x 256 against 192 x 256, the fused q|k|v launch against the two launches), so a change shared by all of them shows only here.

Every input comes from numpy.random.default_rng([SEED, ...shape]); the activations and the outputs have padded leading dimensions, and
a digest covers the whole output buffer with its poisoned border. The shapes are the smallest at which each path can go wrong:

  dtl / tall   one tile and a 2 x 3 grid of tiles, with one, three and four K-tiles (both exits of a two-tile loop body), bias +
               GELU-tanh into a bf16 store and bias only into an f32 store
  qkv          one row tile with one / three K-tiles, and two batch elements of one row tile each with two column tiles
  resid        the residual + gate epilogue of the 192 x 256 kernel with a bf16 mirror: 3072 x 4096 is 256 tiles, the fewest for which
               the dense tile choice is that kernel, and the launch has no workspace, so nothing splits it
  forward      a 2-layer full-width DiT at 1536 tokens: velocity of one forward and the latents after one denoise step (the bf16-partial
               split-K store of FFN-down with the fused finish + norm, the q|k|v launch and the 384 x 256 launch in context)"""
import hashlib

import numpy as np
import torch

SEED = 20
POISON = -777.0
GELU_TANH = 1
DTL_SHAPES = [(192, 256, 64), (384, 768, 192), (192, 256, 256)]      # M, N, K; tile_cfg 75
TALL_SHAPES = [(384, 256, 64), (768, 768, 192), (384, 256, 256)]     # tile_cfg 76
QKV_SHAPES = [(192, 192, 128, 64), (192, 192, 128, 192), (384, 192, 256, 256)]   # rows, rows per batch, D, K
RESID_SHAPE = (3072, 4096, 128)
FORWARD_FHW = (4, 16, 24)


def sha(t):
    """sha256 of a device tensor's bytes, padding and border included"""
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def _bf16(x, pad=0):
    """x [r][c] rounded to bf16 in the first c columns of a [r][c + pad] device tensor; the padding holds a value that would show in
    every result if it were read"""
    buf = torch.full((x.shape[0], x.shape[1] + pad), 3.0, dtype=torch.bfloat16, device="cuda")
    buf[:, :x.shape[1]] = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).cuda()
    return buf


def _f32(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def gemm_cases(ltx, ctx, cfg, shapes):
    d = {}
    for M, N, K in shapes:
        rng = np.random.default_rng([SEED, cfg, M, N, K])
        X = _bf16(rng.standard_normal((M, K)), pad=8)
        W = _bf16(rng.standard_normal((N, K)) * 0.05)
        b = _f32(rng.standard_normal((N,)))
        for name, act, dtype in (("gelu_bf16", GELU_TANH, torch.bfloat16), ("bias_f32", 0, torch.float32)):
            buf = torch.full((M + 2, N + 8), POISON, dtype=dtype, device="cuda")
            f32 = dtype == torch.float32
            ctx._ck(ltx.lib.ltx_op_gemm_bf16(ctx._h, X.data_ptr(), X.stride(0), W.data_ptr(), W.stride(0), b.data_ptr(), M, N, K, act, cfg,
                                             buf.data_ptr() if f32 else None, buf.stride(0) if f32 else 0,
                                             None if f32 else buf.data_ptr(), 0 if f32 else buf.stride(0)))
            torch.cuda.synchronize()
            d[f"cfg{cfg}.{M}x{N}x{K}.{name}"] = sha(buf)
    return d


def qkv_cases(ctx):
    d = {}
    for rows, rpb, D, K in QKV_SHAPES:
        rng = np.random.default_rng([SEED, rows, rpb, D, K])
        X = _bf16(rng.standard_normal((rows, K)), pad=8)
        Wqk = _bf16(rng.standard_normal((2 * D, K)) * 0.05)
        Wv = _bf16(rng.standard_normal((D, K)) * 0.05)
        bqk, bv = _f32(rng.standard_normal((2 * D,))), _f32(rng.standard_normal((D,)))
        qk = torch.full((rows + 2, 2 * D + 8), POISON, dtype=torch.bfloat16, device="cuda")
        vt = torch.full(((rows // rpb) * D + 1, rpb + 4), POISON, dtype=torch.bfloat16, device="cuda")
        ctx.op_qkv_projection(X, Wqk, bqk, Wv, bv, qk, vt, rows=rows, rows_per_batch=rpb, fused=True)
        torch.cuda.synchronize()
        d[f"qkv.{rows}r{rpb}.D{D}.K{K}.qk_out"] = sha(qk)
        d[f"qkv.{rows}r{rpb}.D{D}.K{K}.vt_out"] = sha(vt)
    return d


def resid_tile_cfg(ltx):
    """what the launcher picks for the residual case on this device: the case is about the 192 x 256 kernel (75)"""
    M, N, K = RESID_SHAPE
    return ltx.gemm_dense_tile_cfg(M, N, K, flags=1 | 2 | 4, ncu=torch.cuda.get_device_properties(0).multi_processor_count)


def resid_case(ltx, ctx):
    M, N, K = RESID_SHAPE
    rng = np.random.default_rng([SEED, M, N, K])
    A = _bf16(rng.standard_normal((M, K)), pad=8)
    B = _bf16(rng.standard_normal((N, K)) * 0.05)
    bias, gate = _f32(rng.standard_normal((N,))), _f32(rng.standard_normal((N,)))
    x = torch.full((M + 2, N + 8), POISON, dtype=torch.float32, device="cuda")
    x[:M, :N] = _f32(rng.standard_normal((M, N), dtype=np.float32))
    mirror = torch.full((M + 2, N + 8), POISON, dtype=torch.bfloat16, device="cuda")
    ctx._ck(ltx.lib.ltx_op_gemm_bf16_gated_residual(ctx._h, A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), bias.data_ptr(),
                                                    gate.data_ptr(), 1.0, M, N, K, x.data_ptr(), x.stride(0), mirror.data_ptr(),
                                                    mirror.stride(0)))
    torch.cuda.synchronize()
    return {f"resid.{M}x{N}x{K}.x": sha(x), f"resid.{M}x{N}x{K}.mirror": sha(mirror)}


def two_layer_context(ltx):
    """the 2-layer full-width DiT of tests/test_gemm_tall_gpu.py"""
    ctx = ltx.Context(0)
    cfg = ltx.default_transformer_config(num_layers=2, num_attention_heads=32, cross_attention_dim=32 * 128, caption_channels=256)
    ctx.dit_init_synthetic(cfg, seed=7)
    return ctx


def forward_case(model):
    F, H, W = FORWARD_FHW
    T, S = F * H * W, 64
    rng = np.random.default_rng([SEED, T, S])
    lat = _bf16(rng.standard_normal((T, 128))).view(1, T, 128)
    cx = _bf16(rng.standard_normal((S, 256))).view(1, S, 256)
    noise = _f32(rng.standard_normal((1, 128, F, H, W)))
    ts = torch.full((1,), 0.7, dtype=torch.float32, device="cuda")
    vel = torch.empty((1, T, 128), dtype=torch.float32, device="cuda")
    model.dit_forward_dev(lat, cx, ts, None, F, H, W, vel, ctx_version=5)
    torch.cuda.synchronize()
    stepped = noise.clone()
    model.denoise_dev(stepped, np.array([1.0, 0.8], np.float32), cx, None, F, H, W, ctx_version=5)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(vel).all()) and float(vel.abs().mean()) > 0 and not torch.equal(stepped, noise)
    return {"forward.velocity": sha(vel), "forward.denoise_step": sha(stepped)}


def expected_keys():
    keys = [f"cfg{cfg}.{M}x{N}x{K}.{e}" for cfg, shapes in ((75, DTL_SHAPES), (76, TALL_SHAPES)) for M, N, K in shapes
            for e in ("gelu_bf16", "bias_f32")]
    keys += [f"qkv.{r}r{b}.D{D}.K{K}.{o}" for r, b, D, K in QKV_SHAPES for o in ("qk_out", "vt_out")]
    keys += ["resid.%dx%dx%d.%s" % (*RESID_SHAPE, o) for o in ("x", "mirror")]
    return sorted(keys + ["forward.velocity", "forward.denoise_step"])
