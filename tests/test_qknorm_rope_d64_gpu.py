"""q/k RMSNorm + split RoPE at head dim 64 (csrc/elementwise.hip, qknorm_rope_kernel<64, NP, XB>) through ltx_op_qknorm_rope_hd, against the
oracle's rms_norm + apply_split_rope. Bound: the one test_kernels_gpu.test_qknorm_rope uses, 2^-8 * max|ref| + 1e-4 (one rounding of
the result to bf16)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import attn64_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


def dev_f32(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


@pytest.mark.parametrize("out_scale", [1.0, float(ref.QUERY_PRESCALE)])
@pytest.mark.parametrize("use_rope", [True, False])
@pytest.mark.parametrize("rows", [5, 70])
@pytest.mark.parametrize("D", [128, 2048])
def test_qknorm_rope_d64(gpu_ctx, ltx, D, rows, use_rope, out_scale):
    heads = D // 64
    rng = np.random.default_rng(D + rows)
    x = (rng.standard_normal((rows, D)) * 2).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal((D,))).astype(np.float32)
    cos, sin = ltx.rope_tables_positions(ltx.audio_positions(rows), D)
    out = torch.empty((rows, D), device="cuda", dtype=torch.bfloat16)
    xd, wd, cd, sd = dev_f32(x), dev_f32(w), dev_f32(cos), dev_f32(sin)
    gpu_ctx.op_qknorm_rope_hd(xd, wd, cd if use_rope else None, sd if use_rope else None, rows, out, 64, out_scale)
    torch.cuda.synchronize()
    want = ref.qknorm_rope(x[None], w, cos if use_rope else None, sin if use_rope else None, heads, out_scale)[0]
    got = out.float().cpu().numpy()
    err, bound = np.abs(got - want).max(), 2 ** -8 * np.abs(want).max() + 1e-4
    print(f"max abs {err:.3e} bound {bound:.3e}")
    assert err <= bound


def test_rows_wrap_over_the_table_per_batch_element(gpu_ctx, ltx):
    """rows = B * T: row r uses table row r % T, and a strided input (ldx > D) is read in place."""
    B, T, D = 2, 13, 256
    rng = np.random.default_rng(1)
    x = rng.standard_normal((B * T, D + 64)).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal((D,))).astype(np.float32)
    cos, sin = ltx.rope_tables_positions(ltx.audio_positions(T), D)
    out = torch.empty((B * T, D), device="cuda", dtype=torch.bfloat16)
    xd, wd, cd, sd = dev_f32(x), dev_f32(w), dev_f32(cos), dev_f32(sin)
    gpu_ctx.op_qknorm_rope_hd(xd, wd, cd, sd, T, out, 64)
    torch.cuda.synchronize()
    want = ref.qknorm_rope(x[:, :D].reshape(B, T, D), w, cos, sin, D // 64).reshape(B * T, D)
    assert np.abs(out.float().cpu().numpy() - want).max() <= 2 ** -8 * np.abs(want).max() + 1e-4


@pytest.mark.parametrize("use_rope", [True, False])
def test_head_dim_128_through_the_new_entry_is_the_old_entry(gpu_ctx, ltx, use_rope):
    rows, D = 70, 512
    rng = np.random.default_rng(2)
    xd = dev_f32(rng.standard_normal((rows, D)))
    wd = dev_f32(1 + 0.1 * rng.standard_normal((D,)))
    cos, sin = ltx.rope_tables_1d(rows, D)
    cd, sd = (dev_f32(cos), dev_f32(sin)) if use_rope else (None, None)
    o1 = torch.empty((rows, D), device="cuda", dtype=torch.bfloat16)
    o2 = torch.empty_like(o1)
    gpu_ctx.op_qknorm_rope(xd, wd, cd, sd, rows, o1)
    gpu_ctx.op_qknorm_rope_hd(xd, wd, cd, sd, rows, o2, 128)
    torch.cuda.synchronize()
    assert torch.equal(o1.view(torch.int16), o2.view(torch.int16))
    with pytest.raises(ltx.LTXError, match="head dim 32"):
        gpu_ctx.op_qknorm_rope_hd(xd, wd, cd, sd, rows, o2, 32)
