"""The head-dim-64 flash attention kernel (csrc/attention.hip, attn64_fwd_kernel) through ltx_op_attention_hd, against an f32 softmax on
the SAME bf16 inputs. Bounds: those the head-dim-128 kernels are held to (test_kernels_gpu.test_attention_vs_f32) - max abs 2e-2,
rel-L2 1e-2, every value finite: the differences are accumulation order and the bf16 rounding of P before the PV product."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import attn64_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
SCALE = 1.0 / 8.0


def dev_bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).cuda()


def dev_f32(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def as_f32(t):
    return t.float().cpu().numpy()


def make_vt(vd, Tk):
    B, _, D = vd.shape
    ldvt = ((Tk + 63) // 64) * 64
    vt = torch.zeros((B, D, ldvt), device="cuda", dtype=torch.bfloat16)
    vt[:, :, :Tk] = vd.transpose(1, 2)
    return vt


def inputs(rng, B, H, Tq, Tk, q_scale=1.0):
    D = H * 64
    qd = dev_bf16(rng.standard_normal((B, Tq, D)) * q_scale)
    kd = dev_bf16(rng.standard_normal((B, Tk, D)))
    vd = dev_bf16(rng.standard_normal((B, Tk, D)))
    return qd, kd, vd, make_vt(vd, Tk)


def check(got, want):
    err, rel = np.abs(got - want).max(), np.linalg.norm(got - want) / np.linalg.norm(want)
    print(f"max abs {err:.3e} rel-L2 {rel:.3e}")
    assert np.isfinite(got).all()
    assert err <= 2e-2, f"max abs err {err}"
    assert rel <= 1e-2, f"rel l2 {rel}"


def key_bias(rng, B, Tk, masked_fraction):
    m = (rng.random((B, Tk)) >= masked_fraction).astype(np.float32)
    m[:, 0] = 1
    return m


# the issue's shapes, then one per workgroup size the launcher can pick that they do not reach (ltx_attention_hd_workgroup_queries:
# 128 and 256 queries per workgroup need 128 workgroups), both with ragged Tq / Tk and a second batch element
SHAPES = [(1, 1, 16, 16, 0.0), (1, 2, 64, 64, 0.0), (1, 3, 70, 130, 0.0), (2, 2, 1, 26, 0.0), (1, 4, 26, 1536, 0.0), (1, 4, 1536, 26, 0.0),
          (2, 2, 200, 1024, 0.1), (2, 32, 200, 130, 0.0), (2, 32, 300, 130, 0.0), (2, 32, 200, 70, 0.3), (2, 32, 300, 70, 0.3)]


@pytest.mark.parametrize("B,H,Tq,Tk,masked", SHAPES)
def test_attention_d64_vs_f32(gpu_ctx, B, H, Tq, Tk, masked):
    rng = np.random.default_rng(B * 1000 + H * 100 + Tq + Tk)
    qd, kd, vd, vt = inputs(rng, B, H, Tq, Tk)
    bias = (1 - key_bias(rng, B, Tk, masked)) * np.float32(-10000.0) if masked else None
    o = torch.empty((B, Tq, H * 64), device="cuda", dtype=torch.bfloat16)
    gpu_ctx.op_attention_hd(qd, kd, vt, None if bias is None else dev_f32(bias), H, o, 64, SCALE)
    torch.cuda.synchronize()
    check(as_f32(o), ref.attention_f32(as_f32(qd), as_f32(kd), as_f32(vd), H, SCALE, bias))


def test_every_workgroup_size_is_reached(gpu_ctx):
    sizes = {gpu_ctx.attention_hd_workgroup_queries(B, H, Tq) for B, H, Tq, _, _ in SHAPES}
    assert sizes == {64, 128, 256}


def test_attention_d64_one_batch_fully_masked(gpu_ctx):
    """Batch element 0 has EVERY key masked: softmax(s - 10000) = softmax(s) must come out (finite), as at head dim 128."""
    B, H, Tq, Tk = 2, 2, 200, 1024
    rng = np.random.default_rng(77)
    qd, kd, vd, vt = inputs(rng, B, H, Tq, Tk)
    m = key_bias(rng, B, Tk, 0.1)
    m[0, :] = 0
    bias = (1 - m) * np.float32(-10000.0)
    o = torch.empty((B, Tq, H * 64), device="cuda", dtype=torch.bfloat16)
    gpu_ctx.op_attention_hd(qd, kd, vt, dev_f32(bias), H, o, 64, SCALE)
    torch.cuda.synchronize()
    check(as_f32(o), ref.attention_f32(as_f32(qd), as_f32(kd), as_f32(vd), H, SCALE, bias))


@pytest.mark.parametrize("B,H,Tq,Tk,masked", [(1, 3, 70, 130, 0.0), (2, 2, 200, 1024, 0.1), (2, 32, 300, 70, 0.3)])
def test_attention_d64_prescaled_query(gpu_ctx, ltx, B, H, Tq, Tk, masked):
    """scale <= 0: Q carries (1/8) log2(e), rounded to bf16 once by its producer; the same result as scale = 1/8 on the unscaled Q,
    within the bounds above (reference: f32 softmax of the unscaled f32 Q)."""
    rng = np.random.default_rng(B * 13 + H + Tq + Tk)
    D = H * 64
    q = (rng.standard_normal((B, Tq, D)) * 1.5).astype(np.float32)
    _, kd, vd, vt = inputs(rng, B, H, Tq, Tk)
    bias = (1 - key_bias(rng, B, Tk, masked)) * np.float32(-10000.0) if masked else None
    bd = None if bias is None else dev_f32(bias)
    o = torch.empty((B, Tq, D), device="cuda", dtype=torch.bfloat16)
    gpu_ctx.op_attention_hd(dev_bf16(q * np.float32(ltx.ATTN_QUERY_PRESCALE_64)), kd, vt, bd, H, o, 64, 0.0)
    torch.cuda.synchronize()
    want = ref.attention_f32(q, as_f32(kd), as_f32(vd), H, SCALE, bias)
    check(as_f32(o), want)
    o2 = torch.empty_like(o)
    gpu_ctx.op_attention_hd(dev_bf16(q), kd, vt, bd, H, o2, 64, SCALE)
    torch.cuda.synchronize()
    check(as_f32(o2), want)
    check(as_f32(o), as_f32(o2))


def test_attention_d64_integer_layout(gpu_ctx):
    """One-hot scores: q.k is large for exactly one key per (head, query), so the softmax is a delta and O must be that key's V row
    (small integers, exact in bf16). Pins that head h reads and writes columns 64h .. 64h+63, the key permutation of the QK^T MFMA
    rows and the Vt layout, for H = 3 and ragged Tq / Tk."""
    B, H, Tq, Tk = 1, 3, 150, 200
    D = H * 64
    rng = np.random.default_rng(0)
    sel = rng.integers(0, Tk, (H, Tq))
    q = np.zeros((B, Tq, D), np.float32)
    k = np.zeros((B, Tk, D), np.float32)
    codes = rng.choice([-1.0, 1.0], (H, Tk, 64)).astype(np.float32)
    for h in range(H):
        k[0, :, h * 64:(h + 1) * 64] = codes[h]
        q[0, :, h * 64:(h + 1) * 64] = codes[h][sel[h]] * 16.0  # (q.k_sel) / 8 = 128; the others ~ N(0, 16): 7 sigma below
    v = rng.integers(-8, 9, (B, Tk, D)).astype(np.float32)
    o = torch.empty((B, Tq, D), device="cuda", dtype=torch.bfloat16)
    gpu_ctx.op_attention_hd(dev_bf16(q), dev_bf16(k), make_vt(dev_bf16(v), Tk), None, H, o, 64, SCALE)
    torch.cuda.synchronize()
    got = as_f32(o)
    for h in range(H):
        assert np.abs(got[0, :, h * 64:(h + 1) * 64] - v[0, sel[h], h * 64:(h + 1) * 64]).max() <= 1e-2, h


@pytest.mark.parametrize("B,H,Tq,Tk", [(1, 2, 70, 130), (1, 64, 200, 70), (1, 64, 300, 70), (2, 2, 70, 130), (2, 32, 300, 70)])
def test_attention_d64_rows_past_tq_keep_their_sentinel(gpu_ctx, B, H, Tq, Tk):
    """The entry's output is dense ([B][Tq][H*64], as ltx_op_attention's), so the rows after a batch element's last query are guard
    rows only behind the LAST element: the B = 1 cases put them directly behind the one block whose queries run past Tq, once per
    workgroup size (64, 128, 256 queries). With B = 2 the rows behind element 0 are element 1's: there element 1 must come out bit for
    bit as from a launch of its own, which a late stray store from element 0's last workgroup would break."""
    rng = np.random.default_rng(5)
    qd, kd, vd, vt = inputs(rng, B, H, Tq, Tk)
    D = H * 64
    buf = torch.full((B * Tq + 64, D), 7.0, device="cuda", dtype=torch.bfloat16)
    gpu_ctx.op_attention_hd(qd, kd, vt, None, H, buf[:B * Tq].view(B, Tq, D), 64, SCALE)
    torch.cuda.synchronize()
    assert (as_f32(buf[B * Tq:]) == 7.0).all(), "rows past Tq were written"
    check(as_f32(buf[:B * Tq]).reshape(B, Tq, D), ref.attention_f32(as_f32(qd), as_f32(kd), as_f32(vd), H, SCALE))
    if B > 1:
        alone = torch.full((Tq + 64, D), 7.0, device="cuda", dtype=torch.bfloat16)
        gpu_ctx.op_attention_hd(qd[1:].contiguous(), kd[1:].contiguous(), vt[1:].contiguous(), None, H, alone[:Tq].view(1, Tq, D), 64, SCALE)
        torch.cuda.synchronize()
        assert (as_f32(alone[Tq:]) == 7.0).all()
        assert torch.equal(alone[:Tq].view(torch.int16), buf[Tq:2 * Tq].view(torch.int16))


@pytest.mark.parametrize("use_bias", [False, True])
def test_head_dim_128_through_the_new_entry_is_the_old_entry(gpu_ctx, use_bias):
    B, H, Tq, Tk = 1, 2, 200, 330
    rng = np.random.default_rng(3)
    D = H * 128
    qd = dev_bf16(rng.standard_normal((B, Tq, D)))
    kd = dev_bf16(rng.standard_normal((B, Tk, D)))
    vt = make_vt(dev_bf16(rng.standard_normal((B, Tk, D))), Tk)
    bias = dev_f32((1 - key_bias(rng, B, Tk, 0.3)) * np.float32(-10000.0)) if use_bias else None
    o1 = torch.empty((B, Tq, D), device="cuda", dtype=torch.bfloat16)
    o2 = torch.empty_like(o1)
    scale = 1.0 / math.sqrt(128.0)
    gpu_ctx.op_attention(qd, kd, vt, bias, H, o1, scale)
    gpu_ctx.op_attention_hd(qd, kd, vt, bias, H, o2, 128, scale)
    torch.cuda.synchronize()
    assert torch.equal(o1.view(torch.int16), o2.view(torch.int16))


def test_other_head_dims_are_refused(gpu_ctx, ltx):
    t = torch.zeros((1, 64, 96), device="cuda", dtype=torch.bfloat16)
    with pytest.raises(ltx.LTXError, match="head dim 96") as e:
        gpu_ctx.op_attention_hd(t, t, torch.zeros((1, 96, 64), device="cuda", dtype=torch.bfloat16), None, 1, torch.empty_like(t), 96, 0.1)
    assert e.value.case == "invalidConfiguration"


@pytest.mark.parametrize("B,H,Tq,Tk", [(1, 4, 26, 1536), (2, 32, 300, 130)])
def test_attention_d64_is_repeatable(gpu_ctx, B, H, Tq, Tk):
    rng = np.random.default_rng(11)
    qd, kd, vd, vt = inputs(rng, B, H, Tq, Tk)
    o1 = torch.empty((B, Tq, H * 64), device="cuda", dtype=torch.bfloat16)
    o2 = torch.empty_like(o1)
    gpu_ctx.op_attention_hd(qd, kd, vt, None, H, o1, 64, SCALE)
    gpu_ctx.op_attention_hd(qd, kd, vt, None, H, o2, 64, SCALE)
    torch.cuda.synchronize()
    assert torch.equal(o1.view(torch.int16), o2.view(torch.int16))
