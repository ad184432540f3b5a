"""Stress, boundary and race tests of the head-dim-64 attention kernel (csrc/attention.hip, attn64_fwd_kernel) through
ltx_op_attention_hd. Reference: a float64 softmax on the SAME bf16 inputs (tests/helpers/attn64_ref.py). Bounds: those of the
head-dim-128 kernels (tests/test_kernels_gpu.py) - max abs 2e-2, rel-L2 1e-2, every value finite; 3e-2 / 1e-2 for the two ramp cases, as
there. tests/test_attn64_host.py shows without a GPU that a numpy replay of the kernel's rounding points meets these bounds on every
stress and soft-bias input used here. Every case asserts the kernel instance (queries per workgroup) it runs."""
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
SENTINEL_ROWS = 64


def dev_bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).cuda()


def dev_f32(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def as_f32(t):
    return t.float().cpu().numpy()


def make_vt(vd, Tk, pad=None):
    """V^T [B][D][roundup(Tk, 64)]; the columns past Tk are zero, or `pad` [B][D][ldvt - Tk]."""
    B, _, D = vd.shape
    ldvt = ((Tk + 63) // 64) * 64
    vt = torch.zeros((B, D, ldvt), device="cuda", dtype=torch.bfloat16)
    vt[:, :, :Tk] = vd.transpose(1, 2)
    if pad is not None:
        vt[:, :, Tk:] = pad
    return vt


def launch(ctx, q, k, v, bias, H, scale, instance, head_dim=64, vt=None):
    """One launch on bf16-valued f32 host arrays, into a buffer with sentinel rows behind it; returns the output as f32 [B,Tq,D]."""
    B, Tq, D = q.shape
    Tk = k.shape[1]
    if head_dim == 64:
        assert ctx.attention_hd_workgroup_queries(B, H, Tq) == instance, (B, H, Tq)
    vd = dev_bf16(v)
    buf = torch.full((B * Tq + SENTINEL_ROWS, D), 7.0, device="cuda", dtype=torch.bfloat16)
    ctx.op_attention_hd(dev_bf16(q), dev_bf16(k), make_vt(vd, Tk) if vt is None else vt, dev_f32(bias), H, buf[:B * Tq].view(B, Tq, D), head_dim, scale)
    torch.cuda.synchronize()
    assert (as_f32(buf[B * Tq:]) == 7.0).all(), "rows past the output were written"
    return buf[:B * Tq].view(B, Tq, D)


def check(name, got, want, bounds=(2e-2, 1e-2)):
    err, rel = ref.attention_errors(got, want)
    print(f"{name}: max abs {err:.3e} rel-L2 {rel:.3e}")
    assert np.isfinite(got).all()
    assert err <= bounds[0], f"max abs err {err}"
    assert rel <= bounds[1], f"rel l2 {rel}"


def run_case(ctx, c, instance):
    got = as_f32(launch(ctx, c.q, c.k, c.v, c.bias, c.heads, c.entry_scale, instance))
    check(c.name, got, c.reference(), c.bounds)
    return got


# ---- 1. online-softmax stress ----
@pytest.mark.parametrize("case", ref.STRESS_CASES, ids=ref.case_id)
def test_attention_d64_online_softmax_stress(gpu_ctx, case):
    """Late maximum (the running maximum moves in every tile while every third column of each wave has settled: the ballot-guarded
    rescale), scores near -224 and +224 (the unshifted exponent under- / overflows; also through the prescaled entry), and the ramp to 6
    with one dominant key in the last tile - masked in batch element 1 only, so the two elements must differ there."""
    builder, args = case
    c = builder(*args)
    got = run_case(gpu_ctx, c, args[0])
    if builder is ref.reference_maximum_case:
        row = got[:, ref.DOMINANT_QUERY, :64]
        if c.bias is None:
            assert np.array_equal(got[0], got[1])  # the same inputs in both elements
        else:
            assert np.abs(row[0] - row[1]).max() > 10 * c.bounds[0], "masking the dominant key changed nothing"


# ---- 2. race screen ----
@pytest.mark.parametrize("B,Tq,instance,masked", [(1, 100, 64, False), (2, 200, 128, False), (2, 300, 256, False), (2, 300, 256, True)])
def test_attention_d64_is_repeatable_with_cold_caches(gpu_ctx, B, Tq, instance, masked):
    """Two different inputs launched alternately, 120 times each, the caches flushed with 1 GB of other traffic every eighth launch:
    all outputs of one input are bit-identical to its first, and the first meets the reference bounds (two wrong but stable answers
    must not pass). A ring stage read before its LDS-DMA has landed would hold the OTHER input's keys, or an earlier tile's.
    Tk = 330: six tiles, the last ragged, so both stages are reused twice."""
    H, Tk = 32, 330
    assert gpu_ctx.attention_hd_workgroup_queries(B, H, Tq) == instance
    rng = np.random.default_rng(Tq + Tk + masked)
    D = H * 64
    sets, host = [], []
    for _ in range(2):
        q, k, v = (rng.standard_normal((B, T, D)).astype(np.float32) for T in (Tq, Tk, Tk))
        bias = ref.random_mask_bias(rng, B, Tk) if masked else None
        qd, kd, vd = dev_bf16(q), dev_bf16(k), dev_bf16(v)
        sets.append((qd, kd, make_vt(vd, Tk), dev_f32(bias)))
        host.append((as_f32(qd), as_f32(kd), as_f32(vd), bias))
    trash = torch.empty((512 * 2 ** 20,), device="cuda", dtype=torch.bfloat16)
    first = [None, None]
    o = [torch.empty((B, Tq, D), device="cuda", dtype=torch.bfloat16) for _ in range(2)]
    diff = torch.zeros((), device="cuda", dtype=torch.int64)
    for i in range(240):
        qd, kd, vt, bd = sets[i & 1]
        if i % 8 == 0:
            trash.fill_(float(i))
        gpu_ctx.op_attention_hd(qd, kd, vt, bd, H, o[i & 1], 64, SCALE)
        if first[i & 1] is None:
            first[i & 1] = o[i & 1].clone()
        else:
            diff += (o[i & 1].view(torch.int16) != first[i & 1].view(torch.int16)).sum()
    torch.cuda.synchronize()
    assert int(diff.item()) == 0
    for n in range(2):
        q, k, v, bias = host[n]
        check(f"input {n}", as_f32(first[n]), ref.attention_f64(q, k, v, H, SCALE, bias))


# ---- 3. edge sweep, exact ----
@pytest.mark.parametrize("Tk", ref.EDGE_TK)
@pytest.mark.parametrize("instance,B,H,Tq", ref.EDGE_SHAPES)
def test_attention_d64_edges_exact(gpu_ctx, instance, B, H, Tq, Tk):
    """One-hot scores: O must be the selected key's V row (small integers). Every key of the last partial tile, key 0 and key Tk-1 are
    selected; Tq sits on and next to the instance's workgroup boundaries, which pins the row of query block qb (q0 + 16 qb + c16) for
    1, 2 and 4 query blocks per wave; the rows behind the output keep their sentinel."""
    rng = np.random.default_rng(Tq * 1000 + Tk)
    q, k, v, sel = ref.one_hot_case(rng, B, H, Tq, Tk)
    got = as_f32(launch(gpu_ctx, q, k, v, None, H, SCALE, instance))
    err = np.abs(got - ref.one_hot_expected(v, sel, H)).max()
    assert np.isfinite(got).all() and err <= 1e-2, err


# ---- 4. soft bias in reference units ----
@pytest.mark.parametrize("case", ref.SOFT_BIAS_CASES, ids=ref.case_id)
def test_attention_d64_soft_bias(gpu_ctx, case):
    """bias ~ U(-4, 4): softmax(q.k / 8 + bias) with the bias in the reference's units, with scale = 1/8 and through the prescaled
    entry. A bias taken in another unit (x 1/8, x log2 e) is outside the bounds on these inputs (test_attn64_host.py)."""
    builder, args = case
    run_case(gpu_ctx, builder(*args), args[0])


def test_attention_d128_soft_bias(gpu_ctx):
    """The same soft bias at head dim 128 through the same entry (the 128 tests' biases are all 0 / -10000)."""
    for prescaled in (False, True):
        c = ref.soft_bias_case(64, prescaled, heads=2, head_dim=128)
        got = as_f32(launch(gpu_ctx, c.q, c.k, c.v, c.bias, c.heads, c.entry_scale, None, head_dim=128))
        check(c.name + "-d128", got, c.reference(), c.bounds)


# ---- 5. the pad columns of V^T ----
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("Tk", [1, 26, 70, 130])
@pytest.mark.parametrize("instance", [64, 128, 256])
def test_attention_d64_vt_pad_is_multiplied_by_zero(gpu_ctx, instance, Tk, masked):
    """Columns Tk .. ldvt-1 of V^T are read and multiplied by P = 0 (include/ltxhip.h: they must be finite): with +-1e30 there, and
    with the columns of another V, the output is bit-equal to the zero-padded launch. In the module those columns hold an earlier,
    longer projection."""
    B, H, Tq = ref.INSTANCE_SHAPES[instance]
    rng = np.random.default_rng(instance + Tk + masked)
    D = H * 64
    q, k, v = (ref.oracle.bf16_round(rng.standard_normal((B, T, D)).astype(np.float32)) for T in (Tq, Tk, Tk))
    bias = ref.random_mask_bias(rng, B, Tk) if masked else None
    vd = dev_bf16(v)
    zero = launch(gpu_ctx, q, k, v, bias, H, SCALE, instance)
    check("zero pad", as_f32(zero), ref.attention_f64(q, k, v, H, SCALE, bias))
    npad = ((Tk + 63) // 64) * 64 - Tk
    huge = torch.from_numpy(np.where(rng.random((B, D, npad)) < 0.5, -1e30, 1e30).astype(np.float32)).to(torch.bfloat16).cuda()
    other = dev_bf16(rng.standard_normal((B, D, npad)) * 3.0)
    for name, pad in (("1e30", huge), ("another V", other)):
        got = launch(gpu_ctx, q, k, v, bias, H, SCALE, instance, vt=make_vt(vd, Tk, pad))
        assert torch.equal(got.view(torch.int16), zero.view(torch.int16)), name
