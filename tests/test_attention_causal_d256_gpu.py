"""The causal grouped-query attention kernel at head dim 256 (csrc/attention.hip, attn256_causal_kernel) through
ltx_op_attention_causal, against an f32 softmax on the SAME bf16 inputs, on valid rows only. Bounds: those the head-dim-64 and
head-dim-128 kernels are held to - max abs 2e-2, rel-L2 1e-2, every value finite. Rows below key_start must be exactly zero. Two
bit-exact properties guard the tile skipping: nothing after position p reaches rows <= p, and nothing in the padded K / V rows reaches
any valid row."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gemma_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
SCALE = 1.0 / 16.0  # query_pre_attn_scalar^-0.5 at 256: the caller's, not 1/sqrt(head dim) by construction

# (B, Hq, Hkv, T, key_start per batch element)
SHAPES = [(1, 2, 1, 16, (0,)), (1, 2, 2, 64, (0,)), (1, 4, 2, 70, (5,)), (2, 2, 1, 130, (0, 67)), (1, 2, 1, 257, (64,)), (1, 2, 1, 200, (199,)),
          (2, 16, 8, 1024, (1000, 0))]


def ids(s):
    return f"B{s[0]}-Hq{s[1]}-Hkv{s[2]}-T{s[3]}-ks{'_'.join(map(str, s[4]))}"


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).cuda()


def as_f32(t):
    return t.float().cpu().numpy()


def make_vt(vd):
    B, T, D = vd.shape
    vt = torch.zeros((B, D, ((T + 63) // 64) * 64), device="cuda", dtype=torch.bfloat16)
    vt[:, :, :T] = vd.transpose(1, 2)
    return vt


def make_inputs(shape, seed=0):
    B, Hq, Hkv, T, ks = shape
    rng = np.random.default_rng(seed + B * 1000 + Hq * 100 + T)
    q = dev(rng.standard_normal((B, T, Hq * 256)) * 2.0)  # q.k / 16 ~ N(0, 2^2): a softmax with a few dominant keys
    k = dev(rng.standard_normal((B, T, Hkv * 256)))
    v = dev(rng.standard_normal((B, T, Hkv * 256)))
    return q, k, v, torch.tensor(ks, dtype=torch.int32, device="cuda")


def run(gpu_ctx, q, k, v, ks):
    o = torch.full(q.shape, 7.0, device="cuda", dtype=torch.bfloat16)
    gpu_ctx.op_attention_causal(q, k, make_vt(v), o, SCALE, ks)
    torch.cuda.synchronize()
    return o


_cache = {}


def case(gpu_ctx, shape):
    """One launch and one reference per shape, shared by the tests below and left unchanged."""
    if shape not in _cache:
        q, k, v, ks = make_inputs(shape)
        o = run(gpu_ctx, q, k, v, ks)
        want = ref.attention(as_f32(q), as_f32(k), as_f32(v), shape[1], shape[2], SCALE, shape[4])
        _cache[shape] = (q, k, v, ks, o, want)
    return _cache[shape]


def valid_rows(shape):
    B, _, _, T, ks = shape
    m = np.zeros((B, T), bool)
    for b in range(B):
        m[b, ks[b]:] = True
    return m


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_causal_attention_vs_f32_on_valid_rows(gpu_ctx, shape):
    _, _, _, _, o, want = case(gpu_ctx, shape)
    got, m = as_f32(o), valid_rows(shape)
    assert np.isfinite(got).all()
    err = np.abs(got[m] - want[m]).max()
    rel = np.linalg.norm(got[m] - want[m]) / np.linalg.norm(want[m])
    print(f"{ids(shape)}: max abs {err:.3e} rel-L2 {rel:.3e}")
    assert err <= 2e-2, err
    assert rel <= 1e-2, rel


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_rows_below_key_start_are_exactly_zero(gpu_ctx, shape):
    o = case(gpu_ctx, shape)[4]
    bits = o.view(torch.int16).cpu().numpy()
    assert (bits[~valid_rows(shape)] == 0).all()


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_nothing_after_position_p_reaches_rows_up_to_p(gpu_ctx, shape):
    """Q, K and V rows after p are overwritten: output rows <= p keep every bit. p sits mid-tile, on a tile's last row and on a tile's
    first row where T allows."""
    B, Hq, Hkv, T, _ = shape
    q, k, v, ks, o, _ = case(gpu_ctx, shape)
    for p in sorted({min(T - 1, x) for x in (T // 2, 63, 64, T - 2)} - {T - 1}):
        if p < 0:
            continue
        q2, k2, v2 = q.clone(), k.clone(), v.clone()
        rng = np.random.default_rng(p)
        for t in (q2, k2, v2):
            t[:, p + 1:] = dev(rng.standard_normal(tuple(t[:, p + 1:].shape)) * 3.0)
        o2 = run(gpu_ctx, q2, k2, v2, ks)
        assert torch.equal(o2[:, :p + 1].view(torch.int16), o[:, :p + 1].view(torch.int16)), p


@pytest.mark.parametrize("shape", [s for s in SHAPES if any(s[4])], ids=ids)
def test_padded_keys_and_values_reach_no_valid_row(gpu_ctx, shape):
    """Padded K and V rows overwritten with large finite values (1e4): every valid row keeps every bit."""
    q, k, v, ks, o, _ = case(gpu_ctx, shape)
    k2, v2 = k.clone(), v.clone()
    for b, s in enumerate(shape[4]):
        k2[b, :s] = 1e4
        v2[b, :s] = 1e4
    o2 = run(gpu_ctx, q, k2, v2, ks)
    m = torch.from_numpy(valid_rows(shape)).cuda()
    assert torch.equal(o2.view(torch.int16)[m], o.view(torch.int16)[m])
    assert (o2.view(torch.int16)[~m] == 0).all()


def test_null_key_start_is_no_padding(gpu_ctx):
    shape = SHAPES[2][:4] + ((0,),)
    q, k, v, ks = make_inputs(shape)
    assert torch.equal(run(gpu_ctx, q, k, v, None).view(torch.int16), run(gpu_ctx, q, k, v, ks).view(torch.int16))


def test_rows_past_t_keep_their_sentinel(gpu_ctx):
    shape = (1, 2, 1, 70, (5,))
    q, k, v, ks = make_inputs(shape)
    buf = torch.full((70 + 64, 512), 7.0, device="cuda", dtype=torch.bfloat16)
    gpu_ctx.op_attention_causal(q, k, make_vt(v), buf[:70].view(1, 70, 512), SCALE, ks)
    torch.cuda.synchronize()
    assert (as_f32(buf[70:]) == 7.0).all()


def test_other_head_dims_are_refused(gpu_ctx, ltx):
    t = torch.zeros((1, 64, 128), device="cuda", dtype=torch.bfloat16)
    with pytest.raises(ltx.LTXError, match="head dim 128") as e:
        gpu_ctx.op_attention_causal(t, t, torch.zeros((1, 128, 64), device="cuda", dtype=torch.bfloat16), torch.empty_like(t), 0.1, None, head_dim=128)
    assert e.value.case == "invalidConfiguration"

