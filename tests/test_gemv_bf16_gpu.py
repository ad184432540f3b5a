"""gemv_bf16_kernel (csrc/gemm.hip) through ltx_op_gemv_bf16: the decode path's bf16 x bf16 -> bf16 product at M = 1.

Exact cases use small-integer x and W (|v| <= 8, K <= 15 360): every partial sum stays below 2^24, so ANY summation order is exact
in f32 and the output must equal numpy's in every bit. The random-data case is held to the GEMM tests' own bf16 bound
(tests/test_kernels_gpu.py: 2^-8 max|ref| + 1e-3 against the same bf16-rounded operands)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gemma_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 0x7FC1  # a NaN pattern no kernel writes
NS = (1, 7, 64, 1000, 2049)


def dev_bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).cuda()


def bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def sentinel_bf16(n):
    return torch.full((n,), SENTINEL, dtype=torch.int16, device="cuda").view(torch.bfloat16)


def ints(rng, shape):
    return rng.integers(-8, 9, shape).astype(np.float32)


@pytest.mark.parametrize("K", [8, 384, 520, 3840, 15360])
def test_integer_exact_bf16_and_f32_stores(gpu_ctx, K):
    """Every N of {1, 7, 64, 1000, 2049} at this K: the plain bf16 store and the f32 store (which holds the bf16-rounded value), both
    bit-equal to numpy, with 64 sentinels behind each output untouched. K = 8 and 384 are less than one trip of 512, 520 is one trip
    and a partly filled one, 3840 = 7.5 trips takes every rung of the chunk ladder, 15 360 is the longest row of the model."""
    rng = np.random.default_rng(K)
    x = ints(rng, K)
    xd = dev_bf16(x)
    for N in NS:
        W = ints(rng, (N, K))
        want = ref.bf16(W @ x)
        assert np.abs(W @ x).max() < 2 ** 24
        Wd = dev_bf16(W)
        ob = sentinel_bf16(N + 64)
        of = torch.full((N + 64,), -777.0, device="cuda")
        gpu_ctx.op_gemv_bf16(xd, Wd, N, K, epilogue=0, out_bf16=ob)
        gpu_ctx.op_gemv_bf16(xd, Wd, N, K, epilogue=1, out_f32=of)
        torch.cuda.synchronize()
        assert np.array_equal(bits(ob)[:N], ref.bf16_bits(want)), (N, K)
        assert (bits(ob)[N:] == SENTINEL).all()
        assert np.array_equal(of.cpu().numpy()[:N], want) and (of.cpu().numpy()[N:] == -777.0).all(), (N, K)


def test_padded_weight_rows_and_a_strided_store(gpu_ctx):
    """ldw > K: the pad columns hold NaN and are never read. out_stride > 1 scatters (the step writes V into one column of the V^T
    cache this way): the elements between the outputs keep their sentinels."""
    rng = np.random.default_rng(5)
    N, K, ldw, stride = 77, 520, 536, 192
    x, W = ints(rng, K), ints(rng, (N, K))
    Wp = np.full((N, ldw), np.nan, np.float32)
    Wp[:, :K] = W
    out = sentinel_bf16(N * stride)
    gpu_ctx.op_gemv_bf16(dev_bf16(x), dev_bf16(Wp), N, K, epilogue=0, out_bf16=out, out_stride=stride, ldw=ldw)
    torch.cuda.synchronize()
    got = bits(out).reshape(N, stride)
    assert np.array_equal(got[:, 0], ref.bf16_bits(ref.bf16(W @ x)))
    assert (got[:, 1:] == SENTINEL).all()


@pytest.mark.parametrize("I,K", [(7, 384), (768, 384), (1000, 520), (2049, 3840)])
def test_geglu_epilogue_is_bit_equal_on_exact_sums(gpu_ctx, I, K):
    """The fused gate|up matrix [2I][K]: row n and row n + I give bf16(bf16(gelu_tanh(bf16(g))) * bf16(u)), the rounding points of
    geglu_kernel behind the GEMM's bf16 store. Integer operands (x of +-1) make g and u exact; the gate rows are built so that g is an
    integer of [-8, 8] (the domain tests/test_gemma_rows_gpu.py gives GELU: below -8 the kernel's exp overflows to the limit -0).
    Bit-equal to gemma_ref.geglu and to the library's own geglu pass on the same sums."""
    rng = np.random.default_rng(I + K)
    x = rng.choice(np.array([-1.0, 1.0], np.float32), K)
    W = ints(rng, (2 * I, K))
    target = rng.integers(-8, 9, I).astype(np.float32)
    half = K // 2  # the second half of a gate row cancels the first, then one entry carries the target: |W| <= 16, g == target
    W[:I, half:2 * half] = -W[:I, :half] * x[:half] * x[half:2 * half]
    W[:I, 0] += target * x[0]
    assert np.array_equal(ref.bf16(W), W) and np.array_equal(W[:I] @ x, target)
    gu = ref.bf16(W @ x)
    want = ref.geglu(gu[None])[0]
    out = sentinel_bf16(I + 64)
    gpu_ctx.op_gemv_bf16(dev_bf16(x), dev_bf16(W), I, K, epilogue=2, out_bf16=out)
    torch.cuda.synchronize()
    assert (bits(out)[I:] == SENTINEL).all()
    if I % 8 == 0:  # the widths geglu_kernel takes
        two_pass = torch.empty((1, I), device="cuda", dtype=torch.bfloat16)
        gpu_ctx.op_geglu(dev_bf16(gu[None]), two_pass)
        torch.cuda.synchronize()
        assert np.array_equal(bits(out)[:I], bits(two_pass)[0]), "the fused epilogue differs from geglu_kernel on the stored sums"
    diff = np.nonzero(bits(out)[:I] != ref.bf16_bits(want))[0]
    print(f"I={I} K={K}: {len(diff)} of {I} elements differ from gemma_ref.geglu", [(float(gu[i]), float(gu[I + i])) for i in diff[:4]])
    assert len(diff) == 0


def test_logits_shape_on_rows_copied_back(gpu_ctx, ltx):
    """One launch at the product's logits shape, 262 208 x 3840 (16 388 workgroups of 16 rows), integer weights filled on the device.
    64 rows are copied back and checked bit for bit: the first and last row, both sides of the first, a middle and the last workgroup
    boundary, and 48 drawn at random."""
    N, K = 262208, 3840
    per = ltx.gemv_bf16_rows_per_workgroup(N, 1)
    assert per == 16
    g = torch.Generator(device="cuda").manual_seed(3)
    W = torch.randint(-8, 9, (N, K), dtype=torch.int8, device="cuda", generator=g).to(torch.bfloat16)
    rng = np.random.default_rng(3)
    x = ints(rng, K)
    out = torch.full((N + 64,), -777.0, device="cuda")
    gpu_ctx.op_gemv_bf16(dev_bf16(x), W, N, K, epilogue=1, out_f32=out)
    torch.cuda.synchronize()
    mid = (N // 2) // per * per
    rows = [0, 1, per - 2, per - 1, per, per + 1, mid - 2, mid - 1, mid, mid + 1, N - per - 2, N - per - 1, N - per, N - per + 1, N - 2, N - 1]
    rows = np.array(sorted(set(rows) | set(int(r) for r in rng.choice(N, 64 - len(rows), replace=False))))[:64]
    Wr = W[torch.from_numpy(rows).cuda()].float().cpu().numpy()
    got = out.cpu().numpy()
    assert np.array_equal(got[rows], ref.bf16(Wr @ x))
    assert np.isfinite(got[:N]).all() and (got[N:] == -777.0).all()
    del W


@pytest.mark.parametrize("N,K", [(1000, 3840), (384, 15360)])
def test_random_data_against_f64(gpu_ctx, N, K):
    rng = np.random.default_rng(N)
    x = ref.bf16(rng.standard_normal(K))
    W = ref.bf16(rng.standard_normal((N, K)) / np.sqrt(K))
    want = W.astype(np.float64) @ x.astype(np.float64)
    out = torch.empty(N, device="cuda", dtype=torch.bfloat16)
    gpu_ctx.op_gemv_bf16(dev_bf16(x), dev_bf16(W), N, K, out_bf16=out)
    torch.cuda.synchronize()
    err = np.abs(out.float().cpu().numpy() - want).max()
    bound = 2 ** -8 * np.abs(want).max() + 1e-3
    print(f"N={N} K={K}: max abs error {err:.3e} against f64, bound {bound:.3e}")
    assert err <= bound


def test_refusals_write_nothing(gpu_ctx, ltx):
    """One refusal per requirement of the launcher and the seam, each before the launch: the output keeps its sentinels."""
    K, N = 64, 16
    x, W = dev_bf16(np.ones(K + 8)), dev_bf16(np.ones((2 * N, K + 8)))
    out = sentinel_bf16(N)
    of = torch.full((N,), -777.0, device="cuda")
    ok = dict(x=x, W=W, N=N, K=K, epilogue=0, out_bf16=out)
    gpu_ctx.op_gemv_bf16(**ok)
    torch.cuda.synchronize()
    out.copy_(sentinel_bf16(N))
    bad = [dict(M=2), dict(x=None), dict(W=None), dict(epilogue=3), dict(N=0), dict(K=60), dict(K=0), dict(K=16392, ldw=16392), dict(ldw=K - 8),
           dict(ldw=K + 4), dict(x=x[1:]), dict(W=W[0, 1:], ldw=K + 8), dict(out_bf16=None), dict(out_stride=0), dict(epilogue=1, out_f32=None),
           dict(epilogue=2, out_bf16=None, out_f32=of)]
    for b in bad:
        with pytest.raises(ltx.LTXError) as e:
            gpu_ctx.op_gemv_bf16(**{**ok, **b})
        assert e.value.code == 2, b
    torch.cuda.synchronize()
    assert (bits(out) == SENTINEL).all() and (of == -777.0).all()
