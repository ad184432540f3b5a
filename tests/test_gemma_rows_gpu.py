"""The Gemma-3 text encoder's row kernels (csrc/elementwise.hip: gemma_norm, gemma_qknorm_rope, geglu, gemma_embed, gemma_rope_tables)
through their ltx_op_* seams, against the numpy replay (tests/helpers/gemma_ref.py).

Which comparison applies, per kernel:
  * embedding: BIT-EQUAL. bf16 x bf16 is exact in f32, so the one rounding is the only operation and its order cannot differ.
  * norm (+ residual, + second norm) and q/k-norm + RoPE: BIT-EQUAL. The kernels define the row statistic so that its order does not
    matter (exact f32 squares, summed in f64, rounded to f32 once; correctly rounded division, square root and reciprocal) and round
    every product and sum of the rotation on its own, which is the replay's order.
  * GeGLU: at most 1 bf16 ulp on at most 0.1 % of the elements. GELU is the division-free form of the GEMM epilogue (one hardware
    exp2 and one reciprocal, |error| <= 3e-7 |x| against the tanh form): the operation order of the replay cannot be matched. The f32
    value moves by a few ulp of f32 before its rounding to bf16, which flips the bf16 result only when it sits that close to a rounding
    boundary, a fraction of about 2^-16 per f32 ulp moved. Gates are drawn inside [-8, 8]: below that gelu(x) is under 1e-14 |x|, the
    kernel's exp overflows to the limit -0, and a distance in ulps says nothing about two values that small."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gemma_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = 1e-6
ROWS = (1, 70, 1024)
WIDTHS = (384, 3840)


def dev_bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).cuda()


def dev_f32(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()


def bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def ulp_report(got_bits, want_f32):
    """(largest distance in bf16 ulps, fraction of elements that differ) between bf16 bit patterns and the replay's values."""
    def order(b):  # monotonic integer order of bf16 values
        b = b.astype(np.int32)
        return np.where(b & 0x8000, 0x8000 - b, b)
    d = np.abs(order(got_bits) - order(ref.bf16_bits(want_f32)))
    return int(d.max()), float((d != 0).mean())


def within_one_ulp(got_bits, want_f32, what):
    worst, frac = ulp_report(got_bits, want_f32)
    print(f"{what}: worst {worst} ulp, {frac:.2e} of the elements differ")
    return worst <= 1 and frac <= 1e-3


def norm_weight(rng, D):
    """Stored weights w (bf16 values) whose 1 + w is NOT a bf16 value: odd multiples of 2^-10 below 2^-7 lie strictly between two bf16
    neighbours of 1, so bf16(1 + w) moves the gain by up to 0.3 % - most of a bf16 ulp of the output."""
    w = (rng.integers(0, 4, D) * 2 + 1).astype(np.float32) * np.float32(2.0 ** -10)
    assert np.array_equal(ref.bf16(w), w) and not np.array_equal(ref.bf16(1 + w), 1 + w)
    return w * rng.choice([-1.0, 1.0], D).astype(np.float32)


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("rows", ROWS)
def test_norm_residual_and_second_norm(gpu_ctx, rows, D):
    rng = np.random.default_rng(rows + D)
    r = ref.bf16(rng.standard_normal((rows, D)) * 3.0)
    x = ref.bf16(rng.standard_normal((rows, D)))
    w, w2 = norm_weight(rng, D), norm_weight(rng, D)
    rd, xd, wd, w2d = dev_bf16(r), dev_bf16(x), dev_f32(w), dev_f32(w2)
    h = torch.empty((rows, D), device="cuda", dtype=torch.bfloat16)
    n = torch.empty_like(h)
    gpu_ctx.op_gemma_norm(rd, wd, h=h, x=xd, w2=w2d, n=n, eps=EPS)
    plain = torch.empty_like(h)
    gpu_ctx.op_gemma_norm(rd, wd, h=plain, eps=EPS)  # layer 0's input norm
    n_only = torch.empty_like(h)
    gpu_ctx.op_gemma_norm(rd, wd, x=xd, w2=w2d, n=n_only, eps=EPS)  # the final norm: h is not written
    inplace = xd.clone()
    gpu_ctx.op_gemma_norm(rd, wd, h=inplace, x=inplace, eps=EPS)  # x may alias h
    torch.cuda.synchronize()
    want_h, want_n = ref.norm_residual(r, w, EPS, x, w2)
    assert np.array_equal(bits(h), ref.bf16_bits(want_h)), ulp_report(bits(h), want_h)
    assert np.array_equal(bits(n), ref.bf16_bits(want_n)), ulp_report(bits(n), want_n)
    want_plain = ref.rms_norm(r, w, EPS)
    assert np.array_equal(bits(plain), ref.bf16_bits(want_plain)), ulp_report(bits(plain), want_plain)
    assert np.array_equal(bits(n_only), bits(n)) and np.array_equal(bits(inplace), bits(h))


def test_norm_gain_is_rounded_to_bf16_once(gpu_ctx):
    """A version that applies 1 + w in f32 differs in a quarter of the elements: the case that needs the bf16(1 + w) rounding."""
    rows, D = 70, 3840
    rng = np.random.default_rng(5)
    r = ref.bf16(rng.standard_normal((rows, D)))
    w = norm_weight(rng, D)
    out = torch.empty((rows, D), device="cuda", dtype=torch.bfloat16)
    gpu_ctx.op_gemma_norm(dev_bf16(r), dev_f32(w), h=out, eps=EPS)
    torch.cuda.synchronize()
    ms = (r * r).sum(-1, dtype=np.float64, keepdims=True).astype(np.float32) / np.float32(D)
    unrounded = ref.bf16(r * (np.float32(1) / np.sqrt(ms + np.float32(EPS))) * (np.float32(1) + w))
    assert np.array_equal(bits(out), ref.bf16_bits(ref.rms_norm(r, w, EPS)))
    assert not within_one_ulp(bits(out), unrounded, "f32 gain")


@pytest.mark.parametrize("heads", [(2, 1), (16, 8)], ids=["384-wide model", "3840-wide model"])
@pytest.mark.parametrize("rows", ROWS)
def test_qknorm_rope(gpu_ctx, rows, heads):
    hq, hk = heads
    T = 64 if rows > 64 else rows  # position = row % T: several batch elements where rows allow
    rng = np.random.default_rng(rows + hq)
    x = ref.bf16(rng.standard_normal((rows, (hq + hk) * 256)) * 2.0)
    wq, wk = norm_weight(rng, 256), norm_weight(rng, 256)
    cos, sin = ref.rope_tables(T, 10000.0 if hq == 2 else 1000000.0)
    qk = dev_bf16(x)
    gpu_ctx.op_gemma_qknorm_rope(qk, dev_f32(wq), dev_f32(wk), hq, hk, dev_f32(cos), dev_f32(sin), T, eps=EPS)
    torch.cuda.synchronize()
    want = np.concatenate([ref.qknorm_rope(x[:, :hq * 256], wq, cos, sin, T, EPS), ref.qknorm_rope(x[:, hq * 256:], wk, cos, sin, T, EPS)], axis=1)
    assert np.array_equal(bits(qk), ref.bf16_bits(want)), ulp_report(bits(qk), want)


def test_qknorm_rope_pairs_i_with_i_plus_128(gpu_ctx):
    """The traditional (interleaved) pairing, or a swapped sign, is far outside the limit."""
    rows, T = 8, 8
    rng = np.random.default_rng(1)
    x = ref.bf16(rng.standard_normal((rows, 512)))
    w = np.zeros(256, np.float32)
    cos, sin = ref.rope_tables(T, 10000.0)
    qk = dev_bf16(x)
    gpu_ctx.op_gemma_qknorm_rope(qk, dev_f32(w), dev_f32(w), 1, 1, dev_f32(cos), dev_f32(sin), T, eps=EPS)
    torch.cuda.synchronize()
    y = ref.rms_norm(x.reshape(rows, 2, 256), w, EPS)
    c, s = np.repeat(cos, 2, axis=1)[:, None, :], np.repeat(sin, 2, axis=1)[:, None, :]
    rot = np.stack([-y[..., 1::2], y[..., 0::2]], axis=-1).reshape(y.shape)
    interleaved = ref.bf16(y * c + rot * s).reshape(rows, 512)
    assert np.array_equal(bits(qk), ref.bf16_bits(ref.qknorm_rope(x, w, cos, sin, T, EPS).reshape(rows, 512)))
    assert not within_one_ulp(bits(qk), interleaved, "interleaved")


@pytest.mark.parametrize("base", [10000.0, 1000000.0])
def test_rope_tables_on_the_device(gpu_ctx, base):
    """Against f64 on the host: the kernel evaluates the angle, cos and sin in f64 and rounds once, so an entry is within one f32 ulp
    at 1 (1.2e-7: the rounding's half ulp, and room for the last bit of the two f64 libraries)."""
    T = 1024
    cos = torch.empty((T, 128), device="cuda", dtype=torch.float32)
    sin = torch.empty_like(cos)
    gpu_ctx.op_gemma_rope_tables(T, base, cos, sin)
    torch.cuda.synchronize()
    ang = np.arange(T, dtype=np.float64)[:, None] * base ** (-np.arange(128, dtype=np.float64) / 128.0)[None, :]
    bound = 1.2e-7
    assert (np.abs(cos.cpu().numpy() - np.cos(ang)) <= bound).all() and (np.abs(sin.cpu().numpy() - np.sin(ang)) <= bound).all()
    assert np.array_equal(cos[0].cpu().numpy(), np.ones(128, np.float32)) and np.array_equal(sin[0].cpu().numpy(), np.zeros(128, np.float32))


@pytest.mark.parametrize("inter", [768, 15360])
@pytest.mark.parametrize("rows", ROWS)
def test_geglu(gpu_ctx, rows, inter):
    rng = np.random.default_rng(rows + inter)
    gu = ref.bf16(np.clip(rng.standard_normal((rows, 2 * inter)) * 2.0, -8.0, 8.0))
    out = torch.empty((rows, inter), device="cuda", dtype=torch.bfloat16)
    gpu_ctx.op_geglu(dev_bf16(gu), out)
    torch.cuda.synchronize()
    assert within_one_ulp(bits(out), ref.geglu(gu), "geglu")
    single = ref.bf16(ref.gelu_tanh(gu[:, :inter]) * gu[:, inter:])  # without the rounding of gelu(gate) before the product
    assert not within_one_ulp(bits(out), single, "one rounding")


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("rows", ROWS)
def test_embedding_is_bit_equal(gpu_ctx, rows, D):
    vocab = 512
    rng = np.random.default_rng(rows + D)
    table = ref.bf16(rng.standard_normal((vocab, D)))
    ids = rng.integers(0, vocab, rows).astype(np.int32)
    ids[0] = vocab - 1
    out = torch.empty((rows, D), device="cuda", dtype=torch.bfloat16)
    gpu_ctx.op_gemma_embed(torch.from_numpy(ids).cuda(), dev_bf16(table), out)
    torch.cuda.synchronize()
    assert np.array_equal(bits(out), ref.bf16_bits(ref.embed(ids, table, D)))
    if D == 3840:  # bf16(sqrt(3840)) = 62.0, not 61.97: the unrounded scalar gives other bits
        assert float(ref.bf16(np.float32(math.sqrt(D)))) == 62.0
        assert not np.array_equal(bits(out), ref.bf16_bits(ref.bf16(table[ids] * np.float32(math.sqrt(D)))))


def test_embedding_clamps_ids_on_the_device(gpu_ctx):
    """The device call has no host to report to: ids outside [0, vocab) read the nearest row."""
    table = ref.bf16(np.random.default_rng(0).standard_normal((16, 384)))
    ids = np.array([-5, 0, 15, 16, 2 ** 30], np.int32)
    out = torch.empty((5, 384), device="cuda", dtype=torch.bfloat16)
    gpu_ctx.op_gemma_embed(torch.from_numpy(ids).cuda(), dev_bf16(table), out)
    torch.cuda.synchronize()
    assert np.array_equal(bits(out), ref.bf16_bits(ref.embed(np.clip(ids, 0, 15), table, 384)))
