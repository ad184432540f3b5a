"""The passes of csrc/elementwise.h and csrc/audio.h that test_helper_passes_gpu.py left without a seam of their own - the audio row
passes (pn_pad, upsample_pad, denorm_pad, mel_pack, mean3_act), the VAE encoder's passes (enc_patchify, enc_s2d_residual, enc_finish),
the connector's register plan / gather, sp_vt_interleave, the timestep embedding, the guidance combines (cfg_combine, lincomb, axpby,
ge, scale_inplace), vae_make_mods_batch, clip01, mask_to_bias, the two casts, and the integer plans (i2v_rowmap, i2v_timesteps,
fill_const_i32, gemma_mask_scan) - each on its own through its ltx_op_* seam, against the float64 restatement in
tests/helpers/helper_pass_ref.py. With these, every launch_* of the two headers has a seam and a test at it.

The three comparisons are those of test_helper_passes_gpu.py: BIT-EQUAL on integer / power-of-two data, a COUNTED float64 bound
(U = 2^-24 per rounding, the count stated in the test), and `bf16_rule` for bf16 outputs of inexact arithmetic (tests/
test_helper_passes_host.py shows that an f32 replay of those passes differs from the float64 reference in under 1e-4 of these inputs).

Every output has one tile of sentinel-filled slack behind it, which must keep the sentinel. Every HALOED output (the audio operands:
zeroed once when the buffer is made, never again - "only the interior is ever written") is filled with the sentinel as a whole and
every element outside the interior must keep it.

Grid caps, read from the launchers (elementwise.hip): clip01 65535 * 16 workgroups of 256 elements; cast_f32_bf16 2048 workgroups of
256 threads x 4 elements; cast_bf16_f32 4096 workgroups of 256 elements. One case of each runs one trip past its cap."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import helper_pass_ref as ref  # noqa: E402
import row_pass_cases as cases  # noqa: E402
from guarded_buffers import (SENTINEL_BITS, SENTINEL_F32, bf16_rule, dev, exact_f32, host_bf16, host_f32, out_bf16, out_f32,  # noqa: E402
                             report, same_f32_bits)

pytestmark = pytest.mark.gpu
U = ref.U
SENTINEL_I32 = -1234567

CLIP01_CAP = 65535 * 16 * 256
CAST_F32_BF16_CAP = 2048 * 256 * 4
CAST_BF16_F32_CAP = 4096 * 256


def out_i32(n, slack):
    return torch.full((n + slack,), SENTINEL_I32, dtype=torch.int32, device="cuda")


def host_i32(t, n, shape=None):
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    assert a.size > n and np.all(a[n:] == SENTINEL_I32), "wrote past the valid extent"
    return a[:n].reshape(shape or (n,))


def dev_bits(bits):
    """bf16 BIT PATTERNS (uint16) -> device bf16 tensor"""
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint16).view(np.int16)).cuda().view(torch.bfloat16)


def haloed(plane, C):
    """A sentinel-filled bf16 operand [rows][cols][C] with one row of slack behind it -> (tensor, element count)"""
    n = plane[0] * plane[1] * C
    return out_bf16(n, plane[1] * C), n


def interior(t, n, plane, C, at, hw, c_valid=None):
    """The interior [h][w][c_valid] of a haloed operand, after checking that every element outside it (halo rows and columns, pad
    channels, the slack) kept the sentinel."""
    bits = host_bf16(t, n, (plane[0], plane[1], C))
    (r0, c0), (h, w), cv = at, hw, (C if c_valid is None else c_valid)
    outside = np.ones(bits.shape, bool)
    outside[r0:r0 + h, c0:c0 + w, :cv] = False
    assert np.all(bits[outside] == SENTINEL_BITS), "wrote outside the interior"
    return bits[r0:r0 + h, c0:c0 + w, :cv]


# =====================================================================================================================================
# audio row passes
# =====================================================================================================================================
@pytest.mark.parametrize("H,W,C", cases.PN_PAD_SHAPES)
def test_audio_pn_pad(gpu_ctx, H, W, C):
    """(1, 1, 32): one position in a four-wave workgroup, three waves idle. (3, 5, 96): 15 positions, ragged last workgroup, 1.5 channels
    per lane. (2, 16, 1024): 16 channels per lane. (1, 3, 20): lanes without a channel. Mode 1 on integers is bit-equal; mode 0 follows
    `bf16_rule`, and an all-zero position gives zeros (never 0 / 0)."""
    rng = np.random.default_rng(H + W + C)
    xi = rng.integers(-128, 129, (H, W, C)).astype(np.float32)
    want, plane, at = ref.audio_pn_pad(xi, 1)
    assert plane == (H + 3, W + 2) and at == (2, 1)
    o, n = haloed(plane, C)
    gpu_ctx.op_audio_pn_pad(dev(xi), H, W, C, 1, o)
    assert np.array_equal(interior(o, n, plane, C, at, (H, W)), ref.bf16_bits(want))
    inputs = [cases.pn_pad_input(H, W, C)] + ([np.zeros((H, W, C), np.float32)] if H * W == 1 else [])
    for x in inputs:
        want, _, _ = ref.audio_pn_pad(x, 0)
        o, n = haloed(plane, C)
        gpu_ctx.op_audio_pn_pad(dev(x), H, W, C, 0, o)
        got = interior(o, n, plane, C, at, (H, W))
        assert bf16_rule(got, want, f"audio_pn_pad H={H} W={W} C={C}")
        zero = ~x.any(axis=-1)
        assert zero.any() == (H * W > 1 or not x.any())
        assert np.all(ref.from_bf16_bits(got[zero]) == 0.0)  # NaN would not compare equal


@pytest.mark.parametrize("H,W,C", [(1, 1, 4), (3, 5, 32), (2, 7, 36)])
def test_audio_upsample_pad(gpu_ctx, H, W, C):
    """np.repeat on both axes at (u + 1, v + 1) of a (2H + 2, 2W + 2) plane: ONE zero row on top, where pn_pad has two."""
    x = np.random.default_rng(H * 100 + W * 10 + C).integers(-128, 129, (H, W, C)).astype(np.float32)
    want, plane, at = ref.audio_upsample_pad(x)
    assert plane == (2 * H + 2, 2 * W + 2) and at == (1, 1) and want.shape == (2 * H, 2 * W, C)
    o, n = haloed(plane, C)
    gpu_ctx.op_audio_upsample_pad(dev(x), H, W, C, o)
    assert np.array_equal(interior(o, n, plane, C, at, (2 * H, 2 * W)), ref.bf16_bits(want))


@pytest.mark.parametrize("Cl,T,Wl,Cpad", [(8, 1, 16, 32), (8, 5, 16, 32), (3, 4, 5, 32)])
def test_audio_denorm_pad(gpu_ctx, Cl, T, Wl, Cpad):
    """Integer latent in [-4, 4], std[c][w] = 2^((c Wl + w) % 4), mean[c][w] = a different integer of [-64, 63] at every (c, w)
    (37 (c Wl + w) mod 128: 37 is odd, Cl Wl <= 128): every product and sum is an integer below 256 in magnitude, a bf16 value, and
    an index that is transposed or truncated fetches another mean. Channels Cl .. Cpad-1 keep the sentinel. Then random data."""
    rng = np.random.default_rng(Cl * 1000 + T * 100 + Wl)
    idx = np.arange(Cl * Wl)
    std = (2.0 ** (idx % 4)).astype(np.float32)
    mean = ((37 * idx) % 128 - 64).astype(np.float32)
    assert len(set(mean)) == Cl * Wl
    lat = rng.integers(-4, 5, (Cl, T, Wl)).astype(np.float32)
    d_mean, d_std = dev(mean), dev(std)
    want, plane, at = ref.audio_denorm_pad(lat, mean, std)
    assert plane == (T + 3, Wl + 2) and at == (2, 1) and want.shape == (T, Wl, Cl)
    o, n = haloed(plane, Cpad)
    gpu_ctx.op_audio_denorm_pad(dev(lat), d_mean, d_std, Cl, T, Wl, Cpad, o)
    assert np.array_equal(interior(o, n, plane, Cpad, at, (T, Wl), Cl), ref.bf16_bits(want))
    lat = rng.standard_normal((Cl, T, Wl)).astype(np.float32)
    mean = rng.standard_normal(Cl * Wl).astype(np.float32)
    std = rng.uniform(0.5, 2.0, Cl * Wl).astype(np.float32)
    o, n = haloed(plane, Cpad)
    gpu_ctx.op_audio_denorm_pad(dev(lat), dev(mean), dev(std), Cl, T, Wl, Cpad, o)
    assert bf16_rule(interior(o, n, plane, Cpad, at, (T, Wl), Cl), ref.audio_denorm_pad(lat, mean, std)[0], f"audio_denorm_pad Cl={Cl} T={T} Wl={Wl}")


@pytest.mark.parametrize("T,M", [(1, 64), (5, 64), (3, 20)])
def test_audio_mel_pack(gpu_ctx, T, M):
    """The output pointer is row 0 INSIDE a haloed buffer: two sentinel rows in front of it and two behind must stay."""
    mel = np.random.default_rng(T * 100 + M).integers(-128, 129, (2, T, M)).astype(np.float32)
    want = ref.audio_mel_pack(mel)
    assert np.array_equal(want, mel.astype(np.float64).transpose(1, 0, 2).reshape(T, 2 * M))
    halo = 2
    plane = (T + 2 * halo, 1)
    o, n = haloed(plane, 2 * M)
    gpu_ctx.op_audio_mel_pack(dev(mel), T, M, o[halo * 2 * M:])
    assert np.array_equal(interior(o, n, plane, 2 * M, (halo, 0), (T, 1))[:, 0, :], ref.bf16_bits(want))


@pytest.mark.parametrize("rows,C,ldb", cases.MEAN3_SHAPES)
def test_audio_mean3_act(gpu_ctx, rows, C, ldb):
    """1 x 4: one thread. 7 x 32: dense. 5 x 36 at ldb = 64: the pad columns keep the sentinel. 300 x 64: 4800 threads, 19 workgroups, the
    last ragged. Exact: a + b + c = 3 k with integers (|k| <= 40), slope 0.5 - the sum, the quotient and the halved negative are all
    exact, and the first two elements hold a mean of -0 and of +0, which take the >= 0 branch (bits 0x8000 and 0). Random inputs at the
    product's slopes follow `bf16_rule`."""
    rng = np.random.default_rng(rows + C)
    a = rng.integers(-60, 61, (rows, C)).astype(np.float32)
    b = rng.integers(-60, 61, (rows, C)).astype(np.float32)
    k = rng.integers(-40, 41, (rows, C)).astype(np.float32)
    c = 3 * k - a - b
    for v, z in ((a, -0.0), (b, -0.0), (c, -0.0)):
        v[0, 0], v[0, 1] = z, 0.0
    want = ref.audio_mean3_act(a, b, c, 0.5)
    assert np.signbit(want[0, 0]) and not np.signbit(want[0, 1]) and want[0, 0] == 0 == want[0, 1]
    assert rows * C < 16 or ((want < 0).any() and (want > 0).any())
    plane = (rows, 1)
    o, n = haloed(plane, ldb)
    gpu_ctx.op_audio_mean3_act(dev(a), dev(b), dev(c), rows, C, 0.5, o, ldb)
    assert np.array_equal(interior(o, n, plane, ldb, (0, 0), (rows, 1), C)[:, 0, :], ref.bf16_bits(want))
    a, b, c = cases.mean3_inputs(rows, C)
    d_a, d_b, d_c = dev(a), dev(b), dev(c)
    for slope in cases.MEAN3_SLOPES:
        o, n = haloed(plane, ldb)
        gpu_ctx.op_audio_mean3_act(d_a, d_b, d_c, rows, C, slope, o, ldb)
        got = interior(o, n, plane, ldb, (0, 0), (rows, 1), C)[:, 0, :]
        assert bf16_rule(got, ref.audio_mean3_act(a, b, c, np.float32(slope)), f"audio_mean3_act {rows}x{C} ldb={ldb} slope={slope}")


# =====================================================================================================================================
# VAE encoder passes
# =====================================================================================================================================
@pytest.mark.parametrize("T,H,W", [(1, 4, 4), (2, 8, 12), (3, 4, 20)])
def test_enc_patchify(gpu_ctx, T, H, W):
    """The pixel at (c, t, y, x) carries its own linear index, the low byte in one run and the high byte in another (both below 256:
    bf16 values), so the two outputs together name the source of every element. Channels 48 .. 63 are zero; pw comes before ph."""
    lin = np.arange(3 * T * H * W).reshape(3, T, H, W)
    assert lin.max() < 65536
    n = T * (H // 4) * (W // 4) * 64
    got = []
    for px in (lin % 256, lin // 256):
        o = out_bf16(n, 64)
        gpu_ctx.op_enc_patchify(dev(px), o, T, H, W)
        bits = host_bf16(o, n, (T, H // 4, W // 4, 64))
        assert np.array_equal(bits, ref.bf16_bits(ref.enc_patchify(px)))
        assert not bits[..., 48:].any()
        got.append(ref.from_bf16_bits(bits))
    src = (got[0] + 256 * got[1]).astype(np.int64)
    # element (t, h4, w4, c*16 + pw*4 + ph) is pixel (c, t, 4 h4 + ph, 4 w4 + pw), spelled out for the last patch
    t, h4, w4 = T - 1, H // 4 - 1, W // 4 - 1
    for c, pw, ph in ((0, 0, 0), (1, 3, 0), (2, 1, 2)):
        assert src[t, h4, w4, c * 16 + pw * 4 + ph] == lin[c, t, 4 * h4 + ph, 4 * w4 + pw]


S2D_CHANNELS = {  # factor -> (Cc, Cx, Cout) with G = Cx S / Cout = 1, then 2 or 4; Cc S == Cout
    (2, 1, 1): [(2, 2, 4), (2, 4, 4)],       # G = 1, 2
    (1, 2, 2): [(2, 2, 8), (1, 4, 4)],       # G = 1, 4
    (2, 2, 2): [(2, 2, 16), (1, 2, 8)],      # G = 1, 2
}


@pytest.mark.parametrize("T", [1, 2, 3, 4])
@pytest.mark.parametrize("factor", sorted(S2D_CHANNELS))
def test_enc_s2d_residual(gpu_ctx, factor, T):
    """T = 1, 3 are padded in FRONT with a copy of frame 0 when ft = 2 (padT = 1), T = 2, 4 are not; H x W = 2 x 2 (one output position
    at (1, 2, 2) and (2, 2, 2)) and 4 x 6. Integers with G a power of two: the group sum, its quotient and the sum with the conv are
    exact. The reference is an explicit pad, a reshape / transpose space-to-depth and a group mean."""
    ft, fh, fw = factor
    S = ft * fh * fw
    rng = np.random.default_rng(S * 10 + T)
    for H, W in ((2, 2), (4, 6)):
        for Cc, Cx, Cout in S2D_CHANNELS[factor]:
            G = Cx * S // Cout
            assert Cc * S == Cout and (Cx * S) % Cout == 0 and G in (1, 2, 4)
            conv = rng.integers(-64, 65, (T, H, W, Cc)).astype(np.float32)
            x = rng.integers(-64, 65, (T, H, W, Cx)).astype(np.float32)
            want, _, _ = ref.enc_s2d_residual(conv, x, ft, fh, fw)
            T2 = -(-T // ft)
            assert want.shape == (T2, H // fh, W // fw, Cout)
            o = out_f32(want.size, 256)
            gpu_ctx.op_enc_s2d_residual(dev(conv), Cc, dev(x), Cx, o, Cout, T, H, W, ft, fh, fw)
            assert same_f32_bits(host_f32(o, want.size, want.shape), exact_f32(want)), (H, W, Cc, Cx, Cout)


def test_enc_s2d_residual_random(gpu_ctx):
    """(2, 2, 2) at T = 3 (padded), 4 x 6, Cx = 6 -> Cout = 16: G = 3, not a power of two. G - 1 additions build the group sum (the first
    term is added to an exact zero), one division takes the mean, one addition joins the conv: G + 1 roundings of terms no larger than
    |conv| + mean_g |x|."""
    ft, fh, fw, T, H, W, Cc, Cx, Cout = 2, 2, 2, 3, 4, 6, 2, 6, 16
    G = Cx * 8 // Cout
    assert G == 3
    rng = np.random.default_rng(77)
    conv = rng.standard_normal((T, H, W, Cc)).astype(np.float32)
    x = rng.standard_normal((T, H, W, Cx)).astype(np.float32)
    want, c_part, x_abs = ref.enc_s2d_residual(conv, x, ft, fh, fw)
    o = out_f32(want.size, 256)
    gpu_ctx.op_enc_s2d_residual(dev(conv), Cc, dev(x), Cx, o, Cout, T, H, W, ft, fh, fw)
    got = host_f32(o, want.size, want.shape)
    assert report("enc_s2d_residual G=3", np.abs(got - want), (G + 1) * U * (np.abs(c_part) + x_abs))


@pytest.mark.parametrize("C,P,ldz", [(128, 1, 128), (128, 6, 128), (5, 7, 12)])
def test_enc_finish(gpu_ctx, C, P, ldz):
    """Without statistics a bit-equal transpose of the first C of ldz columns. With integer z and mean and a power-of-two std, each
    different in every channel, bit-equal again. With random statistics 2 U |result|: one subtraction, one correctly rounded division."""
    rng = np.random.default_rng(C + P)
    z = rng.integers(-500, 501, (P, ldz)).astype(np.float32)
    mean = (rng.permutation(C) - C // 2).astype(np.float32)
    std = (2.0 ** (rng.permutation(C) - C // 2)).astype(np.float32)  # 2^-64 .. 2^63: (z - mean) / std stays an exact f32
    assert len(set(mean)) == C == len(set(std))
    d_z = dev(z)
    slack = 32 * max(C, P)
    o = out_f32(C * P, slack)
    gpu_ctx.op_enc_finish(d_z, ldz, o, C, P)
    assert same_f32_bits(host_f32(o, C * P, (C, P)), exact_f32(ref.enc_finish(z, C)))
    o = out_f32(C * P, slack)
    gpu_ctx.op_enc_finish(d_z, ldz, o, C, P, mean=dev(mean), std=dev(std))
    assert same_f32_bits(host_f32(o, C * P, (C, P)), exact_f32(ref.enc_finish(z, C, mean, std)))
    z = rng.standard_normal((P, ldz)).astype(np.float32)
    mean = (0.2 * rng.standard_normal(C)).astype(np.float32)
    std = (1.0 + 0.3 * rng.random(C)).astype(np.float32)
    o = out_f32(C * P, slack)
    gpu_ctx.op_enc_finish(dev(z), ldz, o, C, P, mean=dev(mean), std=dev(std))
    want = ref.enc_finish(z, C, mean, std)
    assert report(f"enc_finish C={C} P={P} ldz={ldz}", np.abs(host_f32(o, C * P, (C, P)) - want), 2 * U * np.abs(want))


# =====================================================================================================================================
# connector registers, sequence-parallel interleave
# =====================================================================================================================================
PLAN_MASKS = {
    "1x1 valid": [[1]],
    "1x1 padded": [[0]],
    "3x9": [[0, 0, 0, 0, 1, 1, 1, 1, 1],      # left-padded, 5 valid
            [1, 1, 1, 1, 0, 0, 0, 0, 0],      # right-padded, 4 valid
            [1, 1, 1, 1, 1, 1, 1, 1, 1]],     # all valid
    "2x5": [[0, 0, 0, 0, 0],                  # all padded
            [1, 0, 1, 1, 0]],                 # holes
}


@pytest.mark.parametrize("name", sorted(PLAN_MASKS))
def test_register_plan(gpu_ctx, name):
    """Exact equality of the int32 plan with the reference (which tests/test_helper_passes_host.py checks against plans worked out by
    hand and against a loop): the valid tokens first, the padded ones after, -1 where the REVERSED mask is 0."""
    mask = np.array(PLAN_MASKS[name], np.int32)
    B, T = mask.shape
    src = out_i32(B * T, 64)
    gpu_ctx.op_register_plan(dev(mask, np.int32), B, T, src)
    assert np.array_equal(host_i32(src, B * T, (B, T)), ref.register_plan(mask))
    # any non-zero entry is valid
    gpu_ctx.op_register_plan(dev(mask * 7, np.int32), B, T, src)
    assert np.array_equal(host_i32(src, B * T, (B, T)), ref.register_plan(mask))


GATHER_CASES = [
    (1, 1, 8, 1, ref.register_plan(PLAN_MASKS["1x1 valid"])),
    (1, 1, 8, 1, ref.register_plan(PLAN_MASKS["1x1 padded"])),
    (2, 9, 264, 4, ref.register_plan(PLAN_MASKS["3x9"])[:2]),                      # registers at p = 5 .. 8 (row 0) and 0 .. 4 (row 1): p % 4 wraps
    (2, 9, 264, 4, np.array([[3, -1, 0, 8, -1, -1, 2, 2, -1], [-1] * 9], np.int32)),  # by hand: p % 4 wraps twice (p = 8), a token taken twice
    (1, 5, 512, 8, ref.register_plan(PLAN_MASKS["2x5"])[1:]),                     # R > T
    (1, 5, 512, 8, ref.register_plan(PLAN_MASKS["2x5"])[:1]),
]


@pytest.mark.parametrize("B,T,D,R,src", GATHER_CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}-{c[3]}-{i}" for i, c in enumerate(GATHER_CASES)])
def test_register_gather(gpu_ctx, B, T, D, R, src):
    """D = 264: one full trip of the 256 threads and a ragged second one. Every element of enc has its own bf16 bit pattern (positive
    normal numbers from 0x0100 up) and every register element its own integer, so the f32 output names the source of every element."""
    assert src.shape == (B, T) and B * T * D < 0x7F00 - 0x0100
    enc_bits = (0x0100 + np.arange(B * T * D)).astype(np.uint16).reshape(B, T, D)
    registers = (100000 + np.arange(R * D)).astype(np.float32).reshape(R, D)
    want = ref.register_gather(ref.from_bf16_bits(enc_bits), registers, src)
    x = out_f32(B * T * D, D)
    gpu_ctx.op_register_gather(dev_bits(enc_bits), dev(registers), dev(src, np.int32), B, T, D, R, x)
    assert same_f32_bits(host_f32(x, B * T * D, (B, T, D)), exact_f32(want))


@pytest.mark.parametrize("N,D,Tn,ld", [(1, 1, 8, 8), (2, 3, 8, 16), (4, 128, 24, 104), (3, 5, 16, 48)])
def test_sp_vt_interleave(gpu_ctx, N, D, Tn, ld):
    """Every element has its own bf16 bit pattern (the pass moves bits; 12288 of them at (4, 128, 24), more than there are bf16-exact
    integers). (4, 128, 24, 104): 3 pieces of 8 keys per row, ld > N Tn - columns 96 .. 103 keep the sentinel. Against
    g.transpose(1, 0, 2).reshape(D, N Tn)."""
    bits = (0x0080 + np.arange(N * D * Tn)).astype(np.uint16).reshape(N, D, Tn)
    assert bits.max() < SENTINEL_BITS
    want = ref.sp_vt_interleave(ref.from_bf16_bits(bits))
    assert np.array_equal(want, ref.from_bf16_bits(bits).transpose(1, 0, 2).reshape(D, N * Tn))
    plane = (D, 1)
    o, n = haloed(plane, ld)
    gpu_ctx.op_sp_vt_interleave(dev_bits(bits), o, N, D, Tn, ld)
    got = interior(o, n, plane, ld, (0, 0), (D, 1), N * Tn)[:, 0, :]
    assert np.array_equal(ref.from_bf16_bits(got), want)


# =====================================================================================================================================
# integer plans: image-to-video row map and timesteps, constant fill, the text encoder's mask scan
# =====================================================================================================================================
@pytest.mark.parametrize("B,T,first,G", [(1, 1, 0, 1), (1, 1, 1, 2), (2, 300, 77, 2), (2, 9, 9, 3)])
def test_i2v_rowmap(gpu_ctx, B, T, first, G):
    """No token, some tokens and every token in frame 0; 600 entries are 2.3 workgroups."""
    o = out_i32(B * T, 256)
    gpu_ctx.op_i2v_rowmap(o, B, T, first, G)
    want = ref.i2v_rowmap(B, T, first, G)
    assert want[B - 1, 0] == (B - 1) * G + (first > 0) and want[B - 1, T - 1] == (B - 1) * G + (first == T)
    assert np.array_equal(host_i32(o, B * T, (B, T)), want)


@pytest.mark.parametrize("B,G", [(1, 1), (2, 2), (8, 7)])
def test_i2v_timesteps(gpu_ctx, B, G):
    """(8, 7): B G + B = 64, every thread of the one wave that writes them."""
    sigma = 0.909375
    o = out_f32(B * G + B, 64)
    gpu_ctx.op_i2v_timesteps(o, B, G, sigma)
    assert same_f32_bits(host_f32(o, B * G + B), ref.i2v_timesteps(B, G, sigma))


@pytest.mark.parametrize("n", [1, 257, 1031])
def test_fill_const_i32(gpu_ctx, n):
    o = out_i32(n, 256)
    gpu_ctx.op_fill_const_i32(o, n, -7)
    assert np.array_equal(host_i32(o, n), np.full(n, -7, np.int32))


@pytest.mark.parametrize("T", [1, 9, 300])
def test_gemma_mask_scan(gpu_ctx, T):
    """All ones, all zeros, left padding down to a single 1 in the last place, right padding, a hole, a value that is neither 0 nor 1;
    T = 300 is more than the 256 threads of the row's workgroup, with the first 1 on either side of 256."""
    rows = [np.ones(T, np.int32), np.zeros(T, np.int32)]
    for start in sorted({T - 1, T // 2, min(T - 1, 255), min(T - 1, 256)}):
        m = np.zeros(T, np.int32)
        m[start:] = 1
        rows.append(m)
        rows.append(m[::-1].copy())              # right padding
        hole = m.copy()
        hole[min(T - 1, start + 1)] = 0
        rows.append(hole)
        two = m.copy()
        two[start // 2] = 2
        rows.append(two)
    mask = np.stack(rows)
    B = len(rows)
    want_start, want_status = ref.gemma_mask_scan(mask)
    assert want_status[0] == 1 and want_status[1] == 0 and want_start[1] == T and want_status[2] == 1 and 0 < want_status.sum() < B
    ks, st = out_i32(B, 64), out_i32(B, 64)
    gpu_ctx.op_gemma_mask_scan(dev(mask, np.int32), B, T, ks, st)
    assert np.array_equal(host_i32(ks, B), want_start)
    assert np.array_equal(host_i32(st, B), want_status)


# =====================================================================================================================================
# timestep embedding
# =====================================================================================================================================
@pytest.mark.parametrize("mult", [1000.0, 1.0])
@pytest.mark.parametrize("n,dim", [(1, 2), (1, 256), (3, 256), (5, 64)])
def test_timestep_embedding(gpu_ctx, n, dim, mult):
    """Cosines in the first half of a row, sines in the second; ts = 0 gives exactly (1, 0). The bound is MEASURED: the error of a numpy
    float32 replay of the same operations against the float64 formula, per row (it grows with t = ts * mult: at t = 1000 the argument
    alone carries 1000 U). The kernel must stay within 4 times that plus 4 U - the 4 covers the last places in which the device's
    expf / sinf / cosf differ from numpy's."""
    vals = np.array([0.0, 1e-3, 0.5, 1.0], np.float32)
    ok = True
    for s in (range(4) if n == 1 else (0, 1)):
        ts = np.resize(np.roll(vals, -s), n)
        want = ref.timestep_embedding(ts, mult, dim)
        assert np.array_equal(want[:, :dim // 2], np.cos(ts.astype(np.float64)[:, None] * mult * ref.timestep_frequencies(dim)[None, :]))
        replay = np.abs(ref.timestep_embedding_f32(ts, mult, dim) - want).max(axis=1, keepdims=True)
        o = out_f32(n * dim, 256)
        gpu_ctx.op_timestep_embedding(dev(ts), mult, o, n, dim)
        got = host_f32(o, n * dim, (n, dim))
        err = np.abs(got - want)
        print(f"timestep_embedding n={n} dim={dim} mult={mult} ts={ts.tolist()}: f32 replay error per row {replay[:, 0].tolist()}, "
              f"kernel error per row {err.max(axis=1).tolist()}")
        ok &= report(f"timestep_embedding n={n} dim={dim} mult={mult}", err, 4 * replay + 4 * U)
        for r in np.flatnonzero(ts == 0):
            assert same_f32_bits(got[r], np.concatenate([np.ones(dim // 2), np.zeros(dim // 2)]))
    assert ok


# =====================================================================================================================================
# guidance combines, modulation tables, clip, bias, casts
# =====================================================================================================================================
COMBINES = {
    # name: (seam call, reference, coefficients of the exact run, of the random run, sum of the absolute terms)
    "cfg_combine": (lambda c, a, b, k, o, n: c.op_cfg_combine(a, b, k[0], o, n), lambda a, b, k: ref.cfg_combine(a, b, *k), (3.0,), (3.3,),
                    lambda a, b, k: np.abs(b) + abs(ref.f32(np.float32(k[0]) - np.float32(1))) * (np.abs(b) + np.abs(a))),
    "lincomb": (lambda c, a, b, k, o, n: c.op_lincomb(a, b, k[0], k[1], o, n), lambda a, b, k: ref.lincomb(a, b, *k), (2.0, -0.5), (0.7, -1.3),
                lambda a, b, k: abs(k[0]) * np.abs(a) + abs(k[1]) * np.abs(b)),
    "axpby": (lambda c, a, b, k, o, n: c.op_axpby(a, b, k[0], k[1], o, n), lambda a, b, k: ref.axpby(a, b, *k), (0.5, 2.0), (0.7, 1.0),
              lambda a, b, k: abs(k[1]) * np.abs(a) + abs(k[0]) * (np.abs(a) + np.abs(b))),
    "ge": (lambda c, a, b, k, o, n: c.op_ge(a, b, k[0], o, n), lambda a, b, k: ref.ge(a, b, *k), (0.25,), (0.3,),
           lambda a, b, k: abs(k[0]) * (np.abs(a) + np.abs(b)) + np.abs(b)),
}


@pytest.mark.parametrize("n", [1, 255, 257, 1031])
@pytest.mark.parametrize("name", sorted(COMBINES))
def test_combines(gpu_ctx, name, n):
    """Exact: multiples of 4 in [-512, 512] with power-of-two coefficients - no rounding anywhere, so only the operand order is left:
    cfg_combine(uncond, cond) is cond + 2 (cond - uncond), not the reverse, axpby is 2 a + 0.5 (a - b), ge is 0.25 (a - b) + b.
    Random: three roundings at most reach the result (a difference or a product, a product, the sum; a multiply-add may fuse and save
    one) of terms whose absolute values sum to the last entry of COMBINES: 3 U of that sum."""
    call, reference, exact_k, random_k, terms = COMBINES[name]
    rng = np.random.default_rng(n)
    a, b = (4 * rng.integers(-128, 129, n)).astype(np.float32), (4 * rng.integers(-128, 129, n)).astype(np.float32)
    o = out_f32(n, 256)
    call(gpu_ctx, dev(a), dev(b), exact_k, o, n)
    assert same_f32_bits(host_f32(o, n), exact_f32(reference(a, b, exact_k)))
    assert n == 1 or not np.array_equal(reference(a, b, exact_k), reference(b, a, exact_k))
    a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    o = out_f32(n, 256)
    call(gpu_ctx, dev(a), dev(b), random_k, o, n)
    k32 = tuple(ref.f32(v) for v in random_k)
    assert report(f"{name} n={n}", np.abs(host_f32(o, n) - reference(a, b, random_k)), 3 * U * terms(a.astype(np.float64), b.astype(np.float64), k32))


@pytest.mark.parametrize("n", [1, 255, 257, 1031])
def test_scale_inplace(gpu_ctx, n):
    """In place; integers by 0.5 bit-equal, random data by 0.7 within the one rounding of the product."""
    rng = np.random.default_rng(n)
    for x, s in ((rng.integers(-512, 513, n).astype(np.float32), 0.5), (rng.standard_normal(n).astype(np.float32), 0.7)):
        o = out_f32(n, 256)
        o[:n] = dev(x)
        gpu_ctx.op_scale_inplace(o, s, n)
        want = ref.scale(x, s)
        if s == 0.5:
            assert same_f32_bits(host_f32(o, n), exact_f32(want))
        else:
            assert report(f"scale_inplace n={n}", np.abs(host_f32(o, n) - want), U * np.abs(want))


def test_vae_make_mods_batch(ltx, gpu_ctx):
    """Three jobs of (rows, C) = (2, 4), (4, 128), (2, 1024) in one launch, the second without te: integers, bit-equal, + 1 on the odd
    rows only. (2, 1024) is 2048 elements for the job's 4 x 256 threads: two trips of the stride loop. Then as many jobs as the struct
    holds; one more is refused (test_rejections)."""
    rng = np.random.default_rng(9)

    def job(rows, C, with_te):
        table = rng.integers(-1000, 1001, (rows, C)).astype(np.float32)
        te = rng.integers(-1000, 1001, (rows, C)).astype(np.float32) if with_te else None
        return table, te, out_f32(rows * C, 256)

    def run(shapes):
        jobs = [job(*s) for s in shapes]
        gpu_ctx.op_vae_make_mods_batch([(dev(t), None if te is None else dev(te), o, s[0], s[1]) for (t, te, o), s in zip(jobs, shapes)])
        for (t, te, o), (rows, C, _) in zip(jobs, shapes):
            want = ref.vae_make_mods(t, te)
            assert same_f32_bits(host_f32(o, rows * C, (rows, C)), exact_f32(want)), (rows, C)

    run([(2, 4, True), (4, 128, False), (2, 1024, True)])
    most = ltx.lib.ltx_vae_mods_max_jobs()
    assert most == 24
    run([(2, 4 + 4 * (i % 3), i % 2 == 0) for i in range(most)])


CLIP_IN = np.array([-3.0, -1.0, -0.5, 0.0, 0.5, 1.0, 3.0], np.float32)


@pytest.mark.parametrize("n", [1, 1031, CLIP01_CAP + 5])
def test_clip01(gpu_ctx, n):
    """The seven values in rotation: 0, 0, 0.25, 0.5, 0.75, 1, 1, every zero a +0 (bits compared). The last length is 5 elements past
    what 65535 * 16 workgroups of 256 cover in one trip (1 GiB of f32; compared on the device)."""
    want7 = ref.clip01(CLIP_IN).astype(np.float32)
    assert want7.tolist() == [0.0, 0.0, 0.25, 0.5, 0.75, 1.0, 1.0] and not np.signbit(want7).any()
    assert (n > CLIP01_CAP) == (n > 2000)
    reps = -(-n // 7)
    x = out_f32(n, 256)
    x[:n] = dev(CLIP_IN).repeat(reps)[:n]
    gpu_ctx.op_clip01(x, n)
    torch.cuda.synchronize()
    want = dev(want7).repeat(reps)[:n]
    assert torch.equal(x[:n].view(torch.int32), want.view(torch.int32))
    assert bool((x[n:] == SENTINEL_F32).all())


@pytest.mark.parametrize("n", [1, 300])
def test_mask_to_bias(gpu_ctx, n):
    """0 -> -10000 and 1 -> 0, and that zero is +0: (1 - 1) * -10000 alone is -0."""
    rng = np.random.default_rng(n)
    for mask in ([np.zeros(1, np.int32), np.ones(1, np.int32)] if n == 1 else [rng.integers(0, 2, n).astype(np.int32)]):
        o = out_f32(n, 256)
        gpu_ctx.op_mask_to_bias(dev(mask, np.int32), o, n)
        want = ref.mask_to_bias(mask)
        assert set(want.tolist()) <= {0.0, -10000.0} and not np.signbit(want[mask == 1]).any()
        assert same_f32_bits(host_f32(o, n), want)


def f32_rounding_cases():
    """Every kind of f32 -> bf16 rounding: ties to even both ways and their neighbours, a round-up into the next exponent, the zeros, f32
    subnormals, the bf16 subnormal range with its ties, the largest finite values (the last rounds to infinity), the infinities."""
    b = lambda u: np.array([u], np.uint32).view(np.float32)[0]
    pos = [b(0x3F800000), b(0x3F808000), b(0x3F807FFF), b(0x3F808001),   # 1, the tie above it (down to even), its neighbours
           b(0x3F818000), b(0x3F817FFF), b(0x3F818001),                  # the tie above 1 + 2^-7 (up to even), its neighbours
           b(0x3FFFFFFF), b(0x3FFF8000), b(0x407FFFFF),                  # round up into the next exponent
           b(0x00000000), b(0x00000001), b(0x007FFFFF), b(0x00008000), b(0x00018000), b(0x00008001), b(0x00010000),
           b(0x00800000), b(0x007F8000),                                 # smallest normal; the tie that rounds up INTO it
           b(0x7F7F0000), b(0x7F7F7FFF), b(0x7F7F8000), b(0x7F7FFFFF), b(0x7F800000),
           np.float32(3.14159274), np.float32(1e-3), np.float32(12345.678)]
    pos = np.array(pos, np.float32)
    return np.concatenate([pos, -pos])


CAST_LENGTHS = [1, 3, 4, 5, 7, 1024, 1027]


@pytest.mark.parametrize("n", CAST_LENGTHS + [CAST_F32_BF16_CAP + 1027])
def test_cast_f32_bf16(gpu_ctx, n):
    """The vector body (4 elements per thread) and the scalar tail at every n % 4; the last length is 1027 elements (n % 4 = 3) past what
    2048 workgroups x 256 threads x 4 cover in one trip. The rounding cases rotate through the array so that each length ends in
    different ones; bit-equal against the definition on the bits, which the host tests tie to helper_pass_ref.bf16. NaN stays NaN."""
    assert (n > CAST_F32_BF16_CAP) == (n > 2000) and (n < 2000 or n % 4 in (0, 3))
    vals = f32_rounding_cases()
    x = np.resize(np.roll(vals, n), n)
    if n >= 4:
        x[n // 2] = np.nan
        x[n - 1] = -np.nan
    nan = np.isnan(x)
    o = out_bf16(n, 1024)
    gpu_ctx.op_cast_f32_bf16(dev(x), o, n)
    got = host_bf16(o, n)
    assert np.array_equal(got[~nan], ref.bf16_rne_bits(x[~nan]))
    assert np.all((got[nan] & 0x7F80) == 0x7F80) and np.all((got[nan] & 0x007F) != 0)
    normal = ~nan & (np.abs(x) >= 2.0 ** -126) & (np.abs(x) < 3.3e38)  # where helper_pass_ref.bf16 is defined: the same bits
    assert np.array_equal(got[normal], ref.bf16_bits(ref.bf16(x[normal])))


@pytest.mark.parametrize("n", CAST_LENGTHS + [65536, CAST_BF16_F32_CAP + 1027])
def test_cast_bf16_f32(gpu_ctx, n):
    """All 65536 bit patterns (n = 65536 holds each once, the longer case many times; the short ones take a window that moves with n):
    the f32 is the pattern shifted up by 16 bits. A NaN must come back as a NaN, whatever its payload."""
    assert (n > CAST_BF16_F32_CAP) == (n > 65536)
    start = 0 if n >= 65536 else 0x7F00 + 31 * n
    bits = ((start + np.arange(n)) % 65536).astype(np.uint16)
    o = out_f32(n, 256)
    gpu_ctx.op_cast_bf16_f32(dev_bits(bits), o, n)
    got = host_f32(o, n)
    want = (bits.astype(np.uint32) << 16).view(np.float32)
    nan = np.isnan(want)
    assert n < 65536 or nan.sum() >= 254
    assert np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))
    assert np.isnan(got[nan]).all()


# =====================================================================================================================================
# rejections
# =====================================================================================================================================
def test_rejections(ltx, gpu_ctx):
    """Every seam refuses, with invalidConfiguration and before anything is launched, a null operand, an empty extent and each shape its
    launcher does not take or would index out of range with. The sentinel-filled outputs are untouched afterwards."""
    N = 4096
    f, h, i = out_f32(N, 256), out_bf16(N, 256), out_i32(N, 256)
    a = dev(np.ones(N, np.float32))
    ab = dev_bits(np.full(N, 0x3F80, np.uint16))
    m = dev(np.ones(N, np.int32), np.int32)
    c = gpu_ctx
    most = ltx.lib.ltx_vae_mods_max_jobs()
    calls = [
        lambda: c.op_cfg_combine(None, a, 2.0, f, 8), lambda: c.op_cfg_combine(a, None, 2.0, f, 8),
        lambda: c.op_cfg_combine(a, a, 2.0, None, 8), lambda: c.op_cfg_combine(a, a, 2.0, f, 0),
        lambda: c.op_lincomb(None, a, 1.0, 1.0, f, 8), lambda: c.op_lincomb(a, a, 1.0, 1.0, f, 0),
        lambda: c.op_axpby(a, None, 1.0, 1.0, f, 8), lambda: c.op_axpby(a, a, 1.0, 1.0, f, -1),
        lambda: c.op_ge(a, a, 0.5, None, 8), lambda: c.op_ge(a, a, 0.5, f, 0),
        lambda: c.op_scale_inplace(None, 2.0, 8), lambda: c.op_scale_inplace(f, 2.0, 0),
        lambda: c.op_clip01(None, 8), lambda: c.op_clip01(f, 0),
        lambda: c.op_mask_to_bias(None, f, 8), lambda: c.op_mask_to_bias(m, None, 8), lambda: c.op_mask_to_bias(m, f, 0),
        lambda: c.op_cast_f32_bf16(None, h, 8), lambda: c.op_cast_f32_bf16(a, None, 8), lambda: c.op_cast_f32_bf16(a, h, 0),
        lambda: c.op_cast_bf16_f32(None, f, 8), lambda: c.op_cast_bf16_f32(ab, None, 8), lambda: c.op_cast_bf16_f32(ab, f, 0),
        lambda: c.op_timestep_embedding(None, 1.0, f, 2, 8), lambda: c.op_timestep_embedding(a, 1.0, None, 2, 8),
        lambda: c.op_timestep_embedding(a, 1.0, f, 0, 8), lambda: c.op_timestep_embedding(a, 1.0, f, 2, 7),
        lambda: c.op_timestep_embedding(a, 1.0, f, 2, 0),
        lambda: c.op_vae_make_mods_batch([]), lambda: c.op_vae_make_mods_batch([(a, a, f, 2, 4)] * (most + 1)),
        lambda: c.op_vae_make_mods_batch([(None, a, f, 2, 4)]), lambda: c.op_vae_make_mods_batch([(a, a, None, 2, 4)]),
        lambda: c.op_vae_make_mods_batch([(a, a, f, 0, 4)]), lambda: c.op_vae_make_mods_batch([(a, a, f, 2, 4), (a, a, f, 2, 0)]),
        lambda: c.op_sp_vt_interleave(None, h, 2, 3, 8, 16), lambda: c.op_sp_vt_interleave(ab, None, 2, 3, 8, 16),
        lambda: c.op_sp_vt_interleave(ab, h, 0, 3, 8, 16), lambda: c.op_sp_vt_interleave(ab, h, 2, 0, 8, 16),
        lambda: c.op_sp_vt_interleave(ab, h, 2, 3, 4, 16), lambda: c.op_sp_vt_interleave(ab, h, 2, 3, 12, 24),
        lambda: c.op_sp_vt_interleave(ab, h, 2, 3, 8, 20), lambda: c.op_sp_vt_interleave(ab, h, 2, 3, 8, 8),
        lambda: c.op_register_plan(None, 2, 4, i), lambda: c.op_register_plan(m, 2, 4, None),
        lambda: c.op_register_plan(m, 0, 4, i), lambda: c.op_register_plan(m, 2, 0, i),
        lambda: c.op_register_gather(None, a, m, 1, 4, 8, 2, f), lambda: c.op_register_gather(ab, None, m, 1, 4, 8, 2, f),
        lambda: c.op_register_gather(ab, a, None, 1, 4, 8, 2, f), lambda: c.op_register_gather(ab, a, m, 1, 4, 8, 2, None),
        lambda: c.op_register_gather(ab, a, m, 1, 4, 8, 0, f), lambda: c.op_register_gather(ab, a, m, 1, 4, 0, 2, f),
        lambda: c.op_register_gather(ab, a, m, 0, 4, 8, 2, f),
        lambda: c.op_enc_patchify(None, h, 1, 4, 4), lambda: c.op_enc_patchify(a, None, 1, 4, 4), lambda: c.op_enc_patchify(a, h, 0, 4, 4),
        lambda: c.op_enc_patchify(a, h, 1, 6, 4), lambda: c.op_enc_patchify(a, h, 1, 4, 2),
        lambda: c.op_enc_s2d_residual(None, 2, a, 2, f, 16, 2, 2, 2, 2, 2, 2), lambda: c.op_enc_s2d_residual(a, 2, a, 2, None, 16, 2, 2, 2, 2, 2, 2),
        lambda: c.op_enc_s2d_residual(a, 2, a, 2, f, 16, 0, 2, 2, 2, 2, 2), lambda: c.op_enc_s2d_residual(a, 2, a, 2, f, 16, 2, 2, 2, 0, 2, 2),
        lambda: c.op_enc_s2d_residual(a, 2, a, 2, f, 16, 2, 3, 2, 2, 2, 2), lambda: c.op_enc_s2d_residual(a, 2, a, 2, f, 16, 2, 2, 3, 2, 2, 2),
        lambda: c.op_enc_s2d_residual(a, 2, a, 2, f, 8, 2, 2, 2, 2, 2, 2),    # Cc S = 16 != Cout
        lambda: c.op_enc_s2d_residual(a, 3, a, 2, f, 24, 2, 2, 2, 2, 2, 2),   # Cx S = 16 is no multiple of Cout = 24
        lambda: c.op_enc_finish(None, 8, f, 8, 4), lambda: c.op_enc_finish(a, 8, None, 8, 4), lambda: c.op_enc_finish(a, 8, f, 8, 0),
        lambda: c.op_enc_finish(a, 8, f, 0, 4), lambda: c.op_enc_finish(a, 7, f, 8, 4),
        lambda: c.op_enc_finish(a, 8, f, 8, 4, mean=a), lambda: c.op_enc_finish(a, 8, f, 8, 4, std=a),
        lambda: c.op_audio_pn_pad(None, 2, 2, 8, 0, h), lambda: c.op_audio_pn_pad(a, 2, 2, 8, 0, None),
        lambda: c.op_audio_pn_pad(a, 0, 2, 8, 0, h), lambda: c.op_audio_pn_pad(a, 2, 2, 0, 1, h), lambda: c.op_audio_pn_pad(a, 2, 2, 8, 2, h),
        lambda: c.op_audio_upsample_pad(None, 2, 2, 8, h), lambda: c.op_audio_upsample_pad(a, 2, 0, 8, h),
        lambda: c.op_audio_upsample_pad(a, 2, 2, 6, h), lambda: c.op_audio_upsample_pad(a, 2, 2, 8, None),
        lambda: c.op_audio_denorm_pad(None, a, a, 3, 2, 4, 8, h), lambda: c.op_audio_denorm_pad(a, None, a, 3, 2, 4, 8, h),
        lambda: c.op_audio_denorm_pad(a, a, None, 3, 2, 4, 8, h), lambda: c.op_audio_denorm_pad(a, a, a, 3, 2, 4, 8, None),
        lambda: c.op_audio_denorm_pad(a, a, a, 3, 0, 4, 8, h), lambda: c.op_audio_denorm_pad(a, a, a, 3, 2, 4, 2, h),
        lambda: c.op_audio_mel_pack(None, 2, 8, h), lambda: c.op_audio_mel_pack(a, 2, 8, None), lambda: c.op_audio_mel_pack(a, 0, 8, h),
        lambda: c.op_audio_mel_pack(a, 2, 0, h),
        lambda: c.op_audio_mean3_act(None, a, a, 2, 8, 0.1, h, 8), lambda: c.op_audio_mean3_act(a, a, None, 2, 8, 0.1, h, 8),
        lambda: c.op_audio_mean3_act(a, a, a, 2, 8, 0.1, None, 8), lambda: c.op_audio_mean3_act(a, a, a, 0, 8, 0.1, h, 8),
        lambda: c.op_audio_mean3_act(a, a, a, 2, 6, 0.1, h, 8), lambda: c.op_audio_mean3_act(a, a, a, 2, 4, 0.1, h, 6),
        lambda: c.op_audio_mean3_act(a, a, a, 2, 8, 0.1, h, 4),
        lambda: c.op_i2v_rowmap(None, 2, 4, 1, 2), lambda: c.op_i2v_rowmap(i, 0, 4, 1, 2), lambda: c.op_i2v_rowmap(i, 2, 0, 0, 2),
        lambda: c.op_i2v_rowmap(i, 2, 4, 5, 2), lambda: c.op_i2v_rowmap(i, 2, 4, -1, 2), lambda: c.op_i2v_rowmap(i, 2, 4, 1, 0),
        lambda: c.op_i2v_timesteps(None, 2, 2, 0.5), lambda: c.op_i2v_timesteps(f, 0, 2, 0.5), lambda: c.op_i2v_timesteps(f, 2, 0, 0.5),
        lambda: c.op_i2v_timesteps(f, 9, 7, 0.5),     # 72 entries for the 64 threads
        lambda: c.op_fill_const_i32(None, 8, 1), lambda: c.op_fill_const_i32(i, 0, 1),
        lambda: c.op_gemma_mask_scan(None, 2, 4, i, i), lambda: c.op_gemma_mask_scan(m, 2, 4, None, i),
        lambda: c.op_gemma_mask_scan(m, 2, 4, i, None), lambda: c.op_gemma_mask_scan(m, 0, 4, i, i),
        lambda: c.op_gemma_mask_scan(m, 2, 0, i, i),
    ]
    for k, call in enumerate(calls):
        with pytest.raises(ltx.LTXError) as e:
            call()
        assert e.value.case == "invalidConfiguration", (k, e.value)
    host_f32(f, 0), host_bf16(h, 0), host_i32(i, 0)  # all sentinel, from the first element on
    assert np.all(a.cpu().numpy() == 1.0)
    # and each seam takes the smallest valid call (the refusals above are of the arguments, not of the seam)
    c.op_cfg_combine(a, a, 2.0, f, 1)
    assert host_f32(f, 1)[0] == 1.0
