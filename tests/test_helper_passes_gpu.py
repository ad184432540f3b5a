"""The helper passes of csrc/elementwise.hip that no other ltx_op_* seam reaches - guidance (mean_var, guidance_rescale, adain), the
scheduler (euler_step, set_frame0, make_mod, patchify / unpatchify), the VAE (vae_prepare, pixelnorm_silu, blend_frames), the latent
upscaler (groupnorm_stats / apply, upscaler_finish) and the connector's feature statistics (fe_stats, fe_norm_concat) - each on its own
through its seam, against the float64 restatement in tests/helpers/helper_pass_ref.py.

Which comparison applies:
  * layout passes: BIT-EQUAL. Inputs are integers (and powers of two where something is scaled), so every intermediate is exact and
    neither a fused multiply-add nor an operation order can move a bit; what is left is the indexing.
  * statistics and f32 arithmetic: a bound against float64 counted from the kernel's operations, U = 2^-24 per rounding
    (helper_pass_ref.gamma). Each test states its count.
  * bf16 outputs: `bf16_rule` - every element within one bf16 ulp (+ 1e-6) of bf16(float64), compared as VALUES, and at most 1e-3 of
    the elements different at all (the cap of test_gemma_rows_gpu.py). An f32 replay of pixel-norm + SiLU differs from the float64 one
    in 3e-5 .. 5e-5 of the elements, so the cap leaves about 20x room for the reference alone.

Every output is allocated with one tile of slack behind its valid extent and filled with a sentinel; the slack must keep it.

Paths that need a case of their own, and the case that takes each:
  * pixelnorm_silu instances: <8> C = 4, 36, 128; <16> C = 256; <32> C = 512; <64> C = 1000, 1024; <64, 8> C = 1028, 2048
    (test_pixelnorm_silu); the ragged last workgroup at P = 1, 3, 1031.
  * make_mod stride loop (grid cap 2048 x 256): test_make_mod[3-8-6-4096], 589824 elements.
  * groupnorm_apply stride loop (grid cap 4096 x 256): test_groupnorm_apply_above_the_grid_cap, 8200 x 128 = 1049600 elements.
  * fe_stats (FE_CHUNK = 16384 elements): one chunk [1-64-valid0]; ragged last chunk of two [1-96-valid1]; four chunks with the
    cross-chunk reduction, and chunks without a valid token (row 1 of [2-200-valid2], left padding: chunks 0 .. 2 of its planes
    hold nothing, their partials are (0, +inf, -inf)); each also with right padding."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import helper_pass_ref as ref  # noqa: E402
# device buffers with a guarded tail and the comparisons: shared with test_row_passes_rest_gpu.py
from guarded_buffers import (bf16_rule, dev, dev_bf16, exact_f32, host_bf16, host_f32, out_bf16, out_f32, report,  # noqa: E402
                             same_f32_bits)

pytestmark = pytest.mark.gpu
U = ref.U


# =====================================================================================================================================
# layout passes: bit-equal
# =====================================================================================================================================
@pytest.mark.parametrize("B,C,T", [(1, 128, 1), (2, 128, 33), (1, 36, 95), (2, 32, 64)])
def test_patchify_and_unpatchify(gpu_ctx, B, C, T):
    """Ragged tiles along both axes ((1, 36, 95): C % 32 = 4, T % 32 = 31), one column (T = 1), full tiles, two batch elements."""
    rng = np.random.default_rng(B * 1000 + C + T)
    lat = rng.integers(-128, 129, (B, C, T)).astype(np.float32)
    slack = 32 * max(C, T)
    tok = out_bf16(B * T * C, slack)
    gpu_ctx.op_patchify_bf16(dev(lat), tok, B, C, T)
    assert np.array_equal(host_bf16(tok, B * T * C, (B, T, C)), ref.bf16_bits(ref.patchify(lat)))
    tok32 = rng.integers(-128, 129, (B, T, C)).astype(np.float32)
    back = out_f32(B * C * T, slack)
    gpu_ctx.op_unpatchify_f32(dev(tok32), back, B, C, T)
    assert same_f32_bits(host_f32(back, B * C * T, (B, C, T)), ref.unpatchify(tok32))
    # the round trip: tokens of the latent, widened to f32, come back as the latent
    trip = out_f32(B * C * T, slack)
    gpu_ctx.op_unpatchify_f32(tok[:B * T * C].float().contiguous(), trip, B, C, T)
    assert same_f32_bits(host_f32(trip, B * C * T, (B, C, T)), lat)


@pytest.mark.parametrize("P", [1, 31, 32, 1031])
@pytest.mark.parametrize("C", [128, 36])
def test_vae_prepare(gpu_ctx, C, P):
    """Dense (chan_stride == P) and as a view at column 5 of a latent 37 columns longer (the temporal tile's view), without noise and
    with noise at scale 0.5 on even integers: 0.5 * even + 0.5 * even, times a power of two, plus an integer - every step exact, and
    the results (|v| <= 36, halves at most) are bf16 values."""
    rng = np.random.default_rng(C * 10000 + P)
    S, off = P + 37, 5
    full = (2 * rng.integers(-4, 5, (C, S))).astype(np.float32)
    noise_full = (2 * rng.integers(-4, 5, (C, S))).astype(np.float32)
    mean = rng.integers(-4, 5, C).astype(np.float32)
    std = rng.choice([0.5, 1.0, 2.0, 4.0], C).astype(np.float32)
    d_mean, d_std = dev(mean), dev(std)
    for strided in (False, True):
        lat = full[:, off:off + P]
        nz = noise_full[:, off:off + P]
        if strided:
            d_lat, d_nz, stride = dev(full)[:, off:], dev(noise_full)[:, off:], S
        else:
            d_lat, d_nz, stride = dev(lat), dev(nz), P
        for noise in (None, nz):
            out = out_bf16(P * C, 32 * C)
            gpu_ctx.op_vae_prepare(d_lat, stride, d_mean, d_std, out, C, P, noise=None if noise is None else d_nz, noise_scale=0.5)
            want = ref.vae_prepare(lat, noise, 0.5, mean, std)
            assert np.array_equal(host_bf16(out, P * C, (P, C)), ref.bf16_bits(want)), (strided, noise is not None)


@pytest.mark.parametrize("P", [1, 31, 32, 1031])
@pytest.mark.parametrize("C", [128, 36])
def test_upscaler_finish(gpu_ctx, C, P):
    """(integer - integer) / power of two: exact"""
    rng = np.random.default_rng(C * 10000 + P + 1)
    x = rng.integers(-64, 65, (P, C)).astype(np.float32)
    mean = rng.integers(-8, 9, C).astype(np.float32)
    std = rng.choice([0.25, 0.5, 1.0, 2.0, 8.0], C).astype(np.float32)
    out = out_f32(C * P, 32 * max(C, P))
    gpu_ctx.op_upscaler_finish(dev(x), dev(mean), dev(std), out, P, C)
    assert same_f32_bits(host_f32(out, C * P, (C, P)), exact_f32(ref.upscaler_finish(x, mean, std)))


@pytest.mark.parametrize("with_noise", [False, True])
def test_set_frame0(gpu_ctx, with_noise):
    """Bit-equal to the float32 replay of cond + (scale * noise) * sigma2, three separately rounded operations; frames 1 and 2 of
    every channel, and the guard behind the latent, keep every bit."""
    C, F, HW = 5, 3, 77
    rng = np.random.default_rng(11)
    lat = rng.standard_normal((C, F, HW)).astype(np.float32)
    cond = rng.standard_normal((C, HW)).astype(np.float32)
    noise = rng.standard_normal((C, HW)).astype(np.float32) if with_noise else None
    scale, sigma2 = np.float32(0.15), np.float32(0.909375) * np.float32(0.909375)
    d = out_f32(C * F * HW, 256)
    d[:C * F * HW] = dev(lat).reshape(-1)
    gpu_ctx.op_set_frame0(d, dev(cond), C, F, HW, noise=None if noise is None else dev(noise), scale=float(scale), sigma2=float(sigma2))
    got = host_f32(d, C * F * HW, (C, F, HW))
    want = ref.set_frame0_f32(lat, cond, noise, scale, sigma2)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got[:, 1:].view(np.uint32), lat[:, 1:].view(np.uint32))
    if with_noise:  # the case needs the three roundings: the fused form gives other bits somewhere
        fused = (cond.astype(np.float64) + (np.float64(scale) * noise) * np.float64(sigma2)).astype(np.float32)
        assert not np.array_equal(fused, want[:, 0])


@pytest.mark.parametrize("sigma_next", [0.0, 0.6])
@pytest.mark.parametrize("skip", [False, True])
def test_euler_step(gpu_ctx, skip, sigma_next):
    """n = 5 * 3 * 77 = 1155 (4.5 workgroups). Bound 4 U max(|x|, |sigma v|): the result takes four f32 roundings (sigma * v, x - ., the
    rescaled difference, the last sum) of quantities no larger than that, and the multiply-add may fuse. With skip_hw = HW frame 0 of
    every channel keeps every bit; the float64 reference says which indices those are."""
    C, F, HW = 5, 3, 77
    n = C * F * HW
    rng = np.random.default_rng(21)
    x = rng.standard_normal(n).astype(np.float32)
    v = rng.standard_normal(n).astype(np.float32)
    sigma = 0.85
    d = out_f32(n, 256)
    d[:n] = dev(x)
    gpu_ctx.op_euler_step(d, dev(v), sigma, sigma_next, n, skip_hw=HW if skip else 0, frames=F if skip else 1)
    got = host_f32(d, n)
    want, kept = ref.euler_step(x, v, sigma, sigma_next, HW if skip else 0, F)
    assert kept.sum() == (C * HW if skip else 0)
    assert np.array_equal(got[kept].view(np.uint32), x[kept].view(np.uint32))
    bound = 4 * U * np.maximum(np.abs(x), np.abs(ref.f32(sigma) * v.astype(np.float64)))
    assert report(f"euler_step skip={skip} sigma_next={sigma_next}", np.abs(got - want)[~kept], bound[~kept])
    assert not np.array_equal(got[~kept], x[~kept])


def test_blend_frames(gpu_ctx):
    """frame_elems = 333 (1.3 workgroups); the buffers hold 6 frames and only n_frames are blended. n_frames = 4: the weights are
    quarters and the inputs multiples of 4 - exact. n_frames = 3: w = f32(i / 3), 1 - w, two products and a sum (the multiply-add may
    fuse): four roundings of terms no larger than max(|r|, |nx|)."""
    E, held = 333, 6
    rng = np.random.default_rng(31)
    for n_frames in (4, 3):
        if n_frames == 4:
            r, nx = (4 * rng.integers(-32, 33, (held, E))).astype(np.float32), (4 * rng.integers(-32, 33, (held, E))).astype(np.float32)
        else:
            r, nx = rng.standard_normal((held, E)).astype(np.float32), rng.standard_normal((held, E)).astype(np.float32)
        d = out_f32(held * E, 256)
        d[:held * E] = dev(r).reshape(-1)
        gpu_ctx.op_blend_frames(d, dev(nx), n_frames, E)
        got = host_f32(d, held * E, (held, E))
        assert np.array_equal(got[n_frames:].view(np.uint32), r[n_frames:].view(np.uint32)), "frames past n_frames were touched"
        want = ref.blend_frames(r[:n_frames], nx[:n_frames], n_frames)
        if n_frames == 4:
            assert same_f32_bits(got[:4], exact_f32(want))
        else:
            bound = 4 * U * np.maximum(np.abs(r[:3]), np.abs(nx[:3]))
            assert report("blend_frames n_frames=3", np.abs(got[:3] - want), bound)
        assert np.array_equal(got[0].view(np.uint32), r[0].view(np.uint32))  # weight 0: frame 0 is the first tile's


@pytest.mark.parametrize("B,L,J,D", [(2, 3, 6, 64), (3, 8, 6, 4096)])
def test_make_mod(gpu_ctx, B, L, J, D):
    """(3, 8, 6, 4096) is 589824 elements, above the 2048 x 256 = 524288 that the capped grid covers in one pass."""
    rng = np.random.default_rng(B + L)
    tables = rng.integers(-1000, 1001, (L, J, D)).astype(np.float32)
    ada = rng.integers(-1000, 1001, (B, J, D)).astype(np.float32)
    n = B * L * J * D
    assert (n > 2048 * 256) == (D == 4096)
    out = out_f32(n, 256)
    gpu_ctx.op_make_mod(dev(tables), dev(ada), out, B, L, J, D)
    assert same_f32_bits(host_f32(out, n, (B, L, J, D)), exact_f32(ref.make_mod(tables, ada)))


# =====================================================================================================================================
# statistics and f32 arithmetic: derived bounds against float64
# =====================================================================================================================================
def mean_bound(n, mean_abs):
    """Each of the 1024 threads adds n / 1024 terms, the tree (6 shuffle levels + the 16 wave sums) then adds 16."""
    return (n / 1024 + 16) * U * mean_abs


def var_bound(n, var, mean_b):
    """The deviations are taken about the ROUNDED mean (+ mean_bound^2 exactly: sum (x - m')^2 / n = var + (m' - m)^2), and every
    square carries one more rounding and the deviation another: n / 1024 + 18 roundings of relative 2 U each (a square doubles the
    relative error of its argument)."""
    return var * (n / 1024 + 18) * 2 * U + mean_b ** 2


@pytest.mark.parametrize("n", [1, 1023, 1173, 100003])
@pytest.mark.parametrize("B", [1, 3])
def test_mean_var(gpu_ctx, B, n):
    """x = 50 + 0.01 z: the one-pass form E[x^2] - E[x]^2 loses every digit of this variance (2500 against 1e-4 in f32). n below,
    just above and far above the 1024 threads, none a multiple of it; B = 3 shows the segment indexing of x and stats."""
    rng = np.random.default_rng(B * 7 + n)
    x = (50.0 + 0.01 * rng.standard_normal((B, n))).astype(np.float32)
    stats = out_f32(2 * B, 64)
    gpu_ctx.op_mean_var(dev(x), n, B, stats)
    got = host_f32(stats, 2 * B, (B, 2)).astype(np.float64)
    m, v = ref.mean_var(x)
    mb = mean_bound(n, np.abs(x.astype(np.float64)).mean(axis=1))
    ok_mean = report(f"mean_var B={B} n={n} mean", np.abs(got[:, 0] - m), mb)
    ok_var = report(f"mean_var B={B} n={n} variance", np.abs(got[:, 1] - v), var_bound(n, v, mb)) if n > 1 else bool(np.all(got[:, 1] == 0))
    assert ok_mean and ok_var
    if n == 100003:  # what the two passes are for
        one_pass = (x * x).mean(axis=1, dtype=np.float32) - x.mean(axis=1, dtype=np.float32) ** 2
        assert np.all(np.abs(one_pass - v) > 10 * var_bound(n, v, mb))


@pytest.mark.parametrize("phi", [0.0, 0.7, 1.0])
def test_guidance_rescale(gpu_ctx, phi):
    """B = 2 with different statistics per batch element, n = 1173 (4.6 workgroups). The statistics come from the float64 reference, so
    only the apply is under test. The rescaled term phi * v * ratio carries the two standard deviations (1.5 U each: the rounding of
    var + 1e-8 is halved by the root, the root adds one), their ratio, the product with v and the product with phi: 5 U of
    |v| ratio. (1 - phi) * v and the final sum add at most U of |v| max(1, ratio) between them where the multiply-add fuses, and the
    whole stays inside 6 U |v| max(1, std_cond / std_cfg). phi = 0 returns cfg bit for bit."""
    B, n = 2, 1173
    rng = np.random.default_rng(41)
    cfg = (rng.standard_normal((B, n)) * np.array([[1.5], [0.4]])).astype(np.float32)
    cond = (rng.standard_normal((B, n)) * np.array([[0.9], [1.1]])).astype(np.float32)
    s_cfg = np.stack(ref.mean_var(cfg), axis=1).astype(np.float32)
    s_cond = np.stack(ref.mean_var(cond), axis=1).astype(np.float32)
    d = out_f32(B * n, 256)
    d[:B * n] = dev(cfg).reshape(-1)
    gpu_ctx.op_guidance_rescale(d, dev(s_cfg), dev(s_cond), phi, n, B)
    got = host_f32(d, B * n, (B, n))
    if phi == 0.0:
        assert np.array_equal(got.view(np.uint32), cfg.view(np.uint32))
        return
    want = ref.guidance_rescale(cfg, s_cfg[:, 1], s_cond[:, 1], phi)
    ratio = np.sqrt(s_cond[:, 1].astype(np.float64) + ref.EPS_STD) / np.sqrt(s_cfg[:, 1].astype(np.float64) + ref.EPS_STD)
    assert ratio[0] < 1 < ratio[1]
    bound = 6 * U * np.abs(cfg) * np.maximum(1.0, ratio)[:, None]
    assert report(f"guidance_rescale phi={phi}", np.abs(got - want), bound)
    assert not np.array_equal(got, cfg)


@pytest.mark.parametrize("device_stats", [False, True], ids=["reference stats", "op_mean_var stats"])
@pytest.mark.parametrize("factor", [1.0, 0.4])
def test_adain(gpu_ctx, factor, device_stats):
    """BC = 5 channels with different statistics, n = 1173. The float64 formula is evaluated on the f32 statistics the kernel reads.
    Count for y = t + mu_ref, t = (x - mu) / (sd + 1e-8) * sd_ref: six roundings reach t (the difference, sqrt(var), + 1e-8, the
    quotient, sqrt(var_ref), the product) and one more the sum: gamma(6) |t| + U |y|. The blend f y + (1 - f) x adds one rounding per
    product and one for the sum (1 - f is rounded to f32 once, to the same number on both sides):
    f err(y) + U (|f y| + |(1 - f) x| + |out|). The (1 + gamma(8)) factor covers the products of these terms."""
    BC, n = 5, 1173
    rng = np.random.default_rng(51)
    x = (rng.standard_normal((BC, n)) * rng.uniform(0.3, 3.0, (BC, 1)) + rng.uniform(-2, 2, (BC, 1))).astype(np.float32)
    r = (rng.standard_normal((BC, 801)) * rng.uniform(0.3, 3.0, (BC, 1)) + rng.uniform(-2, 2, (BC, 1))).astype(np.float32)
    if device_stats:
        sx, sr = out_f32(2 * BC, 64), out_f32(2 * BC, 64)
        gpu_ctx.op_mean_var(dev(x), n, BC, sx)
        gpu_ctx.op_mean_var(dev(r), 801, BC, sr)
        d_sx, d_sr = sx, sr
        sx, sr = host_f32(sx, 2 * BC, (BC, 2)), host_f32(sr, 2 * BC, (BC, 2))
        for s, data in ((sx, x), (sr, r)):  # they are the statistics of their rows, within test_mean_var's bounds
            m, v = ref.mean_var(data)
            mb = mean_bound(data.shape[1], np.abs(data.astype(np.float64)).mean(axis=1))
            assert np.all(np.abs(s[:, 0] - m) <= mb) and np.all(np.abs(s[:, 1] - v) <= var_bound(data.shape[1], v, mb))
    else:
        sx, sr = np.stack(ref.mean_var(x), axis=1).astype(np.float32), np.stack(ref.mean_var(r), axis=1).astype(np.float32)
        d_sx, d_sr = dev(sx), dev(sr)
    d = out_f32(BC * n, 256)
    d[:BC * n] = dev(x).reshape(-1)
    gpu_ctx.op_adain(d, d_sx, d_sr, factor, n, BC)
    got = host_f32(d, BC * n, (BC, n))
    y = ref.adain(x, sx[:, 0], sx[:, 1], sr[:, 0], sr[:, 1], 1.0)
    t = y - sr[:, 0].astype(np.float64)[:, None]
    err_y = ref.gamma(6) * np.abs(t) + U * np.abs(y)
    if factor >= 1.0:
        want, bound = y, err_y
    else:
        f = ref.f32(factor)
        want = ref.adain(x, sx[:, 0], sx[:, 1], sr[:, 0], sr[:, 1], factor)
        bound = f * err_y + U * (np.abs(f * y) + np.abs(ref.f32(1.0 - f) * x.astype(np.float64)) + np.abs(want))
    assert report(f"adain factor={factor} device_stats={device_stats}", np.abs(got - want), bound * (1 + ref.gamma(8)))
    assert not np.array_equal(got, x)


GN_EPS = 1e-5


@pytest.mark.parametrize("P,C,G", [(24, 128, 32), (1031, 96, 32), (777, 128, 1)])
def test_groupnorm_stats(gpu_ctx, P, C, G):
    """Input 20 + z: a one-pass variance would lose four digits. The mean has mean_var's bound with n = P * C / G (the same 1024-thread
    two-pass reduction, strided over the group's channels); rstd = (var + eps)^-1/2 moves by at most half the relative error of
    var + eps (taken at the lower end, var - bound), plus three roundings of its own (the sum, the square root, the reciprocal)."""
    rng = np.random.default_rng(P + C + G)
    x = (20.0 + rng.standard_normal((P, C)) * rng.uniform(0.5, 2.0, (1, C))).astype(np.float32)
    stats = out_f32(2 * G, 64)
    gpu_ctx.op_groupnorm_stats(dev(x), P, C, G, GN_EPS, stats)
    got = host_f32(stats, 2 * G, (G, 2)).astype(np.float64)
    m, rstd, v = ref.groupnorm_stats(x, G, GN_EPS)
    n = P * (C // G)
    grouped = np.abs(x.astype(np.float64)).reshape(P, G, C // G).transpose(1, 0, 2).reshape(G, -1)
    mb = mean_bound(n, grouped.mean(axis=1))
    vb = var_bound(n, v, mb)
    rel = 0.5 * vb / (v + ref.f32(GN_EPS) - vb) + ref.gamma(3)
    ok_mean = report(f"groupnorm_stats P={P} C={C} G={G} mean", np.abs(got[:, 0] - m), mb)
    ok_rstd = report(f"groupnorm_stats P={P} C={C} G={G} rstd", np.abs(got[:, 1] - rstd), rel * rstd)
    assert ok_mean and ok_rstd


def silu_error(pre, err_pre):
    """|SiLU'| <= 1.1 carries the error of the argument. The kernel's SiLU is x * rcp(1 + exp2(-x * log2(e))) on the hardware's
    1-ulp exp2 and reciprocal: relative to the result, 2 U |x| log2(e) for the rounded product in the exponent (and the rounded constant
    in it; the factor e^-x / (1 + e^-x) < 1 is dropped), 2 U for exp2, U for the sum, 2 U for the reciprocal, U for the product:
    (2.9 |x| + 6) U, written (3 |x| + 6) U."""
    return 1.1 * err_pre + (3 * np.abs(pre) + 6) * U * np.abs(ref.silu(pre))


def groupnorm_apply_case(gpu_ctx, P, C, G, seed, variants):
    rng = np.random.default_rng(seed)
    x = (20.0 + rng.standard_normal((P, C)) * rng.uniform(0.5, 2.0, (1, C))).astype(np.float32)
    w = (1.0 + 0.2 * rng.standard_normal(C)).astype(np.float32)
    b = (0.3 * rng.standard_normal(C)).astype(np.float32)
    resid = rng.standard_normal((P, C)).astype(np.float32)
    m, rstd, _ = ref.groupnorm_stats(x, G, GN_EPS)
    stats = np.stack([m, rstd], axis=1).astype(np.float32)  # the f32 statistics the kernel reads; the reference uses the same numbers
    d_x, d_stats, d_w, d_b, d_resid = dev(x), dev(stats), dev(w), dev(b), dev(resid)
    n = P * C
    for with_resid, act, want_f32, want_bf16 in variants:
        o32 = out_f32(n, 256 * 4) if want_f32 else None
        o16 = out_bf16(n, 256 * 4) if want_bf16 else None
        gpu_ctx.op_groupnorm_apply(d_x, d_stats, d_w, d_b, P, C, G, resid=d_resid if with_resid else None, act_silu=act, out_f32=o32, out_bf16=o16)
        want, t, y, pre = ref.groupnorm_apply(x, stats[:, 0], stats[:, 1], w, b, resid if with_resid else None, act)
        # three roundings reach t = (x - mean) * rstd * w, one the sum with b (it may fuse), one the sum with the residual
        err = ref.gamma(3) * np.abs(t) + U * np.abs(y) + (U * np.abs(pre) if with_resid else 0.0)
        if act:
            err = silu_error(pre, err)
        what = f"groupnorm_apply P={P} C={C} G={G} resid={with_resid} silu={act}"
        if want_f32:
            assert report(what + " f32", np.abs(host_f32(o32, n, (P, C)) - want), err * (1 + ref.gamma(8)))
        if want_bf16:
            assert bf16_rule(host_bf16(o16, n, (P, C)), want, what + " bf16")


def test_groupnorm_apply(gpu_ctx):
    """P = 77 positions of C = 96 in 32 groups of 3 channels (7392 elements: a ragged last workgroup); with and without the residual,
    with and without SiLU, as f32 only, bf16 only and both."""
    variants = [(r, a, f, h) for r in (False, True) for a in (False, True) for f, h in ((True, False), (False, True), (True, True))]
    groupnorm_apply_case(gpu_ctx, 77, 96, 32, 61, variants)


def test_groupnorm_apply_above_the_grid_cap(gpu_ctx):
    """8200 x 128 = 1049600 elements against the 4096 x 256 = 1048576 of one pass of the capped grid: the stride loop's second trip
    takes the last 1024."""
    assert 8200 * 128 > 4096 * 256
    groupnorm_apply_case(gpu_ctx, 8200, 128, 32, 62, [(True, True, True, True)])


# =====================================================================================================================================
# bf16 outputs
# =====================================================================================================================================
@pytest.mark.parametrize("C", [4, 36, 128, 256, 512, 1000, 1024, 1028, 2048])
def test_pixelnorm_silu(gpu_ctx, C):
    """Every template instance and both sides of each switch (module docstring), at P = 1, 3 and 1031 (a ragged last workgroup for every
    instance: 32, 16, 8 or 4 positions per workgroup), without modulation and with it."""
    rng = np.random.default_rng(C)
    scale = (1.0 + 0.2 * rng.standard_normal(C)).astype(np.float32)
    shift = (0.3 * rng.standard_normal(C)).astype(np.float32)
    d_scale, d_shift = dev(scale), dev(shift)
    ok = True
    for P in (1, 3, 1031):
        x = (rng.standard_normal((P, C)) * 3.0).astype(np.float32)
        d_x = dev(x)
        for mod in (False, True):
            out = out_bf16(P * C, 32 * C)
            gpu_ctx.op_pixelnorm_silu(d_x, out, P, C, scale=d_scale if mod else None, shift=d_shift if mod else None)
            want = ref.pixelnorm_silu(x, scale if mod else None, shift if mod else None)
            ok &= bf16_rule(host_bf16(out, P * C, (P, C)), want, f"pixelnorm_silu C={C} P={P} modulation={mod}")
    assert ok


STATES, FE_D, FE_EPS = 3, 256, 1e-6
FE_CASES = [(1, 64, [64]), (1, 96, [96]), (2, 200, [200, 1])]


@pytest.mark.parametrize("padding_right", [False, True], ids=["left", "right"])
@pytest.mark.parametrize("B,T,valid", FE_CASES, ids=[f"{b}-{t}-valid{i}" for i, (b, t, _) in enumerate(FE_CASES)])
def test_fe_stats_and_norm_concat(ltx, gpu_ctx, B, T, valid, padding_right):
    """states = 3, D = 256, bf16 hidden states 0.3 + 2.5 z. The mean has mean_var's bound with n = valid * D (a thread adds 8 values per
    2048 of its chunk, the tree and the chunk loop add the rest: fewer additions than that count). range + eps is exact: the minimum and
    maximum of bf16 values are those values, and the difference and the sum with eps are one f32 operation each, replayed here.
    The normalised concat (statistics from the reference, so that only the apply is under test) follows `bf16_rule`; padded tokens are
    zero BITS and element (d, l) lands at d * states + l."""
    rng = np.random.default_rng(B * 1000 + T)
    hs = ref.bf16(0.3 + 2.5 * rng.standard_normal((STATES, B, T, FE_D)))
    mask = np.zeros((B, T), np.int32)
    for b, n in enumerate(valid):
        if padding_right:
            mask[b, :n] = 1
        else:
            mask[b, T - n:] = 1
    chunks = -(-T * FE_D // 16384)
    n_part = ltx.fe_stats_partials_floats(STATES, B, T, FE_D)
    assert n_part == STATES * B * chunks * 3 and chunks == {64: 1, 96: 2, 200: 4}[T]
    d_h, d_m = dev_bf16(hs), dev(mask, np.int32)
    partials = out_f32(n_part, 64)
    stats = out_f32(2 * STATES * B, 64)
    gpu_ctx.op_fe_stats(d_h, d_m, STATES, B, T, FE_D, partials, stats, padding_right=padding_right, eps=FE_EPS)
    got = host_f32(stats, 2 * STATES * B, (STATES, B, 2))
    part = host_f32(partials, n_part, (STATES * B, chunks, 3))
    mean, mn, mx = ref.fe_stats(hs, mask, padding_right, FE_EPS)
    n_el = np.array(valid)[None, :] * FE_D
    v4 = ref.fe_valid(mask, padding_right)[None, :, :, None]
    mean_abs = np.where(v4, np.abs(hs), 0.0).sum(axis=(2, 3)) / n_el
    ok_mean = report(f"fe_stats B={B} T={T} right={padding_right} mean", np.abs(got[..., 0] - mean), mean_bound(n_el, mean_abs))
    range_eps = (mx.astype(np.float32) - mn.astype(np.float32)) + np.float32(FE_EPS)
    assert ok_mean and np.array_equal(got[..., 1].view(np.uint32), range_eps.view(np.uint32))
    empty = np.isinf(part[:, :, 1])  # chunks that saw no valid token
    assert empty.any() == (valid[-1] == 1) and np.all(part[:, :, 0][empty] == 0) and np.all(part[:, :, 2][empty] == -np.inf)
    # the apply, on the reference's statistics as f32
    ref_stats = np.stack([mean.astype(np.float32), range_eps], axis=-1)
    out = out_bf16(B * T * FE_D * STATES, FE_D * STATES)
    gpu_ctx.op_fe_norm_concat(d_h, d_m, dev(ref_stats), STATES, B, T, FE_D, out, padding_right=padding_right, eps=FE_EPS)
    bits = host_bf16(out, B * T * FE_D * STATES, (B, T, FE_D * STATES))
    want = ref.fe_norm_concat(hs, mask, ref_stats[..., 0], ref_stats[..., 1], padding_right)
    valid_bt = ref.fe_valid(mask, padding_right)
    assert not bits[~valid_bt].any()
    assert bf16_rule(bits[valid_bt], want[valid_bt], f"fe_norm_concat B={B} T={T} right={padding_right}")
    # d * states + l, spelled out for one element
    b, t, d, l = B - 1, np.flatnonzero(valid_bt[B - 1])[0], 17, 2
    one = 8.0 * (hs[l, b, t, d] - float(ref_stats[l, b, 0])) / float(ref_stats[l, b, 1])
    assert abs(ref.from_bf16_bits(bits[b, t, d * STATES + l]) - ref.bf16(one)) <= ref.bf16_ulp(ref.bf16(one))
