"""The fused conv epilogues on the tall conv kernel's W == 384 and W == 192 instances, and the decoder under the launcher's A/B options.

  (a) one res-block of the 128-channel stage at config 4's stage geometry (H = 256, W = 384): the launcher's own rule gives the tall
      W == 384 instance with the fused PixelNorm + residual epilogue, compared with oracle.vae_res_block;
  (b) a small decode, latent (1,128,2,2,48), that puts EVERY fused epilogue on a tall instance, compared with oracle.decode_video;
  (c) that decode and decode(2, 8, 12) under the options `conv_persist`, `conv_stagger`, `conv_block`, `conv_halo`, `conv_tall`,
      `conv_no_tail`, `conv_cfg`: bit-equal where the option table says so, within the rounding bound between kernels elsewhere, and
      `conv_halo` = 0 decodes at all (the decoder asks the launcher's rule before it fuses the 128-channel stage's first PixelNorm).
"""
import numpy as np
import pytest
import torch

from test_config4_and_full_res_parity_gpu import vae_from_oracle_weights  # noqa: F401  (module-scoped fixture)
from test_dit_gpu import rel_l2

pytestmark = pytest.mark.gpu

CUS = 256   # MI355X


def _tall_tiles(F, H, W, N):
    """conv_halo2_takes' size rule (gemm.hip): the tall kernel takes a launch whose 384-row tiles cover more than half the chip,
    2 * (M / 384) * (N / 128) > CUs, with M % 384 == 0 and H a multiple of the image rows per tile (1 / 2 / 4 at W = 384 / 192 / 96)"""
    M = F * H * W
    nrt = {384: 1, 192: 2, 96: 4}[W]
    assert M % 384 == 0 and H % nrt == 0 and N % 128 == 0
    return 2 * (M // 384) * (N // 128)


def test_vae_res_block_128ch_at_config4_geometry_on_the_tall_w384_kernel(ltx, oracle, vae_from_oracle_weights):
    """Group 3 (128 channels) at (F = 3, H = 256, W = 384), default options: 2 * (294 912 / 384) * 1 = 1536 > 256 CUs, so both convs
    run on conv3d_halo2_kernel<1> with PixelNorm + SiLU (conv1) and residual (conv2) epilogues. Bounds: the other stages' own
    (test_vae_res_block_at_headline_resolution_vs_oracle): rel-L2 <= 1e-2 on the output, <= 3e-2 on what the block adds."""
    ctx, w = vae_from_oracle_weights
    assert torch.cuda.get_device_properties(0).multi_processor_count == CUS
    group, block, F, H, W = 3, 2, 3, 256, 384
    assert _tall_tiles(F, H, W, 128) == 1536 > CUS and all(ltx.get_option(k) == 1 for k in ("conv_tall", "conv_halo"))
    p = f"up_blocks_{2 * group}.res_blocks.{block}."
    C = oracle.VAE_CHANNELS[group]
    assert C == 128 and w[p + "conv1.conv.weight"].shape[:2] == (C, C)
    rng = np.random.default_rng(100 * group + block)
    x = rng.standard_normal((1, C, F, H, W), dtype=np.float32)
    x_cl = np.ascontiguousarray(x[0].transpose(1, 2, 3, 0))
    xd = torch.from_numpy(x_cl).cuda()
    ctx.vae_res_block_dev(group, block, xd, F, H, W)
    torch.cuda.synchronize()
    got = xd.cpu().numpy()
    ref = oracle.vae_res_block(w, p, x)[0].transpose(1, 2, 3, 0)
    r_out, r_delta = rel_l2(got, ref), rel_l2(got - x_cl, ref - x_cl)
    print(f"res-block group 3 block {block} at {F}x{H}x{W} (tall W == 384 kernel): rel-L2 out {r_out:.3e}, delta {r_delta:.3e}")
    assert np.isfinite(got).all() and r_out <= 1e-2 and r_delta <= 3e-2, (r_out, r_delta)
    assert float(np.linalg.norm(ref - x_cl) / np.linalg.norm(x_cl)) > 1e-2, "the block adds too little to prove anything"
    # the last image rows and the last frame: a wrong last tile would sit here
    assert rel_l2(got[-1, -2:], ref[-1, -2:]) <= 1e-2


TALL_LATENT = (2, 2, 48)


def test_small_decode_with_every_fused_epilogue_on_a_tall_kernel_vs_oracle(ltx, oracle, vae_from_oracle_weights):
    """Latent (1,128,2,2,48): stage widths 48 / 96 / 192 / 384. Checked against conv_halo2_takes (gemm.hip): the 256 -> 128 upsampler
    conv runs at 5 x 8 x 192 with N = 1024, M = 7680 = 20 x 384, H % 2 == 0, 2 * 20 * 8 = 320 > 256 CUs: a tall W == 192 launch with the
    depth-to-space + PixelNorm epilogue (d2s == 1 and N == 8 x 128 is the form that rule admits with pn_out); the 128-channel stage
    runs at 9 x 16 x 384, M = 55 296 = 144 x 384, 2 * 144 * 1 = 288 > 256: the W == 384 instance with PixelNorm + residual in every conv
    (N == 128). Bounds: test_vae_decode_parity's (<= 2e-2 abs on [0,1] frames, rel-L2 <= 3e-2 about the mean,
    clipped share < 0.5)."""
    ctx, w = vae_from_oracle_weights
    assert torch.cuda.get_device_properties(0).multi_processor_count == CUS
    F, H, W = TALL_LATENT
    assert (2 * (2 * F - 1) - 1, 4 * H, 4 * W) == (5, 8, 192) and _tall_tiles(5, 8, 192, 1024) == 320 > CUS
    assert (2 * 5 - 1, 16, 384) == (9, 8 * H, 8 * W) and _tall_tiles(9, 16, 384, 128) == 288 > CUS
    assert ltx.conv_takes_d2s_pn(5, 8, 192, 256)
    rng = np.random.default_rng(46)
    lat = rng.standard_normal((1, 128, F, H, W)).astype(np.float32)
    got = ctx.vae_decode(lat)
    assert got.shape == (8 * (F - 1) + 1, 32 * H, 32 * W, 3) and np.isfinite(got).all()
    ref = np.clip((oracle.decode_video(w, lat, return_raw=True) + 1) / 2, 0, 1)
    err = float(np.abs(got - ref).max())
    rel = float(np.linalg.norm(got - ref) / np.linalg.norm(ref - ref.mean()))
    sat = float(np.mean((ref <= 0) | (ref >= 1)))
    print(f"decode of latent {TALL_LATENT}: max abs {err:.3e}, rel-L2 {rel:.3e}, clipped share {sat:.3f}")
    assert sat < 0.5, "the synthetic decoder saturates: the comparison proves too little"
    assert err <= 2e-2 and rel <= 3e-2, (err, rel)


def _decoder(ctx, F, H, W, seed):
    lat = torch.from_numpy(np.random.default_rng(seed).standard_normal((1, 128, F, H, W), dtype=np.float32)).cuda()

    def run(**opts):
        frames = torch.full((8 * (F - 1) + 1, H * 32, W * 32, 3), float("nan"), dtype=torch.float32, device="cuda")
        with ctx.options(**opts):
            ctx.vae_decode_dev(lat, F, H, W, frames)
            torch.cuda.synchronize()
        return frames

    return run


@pytest.fixture(scope="module", params=[TALL_LATENT, (2, 8, 12)], ids=["latent 2x2x48", "latent 2x8x12"])
def decoder(request, vae_from_oracle_weights):
    ctx, _ = vae_from_oracle_weights
    run = _decoder(ctx, *request.param, seed=8)
    base = run()
    assert bool(torch.isfinite(base).all())
    return run, base


def _defaults_restored(ltx):
    return all(ltx.get_option(name) == default for name, default, *_ in ltx.option_table())


@pytest.mark.parametrize("opts", [{"conv_persist": 0}, {"conv_stagger": 0}, {"conv_block": 0}], ids=str)
def test_decode_options_documented_as_bit_neutral_are(ltx, decoder, opts):
    """The option table marks these three `numerics: no`: one workgroup per tile, unstaggered LDS-DMA issue and the plain tile order
    compute every tile exactly once, by the same instructions."""
    run, base = decoder
    assert not any(dict((t[0], t[4]) for t in ltx.option_table())[k] for k in opts)
    assert torch.equal(run(**opts), base), opts
    assert _defaults_restored(ltx)


def test_decode_runs_without_the_halo_staged_kernels(ltx, decoder):
    """`conv_halo` = 0: every conv on the ring kernel, which has no depth-to-space + PixelNorm epilogue, so the decoder must keep the
    128-channel stage's first PixelNorm as a row pass - the same launches as `conv_halo` = 0 with `conv_d2s_pn` = 0, bit for bit.
    (The decoder used to decide with a copy of the width rule only and the launcher refused the launch: invalidConfiguration.)"""
    run, base = decoder
    off = run(conv_halo=0)
    assert bool(torch.isfinite(off).all())
    with ltx.options(conv_halo=0):
        assert not ltx.conv_takes_d2s_pn(5, 8, 192, 256)
    assert torch.equal(off, run(conv_halo=0, conv_d2s_pn=0))
    r = float((off - base).norm() / base.norm())
    assert r <= 2e-3, r   # another kernel's summation order, and the PixelNorm as a pass: rounding only
    assert _defaults_restored(ltx)


def test_decode_without_tall_tiles_and_with_forced_tile_choices(ltx, decoder):
    """`conv_tall` = 0 (192-row tiles only) must not depend on `conv_persist`; `conv_no_tail` = 1 (no split-K launch for a last partial
    round) and `conv_cfg` = 21 (the 192 x 128 configuration for every conv, conv_out included) must run and stay within the rounding
    bound this suite uses between conv kernels (rel <= 2e-3 of the default decode)."""
    run, base = decoder
    assert torch.equal(run(conv_tall=0), run(conv_tall=0, conv_persist=0))
    for opts in ({"conv_no_tail": 1}, {"conv_cfg": 21}):
        out = run(**opts)
        r = float((out - base).norm() / base.norm())
        print(f"decode with {opts}: rel {r:.3e} of the default decode")
        assert bool(torch.isfinite(out).all()) and r <= 2e-3, (opts, r)
    assert _defaults_restored(ltx)
