"""CPU tests (no GPU): the pure-host part of the path exported by libltxhip.so - shapes, validation, sigma schedules,
RoPE tables, VAE tiling plan, weight-key mapping - pinned by known-answer vectors derived by hand from the
reference source, and checked bit-for-bit against the oracle. Also checks the ABI surface itself.
"""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_version(ltx):
    # the reference's only test: LTXVideo.version == "0.1.0" (Tests/LTXVideoTests/LTXVideoTests.swift:9-11)
    assert ltx.__version__ == "0.1.0"


def test_abi_exports_match_header(ltx):
    """Every function declared in include/ltxhip.h is exported by the library and bound in _lib.SIGNATURES."""
    hdr = open(os.path.join(ROOT, "include", "ltxhip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(ltx_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"ltx_status"}
    assert len(declared) >= 30
    from importlib import import_module

    lib_mod = import_module("ltx-video-swift-mlx_amd._lib")
    so = ctypes.CDLL(lib_mod.SO_PATH)
    for name in sorted(declared):
        assert hasattr(so, name), f"{name} declared in ltxhip.h but not exported"
        assert name in lib_mod.SIGNATURES, f"{name} not bound in _lib.SIGNATURES"
    assert set(lib_mod.SIGNATURES) == declared


def test_abi_revision_and_option_table(ltx):
    """Round 5 (ABI revision 2): the launcher switches are ONE table behind ltx_ctx_set_option - no GPU needed to read or move them - the
    library's soname carries the revision, ltx_denoise_options starts with its size, and the product library contains no getenv of an
    LTX_* name (only the -DLTX_EXPERIMENTS build seeds the table from the environment)."""
    import subprocess

    from importlib import import_module

    lib_mod = import_module("ltx-video-swift-mlx_amd._lib")
    assert ltx.lib.ltx_abi_version() == 2
    hdr = open(os.path.join(ROOT, "include", "ltxhip.h")).read()
    assert re.search(r"#define LTX_ABI_VERSION 2\b", hdr)
    assert lib_mod.DenoiseOptions._fields_[0][0] == "struct_size" and lib_mod.DenoiseOptions.struct_size.offset == 0
    table = ltx.option_table()
    names = [t[0] for t in table]
    assert len(names) == len(set(names)) >= 20 and {"qk_f32", "split_f32", "finish_rows", "conv_persist", "sp_overlap"} <= set(names)
    for name, default, lo, hi, numerics, doc in table:
        assert lo <= default <= hi and doc and ltx.get_option(name) == default, name   # nothing in the environment moved a default
    assert dict((t[0], t[4]) for t in table)["qk_f32"] is True and dict((t[0], t[4]) for t in table)["finish_norm"] is False
    with ltx.options(qk_f32=1, finish_rows=4):
        assert ltx.get_option("qk_f32") == 1 and ltx.get_option("finish_rows") == 4
    assert ltx.get_option("qk_f32") == 0 and ltx.get_option("finish_rows") == 1
    for bad in (("nope", 1), ("finish_rows", 0), ("qk_f32", 2)):
        with pytest.raises(ltx.LTXError):
            ltx.set_option(*bad)
    # soname = ABI revision; no LTX_* string that looks like an environment hook is left in the product library's read-only data
    dyn = subprocess.run(["readelf", "-d", lib_mod.SO_PATH], capture_output=True, text=True).stdout
    if "experiments=0" in ltx.lib.ltx_build_info().decode():
        assert "libltxhip.so.2" in dyn, dyn
        blob = open(lib_mod.SO_PATH, "rb").read()
        for old in (b"LTX_QK_F32", b"LTX_SPLIT_F32", b"LTX_FINISH_ROWS", b"LTX_CONV_PERSIST", b"LTX_ATTN_IMPL", b"LTX_GEMM_FORCE", b"LTX_SP_OVERLAP"):
            assert old not in blob, old


def test_conv_takes_d2s_pn_is_the_conv_launchers_rule(ltx):
    """gemm_conv_takes_d2s_pn through ltx_conv_takes_d2s_pn (host-side, no device): the VAE decoder fuses the 128-channel stage's first
    PixelNorm into the 256 -> 1024 upsampler conv exactly where a halo-staged kernel takes that launch. Known answers from
    conv_halo_takes (gemm.hip): W in {48, 64, 96, 192} or a multiple of 192, H >= 2, at least 192 rows, M * C < 2^31 (32-bit element
    offsets), and option `conv_halo` on."""
    assert ltx.conv_takes_d2s_pn(13, 64, 96, 256)          # the headline decode (768 x 512 x 25)
    assert ltx.conv_takes_d2s_pn(5, 8, 192, 256) and ltx.conv_takes_d2s_pn(13, 128, 192, 256) and ltx.conv_takes_d2s_pn(3, 8, 48, 256)
    assert not ltx.conv_takes_d2s_pn(13, 64, 80, 256)      # 192 % 80 != 0
    assert not ltx.conv_takes_d2s_pn(13, 1, 192, 256)      # one image row
    assert not ltx.conv_takes_d2s_pn(1, 2, 48, 256)        # 96 rows: less than one tile
    assert not ltx.conv_takes_d2s_pn(13, 64, 96, 128)      # N = 512: not eight sub-positions of 128 channels
    # 32-bit element offsets: F x 8 x 192 rows x 256 channels reaches 2^31 between F = 5461 and 5462
    assert 5461 * 8 * 192 * 256 < 2 ** 31 <= 5462 * 8 * 192 * 256
    assert ltx.conv_takes_d2s_pn(5461, 8, 192, 256) and not ltx.conv_takes_d2s_pn(5462, 8, 192, 256)
    with ltx.options(conv_halo=0):
        assert not ltx.conv_takes_d2s_pn(13, 64, 96, 256) and not ltx.conv_takes_d2s_pn(5, 8, 192, 256)
    assert ltx.get_option("conv_halo") == 1 and ltx.conv_takes_d2s_pn(13, 64, 96, 256)


# ---- R1 ----
@pytest.mark.parametrize("whf,expect", [((256, 256, 9), (2, 8, 8)), ((768, 512, 25), (4, 16, 24)),
                                        ((1536, 1024, 25), (4, 32, 48)), ((768, 512, 201), (26, 16, 24)),
                                        ((704, 480, 121), (16, 15, 22))])
def test_latent_shape_kat(ltx, oracle, whf, expect):
    assert ltx.latent_shape(*whf) == expect == oracle.latent_shape(*whf)


def test_token_counts():
    # SURVEY section 0 table
    for (f, h, w), t in {(2, 8, 8): 128, (4, 16, 24): 1536, (4, 32, 48): 6144, (26, 16, 24): 9984}.items():
        assert f * h * w == t


def test_validate_matches_oracle_and_messages(ltx, oracle):
    cases = [(768, 512, 25, 8, 1.0, False), (770, 512, 25, 8, 1.0, False), (768, 500, 25, 8, 1.0, False),
             (768, 512, 24, 8, 1.0, False), (32, 512, 25, 8, 1.0, False), (4096, 512, 25, 8, 1.0, False),
             (768, 32, 25, 8, 1.0, False), (768, 512, 1, 8, 1.0, False), (768, 512, 265, 8, 1.0, False),
             (768, 512, 25, 0, 1.0, False), (768, 512, 25, 101, 1.0, False), (768, 512, 25, 8, 0.5, False),
             (768, 512, 25, 8, 21.0, False), (800, 512, 25, 8, 1.0, True), (768, 512, 25, 8, 1.0, True),
             (770, 500, 24, 0, 0.0, False)]
    for c in cases:
        want = oracle.validate_generation_config(*c)
        try:
            ltx.validate_generation_config(*c)
            got = None
        except ltx.LTXError as e:
            assert e.case == "invalidConfiguration"
            got = str(e).split(": ", 1)[1]
        assert got == want, (c, got, want)
    # first failing check wins, in the reference's order (LTXConfig.swift:310-353)
    with pytest.raises(ltx.LTXError, match="Width must be divisible by 32, got 770"):
        ltx.validate_generation_config(770, 500, 24, 0, 0.0)
    with pytest.raises(ltx.LTXError, match=r"Number of frames must be 8n \+ 1"):
        ltx.validate_generation_config(768, 512, 24, 8, 1.0)


# ---- R3 ----
def test_sigma_tables(ltx, oracle):
    # constants copied by value from LTXScheduler.swift:18-36
    raw = ltx.sigmas(True, 8, 0)
    assert raw.tolist() == [np.float32(v) for v in [1.0, 0.99375, 0.9875, 0.98125, 0.975, 0.909375, 0.725, 0.421875, 0.0]]
    assert ltx.stage2_sigmas().tolist() == [np.float32(v) for v in [0.909375, 0.725, 0.421875, 0.0]]
    assert oracle.DISTILLED_SIGMA_VALUES[5:] == oracle.STAGE_2_DISTILLED_SIGMA_VALUES


def test_sigma_kat_t1536(ltx):
    # SURVEY R3 known-answer vector (derived from the formulas, f32, printed to 8 significant digits): T=1536
    kat = np.array([1.0, 0.99405915, 0.98806733, 0.98202413, 0.97592908, 0.90860569, 0.68004858, 0.10000002, 0.0], np.float32)
    got = ltx.sigmas(True, 8, 1536)
    assert np.all(np.abs(got.astype(np.float64) - kat.astype(np.float64)) <= 1e-8), got
    # exact bit patterns with a correctly rounded expf (glibc; see oracle._expf for the 1-ulp numpy caveat)
    bits = [0x3f800000, 0x3f7e7aa9, 0x3f7cf1fb, 0x3f7b65ef, 0x3f79d67d, 0x3f689a62, 0x3f2e17aa, 0x3dccccd0, 0x0]
    assert got.view(np.uint32).tolist() == bits
    # num_steps is ignored in distilled mode (always the 8-step table: LTXScheduler.swift:86-88)
    assert np.array_equal(ltx.sigmas(True, 3, 1536), got)
    # T >= 4096 and T = 128 vectors of SURVEY R3 to the digits it prints (its 7th entries are 1-2 ulp off because
    # it was evaluated with numpy's float32 exp)
    k4096 = [1.0, 0.99514461, 0.99023592, 0.98527282, 0.98025471, 0.92397928, 0.72058177, 0.09999996, 0.0]
    k128 = [1.0, 0.99287611, 0.98571050, 0.97850257, 0.97125220, 0.89245450, 0.64141822, 0.10000002, 0.0]
    assert np.all(np.abs(ltx.sigmas(True, 8, 4096).astype(np.float64) - np.array(k4096)) <= 5e-7)
    assert np.all(np.abs(ltx.sigmas(True, 8, 128).astype(np.float64) - np.array(k128)) <= 5e-7)


def test_sigma_clamp_and_terminal(ltx):
    a, b = ltx.sigmas(True, 8, 4096), ltx.sigmas(True, 8, 9984)
    assert np.array_equal(a, b)  # min(tokens, 4096)
    for t in (128, 1536, 6144):
        s = ltx.sigmas(True, 8, t)
        assert s[0] == 1.0 and s[-1] == 0.0 and abs(s[-2] - 0.1) < 1e-6 and np.all(np.diff(s) < 0)
    d = ltx.sigmas(False, 40, 1536)
    assert len(d) == 41 and d[0] == 1.0 and d[-1] == 0.0 and abs(d[-2] - 0.1) < 1e-6 and np.all(np.diff(d) < 0)


def test_sigma_matches_oracle_bitwise(ltx, oracle):
    for t in (0, 128, 1000, 1536, 4096, 6144, 9984):
        for dist, n in ((True, 8), (False, 40), (False, 8), (False, 3), (False, 1)):
            a, b = ltx.sigmas(dist, n, t), oracle.sigmas(dist, n, t)
            assert np.array_equal(a, b, equal_nan=True), (t, dist, n, a, b)


# ---- R8 / R9 ----
def test_position_grid_kat(oracle):
    # temporal mid-coordinates of latent frames 0..3 at 24 fps, spatial 32j+16
    g = oracle.position_grid(4, 2, 3)
    t = g[0].reshape(4, 2, 3)[:, 0, 0]
    assert np.allclose(t, [1 / 48, 5 / 24, 13 / 24, 21 / 24], rtol=0, atol=1e-7)
    assert g[1].reshape(4, 2, 3)[0, :, 0].tolist() == [16.0, 48.0]
    assert g[2].reshape(4, 2, 3)[0, 0, :].tolist() == [16.0, 48.0, 80.0]
    # token order: w fastest, then h, then f (LatentUtils.swift:20-34)
    assert g[2][:3].tolist() == [16.0, 48.0, 80.0] and g[1][3] == 48.0


def test_rope_tables_structure(ltx, oracle):
    cfg = ltx.default_transformer_config()
    F, H, W = 2, 3, 4
    cos, sin = ltx.rope_tables(cfg, F, H, W)
    assert cos.shape == (F * H * W, 2048)
    # 4096/6 = 682 frequency indices x 3 dims = 2046 -> two identity slots padded at the FRONT (head 0)
    assert np.all(cos[:, :2] == 1.0) and np.all(sin[:, :2] == 0.0)
    assert np.allclose(cos ** 2 + sin ** 2, 1.0, atol=1e-6)
    # first frequency index = theta^0 * pi/2 : angle = pi/2 * (2*coord/max - 1)
    t0 = (1 / 48) / 20 * 2 - 1
    assert abs(cos[0, 2] - np.float32(np.cos(np.pi / 2 * t0))) <= 1e-7
    oc, osn = oracle.rope_tables(F, H, W)
    assert np.array_equal(cos, oc) and np.array_equal(sin, osn)


def test_rope_tables_small_dims_match_oracle(ltx, oracle):
    for heads in (2, 4):
        cfg = ltx.default_transformer_config(num_attention_heads=heads, cross_attention_dim=heads * 128)
        cos, sin = ltx.rope_tables(cfg, 2, 5, 7)
        oc, osn = oracle.rope_tables(2, 5, 7, dim=heads * 128, num_heads=heads)
        assert np.array_equal(cos, oc) and np.array_equal(sin, osn)


# ---- R19 ----
def test_tile_plan_kats(ltx, oracle):
    # config 5 (F'=26): tile 8 ov 1 -> 180 frames (not 201); tile 6 ov 1 -> 173; F'=16 tile 8 -> 107
    assert ltx.vae_tile_plan(26, 8, 1) == ([(0, 8), (7, 15), (14, 22), (21, 26)], 180)
    assert ltx.vae_tile_plan(26, 6, 1) == ([(0, 6), (5, 11), (10, 16), (15, 21), (20, 26)], 173)
    assert ltx.vae_tile_plan(16, 8, 1) == ([(0, 8), (7, 15), (14, 16)], 107)
    assert ltx.vae_tile_plan(4, 8, 1) == ([(0, 4)], 25)     # untiled when F' <= tile
    assert ltx.vae_tile_plan(26, 0, 1) == ([(0, 26)], 201)  # tiling disabled (default preset)
    for n in range(1, 40):
        for tile in (0, 2, 3, 6, 8):
            for ov in (0, 1, 2):
                if tile and tile <= ov:
                    continue
                assert ltx.vae_tile_plan(n, tile, ov) == tuple(oracle.vae_tile_plan(n, tile, ov)) or \
                    list(ltx.vae_tile_plan(n, tile, ov)) == list(oracle.vae_tile_plan(n, tile, ov))
    with pytest.raises(ltx.LTXError):
        ltx.vae_tile_plan(26, 2, 2)  # stride 0: the reference would never terminate


# ---- R20 ----
KEY_KATS = {
    "model.diffusion_model.proj_in.weight": "patchify_proj.weight",
    "model.diffusion_model.adaln_single.emb.timestep_embedder.linear_1.bias": "adaln_single.emb.linear_1.bias",
    "model.diffusion_model.time_embed.emb.timestep_embedder.linear_2.weight": "adaln_single.emb.linear_2.weight",
    "model.diffusion_model.time_embed.linear.weight": "adaln_single.linear.weight",
    "model.diffusion_model.adaln_single.linear.bias": "adaln_single.linear.bias",
    "model.diffusion_model.caption_projection.linear_1.weight": "caption_projection.linear_1.weight",
    "model.diffusion_model.scale_shift_table": "scale_shift_table",
    "model.diffusion_model.proj_out.bias": "proj_out.bias",
    "model.diffusion_model.transformer_blocks.7.attn1.norm_q.weight": "transformer_blocks.7.attn1.q_norm.weight",
    "model.diffusion_model.transformer_blocks.7.attn2.norm_k.weight": "transformer_blocks.7.attn2.k_norm.weight",
    "model.diffusion_model.transformer_blocks.47.attn2.to_out.0.bias": "transformer_blocks.47.attn2.to_out.bias",
    "model.diffusion_model.transformer_blocks.0.ff.net.0.proj.weight": "transformer_blocks.0.ff.project_in.proj.weight",
    "model.diffusion_model.transformer_blocks.0.ff.net.2.bias": "transformer_blocks.0.ff.project_out.bias",
    "model.diffusion_model.transformer_blocks.0.scale_shift_table": "transformer_blocks.0.scale_shift_table",
    # the dual model's loaders rename through the same function (transformer_module_spelling): one dual-block checkpoint key per rule ...
    "model.diffusion_model.transformer_blocks.1.attn2.norm_q.weight": "transformer_blocks.1.attn2.q_norm.weight",
    "model.diffusion_model.transformer_blocks.1.attn1.norm_k.weight": "transformer_blocks.1.attn1.k_norm.weight",
    "model.diffusion_model.transformer_blocks.1.attn1.to_out.0.weight": "transformer_blocks.1.attn1.to_out.weight",
    "model.diffusion_model.transformer_blocks.1.ff.net.0.proj.bias": "transformer_blocks.1.ff.project_in.proj.bias",
    "model.diffusion_model.transformer_blocks.1.ff.net.2.weight": "transformer_blocks.1.ff.project_out.weight",
    # ... and one top-level dual key per rule
    "model.diffusion_model.proj_in.bias": "patchify_proj.bias",
    "model.diffusion_model.time_embed.emb.timestep_embedder.linear_1.weight": "adaln_single.emb.linear_1.weight",
    "model.diffusion_model.time_embed.linear.bias": "adaln_single.linear.bias",
    "model.diffusion_model.adaln_single.emb.timestep_embedder.linear_2.bias": "adaln_single.emb.linear_2.bias",
    # skipped
    "model.diffusion_model.transformer_blocks.0.attn1.to_q.weight_scale": None,
    "model.diffusion_model.transformer_blocks.0.audio_attn1.to_q.weight": None,
    "model.diffusion_model.audio_proj_in.weight": None,
    "model.diffusion_model.av_ca_video_scale_shift_adaln_single.linear.weight": None,
    "model.diffusion_model.video_embeddings_connector.learnable_registers": None,
    "model.diffusion_model.transformer_blocks.0.scale_shift_table_a2v_ca_video": None,
    "vocoder.conv_pre.weight": None,
    "vae.decoder.conv_in.conv.weight": None,
    "transformer_blocks.0.attn1.to_q.weight": None,  # no model.diffusion_model. prefix -> not a transformer key
}
VAE_KATS = {
    "decoder.conv_in.conv.weight": "conv_in.conv.weight",
    "vae.decoder.conv_out.conv.bias": "conv_out.conv.bias",
    "decoder.mid_block.resnets.3.conv2.conv.weight": "up_blocks_0.res_blocks.3.conv2.conv.weight",
    "decoder.mid_block.time_embedder.timestep_embedder.linear_1.weight": "up_blocks_0.time_embedder.timestep_embedder.linear_1.weight",
    "decoder.up_blocks.0.upsamplers.0.conv.conv.weight": "up_blocks_1.conv.conv.weight",
    "decoder.up_blocks.0.resnets.4.scale_shift_table": "up_blocks_2.res_blocks.4.scale_shift_table",
    "decoder.up_blocks.2.upsamplers.0.conv.conv.bias": "up_blocks_5.conv.conv.bias",
    "decoder.up_blocks.2.resnets.0.conv1.conv.weight": "up_blocks_6.res_blocks.0.conv1.conv.weight",
    "decoder.up_blocks.3.conv.conv.weight": "up_blocks_3.conv.conv.weight",  # legacy unified layout
    "decoder.last_scale_shift_table": "last_scale_shift_table",
    "decoder.timestep_scale_multiplier": "timestep_scale_multiplier",
    "latents_mean": "mean_of_means",
    "latents_std": "std_of_means",
    "vae.per_channel_statistics.mean-of-means": "mean_of_means",
    "per_channel_statistics.std-of-means": "std_of_means",
    "per_channel_statistics.channel": None,
    "encoder.conv_in.conv.weight": None,
}
LORA_KATS = {
    "diffusion_model.transformer_blocks.0.attn1.to_out.0": "transformer_blocks.0.attn1.to_out.weight",
    "diffusion_model.transformer_blocks.5.ff.net.0.proj": "transformer_blocks.5.ff.project_in.proj.weight",
    "diffusion_model.transformer_blocks.5.ff.net.2": "transformer_blocks.5.ff.project_out.weight",
    "transformer_blocks.1.attn2.to_k": "transformer_blocks.1.attn2.to_k.weight",
    "diffusion_model.adaln_single.emb.timestep_embedder.linear_1": "adaln_single.emb.linear_1.weight",
}


def test_key_mapping_kats(ltx, oracle):
    for k, v in KEY_KATS.items():
        assert ltx.map_transformer_key(k) == v == oracle.map_transformer_key(k), k
    for k, v in VAE_KATS.items():
        assert ltx.map_vae_key(k) == v == oracle.map_vae_key(k), k
    for k, v in LORA_KATS.items():
        assert ltx.map_lora_key(k) == v == oracle.map_lora_key(k), k


def test_dual_checkpoint_keys_map_back_through_the_shared_rename(ltx):
    """Every video-side key of the dual model in its checkpoint spelling comes back as its module key, and no rename rule fires on a
    key it was not written for: the block rules leave the top-level keys alone and the top-level rules leave the block keys alone.
    (ltx_map_transformer_key drops the audio side, which goes through the same renames under an "audio_" name.)"""
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
    import dual_block_ref
    import dual_model_ref

    keys = list(dual_model_ref.param_shapes(2, 1, 1))
    assert not [k for k in dual_block_ref.param_shapes(2, 1, 1) if k.startswith("proj_in.") or ".emb.timestep_embedder." in k]
    top = dual_model_ref.top_shapes(1, 1)
    for k in top:
        ck = dual_model_ref.checkpoint_spelling(k)
        assert not any(r in ck for r in (".norm_q.", ".norm_k.", ".to_out.0.", "ff.net.")), ck
    video = [k for k in keys if ltx.map_transformer_key("model.diffusion_model." + k) is not None]
    assert len(video) > len(keys) // 4 and any(k in top for k in video) and any(k.startswith("transformer_blocks.1.") for k in video)
    for k in video:
        assert ltx.map_transformer_key("model.diffusion_model." + dual_model_ref.checkpoint_spelling(k)) == k, k
    for k in keys:  # the Python restatement the GPU round-trip tests write their files with agrees on every key, audio included
        assert dual_model_ref.module_spelling(dual_model_ref.checkpoint_spelling(k)) == k, k


def test_key_mapping_roundtrip_covers_all_params(ltx, oracle):
    """Every module parameter (SURVEY R20 list) is reachable from a checkpoint-style file key."""
    ocfg = oracle.DiTConfig(num_layers=3, num_heads=2, caption_channels=128)
    shapes = oracle.dit_param_shapes(ocfg)
    file_keys = oracle.dit_file_keys({k: None for k in shapes})
    mapped = {ltx.map_transformer_key(k) for k in file_keys}
    assert mapped == set(shapes)
    vshapes = oracle.vae_param_shapes()
    vfile = oracle.vae_file_keys({k: None for k in vshapes})
    assert {ltx.map_vae_key(k) for k in vfile} == set(vshapes)


def test_ctx_create_without_gpu_fails_loudly(ltx):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(ltx.LTXError) as e:
        ltx.Context(0, use_torch_stream=False)
    assert e.value.case == "hipError"


# ---------------------------------------------------------------------------------------------------------------
# text-embedding connector host logic
# ---------------------------------------------------------------------------------------------------------------
def test_text_encoder_key_mapping(ltx, oracle):
    kat = {
        # unified checkpoint (ModelDownloader.swift:1353-1399 then :935-940)
        "model.diffusion_model.text_embedding_projection.aggregate_embed.weight": "feature_extractor.aggregate_embed.weight",
        "model.diffusion_model.video_embeddings_connector.learnable_registers": "embeddings_connector.learnable_registers",
        "model.diffusion_model.video_embeddings_connector.transformer_blocks.1.attn1.to_out.0.bias":
            "embeddings_connector.transformer_1d_blocks.1.attn1.to_out.bias",
        "model.diffusion_model.video_embeddings_connector.transformer_blocks.0.attn1.norm_q.weight":
            "embeddings_connector.transformer_1d_blocks.0.attn1.q_norm.weight",
        "model.diffusion_model.video_embeddings_connector.transformer_blocks.0.ff.net.0.proj.weight":
            "embeddings_connector.transformer_1d_blocks.0.ff.project_in.proj.weight",
        "model.diffusion_model.video_embeddings_connector.transformer_blocks.0.ff.net.2.bias":
            "embeddings_connector.transformer_1d_blocks.0.ff.project_out.bias",
        "model.diffusion_model.audio_embeddings_connector.transformer_blocks.0.attn1.norm_k.weight":
            "audio_embeddings_connector.transformer_1d_blocks.0.attn1.k_norm.weight",
        # standalone connector file (:920-933)
        "text_proj_in.weight": "feature_extractor.aggregate_embed.weight",
        "video_connector.transformer_blocks.0.attn1.to_k.weight": "embeddings_connector.transformer_1d_blocks.0.attn1.to_k.weight",
        "audio_connector.learnable_registers": "audio_embeddings_connector.learnable_registers",
        # not text-encoder tensors
        "model.diffusion_model.transformer_blocks.0.attn1.to_q.weight": None,
        "vae.decoder.conv_in.conv.weight": None,
    }
    for k, v in kat.items():
        assert ltx.map_text_encoder_key(k) == v, k
        assert oracle.map_text_encoder_key(k) == v, k
    w = oracle.connector_param_shapes(dim=256, layers=2, registers=8, states=5)
    for unified in (True, False):
        for fk in oracle.connector_file_keys({k: None for k in w}, unified=unified):
            assert ltx.map_text_encoder_key(fk) in w


def test_rope_tables_1d(ltx, oracle):
    """Positions 0..T-1 scaled to [-1,1) over max_pos 4096, dim/2 log-spaced frequencies pi/2 .. theta*pi/2, f64 math."""
    for T, dim in ((8, 256), (128, 3840)):
        c, s = ltx.rope_tables_1d(T, dim)
        oc, os_ = oracle.rope_tables_1d(T, dim, num_heads=dim // 128)
        assert np.array_equal(c.view(np.uint32), oc.view(np.uint32))
        assert np.array_equal(s.view(np.uint32), os_.view(np.uint32))
    c, s = ltx.rope_tables_1d(4, 256)
    # token 0: scaled position -1 -> angle -idx; first frequency index = pi/2: cos(-pi/2) ~ 6.1e-17, sin = -1
    assert abs(c[0, 0]) < 1e-7 and s[0, 0] == np.float32(-1.0)
    # last frequency = theta*pi/2 at position 2/4096*2-1
    import math
    ang = 10000.0 * math.pi / 2 * (2.0 / 4096 * 2 - 1)
    assert c[2, -1] == np.float32(math.cos(ang)) and s[2, -1] == np.float32(math.sin(ang))


def test_connector_oracle_internals(oracle):
    """Hand-checkable pieces of the restatement: per-layer statistics ignore padded tokens; register plan."""
    rng = np.random.default_rng(0)
    B, T, D, L = 1, 4, 8, 2
    x = oracle.bf16_round(rng.standard_normal((B, T, D, L)).astype(np.float32))
    x[0, 0] = 1000.0  # padded token must not influence mean / range
    nc = oracle.norm_and_concat(x, np.array([3]), "left")
    assert np.all(nc[0, 0] == 0)
    v = x[0, 1:, :, 1].astype(np.float64)
    exp = 8.0 * (x[0, 2, 5, 1] - v.sum() / (3 * D + 1e-6)) / (v.max() - v.min() + 1e-6)
    assert abs(nc[0, 2, 5 * L + 1] - exp) <= abs(exp) * 2.0 ** -7
    hid = np.arange(8, dtype=np.float32).reshape(1, 8, 1) + 1
    reg = -np.arange(4, dtype=np.float32).reshape(4, 1) - 1
    out = oracle.replace_padded_with_registers(hid, np.array([[0, 0, 0, 1, 1, 1, 1, 1]], bool), reg)
    assert out[0, :, 0].tolist() == [4, 5, 6, 7, 8, -2, -3, -4]  # 5 valid tokens first, then registers 5%4, 6%4, 7%4


def test_vae_encoder_key_mapping_and_shapes(ltx, oracle):
    kat = {
        "encoder.conv_in.conv.weight": "conv_in.conv.weight",
        "encoder.down_blocks.0.resnets.3.conv2.conv.bias": "down_blocks_0.resnets.resnets.3.conv2.conv.bias",
        "encoder.down_blocks.2.downsamplers.0.conv.conv.weight": "down_blocks_2.downsamplers.conv.conv.weight",
        "encoder.mid_block.resnets.1.conv1.conv.weight": "mid_block.resnets.1.conv1.conv.weight",
        "encoder.down_blocks_1.resnets.resnets.0.conv1.conv.weight": "down_blocks_1.resnets.resnets.0.conv1.conv.weight",
        "decoder.conv_in.conv.weight": None,
        "latents_mean": None,
    }
    for k, v in kat.items():
        assert ltx.map_vae_encoder_key(k) == v, k
        assert oracle.map_vae_encoder_key(k) == v, k
    sh = oracle.vae_encoder_param_shapes(128)
    assert sh["conv_out.conv.weight"] == (129, 2048, 3, 3, 3) and sh["down_blocks_3.downsamplers.conv.conv.weight"] == (256, 1024, 3, 3, 3)
    assert sh["down_blocks_1.downsamplers.conv.conv.weight"] == (256, 256, 3, 3, 3)
    for fk in oracle.vae_encoder_file_keys({k: None for k in sh}):
        assert ltx.map_vae_encoder_key(fk) in sh
    # latent frame count: three causal temporal halvings with front padding
    assert [ltx.vae_encoder_latent_frames(t) for t in (1, 2, 8, 9, 17, 25, 121)] == [1, 1, 1, 2, 3, 4, 16]
    # oracle index helpers
    x = np.arange(2 * 3 * 4 * 4, dtype=np.float32).reshape(1, 2, 3, 4, 4)
    s = oracle.space_to_depth(x, (2, 2, 2))
    assert s.shape == (1, 16, 2, 2, 2)
    assert s[0, 0, 0, 0, 0] == x[0, 0, 0, 0, 0] and s[0, 4, 0, 0, 0] == x[0, 0, 0, 0, 0]  # padded front frame = frame 0 (it=0 and it=1)
    assert s[0, 1, 1, 0, 0] == x[0, 0, 1, 0, 1] and s[0, 8 + 7, 1, 1, 1] == x[0, 1, 2, 3, 3]
    p = oracle.encoder_patchify(np.arange(3 * 8 * 8, dtype=np.float32).reshape(1, 3, 1, 8, 8))
    assert p.shape == (1, 48, 1, 2, 2) and p[0, 16 + 1 * 4 + 2, 0, 1, 0] == 64 + (4 + 2) * 8 + (0 + 1)  # c=1, pw=1, ph=2


def test_frame_export_u8_and_png(ltx, tmp_path):
    """VideoExporter.tensorToImages (VideoExporter.swift:563-580): uint8(clip(x,0,1)*255) truncates; the PNG writer emits a
    valid file (checked with an independent decoder: zlib + manual chunk walk)."""
    import struct
    import zlib

    x = np.array([-0.5, 0.0, 0.5, 0.999, 1.0, 1.7, 127.5 / 255, 254.999 / 255, np.nan], np.float32)
    exp = [0, 0, 127, 254, 255, 255, int(np.float32(127.5 / 255) * np.float32(255)), int(np.float32(254.999 / 255) * np.float32(255)), 0]
    assert ltx.frames_to_u8(x).tolist() == exp
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    p = tmp_path / "f.png"
    ltx.write_png(p, img)
    raw = p.read_bytes()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, hdr = 8, b"", None
    while pos < len(raw):
        n, typ = struct.unpack(">I4s", raw[pos:pos + 8])
        body = raw[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(typ + body)
        if typ == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        if typ == b"IDAT":
            idat += body
        pos += 12 + n
    assert hdr == (53, 37, 8, 2, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(37, 53 * 3 + 1)
    assert (rows[:, 0] == 0).all() and np.array_equal(rows[:, 1:].reshape(37, 53, 3), img)


# ---- MLX-compatible noise ----
def test_threefry2x32_known_answers(ltx, oracle):
    """Random123's threefry2x32-20 known-answer vectors (the same three the JAX and MLX test suites use) pin the hash."""
    kat = [((0, 0), (0, 0), (0x6B200159, 0x99BA4EFE)),
           ((0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF), (0x1CB996FC, 0xBB002BE7)),
           ((0x13198A2E, 0x03707344), (0x243F6A88, 0x85A308D3), (0xC4923A9C, 0x483DF7A0))]
    for key, ctr, want in kat:
        assert tuple(int(v) for v in ltx.threefry2x32(key, ctr)) == want
        a, b = oracle.threefry2x32(key, np.array([ctr[0]], np.uint32), np.array([ctr[1]], np.uint32))
        assert (int(a[0]), int(b[0])) == want


def test_mlx_random_normal_matches_the_restatement(ltx, oracle):
    """Library vs oracle on the draw pipeline (bits layout for even / odd counts, key split per draw, uniform -> erfinv):
    two restatements of the same published algorithm, NOT a check against MLX itself."""
    for seed, shape, draw in [(42, (1, 128, 2, 8, 8), 0), (0, (7,), 0), (2**40 + 5, (3, 11), 2), (42, (1, 128, 4, 16, 24), 1)]:
        got = ltx.mlx_random_normal(seed, shape, draw)
        want = oracle.mlx_random_normal(seed, shape, draw)
        assert got.shape == tuple(shape)
        np.testing.assert_allclose(got, want, rtol=2e-6, atol=1e-7)  # libm logf vs numpy log: <= 1 ulp apart
    x = ltx.mlx_random_normal(42, (1, 128, 4, 16, 24))
    assert abs(float(x.mean())) < 0.01 and abs(float(x.std()) - 1.0) < 0.01 and np.isfinite(x).all()
    assert not np.array_equal(x, ltx.mlx_random_normal(43, (1, 128, 4, 16, 24)))
    assert not np.array_equal(x, ltx.mlx_random_normal(42, (1, 128, 4, 16, 24), 1))  # second draw after the same seed


def test_attention_key_split_plan(ltx):
    """Host logic of the attention launcher's key split (attention.h): only launches that leave most CUs idle AND have at least four
    key tiles are divided, into at most 8 non-empty ranges of whole 64-key tiles. No reference counterpart (one SDPA call,
    LTXAttention.swift:209); the plan decides which kernel arrangement computes it."""
    ks = ltx.Context.attention_key_splits
    assert ks(1, 32, 1536, 1024) == 1   # config 2: 256 workgroups already
    assert ks(1, 32, 128, 128) == 1     # config 1 self-attention: two key tiles
    assert ks(1, 32, 128, 1024) == 8    # config 1 cross-attention: 32 workgroups x 16 tiles -> 256 x 2
    assert ks(2, 32, 128, 1024) == 4    # CFG pair: 64 workgroups
    assert ks(1, 32, 384, 1024) == 4    # 64 workgroups
    assert ks(1, 32, 768, 1024) == 2    # 128 workgroups
    assert ks(1, 32, 960, 1024) == 1    # 160 workgroups: left alone
    assert ks(1, 1, 35, 257) == 2       # ragged: 192 + 65 keys
    assert ks(0, 1, 1, 1) == 1 and ks(1, 1, 1, 1 << 20) == 8
    for B, H, Tq, Tk in [(1, 2, 100, 1000), (1, 3, 1, 4097), (2, 5, 191, 333), (1, 32, 128, 1000)]:
        z = ks(B, H, Tq, Tk)
        assert 1 <= z <= 8
        if z > 1:
            keys = -(-(-(-Tk // z)) // 64) * 64   # what the launcher gives a range
            assert (z - 1) * keys < Tk <= z * keys, (B, H, Tq, Tk, z, keys)
