"""CPU side of the 384 x 256 GEMM kernel (gemm_bf16_kernel_tall, tile_cfg 76): the generated stream carries the static RAW / WAR wait
proof and the operand proof and matches the committed files; the checker rejects both injected races; the sibling generators still emit
their committed files; the stream has the shape its design fixes; the launcher's decision table, pinned through the host-only hook; the
option row."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ltx-video-swift-mlx_amd", "csrc")
TALL = os.path.join(ROOT, "tools", "gen_gemm_asm_tall.py")
DTL = os.path.join(ROOT, "tools", "gen_gemm_asm_dtl.py")
QKV = os.path.join(ROOT, "tools", "gen_gemm_asm_qkv.py")
ENV = {k: v for k, v in os.environ.items() if k not in ("TALL_KNOBS", "DTL_KNOBS", "QKV_KNOBS")}


def test_tall_stream_is_proven_and_matches_the_committed_files():
    r = subprocess.run([sys.executable, TALL, "--check"], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0 and "wait coverage ok" in r.stdout and "matches" in r.stdout and "DIFFER" not in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("flag,kind", [("--inject-raw-race", "RAW"), ("--inject-war-race", "WAR")])
def test_tall_checker_rejects_injected_races(flag, kind):
    r = subprocess.run([sys.executable, TALL, "--check", flag], capture_output=True, text=True, env=ENV)
    assert r.returncode != 0 and "WaitCoverageError: " + kind in r.stderr, r.stderr[-400:]


@pytest.mark.parametrize("gen", [DTL, QKV], ids=["dtl", "qkv"])
def test_sibling_generators_still_emit_their_committed_files(gen):
    r = subprocess.run([sys.executable, gen, "--check"], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0 and "wait coverage ok" in r.stdout and "matches" in r.stdout and "DIFFER" not in r.stdout, r.stdout + r.stderr


def test_tall_stream_shape():
    """The loop body is two K-tiles long: 2 x 192 MFMAs (12 x 8 accumulators x 2 k-steps per tile) of the one instruction every GEMM
    kernel here accumulates with, 40 fragment reads and 20 LDS-DMA pieces per K-tile, two barriers per K-tile, and one counted vmcnt
    per K-tile that leaves exactly the 8 newer weight pieces in flight. No VALU instruction in the loop."""
    inc = open(os.path.join(CSRC, "gemm_tall_384x256.inc")).read()
    loop = inc[inc.index('"10:'):inc.index('"s_branch 10b')]
    tiles = 2
    assert len(re.findall(r"v_mfma_f32_16x16x32_bf16", loop)) == 192 * tiles and len(re.findall(r"v_mfma", inc)) == 192 * tiles
    assert len(re.findall(r"ds_read_b128", loop)) == 40 * tiles and len(re.findall(r"buffer_load_dwordx4", loop)) == 20 * tiles
    assert len(re.findall(r"s_barrier", loop)) == 2 * tiles and re.findall(r"vmcnt\((\d+)\)", loop) == ["8"] * tiles
    ops = set(re.findall(r'^"([a-z][a-z_0-9]*)', loop, flags=re.M))
    assert ops == {"v_mfma_f32_16x16x32_bf16", "ds_read_b128", "buffer_load_dwordx4", "s_add_u32", "s_nop", "s_waitcnt", "s_barrier", "s_sub_u32",
                   "s_cmp_eq_u32", "s_cbranch_scc1"}, ops
    # all 160 KB of LDS: two 48 KB activation slots, two 32 KB weight slots; the last LDS-DMA piece ends at the last byte
    dst = [int(x) for x in re.findall(r"s_add_u32 m0, %\[wlds\], (\d+)", inc)]
    assert max(dst) + 4096 == 2 * 384 * 128 + 2 * 256 * 128 == 163840 and min(dst) == 0


# flags of ltx_gemm_dense_tile_cfg: 1 f32 output, 2 bf16 output, 4 gated residual, 8 transposed bf16 output, 16 per-row bias
@pytest.mark.parametrize("shape,act,flags,want", [
    ((1536, 16384, 4096), 1, 2, 76),    # FFN-up at 1536 tokens: 4 x 64 tiles = one round
    ((3072, 16384, 4096), 1, 2, 76),    # two rounds
    ((1536, 16384, 4096), 0, 1, 76),    # f32 store
    ((1536, 8192, 4096), 0, 2, 75),     # 128 tall tiles: half a round
    ((9984, 16384, 4096), 1, 2, 75),    # 26 x 64 = 6.5 rounds
    ((1536, 4096, 4096), 0, 2, 21),
    ((1536, 16384, 4096), 0, 1 | 4, 75),   # gated residual: never the 384 x 256 kernel
    ((3072, 16384, 4096), 0, 1 | 2 | 4, 75),
    ((1536, 16384, 4096), 0, 2 | 16, 75),  # per-row bias
])
def test_decision_table_with_256_cus(ltx, shape, act, flags, want):
    assert ltx.gemm_dense_tile_cfg(*shape, act=act, flags=flags, ncu=256) == want


def test_decision_follows_the_option_and_the_cu_count(ltx):
    assert ltx.get_option("gemm_tall") == 1
    ltx.set_option("gemm_tall", 0)
    try:
        assert ltx.gemm_dense_tile_cfg(1536, 16384, 4096, act=1, flags=2, ncu=256) == 75
    finally:
        ltx.set_option("gemm_tall", 1)
    assert ltx.gemm_dense_tile_cfg(1536, 16384, 4096, act=1, flags=2, ncu=256) == 76
    assert ltx.gemm_dense_tile_cfg(1536, 16384, 4096, act=1, flags=2, ncu=128) == 76    # two rounds of 128
    assert ltx.gemm_dense_tile_cfg(1536, 16384, 4096, act=1, flags=2, ncu=304) == 75    # 256 tiles are no whole round of 304
    assert ltx.gemm_dense_tile_cfg(1536, 16384, 100, ncu=256) == -1


def test_option_row(ltx):
    row = [t for t in ltx.option_table() if t[0] == "gemm_tall"]
    assert len(row) == 1 and row[0][1:5] == (1, 0, 1, 0)   # default 1, range 0 / 1, bit-neutral
