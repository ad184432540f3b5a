"""CPU side of the fused q|k + V projection (gemm_bf16_kernel_qkv): the generated 192 x 384 stream carries the same static RAW / WAR
wait proof as the 192 x 256 stream and matches the committed files; the checker rejects both injected races; the 192 x 256 generator
still emits its committed file; the new entry point and its switch are declared, exported and bound."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QKV = os.path.join(ROOT, "tools", "gen_gemm_asm_qkv.py")
DTL = os.path.join(ROOT, "tools", "gen_gemm_asm_dtl.py")


def test_qkv_stream_is_proven_and_matches_the_committed_files():
    r = subprocess.run([sys.executable, QKV, "--check"], capture_output=True, text=True)
    assert r.returncode == 0 and "wait coverage ok" in r.stdout and "matches" in r.stdout and "DIFFER" not in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("flag,kind", [("--inject-raw-race", "RAW"), ("--inject-war-race", "WAR")])
def test_qkv_checker_rejects_injected_races(flag, kind):
    r = subprocess.run([sys.executable, QKV, "--check", flag], capture_output=True, text=True)
    assert r.returncode != 0 and "WaitCoverageError: " + kind in r.stderr, r.stderr[-400:]


def test_gemm_192x256_generator_still_emits_its_committed_file():
    r = subprocess.run([sys.executable, DTL, "--check"], capture_output=True, text=True)
    assert r.returncode == 0 and "matches" in r.stdout, r.stdout + r.stderr


def test_qkv_stream_shape():
    """What the issue fixes about the stream: 2 x 144 MFMAs of the one instruction every GEMM kernel here accumulates with, 18 fragment
    reads per 72 MFMAs, 18 LDS-DMA pieces per K-tile, two barriers per K-tile, and a counted wait that leaves exactly tile t+2 in flight."""
    inc = open(os.path.join(ROOT, "ltx-video-swift-mlx_amd", "csrc", "gemm_qkv_192x384.inc")).read()
    loop = inc[inc.index('"10:'):inc.index('"s_branch 10b')]
    assert len(re.findall(r"v_mfma_f32_16x16x32_bf16", loop)) == 288 and len(re.findall(r"v_mfma", inc)) == 288
    assert len(re.findall(r"ds_read_b128", loop)) == 2 * 36 and len(re.findall(r"buffer_load_dwordx4", loop)) == 2 * 18
    assert len(re.findall(r"s_barrier", loop)) == 4 and re.findall(r"vmcnt\((\d+)\)", loop) == ["18", "18"]


def test_entry_point_and_switch_are_declared_exported_and_bound(ltx):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ltxhip.h")).read(), flags=re.S)
    from importlib import import_module

    lib_mod = import_module("ltx-video-swift-mlx_amd._lib")
    so = ctypes.CDLL(lib_mod.SO_PATH)
    assert "ltx_op_qkv_projection" in hdr and hasattr(so, "ltx_op_qkv_projection") and "ltx_op_qkv_projection" in lib_mod.SIGNATURES
    assert hasattr(ltx.Context, "op_qkv_projection")
    row = [t for t in ltx.option_table() if t[0] == "qkv_fused"]
    assert len(row) == 1 and row[0][2:5] == (0, 1, 0)   # 0 / 1, bit-neutral
    assert ltx.lib.ltx_op_qkv_projection(None, None, 0, 0, 0, None, None, None, None, 0, 0, None, 0, None, 0, 1) == 2   # no context: refused
