"""The three GEMM kernels with a generated gfx950 main loop (csrc/gemm_asm_tiles.inc) against bits recorded before their shared
prologue, plain-store epilogue and launcher were written once: tests/golden/gemm_asm_family_digests.json holds one sha256 per output
buffer (tests/golden/make_golden.py --gemm-asm-family-digests; cases, shapes and inputs in tests/helpers/gemm_asm_family.py). Bytes are
compared, poisoned border included, so there is no tolerance: another order of the epilogue's floating-point operations, a wrong row
or column base, a store past the tile or a dropped K-tile changes a digest.

The residual case runs at (3072, 4096, 128): 256 tiles of 192 x 256, the fewest for which the dense tile choice is that kernel;
ltx_op_gemm_bf16_gated_residual passes no workspace, so the launcher neither splits K nor (256 tiles on 256 CUs) the rows."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gemm_asm_family as fam  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_asm_family_digests.json")


@pytest.fixture(scope="module")
def want():
    with open(GOLDEN) as f:
        w = json.load(f)
    assert w["seed"] == fam.SEED and sorted(w["digests"]) == fam.expected_keys()
    return w["digests"]


def _compare(got, want):
    wrong = sorted(k for k in got if got[k] != want[k])
    print(f"{len(got)} digests, {len(wrong)} differ")
    assert got and not wrong, wrong


def test_192x256_kernel_plain_stores(ltx, gpu_ctx, want):
    _compare(fam.gemm_cases(ltx, gpu_ctx, 75, fam.DTL_SHAPES), want)


def test_384x256_kernel(ltx, gpu_ctx, want):
    _compare(fam.gemm_cases(ltx, gpu_ctx, 76, fam.TALL_SHAPES), want)


def test_fused_qkv_kernel(gpu_ctx, want):
    _compare(fam.qkv_cases(gpu_ctx), want)


def test_192x256_kernel_residual_epilogue(ltx, gpu_ctx, want):
    assert fam.resid_tile_cfg(ltx) == 75   # or the launch below would test another kernel
    _compare(fam.resid_case(ltx, gpu_ctx), want)


def test_forward_and_denoise_step(ltx, want):
    model = fam.two_layer_context(ltx)
    try:
        _compare(fam.forward_case(model), want)
    finally:
        model.close()
