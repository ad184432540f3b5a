"""Every instantiation of the DiT's two row-pass kernel families (csrc/elementwise.hip: q/k RMSNorm + split RoPE, norm + modulation)
against bits recorded before the families were rewritten from shared pieces and their launchers took argument structs:
tests/golden/row_passes_digests.json holds one sha256 per output buffer (tests/golden/make_golden.py --row-passes-digests; cases,
shapes and inputs in tests/helpers/row_passes.py). Bytes are compared, sentinel columns and guard rows included, so there is no
tolerance: another summation order, another rounding point, a fused multiply-add where there was none, a column map that is off by a
chunk or a launcher that picks another instantiation changes a digest."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import row_passes as rp  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "row_passes_digests.json")


@pytest.fixture(scope="module")
def want():
    with open(GOLDEN) as f:
        w = json.load(f)
    assert w["seed"] == rp.SEED and sorted(w["digests"]) == rp.expected_keys()
    return w["digests"]


def _compare(got, want):
    wrong = sorted(k for k in got if got[k] != want[k])
    print(f"{len(got)} digests, {len(wrong)} differ")
    assert got and not wrong, wrong


def test_the_cases_cover_every_instantiation(want):
    launched = {k for ks in rp.covers().values() for k in ks}
    assert len(rp.KERNELS) == 26 and sorted(launched) == rp.KERNELS


@pytest.mark.gpu
def test_generic_qk_kernel_head_dim_128(gpu_ctx, want):
    _compare(rp.qk128_cases(gpu_ctx), want)


@pytest.mark.gpu
def test_generic_qk_kernel_head_dim_64(gpu_ctx, want):
    _compare(rp.qk64_cases(gpu_ctx), want)


@pytest.mark.gpu
def test_head_dim_64_attention_module_with_a_bf16_context(gpu_ctx, want):
    _compare(rp.attn64_cases(gpu_ctx), want)


@pytest.mark.gpu
def test_full_width_qk_pair_and_rows_kernels(ltx, gpu_ctx, want):
    _compare(rp.full_width_cases(ltx, gpu_ctx), want)
    assert ltx.get_option("qknorm_no_pair") == 0


@pytest.mark.gpu
def test_norm_mod_kernel(gpu_ctx, want):
    _compare(rp.norm_cases(gpu_ctx), want)


@pytest.mark.gpu
def test_norm_mod_rows_kernels(ltx, gpu_ctx, want):
    _compare(rp.normrows_cases(ltx, gpu_ctx), want)
    assert ltx.get_option("norm_rows") == 0


@pytest.mark.gpu
def test_norm_mod2_kernel(gpu_ctx, want):
    _compare(rp.norm2_cases(gpu_ctx), want)
