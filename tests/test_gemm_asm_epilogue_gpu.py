"""Every epilogue form of the three GEMM kernels with a generated main loop (192 x 256, 192 x 384 q|k|v, 384 x 256) against bits
recorded from the library of the commit BEFORE the plain stores were specialised per launch (one variant picked outside the loop over
row groups, per-lane row pointers, a two-instruction bf16 pack, GELU-tanh on pairs): tests/golden/gemm_asm_epilogue_digests.json, one
sha256 per output buffer with its poisoned border, so there is no tolerance. Cases, shapes and inputs: tests/helpers/gemm_asm_epilogue.py."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gemm_asm_epilogue as epi  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def want():
    with open(epi.GOLDEN) as f:
        w = json.load(f)
    assert w["seed"] == epi.SEED
    return w["digests"]


def _compare(got, want):
    missing = sorted(k for k in got if k not in want)
    assert got and not missing, missing
    wrong = sorted(k for k in got if got[k] != want[k])
    print(f"{len(got)} digests, {len(wrong)} differ")
    assert not wrong, wrong


def test_golden_file_holds_exactly_the_cases(want):
    """no GPU work: the names the tests below produce are the names recorded (a dropped case would otherwise go unnoticed)"""
    keys = []
    for cfg, sizes in epi.SIZES.items():
        for size in sizes:
            for K in epi.KS:
                for name, (_, _, f32, bf16) in epi.VARIANTS.items():
                    for b in ("bias", "nobias"):
                        keys += [f"cfg{cfg}.{size}.K{K}.{name}.{b}.out_{o}" for o, on in (("f32", f32), ("bf16", bf16)) if on]
        keys.append(f"cfg{cfg}.overflow.gelu_bf16")
    for size in epi.SIZES[75]:
        keys += [f"cfg75.{size}.rowbias.bf16.out_bf16", f"cfg75.{size}.rowbias.f32_bf16.out_bf16", f"cfg75.{size}.rowbias.f32_bf16.out_f32"]
        keys += [f"cfg75.{size}.K{K}.split2_{p}.out_{o}" for K in (128, 192) for p in ("f32", "bf16") for o in ("f32", "bf16")]
    for form in epi.RESID_FORMS:
        keys += [f"cfg75.resid.{form}.K{K}.x" for K in (64, 192)]
        if form in ("gate_two_batches", "gate_scalar_src_mirror"):
            keys += [f"cfg75.resid.{form}.K{K}.mirror" for K in (64, 192)]
    keys += [f"qkv.{size}.K{K}.{b}.{o}" for size in epi.QKV_SIZES for K in epi.KS for b in ("bias", "nobias") for o in ("qk_out", "vt_out")]
    assert sorted(keys) == sorted(want)


@pytest.mark.parametrize("cfg,size", [(cfg, size) for cfg in epi.SIZES for size in epi.SIZES[cfg]])
def test_plain_store_variants(ltx, gpu_ctx, want, cfg, size):
    _compare(epi.plain_cases(ltx, gpu_ctx, cfg, size), want)


def test_192x256_row_bias(ltx, gpu_ctx, want):
    _compare(epi.row_bias_cases(ltx, gpu_ctx), want)


@pytest.mark.parametrize("form", epi.RESID_FORMS)
def test_192x256_residual_and_gate(ltx, gpu_ctx, want, form):
    _compare(epi.resid_cases(ltx, gpu_ctx, form), want)


@pytest.mark.parametrize("partial", ["f32", "bf16"])
def test_192x256_split_k_partial_stores(ltx, gpu_ctx, want, partial):
    _compare(epi.splitk_cases(ltx, gpu_ctx, partial), want)


@pytest.mark.parametrize("cfg", sorted(epi.SIZES))
def test_gelu_past_the_exponent_range(ltx, gpu_ctx, want, cfg):
    got, largest, neg_zero = epi.overflow_cases(ltx, gpu_ctx, cfg)
    print(f"largest stored value {largest}, {neg_zero} stored -0")
    assert largest >= 40.0 and neg_zero > 0   # the inputs do reach both ends: x stays x, exp overflow gives -0
    _compare(got, want)


@pytest.mark.parametrize("size", sorted(epi.QKV_SIZES))
def test_fused_qkv_stores(gpu_ctx, want, size):
    _compare(epi.qkv_cases(gpu_ctx, size), want)
