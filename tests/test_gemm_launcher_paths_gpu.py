"""The branches of launch_gemm_bf16 that launch more than one kernel or choose a split count, against bits recorded before the launcher
read its options once and wrote each rule once: tests/golden/gemm_launcher_paths_digests.json holds one sha256 per output buffer
(tests/golden/make_golden.py --gemm-launcher-paths-digests; cases, shapes and inputs in tests/helpers/gemm_launcher_paths.py). Bytes are
compared, poisoned border included, so there is no tolerance: another split count, a row or tile window that starts elsewhere, a finish
pass over the wrong rows or another kernel for a part of the output changes a digest.

The shapes follow the launcher's rules for 256 CUs; on another CU count the branches are other ones and the file skips."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import gemm_launcher_paths as paths  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_launcher_paths_digests.json")


@pytest.fixture(scope="module")
def want():
    import torch

    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    if ncu != paths.NCU:
        pytest.skip(f"the cases are the launcher's branches on {paths.NCU} CUs; this device has {ncu}")
    with open(GOLDEN) as f:
        w = json.load(f)
    assert w["seed"] == paths.SEED and sorted(w["digests"]) == paths.expected_keys()
    return w["digests"]


def _compare(got, want):
    wrong = sorted(k for k in got if got[k] != want[k])
    print(f"{len(got)} digests, {len(wrong)} differ")
    assert got and not wrong, wrong


def test_row_split_of_a_ragged_last_round(ltx, gpu_ctx, want):
    assert paths.rowsplit_tile_cfg(ltx) == 75   # or there is no row split to test
    _compare(paths.rowsplit_cases(ltx, gpu_ctx), want)


def test_few_row_launch_with_a_launcher_chosen_split(ltx, gpu_ctx, want):
    _compare(paths.fewrow_cases(ltx, gpu_ctx), want)


def test_192x256_split_k_with_the_fused_finish_and_norm(ltx, gpu_ctx, want):
    _compare(paths.dtl_split_cases(ltx, gpu_ctx), want)


@pytest.mark.parametrize("geom,name,options", paths.CONV_CASES, ids=[c[1] for c in paths.CONV_CASES])
def test_conv_launch_paths(ltx, gpu_ctx, want, geom, name, options):
    _compare(paths.conv_cases(ltx, gpu_ctx, geom, name, options), want)
