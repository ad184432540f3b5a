"""The parameter tables of the five transformer-family models (csrc/params.cpp): DiT, text-embedding connector, attention module, dual
blocks, dual model.

Synthetic weights: after ``*_init_synthetic(seed=7)`` at each model's smallest legal shape, every parameter's bytes match the sha256
recorded in tests/golden/synthetic_param_digests.json (tests/golden/make_golden.py --synthetic-digests; shapes and the connector's
stand-in for an export in tests/helpers/synthetic_params.py). Bytes are compared, so there is no tolerance: a parameter placed at
another offset, a view onto the wrong block, a different walk of the seeds or another distribution rule changes a digest.

Load rule: a 2-D file tensor for a matrix parameter must be [rows, cols]; a same-size transposed Linear weight is weightLoadingFailed."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import synthetic_params as sp  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "synthetic_param_digests.json")


@pytest.fixture(scope="module")
def ctx(ltx):
    c = ltx.Context(0)
    yield c
    c.close()


def test_synthetic_weights_match_the_recorded_digests(ltx, oracle, ctx):
    with open(GOLDEN) as f:
        want = json.load(f)
    assert want["seed"] == sp.SEED
    got = sp.digests(ltx, oracle, ctx)
    keys = sp.expected_keys(oracle)
    assert sorted(got) == sorted(want["models"]) == sorted(keys)
    for model in sorted(got):
        assert sorted(want["models"][model]) == keys[model], model
        wrong = [k for k in keys[model] if got[model][k] != want["models"][model][k]]
        print(f"{model}: {len(keys[model])} digests, {len(wrong)} differ")
        assert not wrong, (model, wrong[:8])


def test_a_transposed_linear_weight_is_refused(ltx, oracle, ctx, tmp_path):
    from safetensors.numpy import save_file

    w = oracle.synth_dit_weights(oracle.DiTConfig(**sp.DIT), seed=sp.SEED)
    assert w["patchify_proj.weight"].shape == (128, 64)

    def write(path, weights):
        save_file({k: np.ascontiguousarray(v, dtype=np.float32) for k, v in oracle.dit_file_keys(weights).items()}, str(path))

    write(tmp_path / "good.safetensors", w)
    ctx.dit_load(tmp_path / "good.safetensors", sp.dit_cfg(ltx))
    assert ctx.load_report() == {"loaded": len(w), "missing": 0, "unmatched": 0}
    assert np.array_equal(ctx.dit_export_param("patchify_proj.weight"), w["patchify_proj.weight"].ravel())
    bad = dict(w)
    bad["patchify_proj.weight"] = np.ascontiguousarray(w["patchify_proj.weight"].T)  # [64, 128]: the same element count
    write(tmp_path / "transposed.safetensors", bad)
    with pytest.raises(ltx.LTXError, match=r"expected \[128, 64\]") as e:
        ctx.dit_load(tmp_path / "transposed.safetensors", sp.dit_cfg(ltx))
    assert e.value.case == "weightLoadingFailed"
    with pytest.raises(ltx.LTXError) as e:  # the failed load published no model
        ctx.dit_export_param("patchify_proj.weight")
    assert e.value.case == "modelNotLoaded"
