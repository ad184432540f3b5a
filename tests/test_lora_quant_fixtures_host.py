"""The preconditions of the bit-exact LoRA / requantisation / encoder GPU tests, as facts about the reference alone (no GPU): the
partial-sum bound of every LoRA fixture, "the merge changes more than half of the elements", "the requantisation changes most
groups", and oracle.fake_quant finite and warning-free on every crafted group. A change to tests/helpers/lora_quant_cases.py can then
not quietly empty the GPU tests."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lora_quant_cases as lq  # noqa: E402


@pytest.fixture(scope="module")
def model(oracle):
    ocfg = oracle.DiTConfig(num_layers=lq.LAYERS, num_heads=lq.HEADS, caption_channels=lq.CAPTION)
    return ocfg, oracle.synth_dit_weights(ocfg, seed=31)


def test_reachable_linears_are_all_the_linears_but_patchify(oracle, model):
    ocfg, w = model
    named = {mk for _, mk, _, _ in lq.reachable_linears(ocfg)}
    linears = {k for k, v in w.items() if k.endswith(".weight") and v.ndim == 2}
    assert named == linears - {"patchify_proj.weight"}
    for base, mk, out, inn in lq.reachable_linears(ocfg):
        assert oracle.map_lora_key(base) == mk and w[mk].shape == (out, inn)
    assert oracle.map_lora_key("diffusion_model.proj_in") not in w   # the file's name of patchify_proj is not translated


@pytest.mark.parametrize("name", list(lq.RECIPES))
def test_lora_fixture_is_exact_and_strong_enough(oracle, model, name):
    ocfg, w = model
    recipe = lq.RECIPES[name]
    lora, meta = lq.make_exact_lora(recipe, lq.reachable_linears(ocfg))
    assert len(meta) == len(lq.reachable_linears(ocfg))
    worst = 0
    for mk, (up, down, su, sd) in meta.items():
        worst = max(worst, lq.partial_sum_bound(up, down))
        assert up.shape[1] == recipe.rank == down.shape[0]
    assert worst <= lq.BOUND, worst
    # the file's values are the integers times a power of two, and survive bf16 and f16 unchanged
    for k, v in lora.items():
        if ".lora_" in k:
            assert np.array_equal(oracle.bf16_round(v), v) and np.array_equal(v.astype(np.float16).astype(np.float32), v), k
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        wf, n = lq.oracle_fuse(oracle, w, lora, recipe.scale)
    assert n == len(meta)
    keys = lq.fused_module_keys(oracle, w, lora)
    assert keys == set(meta)
    for k in keys:
        assert np.isfinite(wf[k]).all()
        assert float((wf[k] != w[k]).mean()) > 0.5, (k, float((wf[k] != w[k]).mean()))        # the merge is no no-op ...
        assert float(np.abs(wf[k] - w[k]).std()) < 4 * float(w[k].std()), k                   # ... and does not swamp the weights
    for k in set(w) - keys:
        assert wf[k] is w[k]
    for bits in (8, 4):
        wq, want = lq.requant_reference(oracle, w, lora, recipe.scale, bits, keys)
        for k in keys:
            assert lq.changed_group_share(want[k], wq[k]) > 0.5, (bits, k, lq.changed_group_share(want[k], wq[k]))


def test_skipped_layers_are_skipped_by_the_reference(oracle, model):
    ocfg, w = model
    layers = lq.reachable_linears(ocfg)
    lora, meta = lq.make_exact_lora(lq.RECIPES["r16-alpha"], layers)
    lq.drop_up_half(lora, "diffusion_model.transformer_blocks.0.attn2.to_out.0")
    lora["diffusion_model.transformer_blocks.0.ff.net.2.alpha"] = np.array([64.0, 64.0], np.float32)
    wf, n = lq.oracle_fuse(oracle, w, lora, 0.8)
    assert n == len(layers) - 1
    assert wf["transformer_blocks.0.attn2.to_out.weight"] is w["transformer_blocks.0.attn2.to_out.weight"]
    assert wf["patchify_proj.weight"] is w["patchify_proj.weight"]
    # the two-element alpha is no alpha: the layer merges at the plain fuse scale, which differs from the alpha / rank merge
    one = dict(lora)
    one["diffusion_model.transformer_blocks.0.ff.net.2.alpha"] = np.array(8.0, np.float32)
    k = "transformer_blocks.0.ff.project_out.weight"
    assert not np.array_equal(lq.oracle_fuse(oracle, w, one, 0.8)[0][k], wf[k])


@pytest.mark.parametrize("bits", [8, 4])
def test_fake_quant_is_finite_and_silent_on_the_crafted_groups(oracle, model, bits):
    ocfg, w = model
    groups = lq.crafted_groups(oracle)
    assert len(groups) == 14
    m = np.stack(list(groups.values()))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with np.errstate(all="raise"):
            q = oracle.fake_quant(m, bits)
    assert np.isfinite(q).all() and np.isfinite(oracle.bf16_round(q)).all()
    names = list(groups)
    for n in ("zero", "under_floor", "tiny_normal"):
        assert not q[names.index(n)].any(), n                       # at or under the 1e-7 floor: every code is 0, the bias is 0
    for n in ("const_pos", "const_neg"):
        assert np.array_equal(oracle.bf16_round(q[names.index(n)]), m[names.index(n)]), n
    if bits == 8:
        # the half-step ramp does land on ties: (w - bias) / scale = 254.5 - k exactly
        h = m[names.index("half_steps")]
        t = (h - np.float32(255.0 / 256.0)) / np.float32(-2.0 ** -8)
        assert int((np.abs(t - np.floor(t)) == 0.5).sum()) == 62
    wa, where = lq.plant_groups(w, groups)
    for k in lq.ADVERSARIAL_KEYS:
        flat, orig = wa[k].reshape(-1, 64), w[k].reshape(-1, 64)
        assert len(where[k]) >= 28 and 0 in where[k] and flat.shape[0] - 1 in where[k]
        untouched = np.setdiff1d(np.arange(flat.shape[0]), where[k])
        assert np.array_equal(flat[untouched], orig[untouched]) and np.array_equal(oracle.bf16_round(wa[k]), wa[k])
