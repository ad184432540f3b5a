"""LoRA fusion and the de-quantise -> merge -> re-encode chain, pinned bit for bit (csrc/lora_quant.hip: dit_fuse_lora, lora_add_kernel,
quant_decode_kernel, launch_encode through a slot's row view).

The LoRA factors are small integers times a power of two with sum_r |up[o, r]| * |down[r, i]| <= 256 (tests/helpers/lora_quant_cases.py;
the bound is asserted here and in test_lora_quant_fixtures_host.py), so up @ down is exact in bf16 whatever the accumulation order, the
rank padding (1 -> 64, 65 -> 128, 160 -> 192) or a K split. What remains is eff = scale * (alpha / rank), bf16(delta * eff) and
bf16(W + d): single f32 operations that numpy float32 reproduces exactly. Every comparison below is an equality of bit patterns of the
exported weights; there is no tolerance."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lora_quant_cases as lq  # noqa: E402
from test_dit_gpu import small_cfg, write_dit_file  # noqa: E402

pytestmark = pytest.mark.gpu

MISSING_UP = "diffusion_model.transformer_blocks.0.attn2.to_out.0"   # keeps its down half only: passed over, not counted
WIDE_ALPHA = "diffusion_model.transformer_blocks.0.ff.net.2"         # a two-element .alpha: no alpha, the plain fuse scale applies


@pytest.fixture(scope="module")
def base(ltx, oracle, tmp_path_factory):
    cfg, ocfg = small_cfg(ltx, oracle, heads=lq.HEADS, layers=lq.LAYERS, caption=lq.CAPTION)
    w = oracle.synth_dit_weights(ocfg, seed=31)
    path = tmp_path_factory.mktemp("lora_exact") / "dit.safetensors"
    write_dit_file(oracle, w, path)
    return cfg, ocfg, w, path


def _save(lora, path, dtype="f32"):
    if dtype == "f32":
        from safetensors.numpy import save_file

        save_file({k: np.ascontiguousarray(v, dtype=np.float32) for k, v in lora.items()}, str(path))
    else:
        import torch
        from safetensors.torch import save_file

        td = {"bf16": torch.bfloat16, "f16": torch.float16}[dtype]
        save_file({k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(td).contiguous() for k, v in lora.items()}, str(path))


def _export_all(ctx, w):
    return {k: ctx.dit_export_param(k) for k in w}


def _loaded(ltx, base, bits):
    """The model, quantised after the load when bits is 8 or 4, and its exports before any fuse."""
    cfg, ocfg, w, path = base
    ctx = ltx.Context(0)
    ctx.dit_load(path, cfg)
    if bits != 16:
        ctx.dit_quantize(bits)
    return ctx, _export_all(ctx, w)


def _full_file(oracle, base, recipe):
    cfg, ocfg, w, path = base
    lora, meta = lq.make_exact_lora(recipe, lq.reachable_linears(ocfg))
    lq.drop_up_half(lora, MISSING_UP)
    del meta[oracle.map_lora_key(MISSING_UP)]
    lora[WIDE_ALPHA + ".alpha"] = np.array([64.0, 64.0], np.float32)
    assert max(lq.partial_sum_bound(up, down) for up, down, _, _ in meta.values()) <= lq.BOUND
    return lora, meta


def _check(oracle, ctx, w, before, lora, scale, bits, n_fused):
    """Every fused key equals the numpy float32 composition, every other parameter its export before the fuse - bit for bit."""
    keys = lq.fused_module_keys(oracle, w, lora)
    if bits == 16:
        want, n_ref = lq.oracle_fuse(oracle, w, lora, scale)
        ref_before = w
    else:
        n_ref = len(keys)
        ref_before, want = lq.requant_reference(oracle, w, lora, scale, bits, keys)
    assert n_fused == n_ref == len(keys)
    after = _export_all(ctx, w)
    bad = []
    for k in w:
        if k in keys:
            assert lq.same_bits(before[k], ref_before[k]), k   # the starting point is the reference's too
            # the reference itself must move: most elements (bf16 model) / most groups (quantised model), else equality proves little
            if bits == 16:
                assert float((want[k] != w[k]).mean()) > 0.5, k
            else:
                assert lq.changed_group_share(want[k], ref_before[k]) > 0.5, k
            if not lq.same_bits(after[k], want[k]):
                d = after[k].reshape(want[k].shape) != want[k]
                bad.append((k, "fused", float(d.mean()), float(np.abs(after[k].reshape(want[k].shape) - want[k]).max())))
        elif not lq.same_bits(after[k], before[k]):
            bad.append((k, "not named by the file, yet changed", float((after[k] != before[k]).mean())))
    assert not bad, bad
    assert all(np.isfinite(v).all() for v in after.values())


@pytest.mark.parametrize("name", list(lq.RECIPES))
def test_fuse_into_bf16_model_is_the_float32_composition(ltx, oracle, base, tmp_path, name):
    """Ranks 1, 16, 64, 65, 160; alpha present and absent; scale 0.8 with alpha / rank = 8 / 65; lora_down / lora_up and lora_A / lora_B,
    with and without '.weight'; all 26 Linears a LoRA key reaches; `proj_in` (patchify_proj under its file name, which map_lora_key does
    not translate: skipped as the reference skips it), a layer without its up half (skipped, not counted) and a two-element .alpha
    (ignored)."""
    cfg, ocfg, w, path = base
    recipe = lq.RECIPES[name]
    lora, meta = _full_file(oracle, base, recipe)
    _save(lora, tmp_path / "lora.safetensors")
    ctx, before = _loaded(ltx, base, 16)
    try:
        n = ctx.fuse_lora(tmp_path / "lora.safetensors", scale=recipe.scale)
        assert n == len(lq.reachable_linears(ocfg)) - 1
        _check(oracle, ctx, w, before, lora, recipe.scale, 16, n)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["r16-alpha", "r65-alpha"])
@pytest.mark.parametrize("bits", [8, 4])
def test_fuse_into_quantised_model_is_decode_merge_encode(ltx, oracle, base, tmp_path, bits, name):
    """wq = bf16(fake_quant(W)) (quant_decode_kernel's store), merged = bf16(wq + d) (lora_add_kernel), want = bf16(fake_quant(merged))
    (launch_encode into the slot, then the export's decode) - including the to_q / to_k row views of the fused matrix and the 4-bit
    nibble packing. Keys the file does not name export what they exported after dit_quantize; the memory books do not move."""
    cfg, ocfg, w, path = base
    recipe = lq.RECIPES[name]
    lora, meta = _full_file(oracle, base, recipe)
    _save(lora, tmp_path / "lora.safetensors")
    ctx, before = _loaded(ltx, base, bits)
    try:
        mem = ctx.dit_memory_info()
        n = ctx.fuse_lora(tmp_path / "lora.safetensors", scale=recipe.scale)
        assert ctx.dit_memory_info() == mem
        _check(oracle, ctx, w, before, lora, recipe.scale, bits, n)
    finally:
        ctx.close()


@pytest.mark.parametrize("half", ["to_q", "to_k"])
@pytest.mark.parametrize("bits", [16, 8, 4])
def test_fusing_one_half_of_the_q_k_matrix_leaves_the_other_alone(ltx, oracle, base, tmp_path, bits, half):
    """A file that names only attn1.to_k (to_q) of block 1: that view merges, attn1.to_q (to_k) of block 1 and both of block 0 - and every
    other parameter - keep their bits. In a quantised model the view's code offset (off * bits / 8) and scale / bias offset (off / 64)
    are what this sees: one row off and a neighbour's groups change."""
    cfg, ocfg, w, path = base
    layer = [l for l in lq.reachable_linears(ocfg) if l[0] == f"diffusion_model.transformer_blocks.1.attn1.{half}"]
    assert len(layer) == 1
    lora, meta = lq.make_exact_lora(lq.RECIPES["r16-alpha"], layer, extras=False)
    assert lq.partial_sum_bound(*meta[layer[0][1]][:2]) <= lq.BOUND
    _save(lora, tmp_path / "lora.safetensors")
    ctx, before = _loaded(ltx, base, bits)
    try:
        n = ctx.fuse_lora(tmp_path / "lora.safetensors", scale=0.8)
        assert n == 1
        _check(oracle, ctx, w, before, lora, 0.8, bits, n)
    finally:
        ctx.close()


def test_file_dtype_does_not_change_the_merge(ltx, oracle, base, tmp_path):
    """The same factors (exact in f32, bf16 and f16) written in each of the three types st_to_bf16 takes: identical merged weights."""
    cfg, ocfg, w, path = base
    recipe = lq.RECIPES["r65-alpha"]
    lora, meta = _full_file(oracle, base, recipe)
    for k, v in lora.items():
        if ".lora_" in k:
            assert np.array_equal(v.astype(np.float16).astype(np.float32), v) and np.array_equal(oracle.bf16_round(v), v)
    want, n_ref = lq.oracle_fuse(oracle, w, lora, recipe.scale)
    keys = lq.fused_module_keys(oracle, w, lora)
    for dtype in ("f32", "bf16", "f16"):
        lpath = tmp_path / f"lora_{dtype}.safetensors"
        _save(lora, lpath, dtype)
        ctx = ltx.Context(0)
        try:
            ctx.dit_load(path, cfg)
            assert ctx.fuse_lora(lpath, scale=recipe.scale) == n_ref
            bad = [k for k in keys if not lq.same_bits(ctx.dit_export_param(k), want[k])]
            assert not bad, (dtype, bad)
        finally:
            ctx.close()
