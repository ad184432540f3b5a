"""A weight change behind a cached text context. The caption projection and every block's cross-attention K / V are kept per context
version (DiTModel::ctx_cache, csrc/dit.cpp prepare_context); dit_fuse_lora, dit_quantize, dit_load_safetensors and dit_init_synthetic
reset the entries' versions after they changed weights. Here one non-zero version is used throughout:

    a = forward(v);  change the weights;  b = forward(v);  c = forward(0)

b and c must be equal bit for bit (the cached products were rebuilt from the new weights), a and b must differ - and the oracle must
differ over the same change too, so that the second half cannot be vacuous. A stale entry would leave b == a where only cached
products changed (a LoRA on attn2.to_k / to_v or on the caption projection) and b != c everywhere else.
ltx_dit_load and ltx_dit_init_synthetic build a new model object (replace_model), so for those two the sequence checks the entry point
as a whole: no cached product survives it."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import lora_quant_cases as lq  # noqa: E402
from test_dit_gpu import rel_l2, small_cfg, write_dit_file  # noqa: E402

pytestmark = pytest.mark.gpu

VERSION = 0x5EED5EED5EED
F, H, W, S = lq.FRAMES, lq.HEIGHT, lq.WIDTH, lq.TEXT
T = F * H * W


@pytest.fixture(scope="module")
def base(ltx, oracle, tmp_path_factory):
    cfg, ocfg = small_cfg(ltx, oracle, heads=lq.HEADS, layers=lq.LAYERS, caption=lq.CAPTION)
    w = oracle.synth_dit_weights(ocfg, seed=31)
    tmp = tmp_path_factory.mktemp("text_cache")
    write_dit_file(oracle, w, tmp / "dit.safetensors")
    rng = np.random.default_rng(4)
    latent = oracle.bf16_round(rng.standard_normal((1, T, 128)).astype(np.float32))
    context = oracle.bf16_round(rng.standard_normal((1, S, lq.CAPTION)).astype(np.float32))
    return cfg, ocfg, w, tmp, latent, context


def _dev_bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).cuda()


def _lora_file(oracle, ocfg, tmp, wanted):
    from safetensors.numpy import save_file

    layers = [l for l in lq.reachable_linears(ocfg) if any(l[0].endswith(s) for s in wanted)]
    lora, meta = lq.make_exact_lora(lq.RECIPES["r16-alpha"], layers, extras=False)
    assert layers and max(lq.partial_sum_bound(up, down) for up, down, _, _ in meta.values()) <= lq.BOUND
    path = tmp / ("lora_" + "_".join(s.replace(".", "") for s in wanted) + ".safetensors")
    save_file(lora, str(path))
    return lora, len(layers), path


def _change(kind, ltx, oracle, ctx, base):
    """Apply one weight change to the loaded model; -> the oracle's weights after it."""
    cfg, ocfg, w, tmp, _, _ = base
    if kind in ("lora_cross_kv", "lora_caption"):
        wanted = ("attn2.to_k", "attn2.to_v") if kind == "lora_cross_kv" else ("caption_projection.linear_2",)
        lora, n, path = _lora_file(oracle, ocfg, tmp, wanted)
        assert ctx.fuse_lora(path, scale=0.8) == n
        return lq.oracle_fuse(oracle, w, lora, 0.8)[0]
    if kind == "quantize8":
        ctx.dit_quantize(8)
        return oracle.quantize_dit_weights(w, 8)
    if kind == "init_synthetic":
        ctx.dit_init_synthetic(cfg, seed=6)
        return {k: ctx.dit_export_param(k).reshape(v.shape) for k, v in w.items()}
    if kind == "load":
        w2 = oracle.synth_dit_weights(ocfg, seed=32)
        write_dit_file(oracle, w2, tmp / "dit2.safetensors")
        ctx.dit_load(tmp / "dit2.safetensors", cfg)
        return w2
    raise AssertionError(kind)


@pytest.mark.parametrize("kind", ["lora_cross_kv", "lora_caption", "quantize8", "init_synthetic", "load"])
def test_forward_after_a_weight_change_rebuilds_the_cached_context(ltx, oracle, base, kind):
    cfg, ocfg, w, tmp, latent, context = base
    lat, cx = _dev_bf16(latent), _dev_bf16(context)
    ts = torch.full((1,), 0.8, dtype=torch.float32, device="cuda")

    def forward(ctx, version):
        vel = torch.full((1, T, 128), float("nan"), dtype=torch.float32, device="cuda")
        ctx.dit_forward_dev(lat, cx, ts, None, F, H, W, vel, ctx_version=version)
        torch.cuda.synchronize()
        return vel.cpu().numpy()

    ctx = ltx.Context(0)
    try:
        ctx.dit_load(tmp / "dit.safetensors", cfg)
        a = forward(ctx, VERSION)
        assert lq.same_bits(a, forward(ctx, VERSION)) and lq.same_bits(a, forward(ctx, 0))   # cached == recomputed to begin with
        w_after = _change(kind, ltx, oracle, ctx, base)
        b = forward(ctx, VERSION)
        c = forward(ctx, 0)
    finally:
        ctx.close()
    assert np.isfinite(a).all() and np.isfinite(c).all()
    assert lq.same_bits(b, c), (kind, "stale text cache", float(np.abs(b - c).max()))
    assert not lq.same_bits(a, b)
    tsn = np.array([0.8], np.float32)
    ref_a = oracle.dit_forward(w, ocfg, latent, context, tsn, None, F, H, W)
    ref_b = oracle.dit_forward(w_after, ocfg, latent, context, tsn, None, F, H, W)
    assert rel_l2(ref_b, ref_a) > 1e-3, (kind, rel_l2(ref_b, ref_a))   # the change is real in the reference too


def test_denoise_after_fuse_lora_rebuilds_the_cached_context(ltx, oracle, base):
    """One Euler step (two sigmas) through denoise_dev with the same version before and after a LoRA on attn2.to_k / to_v, against the
    same call with version 0 (context recomputed every step)."""
    cfg, ocfg, w, tmp, latent, context = base
    cx = _dev_bf16(context)
    sig = np.array([1.0, 0.8], np.float32)
    noise = np.random.default_rng(6).standard_normal((1, 128, F, H, W)).astype(np.float32)

    def denoise(ctx, version):
        x = torch.from_numpy(noise).cuda()
        ctx.denoise_dev(x, sig, cx, None, F, H, W, ctx_version=version)
        torch.cuda.synchronize()
        return x.cpu().numpy()

    ctx = ltx.Context(0)
    try:
        ctx.dit_load(tmp / "dit.safetensors", cfg)
        a = denoise(ctx, VERSION)
        assert lq.same_bits(a, denoise(ctx, 0))
        lora, n, path = _lora_file(oracle, ocfg, tmp, ("attn2.to_k", "attn2.to_v"))
        assert ctx.fuse_lora(path, scale=0.8) == n
        b = denoise(ctx, VERSION)
        c = denoise(ctx, 0)
    finally:
        ctx.close()
    assert np.isfinite(c).all()
    assert lq.same_bits(b, c), ("stale text cache", float(np.abs(b - c).max()))
    assert not lq.same_bits(a, b)
    wf = lq.oracle_fuse(oracle, w, lora, 0.8)[0]
    ref_a = oracle.denoise(w, ocfg, noise, sig, context, None, F, H, W)
    ref_b = oracle.denoise(wf, ocfg, noise, sig, context, None, F, H, W)
    assert rel_l2(ref_b, ref_a) > 1e-3, rel_l2(ref_b, ref_a)
