"""The per-prompt text cache of the dual model (csrc/dual_model.cpp dual_model_prepare_text, csrc/dual_block.cpp dual_prepare_text,
csrc/attn_module.cpp attn_module_build_kv): ltx_dual_model_prepare_text_dev runs both caption projections, both mask biases and, per
block, the k GEMM, k norm and V^T GEMMs of the two text cross-attentions ONCE; a forward with text_cache = 1 reads them. The launches and
their operands are those of the forward that recomputes them, so both velocities must be BIT-EQUAL to the uncached forward's - at B 1 and
2, with and without masks, at the narrow width and at full width (where a launcher decision that depends on the width is taken)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import dual_model_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
NARROW = dict(Hv=4, Ha=4, F=2, H=6, W=8, T_a=26, S=70, caption_channels=256)
L_NARROW = 2


def ceil64(n):
    return (n + 63) // 64 * 64


def cache_bytes(L, B, S, Dv, Da):
    return L * B * (S + ceil64(S)) * (Dv + Da) * 2


def tensors(inp):
    bf = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda().to(torch.bfloat16)  # noqa: E731
    t = {k: bf(inp[k]) for k in ("video_latent", "audio_latent", "video_context", "audio_context")}
    for k in ("video_timesteps", "audio_timesteps"):
        t[k] = torch.from_numpy(inp[k]).cuda()
    for k in ("video_mask", "audio_mask"):
        t[k] = torch.from_numpy(np.ascontiguousarray(inp[k], dtype=np.int32)).cuda()
    return t


def forward(ctx, inp, t, masks=True, cached=False, out=None, **kw):
    """One forward into fresh (or the caller's) velocity tensors. Cached: the context and mask pointers are NULL."""
    B, Tv = inp["B"], inp["F"] * inp["H"] * inp["W"]
    vv = torch.full((B, Tv, 128), 7.0, device="cuda") if out is None else out[0]
    va = torch.full((B, inp["T_a"], 128), 7.0, device="cuda") if out is None else out[1]
    if cached:
        ctx.dual_model_forward_dev(t["video_latent"], t["audio_latent"], None, None, t["video_timesteps"], t["audio_timesteps"], vv, va,
                                   inp["F"], inp["H"], inp["W"], text_cache=1, **dict(dict(S=inp["S"]), **kw))
    else:
        ctx.dual_model_forward_dev(t["video_latent"], t["audio_latent"], t["video_context"], t["audio_context"], t["video_timesteps"],
                                   t["audio_timesteps"], vv, va, inp["F"], inp["H"], inp["W"], video_mask=t["video_mask"] if masks else None,
                                   audio_mask=t["audio_mask"] if masks else None, **kw)
    torch.cuda.synchronize()
    return vv, va


def prepare(ctx, t, masks=True):
    ctx.dual_model_prepare_text(t["video_context"], t["audio_context"], t["video_mask"] if masks else None, t["audio_mask"] if masks else None)


@pytest.fixture(scope="module")
def model(gpu_ctx, ltx):
    cfg = ltx.default_dual_model_config(num_layers=L_NARROW, video_heads=NARROW["Hv"], audio_heads=NARROW["Ha"],
                                        caption_channels=NARROW["caption_channels"])
    init = lambda: gpu_ctx.dual_model_init_synthetic(cfg, seed=51)  # noqa: E731
    init()
    yield {"init": init}
    gpu_ctx.dual_model_unload()


@pytest.mark.parametrize("masks", [True, False], ids=["masked", "null-masks"])
@pytest.mark.parametrize("B", [1, 2])
def test_cached_forward_is_bit_equal_to_the_uncached_forward(gpu_ctx, model, B, masks):
    inp = ref.make_inputs(B, seed=B, **NARROW)
    t = tensors(inp)
    want = forward(gpu_ctx, inp, t, masks)
    prepare(gpu_ctx, t, masks)
    got = forward(gpu_ctx, inp, t, masks, cached=True)
    again = forward(gpu_ctx, inp, t, masks)            # the cache does not disturb the uncached path, nor the reverse
    got2 = forward(gpu_ctx, inp, t, masks, cached=True)
    for w, g, a, g2 in zip(want, got, again, got2):
        assert torch.isfinite(w).all() and not (w == 7.0).all()
        assert torch.equal(w, g) and torch.equal(w, a) and torch.equal(w, g2)
    if masks:  # the cached mask is the prompt's: the null-mask result differs
        other = forward(gpu_ctx, inp, t, False)
        assert not torch.equal(other[0], got[0])


def test_a_second_prompt_replaces_the_first(gpu_ctx, model):
    inp1, inp2 = ref.make_inputs(2, seed=2, **NARROW), ref.make_inputs(2, seed=12, **NARROW)
    t1, t2 = tensors(inp1), tensors(inp2)
    for k in ("video_latent", "audio_latent", "video_timesteps", "audio_timesteps"):  # the same latents: only the text differs
        t2[k] = t1[k]
    prepare(gpu_ctx, t1)
    first = forward(gpu_ctx, inp1, t1, cached=True)
    prepare(gpu_ctx, t2)
    second = forward(gpu_ctx, inp1, t1, cached=True)
    want = forward(gpu_ctx, inp2, t2)
    for f, s, w in zip(first, second, want):
        assert torch.equal(s, w) and not torch.equal(s, f)


def test_cache_info_reports_shape_bytes_and_builds(gpu_ctx, model):
    model["init"]()
    assert gpu_ctx.dual_model_text_cache_info() == {"B": 0, "S": 0, "bytes": 0, "builds": 0}
    Dv, Da = NARROW["Hv"] * 128, NARROW["Ha"] * 64
    for n, (B, S) in enumerate(((1, 70), (2, 70), (2, 64), (1, 70)), start=1):
        inp = ref.make_inputs(B, seed=3, **dict(NARROW, S=S))
        prepare(gpu_ctx, tensors(inp))
        info = gpu_ctx.dual_model_text_cache_info()
        assert info == {"B": B, "S": S, "bytes": cache_bytes(L_NARROW, B, S, Dv, Da), "builds": n}, info
    torch.cuda.synchronize()


def test_a_cached_forward_without_a_matching_cache_is_refused_and_writes_nothing(gpu_ctx, ltx, model):
    model["init"]()                                    # a fresh model holds no cache
    inp = ref.make_inputs(2, seed=2, **NARROW)
    t = tensors(inp)
    out = (torch.full((2, 96, 128), 7.0, device="cuda"), torch.full((2, 26, 128), 7.0, device="cuda"))

    def refused(inp_, t_, match="text_cache", case="invalidConfiguration", **kw):
        with pytest.raises(ltx.LTXError, match=match) as e:
            forward(gpu_ctx, inp_, t_, cached=True, out=out, **kw)
        assert e.value.case == case

    refused(inp, t)                                    # never prepared
    prepare(gpu_ctx, t)
    forward(gpu_ctx, inp, t, cached=True)              # now it runs
    one = ref.make_inputs(1, seed=2, **NARROW)
    refused(one, tensors(one))                         # another B
    refused(inp, t, S=64)                              # another S
    model["init"]()                                    # init_synthetic drops the cache
    refused(inp, t)
    prepare(gpu_ctx, t)
    gpu_ctx.dual_model_unload()                        # so does unload
    refused(inp, t, match="not loaded", case="modelNotLoaded")
    with pytest.raises(ltx.LTXError, match="not loaded"):
        gpu_ctx.dual_model_text_cache_info()
    model["init"]()
    refused(inp, t)
    with pytest.raises(ltx.LTXError, match="null") as e:  # prepare itself: a NULL context, B out of range
        gpu_ctx.dual_model_prepare_text(t["video_context"], None, B=2, S=70)
    assert e.value.case == "invalidConfiguration"
    with pytest.raises(ltx.LTXError, match="B=9"):
        gpu_ctx.dual_model_prepare_text(t["video_context"], t["audio_context"], B=9, S=70)
    assert gpu_ctx.dual_model_text_cache_info()["builds"] == 0
    torch.cuda.synchronize()
    assert (out[0] == 7.0).all() and (out[1] == 7.0).all(), "a refused call wrote"


def test_full_width_cached_forward_is_bit_equal(gpu_ctx, ltx, model):
    """32 x 128 / 32 x 64, L = 1, caption_channels 3840, (F, H, W) = (1, 4, 8), T_a = 26, S = 70, B = 1: the K = 4096 / 2048 key and
    value projections at their real widths, where the GEMM launcher's choices (split-K among them) depend on the width."""
    shape = dict(Hv=32, Ha=32, F=1, H=4, W=8, T_a=26, S=70, caption_channels=3840)
    inp = ref.make_inputs(1, seed=7, **shape)
    t = tensors(inp)
    gpu_ctx.dual_model_init_synthetic(ltx.default_dual_model_config(num_layers=1), seed=52)
    try:
        want = forward(gpu_ctx, inp, t)
        prepare(gpu_ctx, t)
        got = forward(gpu_ctx, inp, t, cached=True)
        assert gpu_ctx.dual_model_text_cache_info() == {"B": 1, "S": 70, "bytes": cache_bytes(1, 1, 70, 4096, 2048), "builds": 1}
    finally:
        gpu_ctx.dual_model_unload()
        model["init"]()
    for w, g in zip(want, got):
        assert torch.isfinite(w).all() and torch.equal(w, g)
