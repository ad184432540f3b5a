"""CPU reference of the joint video + audio denoise loop (generateVideoWithAudio, LTXPipeline.swift:1276-1417) and of the one launch
between two forwards (dual_step_kernel, csrc/elementwise.hip).

`step` is the numpy float32 replay of the step: every operation is one numpy array op on float32, so every operation is rounded on its
own, as the reference's separate MLX array ops are. `loop` is the loop around a forward that the caller supplies: `ref_forward` builds
one from tests/helpers/dual_model_ref.py (the f32 reference, or with replay=True the library's rounding points); the GPU tests pass the
library's own uncached forward instead and get the composition the loop must equal bit for bit. `mistake=` builds one deliberately WRONG
loop, which tests/test_dual_denoise_host.py uses to show that the GPU tests' inputs make each piece visible."""
import numpy as np

import dual_model_ref as model
import ltx_oracle as oracle

F32 = np.float32
MISTAKES = ("cfg_order", "rescale_audio", "audio_context_zeros", "mask_one_stream")
# (sigma, sigma_next) pairs of the step tests: the two Euler forms differ in 27-34 % of their f32 results for N(0, 1) operands (n = 4096)
SIGMA_PAIRS = ((1.0, 0.99375), (0.909375, 0.725), (0.6, 0.25))
rel_l2, update_bound = model.rel_l2, model.update_bound


def cfg(v_cond, v_uncond, cfg_scale):
    """applyCFG (LatentUtils.swift:131-141): cond + (scale - 1) * (cond - uncond), three f32 ops."""
    if v_uncond is None:
        return v_cond.astype(F32)
    sm1 = F32(F32(cfg_scale) - F32(1.0))
    d = (v_cond - v_uncond).astype(F32)
    g = (sm1 * d).astype(F32)
    return (v_cond + g).astype(F32)


def euler(x, v, form, sigma, sigma_next):
    """form 0: LTXScheduler.step (LTXScheduler.swift:305-327); form 1: the audio line (LTXPipeline.swift:1402). f32 op by f32 op."""
    s, sn = F32(sigma), F32(sigma_next)
    if form == 0:
        sv = (s * v).astype(F32)
        den = (x - sv).astype(F32)
        if not sn > 0:
            return den
        back = (x - den).astype(F32)
        num = (sn * back).astype(F32)
        q = (num / s).astype(F32)
        return (den + q).astype(F32)
    ds = F32(sn - s)
    dv = (ds * v).astype(F32)
    return (x + dv).astype(F32)


def step(x, v_cond, v_uncond, cfg_scale, form, sigma, sigma_next):
    """(x', guided velocity, bf16 bit patterns of x') of one job of the step."""
    x, v_cond = np.asarray(x, F32), np.asarray(v_cond, F32)
    v = cfg(v_cond, None if v_uncond is None else np.asarray(v_uncond, F32), cfg_scale)
    y = euler(x, v, form, sigma, sigma_next)
    return y, v, oracle.f32_to_bf16_bits(y)


def guidance_rescale(v, cond, phi, var_dtype=np.float64):
    """applyGuidanceRescale (LatentUtils.swift:164-183) over the whole tensor (B = 1): the two variances in `var_dtype`, the rest f32."""
    eps = F32(1e-8)
    cfg_std = np.sqrt(F32(np.var(v.astype(var_dtype))) + eps, dtype=F32)
    cond_std = np.sqrt(F32(np.var(cond.astype(var_dtype))) + eps, dtype=F32)
    rescaled = (v * F32(cond_std / cfg_std)).astype(F32)
    return (F32(phi) * rescaled + F32(F32(1.0) - F32(phi)) * v).astype(F32)


def pack_video(latent):
    """[C][F][H][W] -> tokens [F*H*W][C] (patchify, LatentUtils.swift:20-34)."""
    C = latent.shape[0]
    return np.ascontiguousarray(latent.reshape(C, -1).T)


def unpack_video(tokens, F, H, W):
    return np.ascontiguousarray(tokens.T).reshape(tokens.shape[1], F, H, W)


def pack_audio(latent):
    """(8, T_a, 16) -> (T_a, 128) (packAudioLatents, LTXPipeline.swift:540-544)."""
    return np.ascontiguousarray(latent.transpose(1, 0, 2).reshape(latent.shape[1], -1))


def unpack_audio(tokens):
    return np.ascontiguousarray(tokens.reshape(tokens.shape[0], 8, 16).transpose(1, 0, 2))


def make_case(Hv, Ha, F, H, W, T_a, S, caption_channels, cfg, seed=0, audio_context=False, masked=True):
    """Inputs of one loop: N(0, 1) latents in the caller's layouts, bf16 contexts of scale 4 ([negative, positive] with cfg), an int32
    mask with a third of the keys masked, differently per batch element."""
    rng = np.random.default_rng(seed)
    nb = 2 if cfg else 1
    c = {"Hv": Hv, "Ha": Ha, "F": F, "H": H, "W": W, "T_a": T_a, "S": S, "nb": nb}
    c["video_latent"] = rng.standard_normal((128, F, H, W)).astype(F32)
    c["audio_latent"] = rng.standard_normal((8, T_a, 16)).astype(F32)
    c["video_context"] = oracle.bf16_round((4.0 * rng.standard_normal((nb, S, caption_channels))).astype(F32))
    c["audio_context"] = oracle.bf16_round((4.0 * rng.standard_normal((nb, S, caption_channels))).astype(F32)) if audio_context else None
    m = (rng.random((nb, S)) >= 1.0 / 3.0).astype(np.int32)
    m[:, 0] = 1
    c["mask"] = m if masked else None
    return c


def ref_forward(w, L, replay=False):
    """A forward for `loop` from the numpy model: (inp dict of dual_model_ref.forward) -> (video velocity, audio velocity)."""
    tabs = {}

    def fwd(inp):
        key = (inp["F"], inp["H"], inp["W"], inp["T_a"])
        if key not in tabs:
            tabs[key] = model.blocks.tables(None, inp["F"], inp["H"], inp["W"], inp["T_a"], inp["Hv"], inp["Ha"])
        return model.forward(w, L, inp, tabs[key], replay=replay)
    return fwd


def loop(forward, case, sigmas, cfg_scale=1.0, rescale=0.0, mistake=None, var_dtype=np.float64, on_step=None):
    """The loop of LTXPipeline.swift:1276-1417 around `forward`. Returns (video latent [C][F][H][W], audio latent [8][T_a][16], stats
    [steps][8]: mean and std of the video velocity, the video latent, the audio velocity, the audio latent)."""
    assert mistake is None or mistake in MISTAKES, mistake
    use_cfg = cfg_scale > 1.0
    B = 2 if use_cfg else 1
    assert case["nb"] == B
    xv, xa = pack_video(case["video_latent"]), pack_audio(case["audio_latent"])
    cv = case["video_context"]
    ca = case["audio_context"] if case["audio_context"] is not None else cv  # audioEncoding ?? videoEncoding
    if mistake == "audio_context_zeros" and case["audio_context"] is None:
        ca = np.zeros_like(cv)
    mask = case["mask"] if case["mask"] is not None else np.ones((B, case["S"]), np.int32)  # a null mask is an all-ones mask
    amask = np.ones_like(mask) if mistake == "mask_one_stream" else mask
    stats = []
    for i in range(len(sigmas) - 1):
        sigma, sigma_next = F32(sigmas[i]), F32(sigmas[i + 1])
        if on_step:
            on_step(i, float(sigma))
        inp = {k: case[k] for k in ("Hv", "Ha", "F", "H", "W", "T_a", "S")}
        inp["B"] = B
        inp["video_latent"] = np.repeat(oracle.bf16_round(xv)[None], B, axis=0)   # patchify(...).asType(.bfloat16), :1306-1307
        inp["audio_latent"] = np.repeat(oracle.bf16_round(xa)[None], B, axis=0)
        inp["video_context"], inp["audio_context"] = cv, ca
        inp["video_timesteps"] = inp["audio_timesteps"] = np.full(B, sigma, F32)
        inp["video_mask"], inp["audio_mask"] = mask, amask
        inp["null_mask"] = case["mask"] is None  # for a forward that can take a null mask as such
        vv, va = forward(inp)
        vv, va = np.asarray(vv, F32), np.asarray(va, F32)
        neg, pos = (1, 0) if mistake == "cfg_order" else (0, 1)  # batch order [negative, positive]
        v_v = cfg(vv[pos], vv[neg], cfg_scale) if use_cfg else vv[0]
        v_a = cfg(va[pos], va[neg], cfg_scale) if use_cfg else va[0]
        if rescale > 0:  # the video velocity only (:1352-1359)
            v_v = guidance_rescale(v_v, vv[pos], rescale, var_dtype)
            if mistake == "rescale_audio":
                v_a = guidance_rescale(v_a, va[pos], rescale, var_dtype)
        xv = euler(xv, v_v, 0, sigma, sigma_next)
        xa = euler(xa, v_a, 1, sigma, sigma_next)
        stats.append([f(t.astype(np.float64)) for t in (v_v, xv, v_a, xa) for f in (np.mean, np.std)])
    return unpack_video(xv, case["F"], case["H"], case["W"]), unpack_audio(xa), np.asarray(stats, np.float64)
