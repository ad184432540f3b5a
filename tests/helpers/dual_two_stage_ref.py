"""CPU reference of the two-stage video + audio path (generateVideoWithAudioTwoStage, LTXPipeline.swift:1613-1817) and of the one launch
between its stages (dual_restage_kernel, csrc/elementwise.hip), in numpy f32 on the primitives of dual_denoise_ref / dual_i2v_ref.

`restage_video` / `restage_audio` are the numpy float32 replay of the restage launch: every operation is one numpy array op on float32,
so every operation is rounded on its own, as the reference's separate MLX array ops are (numpy's float32 sqrt and division are correctly
rounded). `stage` is one denoise loop in the reference's order (frame 0 re-noised at the START of a step) with the video's Euler form a
parameter: stage 1 steps the video with LTXScheduler.step (form 0), stage 2 with x + dt * v (form 1, :1799-1811); the audio is form 1 in
both. `two_stage` chains stage 1, the upscaler, AdaIN, the re-noise, frame 0 and stage 2 around a forward and an upscaler the caller
supplies: the numpy model and oracle.upsample_latents give the f32 reference, the library's own forward and upscaler give what the GPU
tests compose. `mistake=` builds one deliberately WRONG bridge:
  adain_skipped        the upscaled latent is re-noised as it is
  adain_swapped        the two sets of statistics exchanged: normalised by the reference's, rescaled to the latent's own
  scales_swapped       (1 - s) * noise + s * y
  audio_not_renoised   the audio latent enters stage 2 as stage 1 left it
  audio_noise_planes   the packed audio noise [T_a][128] read as [8][T_a][16] and packed
  frame0_first         frame 0 set to the image latent BEFORE the re-noise, which then blends noise into it
  cond_naive           the stage-1 image latent, each pixel repeated 2 x 2, in place of the stage-2 image latent"""
import numpy as np

import dual_denoise_ref as dd
import dual_i2v_ref as iv
import dual_model_ref as model
import ltx_oracle as oracle

F32 = np.float32
MISTAKES = ("adain_skipped", "adain_swapped", "scales_swapped", "audio_not_renoised", "audio_noise_planes", "frame0_first", "cond_naive")
rel_l2, update_bound = model.rel_l2, model.update_bound

# the setting the GPU parity test and the CPU visibility test share: the narrow boosted model of the dual tests, stage 1 at (2, 3, 4),
# stage 2 at (2, 6, 8), image-to-video with re-noising at scale 0.5 in both stages, distilled schedules
NARROW = dict(Hv=4, Ha=4, F=2, H=3, W=4, T_a=26, S=70, caption_channels=256)
L_NARROW = 2
SIGMAS1 = [1.0, 0.725, 0.25, 0.0]
SIGMAS2 = [0.909375, 0.725, 0.421875, 0.0]  # STAGE_2_DISTILLED_SIGMA_VALUES = ltx_stage2_sigmas
NOISE_SCALE = 0.5
UPSCALER_MID, UPSCALER_SEED = 64, 4
UPSCALER_BOUND, TWO_STAGE_CAP = 3e-2, 5e-2  # the project's bounds on the upscaled latent and on a two-stage latent (tests/test_two_stage_gpu.py)


def vae_stats():
    """The per-channel statistics of tests/test_two_stage_gpu.py's vae_stats_ctx."""
    rng = np.random.default_rng(0)
    return (0.2 * rng.standard_normal(128)).astype(F32), (1.0 + 0.3 * rng.random(128)).astype(F32)


def parity_bound(replay, e_up, y, z0, s):
    """The bound of the parity test: 2 x (the rounding-point replay + the upscaler's own error as it enters stage 2), capped. The
    upscaled latent enters the stage-2 start latent z0 = s * noise + (1 - s) * y scaled by (1 - s) * |y| / |z0|."""
    allowance = float(e_up) * float(F32(1.0) - F32(s)) * float(np.linalg.norm(y) / np.linalg.norm(z0))
    return min(2.0 * (float(replay) + allowance), TWO_STAGE_CAP), allowance


def adain_ops(x, stats, stats_ref):
    """AdaIN at factor 1 (LatentUtils.swift:201-227) on x [C][T] from {mean, variance} pairs [C][2], f32 op by f32 op."""
    x = np.asarray(x, F32)
    st, sr = np.asarray(stats, F32), np.asarray(stats_ref, F32)
    mu, sd = st[:, 0:1], np.sqrt(st[:, 1:2], dtype=F32)
    mur, sdr = sr[:, 0:1], np.sqrt(sr[:, 1:2], dtype=F32)
    d = (x - mu).astype(F32)
    den = (sd + F32(1e-8)).astype(F32)
    q = (d / den).astype(F32)
    m = (q * sdr).astype(F32)
    return (m + mur).astype(F32)


def blend(noise, y, s):
    """s * noise + (1.0f - s) * y (:1730-1731): 1 - s is one f32 scalar, then two multiplies and one add."""
    s = F32(s)
    r = F32(F32(1.0) - s)
    a = (s * np.asarray(noise, F32)).astype(F32)
    b = (r * np.asarray(y, F32)).astype(F32)
    return (a + b).astype(F32)


def restage_video(x, stats, stats_ref, noise=None, s=0.0, cond=None, cond_noise=None, cond_scale=0.0, cond_sigma2=0.0):
    """The video job: x, noise [C][T]; cond, cond_noise [C][HW]. Returns (latent [T][C] f32, its bf16 bit patterns)."""
    y = adain_ops(x, stats, stats_ref)
    if noise is not None:
        y = blend(noise, y, s)
    if cond is not None:
        HW = cond.shape[1]
        y[:, :HW] = cond if cond_noise is None else iv.noised(np.asarray(cond, F32), np.asarray(cond_noise, F32), cond_scale, F32(cond_sigma2))
    lat = np.ascontiguousarray(y.T)
    return lat, oracle.f32_to_bf16_bits(lat)


def restage_audio(x, noise=None, s=0.0):
    """The audio job on the packed latent [T_a][128]."""
    y = np.asarray(x, F32) if noise is None else blend(noise, x, s)
    return y, oracle.f32_to_bf16_bits(y)


def mean_var(x):
    """{mean, population variance} per channel of x [C][T] -> [C][2] f32, in float64 as the oracle's AdaIN takes them."""
    x64 = np.asarray(x).reshape(x.shape[0], -1).astype(np.float64)
    return np.stack([x64.mean(1), x64.var(1)], axis=1).astype(F32)


def stage(forward_fn, dims, lat, xa, ctx, sigmas, video_form, cond=None, noise=None, noise_scale=0.0, on_step=None):
    """One loop: lat [C][F][H][W], xa packed [T_a][128]; dims = dict(Hv, Ha, F, H, W, T_a, S); ctx = dict(video_context, audio_context,
    mask). Returns (lat, xa)."""
    F, H, W = dims["F"], dims["H"], dims["W"]
    lat = np.array(lat, F32)
    cv = ctx["video_context"]
    ca = ctx["audio_context"] if ctx["audio_context"] is not None else cv
    mask = ctx["mask"] if ctx["mask"] is not None else np.ones((1, dims["S"]), np.int32)
    renoise = cond is not None and noise is not None and noise_scale > 0
    for i in range(len(sigmas) - 1):
        sigma, sigma_next = F32(sigmas[i]), F32(sigmas[i + 1])
        if on_step:
            on_step(i, float(sigma))
        if renoise and sigma > 0:
            lat[:, 0:1] = iv.noised(cond, noise[i], noise_scale, F32(sigma * sigma))
        xv = dd.pack_video(lat)
        inp = dict(dims)
        inp["B"] = 1
        inp["video_latent"], inp["audio_latent"] = oracle.bf16_round(xv)[None], oracle.bf16_round(xa)[None]
        inp["video_context"], inp["audio_context"] = cv, ca
        inp["sigma"], inp["i2v"] = sigma, cond is not None
        inp["video_timesteps"] = inp["audio_timesteps"] = np.full(1, sigma, F32)
        inp["video_token_timesteps"] = iv.i2v_token_timesteps(1, F, H, W, sigma) if cond is not None else np.full((1, F * H * W), sigma, F32)
        inp["video_mask"] = inp["audio_mask"] = mask
        inp["null_mask"] = ctx["mask"] is None
        vv, va = forward_fn(inp)
        stepped = dd.euler(xv, np.asarray(vv, F32)[0], video_form, sigma, sigma_next)
        if cond is not None:
            stepped[:H * W] = xv[:H * W]
        lat = dd.unpack_video(stepped, F, H, W)
        xa = dd.euler(xa, np.asarray(va, F32)[0], 1, sigma, sigma_next)
    return lat, xa


def make_case(Hv, Ha, F, H, W, T_a, S, caption_channels, steps1, steps2, seed=1):
    """Inputs of one two-stage run, in the reference's order of drawing after the stage-1 case of dual_denoise_ref.make_case: the image
    latents at both resolutions, the per-step frame-0 draws of both stages, the stage-2 video noise and the PACKED audio noise."""
    c = dd.make_case(Hv=Hv, Ha=Ha, F=F, H=H, W=W, T_a=T_a, S=S, caption_channels=caption_channels, cfg=False, seed=seed)
    rng = np.random.default_rng(seed + 100)
    c["cond1"] = rng.standard_normal((128, 1, H, W)).astype(F32)
    c["cond2"] = rng.standard_normal((128, 1, 2 * H, 2 * W)).astype(F32)
    c["cnoise1"] = rng.standard_normal((steps1, 128, 1, H, W)).astype(F32)
    c["cnoise2"] = rng.standard_normal((steps2, 128, 1, 2 * H, 2 * W)).astype(F32)
    c["video_noise2"] = rng.standard_normal((128, F, 2 * H, 2 * W)).astype(F32)
    c["audio_noise2"] = rng.standard_normal((T_a, 128)).astype(F32)
    return c


def stage1(forward_fn, case, sigmas1, i2v=False, renoise=False, noise_scale=0.0, on_step=None):
    """Stage 1 (:1613-1685): (video latent [C][F][H][W], packed audio latent)."""
    dims = {k: case[k] for k in ("Hv", "Ha", "F", "H", "W", "T_a", "S")}
    lat = np.array(case["video_latent"], F32)
    if i2v:
        lat[:, 0:1] = case["cond1"]
    return stage(forward_fn, dims, lat, dd.pack_audio(case["audio_latent"]), case, sigmas1, 0, case["cond1"] if i2v else None,
                 case["cnoise1"] if renoise else None, noise_scale, on_step)


def bridge(case, lat1, xa, upscale_fn, s, i2v=False, mistake=None):
    """:1688-1752: (stage-2 start latent [C][F][2H][2W] before step 0's re-noise, packed audio latent, the AdaIN output)."""
    assert mistake is None or mistake in MISTAKES, mistake
    up = np.asarray(upscale_fn(lat1[None]), F32)
    if mistake == "adain_skipped":
        y = up[0]
    elif mistake == "adain_swapped":
        C = up.shape[1]
        y = adain_ops(up[0].reshape(C, -1), mean_var(lat1), mean_var(up[0])).reshape(up[0].shape)
    else:
        y = oracle.adain_filter_latent(up, lat1[None])[0]
    z = blend(y, case["video_noise2"], s) if mistake == "scales_swapped" else None
    cond2 = np.repeat(np.repeat(case["cond1"], 2, axis=2), 2, axis=3) if mistake == "cond_naive" else case["cond2"]
    if z is None:
        src = np.array(y, F32)
        if i2v and mistake == "frame0_first":
            src[:, 0:1] = cond2
        z = blend(case["video_noise2"], src, s)
    an = case["audio_noise2"]
    if mistake == "audio_noise_planes":
        an = dd.pack_audio(an.reshape(8, -1, 16))
    xa2 = np.asarray(xa, F32) if mistake == "audio_not_renoised" else blend(an, xa, s)
    if i2v and mistake != "frame0_first":
        z[:, 0:1] = cond2
    return z, xa2, y, cond2


def two_stage(forward_fn, case, sigmas1, sigmas2, upscale_fn, i2v=False, renoise=False, noise_scale=0.0, mistake=None, video_form2=1,
              renoise2=None, first=None, on_step=None):
    """Both stages. Returns dict(video [C][F][2H][2W], audio [8][T_a][16], stage1 [C][F][H][W], y the AdaIN output, z0 the stage-2 start
    latent). `first` is a stage1() result to reuse; `renoise2` overrides `renoise` for stage 2."""
    steps1 = len(sigmas1) - 1
    lat1, xa = first if first is not None else stage1(forward_fn, case, sigmas1, i2v, renoise, noise_scale, on_step)
    s = F32(sigmas2[0])
    z, xa2, y, cond2 = bridge(case, lat1, xa, upscale_fn, s, i2v, mistake)
    dims = {k: case[k] for k in ("Hv", "Ha", "F", "T_a", "S")}
    dims["H"], dims["W"] = 2 * case["H"], 2 * case["W"]
    rn2 = renoise if renoise2 is None else renoise2
    step2 = (lambda i, sig: on_step(steps1 + i, sig)) if on_step else None
    v, a = stage(forward_fn, dims, z, xa2, case, sigmas2, video_form2, cond2 if i2v else None, case["cnoise2"] if rn2 else None, noise_scale, step2)
    return {"video": v, "audio": dd.unpack_audio(a), "stage1": lat1, "xa1": xa, "y": y, "z0": z}
