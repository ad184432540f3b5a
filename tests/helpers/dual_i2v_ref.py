"""CPU reference of image-to-video in the joint video + audio path: the dual model with PER-TOKEN video timesteps
(LTX2Transformer.swift:285-312: the adaLN rows, both cross-modal embedders and the output head read the flattened per-token timesteps)
and the image-to-video loop of generateVideoWithAudio (LTXPipeline.swift:1261-1399), in numpy f32 on the primitives of
dual_model_ref / dual_block_ref / dual_denoise_ref.

`forward` materialises the per-token modulation - temb_video [B][T][6][Dv], cross_video_ss [B][T][5][Dv] and a per-token head - and runs
a restatement of dual_block_ref.block whose video rows are indexed per token; with one timestep for all tokens it IS
dual_model_ref.forward, bit for bit (tests/test_dual_i2v_host.py pins that). The embedders run once on the distinct (batch element,
timestep) pairs in order of first appearance and their rows are gathered per token: an embedder is a function of one timestep, and a
matrix product over 96 equal rows is not bit-equal to one over a single row on every BLAS. `replay=True` applies the library's rounding
points. `loop` is the image-to-video loop around a forward the caller supplies, in the reference's order (re-noise at the START of a
step with that step's sigma); `step_keep` is the float32 replay of the step launch's frozen prefix, which writes the same frame 0 at the
END of the step before. `mistake=` builds one deliberately WRONG variant:
  frame0_sigma       frame-0 tokens run at sigma instead of 0
  cross_per_batch    the cross-modal rows (av_ca_video_scale_shift, av_ca_a2v_gate) take one timestep per batch element - that of the
                     unconditioned tokens - while adaLN and the head are per token
  head_per_batch     the output head takes that one timestep for all tokens
  euler_frame0       frame 0 is stepped by Euler like every other frame
  renoise_sigma      re-noise with sigma instead of sigma^2
  renoise_this_sigma the step launch re-noises with ITS sigma instead of the next step's: frame 0 of step i carries sigma[i-1]^2"""
import numpy as np

import dual_block_ref as blocks
import dual_denoise_ref as dd
import dual_model_ref as model
import ltx_oracle as oracle

F32 = np.float32
MODEL_MISTAKES = ("cross_per_batch", "head_per_batch")
LOOP_MISTAKES = ("frame0_sigma", "euler_frame0", "renoise_sigma", "renoise_this_sigma")
MISTAKES = ("frame0_sigma",) + MODEL_MISTAKES + LOOP_MISTAKES[1:]
rel_l2, cosine, update_bound = model.rel_l2, model.cosine, model.update_bound


def timestep_groups(token_timesteps):
    """[B][T] -> (values [B][G], group [B][T]): the distinct timesteps of each batch element in order of first appearance; unused slots
    repeat the element's first value. The restatement tests/test_dual_i2v_host.py holds ltx.timestep_groups against."""
    tt = np.asarray(token_timesteps, F32)
    vals, grp = [], np.zeros(tt.shape, np.int32)
    for b in range(tt.shape[0]):
        v = []
        for t in range(tt.shape[1]):
            hit = [g for g, u in enumerate(v) if u == tt[b, t]]
            if not hit:
                v.append(tt[b, t])
            grp[b, t] = hit[0] if hit else len(v) - 1
        vals.append(v)
    G = max(len(v) for v in vals)
    return np.asarray([v + [v[0]] * (G - len(v)) for v in vals], F32), grp


def i2v_token_timesteps(B, F, H, W, sigma):
    """sigma * (1 - mask) (:1296-1299): frame-0 tokens 0, the rest sigma; sigma a scalar or one value per batch element."""
    tt = np.empty((B, F * H * W), F32)
    tt[:] = np.asarray(sigma, F32).reshape(-1, 1)
    tt[:, :H * W] = 0
    return tt


def embed_tokens(w, inp, mult=1000.0, mistake=None):
    """The timestep path with per-token video timesteps inp["video_token_timesteps"] [B][T]: temb_v [B][T][6][Dv], cross_v [B][T][5][Dv],
    embts_v [B][T][Dv]; the audio side as dual_model_ref.embed ([B][6][Da], [B][5][Da], [B][Da])."""
    B = inp["B"]
    tt = np.asarray(inp["video_token_timesteps"], F32)
    T = tt.shape[1]
    vals, grp = timestep_groups(tt)
    G = vals.shape[1]
    flat = dict(inp)
    flat["B"] = B * G
    flat["video_timesteps"] = vals.reshape(-1)
    flat["audio_timesteps"] = np.repeat(np.asarray(inp["audio_timesteps"], F32), G)  # unused rows; the audio side comes from `e_a`
    e_v = model.embed(w, flat, mult, F32)
    one = dict(inp)
    one["video_timesteps"] = vals[:, 0]
    e_a = model.embed(w, one, mult, F32)
    rows = grp + (np.arange(B) * G)[:, None]                       # [B][T] -> row of the [B*G] tensors
    last = np.repeat(rows[:, -1:], T, axis=1)                      # the unconditioned tokens' row, for every token
    pick = lambda t, r: t.astype(F32)[r]                            # noqa: E731  [B*G][...] -> [B][T][...]
    return {"temb_v": pick(e_v["temb_v"], rows), "cross_v": pick(e_v["cross_v"], last if mistake == "cross_per_batch" else rows),
            "embts_v": pick(e_v["embts_v"], last if mistake == "head_per_batch" else rows),
            "temb_a": e_a["temb_a"].astype(F32), "cross_a": e_a["cross_a"].astype(F32), "embts_a": e_a["embts_a"]}


def block(w, i, xv, xa, inp, tabs, replay=False, eps=1e-6):
    """dual_block_ref.block with the video modulation rows per token: inp["temb_video"] [B][T][6][Dv], inp["cross_video_ss"] [B][T][5][Dv]."""
    p = f"transformer_blocks.{i}."
    Hv, Ha = inp["Hv"], inp["Ha"]
    one = F32(1)
    norm = lambda x: oracle.rms_norm(x, None, eps)  # noqa: E731
    mv = w[p + "scale_shift_table"][None, None].astype(F32) + inp["temb_video"]                   # [B][T][6][Dv]
    ma = w[p + "audio_scale_shift_table"][None].astype(F32) + inp["temb_audio"]                   # [B][6][Da]
    cv = w[p + "scale_shift_table_a2v_ca_video"][None, None].astype(F32) + inp["cross_video_ss"]  # [B][T][5][Dv]
    ca = w[p + "scale_shift_table_a2v_ca_audio"][None].astype(F32) + inp["cross_audio_ss"]
    tok = lambda t, r: t[:, :, r]               # noqa: E731
    row = lambda t, r: t[:, r][:, None, :]      # noqa: E731
    att, ff = blocks.attention, blocks.feed_forward
    n = norm(xv) * (one + tok(mv, 1)) + tok(mv, 0)
    xv = xv + att(w, p + "attn1.", n, Hv, 128, q_tables=tabs["video"], replay=replay, eps=eps) * tok(mv, 2)
    n = norm(xa) * (one + row(ma, 1)) + row(ma, 0)
    xa = xa + att(w, p + "audio_attn1.", n, Ha, 64, q_tables=tabs["audio"], replay=replay, eps=eps) * row(ma, 2)
    xv = xv + att(w, p + "attn2.", norm(xv), Hv, 128, context=inp["context_video"], bias=inp["bias_video"], kv_bf16=True, replay=replay, eps=eps)
    xa = xa + att(w, p + "audio_attn2.", norm(xa), Ha, 64, context=inp["context_audio"], bias=inp["bias_audio"], kv_bf16=True, replay=replay, eps=eps)
    nv, na = norm(xv), norm(xa)
    q = nv * (one + tok(cv, 0)) + tok(cv, 1)
    c = na * (one + row(ca, 0)) + row(ca, 1)
    xv = xv + att(w, p + "audio_to_video_attn.", q, Ha, 64, context=c, q_tables=tabs["cross_video"], k_tables=tabs["cross_audio"], replay=replay,
                  eps=eps) * tok(cv, 4)
    q = na * (one + row(ca, 2)) + row(ca, 3)
    c = nv * (one + tok(cv, 2)) + tok(cv, 3)
    xa = xa + att(w, p + "video_to_audio_attn.", q, Ha, 64, context=c, q_tables=tabs["cross_audio"], k_tables=tabs["cross_video"], replay=replay,
                  eps=eps) * row(ca, 4)
    n = norm(xv) * (one + tok(mv, 4)) + tok(mv, 3)
    xv = xv + ff(w, p + "ff.", n, replay) * tok(mv, 5)
    n = norm(xa) * (one + row(ma, 4)) + row(ma, 3)
    xa = xa + ff(w, p + "audio_ff.", n, replay) * row(ma, 5)
    return xv.astype(F32), xa.astype(F32)


def head_tokens(w, x, table, embts, proj, replay=False, eps=1e-6):
    """dual_model_ref.head with embedded timesteps per token: embts [B][T][D]."""
    ss = w[table][None, None].astype(F32) + embts[:, :, None, :].astype(F32)  # [B][T][2][D]
    shift, scale = ss[:, :, 0], ss[:, :, 1]
    n = oracle.layer_norm(x, eps) * (F32(1) + scale) + shift
    if replay:
        n = oracle.bf16_round(n.astype(F32))
    return oracle.linear(n.astype(F32), w[proj + ".weight"], w[proj + ".bias"])


def forward(w, L, inp, tabs=None, replay=False, mistake=None, mult=1000.0, eps=1e-6):
    """dual_model_ref.forward with inp["video_token_timesteps"] [B][T] in place of inp["video_timesteps"]."""
    assert mistake is None or mistake in MODEL_MISTAKES, mistake
    Hv, Ha = inp["Hv"], inp["Ha"]
    if tabs is None:
        tabs = blocks.tables(None, inp["F"], inp["H"], inp["W"], inp["T_a"], Hv, Ha)
    xv = oracle.linear(inp["video_latent"], w["patchify_proj.weight"], w["patchify_proj.bias"])
    xa = oracle.linear(inp["audio_latent"], w["audio_patchify_proj.weight"], w["audio_patchify_proj.bias"])
    if replay:
        xv, xa = oracle.bf16_round(xv), oracle.bf16_round(xa)
    e = embed_tokens(w, inp, mult, mistake)
    pv = model.caption_projection(w, "caption_projection", inp["video_context"], replay)
    pa = model.caption_projection(w, "audio_caption_projection", inp["audio_context"], replay)
    b = dict(inp)
    b.update(context_video=pv, context_audio=pa, bias_video=oracle.mask_to_bias(inp["video_mask"]), bias_audio=oracle.mask_to_bias(inp["audio_mask"]),
             temb_video=e["temb_v"], temb_audio=e["temb_a"], cross_video_ss=e["cross_v"], cross_audio_ss=e["cross_a"])
    for i in range(L):
        xv, xa = block(w, i, xv, xa, b, tabs, replay=replay, eps=eps)
    vv = head_tokens(w, xv, "scale_shift_table", e["embts_v"], "proj_out", replay, eps)
    va = model.head(w, xa, "audio_scale_shift_table", e["embts_a"], "audio_proj_out", False, replay, eps)
    return vv.astype(F32), va.astype(F32)


def ref_forward(w, L, replay=False, mistake=None):
    """A forward for `loop` from the numpy model."""
    tabs = {}

    def fwd(inp):
        key = (inp["F"], inp["H"], inp["W"], inp["T_a"])
        if key not in tabs:
            tabs[key] = blocks.tables(None, inp["F"], inp["H"], inp["W"], inp["T_a"], inp["Hv"], inp["Ha"])
        return forward(w, L, inp, tabs[key], replay=replay, mistake=mistake)
    return fwd


def noised(cond, noise, scale, sigma2):
    """cond + (scale * noise) * sigma2, three f32 array ops (:1292); sigma2 is the f32 product the caller made."""
    a = (F32(scale) * noise).astype(F32)
    b = (a * F32(sigma2)).astype(F32)
    return (cond + b).astype(F32)


def step_keep(x, v_cond, v_uncond, cfg_scale, form, sigma, sigma_next, n_keep=0, keep_src=None, keep_noise=None, keep_scale=0.0):
    """The float32 replay of one job of the step launch with a frozen prefix (csrc/elementwise.h, DualStepJob): (x', guided velocity,
    bf16 bit patterns of x'). Elements i < n_keep: x' = keep_src + (keep_scale * keep_noise) * (sigma_next * sigma_next), or x without
    noise; the velocity is the whole job's."""
    y, v, _ = dd.step(x, v_cond, v_uncond, cfg_scale, form, sigma, sigma_next)
    x = np.asarray(x, F32)
    if n_keep:
        y = y.copy()
        y[:n_keep] = x[:n_keep]
        if keep_noise is not None:
            sn2 = F32(F32(sigma_next) * F32(sigma_next))
            y[:n_keep] = noised(np.asarray(keep_src, F32)[:n_keep], np.asarray(keep_noise, F32)[:n_keep], keep_scale, sn2)
    return y, v, oracle.f32_to_bf16_bits(y)


def make_cond(case, steps, seed=7):
    """The image latent [C][1][H][W] (N(0, 1), as an encoded image is normalised) and the caller's re-noising draws [steps][C][1][H][W]."""
    rng = np.random.default_rng(seed)
    C, H, W = case["video_latent"].shape[0], case["H"], case["W"]
    return rng.standard_normal((C, 1, H, W)).astype(F32), rng.standard_normal((steps, C, 1, H, W)).astype(F32)


def loop(forward_fn, case, sigmas, cond, noise=None, noise_scale=0.0, cfg_scale=1.0, rescale=0.0, mistake=None, var_dtype=np.float64):
    """The image-to-video loop of LTXPipeline.swift:1261-1399 around `forward_fn`, in the caller's layouts: video latent [C][F][H][W] with
    frame 0 set to `cond` (:1264), per step the re-noising of frame 0 (:1289-1294), per-token timesteps sigma * (1 - mask) (:1296-1299),
    the forward (B = 2 on duplicated tokens with CFG), CFG / rescale as dual_denoise_ref.loop, Euler on frames 1 .. only (:1383-1393) and
    the audio line. Returns (video latent, audio latent)."""
    assert mistake is None or mistake in LOOP_MISTAKES, mistake
    use_cfg = cfg_scale > 1.0
    B = 2 if use_cfg else 1
    assert case["nb"] == B and case["F"] >= 2
    F, H, W = case["F"], case["H"], case["W"]
    lat = np.array(case["video_latent"], F32)            # [C][F][H][W]
    lat[:, 0:1] = cond
    xa = dd.pack_audio(case["audio_latent"])
    cv = case["video_context"]
    ca = case["audio_context"] if case["audio_context"] is not None else cv
    mask = case["mask"] if case["mask"] is not None else np.ones((B, case["S"]), np.int32)
    renoise = noise is not None and noise_scale > 0
    for i in range(len(sigmas) - 1):
        sigma, sigma_next = F32(sigmas[i]), F32(sigmas[i + 1])
        if renoise and sigma > 0:
            s_used = F32(sigmas[i - 1]) if (mistake == "renoise_this_sigma" and i > 0) else sigma
            factor = s_used if mistake == "renoise_sigma" else F32(s_used * s_used)
            lat[:, 0:1] = noised(cond, noise[i], noise_scale, factor)
        xv = dd.pack_video(lat)
        inp = {k: case[k] for k in ("Hv", "Ha", "F", "H", "W", "T_a", "S")}
        inp["B"] = B
        inp["video_latent"] = np.repeat(oracle.bf16_round(xv)[None], B, axis=0)
        inp["audio_latent"] = np.repeat(oracle.bf16_round(xa)[None], B, axis=0)
        inp["video_context"], inp["audio_context"] = cv, ca
        inp["sigma"] = sigma
        inp["video_token_timesteps"] = np.full((B, F * H * W), sigma, F32) if mistake == "frame0_sigma" else i2v_token_timesteps(B, F, H, W, sigma)
        inp["audio_timesteps"] = np.full(B, sigma, F32)
        inp["video_mask"] = inp["audio_mask"] = mask
        inp["null_mask"] = case["mask"] is None
        vv, va = forward_fn(inp)
        vv, va = np.asarray(vv, F32), np.asarray(va, F32)
        v_v = dd.cfg(vv[1], vv[0], cfg_scale) if use_cfg else vv[0]   # batch order [negative, positive]
        v_a = dd.cfg(va[1], va[0], cfg_scale) if use_cfg else va[0]
        if rescale > 0:
            v_v = dd.guidance_rescale(v_v, vv[B - 1], rescale, var_dtype)
        stepped = dd.euler(xv, v_v, 0, sigma, sigma_next)
        if mistake != "euler_frame0":
            stepped[:H * W] = xv[:H * W]                                # frame 0 is the first H*W tokens
        lat = dd.unpack_video(stepped, F, H, W)
        xa = dd.euler(xa, v_a, 1, sigma, sigma_next)
    return lat, dd.unpack_audio(xa)
