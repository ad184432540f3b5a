// dual_denoise.cpp - see dual_denoise.h.
#include "dual_denoise.h"

#include <math.h>

#include <algorithm>

#include "dual_model.h"
#include "elementwise.h"

namespace {
constexpr int kAudioChannels = 8, kAudioMelBins = 16;  // audioLatentChannels x audioLatentMelBins = the 128 audio token channels

// (8, T_a, 16) <-> (T_a, 128): token t holds channel c's 16 bins at columns 16 c .. (packAudioLatents / unpackAudioLatents)
void pack_audio(float* planes, float* tokens, int Ta, bool unpack, hipStream_t st) {
    const size_t row = kAudioMelBins * 4, tok_row = (size_t)kAudioChannels * kAudioMelBins * 4;
    for (int c = 0; c < kAudioChannels; ++c) {
        float* pl = planes + (size_t)c * Ta * kAudioMelBins;
        float* tk = tokens + c * kAudioMelBins;
        if (unpack)
            HIP_CHECK(hipMemcpy2DAsync(pl, row, tk, tok_row, row, Ta, hipMemcpyDeviceToDevice, st));
        else
            HIP_CHECK(hipMemcpy2DAsync(tk, tok_row, pl, row, row, Ta, hipMemcpyDeviceToDevice, st));
    }
}

// What a run derives from its parameters, and where its pieces lie in ctx->dual_dn. The offsets depend on the reserve_* fields and on
// B, T_a and whether the run is image-to-video - not on the run's own Tv or step count once those are within the reserve.
struct Plan {
    bool use_cfg = false, i2v = false, renoise = false;
    int steps = 0, C = 0, Ca = 0, Tv = 0, Ta = 0, B = 1, HW = 0, G = 1, n_noise = 0;
    long nv = 0, na = 0, nk = 0;
    size_t o_xv = 0, o_xa = 0, o_vv = 0, o_va = 0, o_vg = 0, o_tv = 0, o_ta = 0, o_ts = 0, o_rs = 0, o_ss = 0, o_map = 0, o_kc = 0, o_kn = 0, bytes = 0;
};

Plan make_plan(const DualModel* m, const DualDenoiseParams& p) {
    Plan q;
    q.use_cfg = p.cfg_scale > 1.0f;
    q.steps = p.n_sigmas - 1;
    q.C = m->cfg.in_channels;
    q.Ca = kAudioChannels * kAudioMelBins;
    q.Tv = p.F * p.H * p.W; q.Ta = p.T_a; q.B = q.use_cfg ? 2 : 1;
    q.nv = (long)q.Tv * q.C; q.na = (long)q.Ta * q.Ca;
    q.i2v = p.cond_latent != nullptr;
    q.HW = p.H * p.W; q.G = q.i2v ? 2 : 1;      // timestep groups per batch element: 0 = sigma, 1 = frame-0 tokens at 0
    q.nk = q.i2v ? (long)q.HW * q.C : 0;        // frame 0 in token layout: the first H*W*C elements
    q.renoise = q.i2v && p.image_cond_noise_scale > 0.f && p.cond_noise;
    q.n_noise = q.renoise ? q.steps - 1 : 0;    // slices of steps 1 ..; step 0's is applied at entry in the caller's layout
    // one allocation, carved: [xv][xa][vel_v B][vel_a B][guided v][tok_v B][tok_a B][ts 4][rescale stats 4][step stats 8 steps]
    const long Tv_c = std::max<long>(q.Tv, p.reserve_Tv), nv_c = Tv_c * q.C;
    const int steps_c = std::max(q.steps, p.reserve_steps), B = q.B;
    const bool renoise_c = q.renoise || (q.i2v && p.reserve_renoise);
    const long nk_c = q.i2v ? nv_c / p.F : 0;
    size_t off = 0;
    auto carve = [&](size_t bytes) {
        const size_t at = off;
        off = (off + bytes + 255) & ~(size_t)255;
        return at;
    };
    q.o_xv = carve(nv_c * 4); q.o_xa = carve(q.na * 4); q.o_vv = carve(B * nv_c * 4); q.o_va = carve(B * q.na * 4); q.o_vg = carve(nv_c * 4);
    q.o_tv = carve(B * nv_c * 2); q.o_ta = carve(B * q.na * 2); q.o_ts = carve(32); q.o_rs = carve(16); q.o_ss = carve((size_t)steps_c * 32);
    q.o_map = carve(q.i2v ? (size_t)B * Tv_c * 4 : 0); q.o_kc = carve(renoise_c ? nk_c * 4 : 0);
    q.o_kn = carve(renoise_c ? (size_t)(steps_c - 1) * nk_c * 4 : 0);
    q.bytes = off;
    return q;
}
}  // namespace

void dual_denoise_check(ltx_ctx* ctx, const DualDenoiseParams& p) {
    DualModel* m = ctx->dual_model;
    if (!m) LTX_THROW(LTXS_MODEL_NOT_LOADED, "Model not loaded: dual transformer model not loaded");
    // every check comes before the first launch, the forward's and the step's included
    LTX_REQUIRE(p.n_sigmas >= 2 && p.sigmas, "dual denoise: %d sigmas (at least 2)", p.n_sigmas);
    LTX_REQUIRE(p.F >= 1 && p.H >= 1 && p.W >= 1 && p.T_a >= 1 && p.S >= 1 && p.T_a <= (1 << 20) && p.S <= (1 << 20) && (long)p.F * p.H * p.W <= (1 << 20),
                "dual denoise: bad shapes F=%d H=%d W=%d T_a=%d S=%d", p.F, p.H, p.W, p.T_a, p.S);
    LTX_REQUIRE(p.video_latent && p.audio_latent && p.video_context, "dual denoise: null latent or context pointer");
    const bool use_cfg = p.cfg_scale > 1.0f;
    LTX_REQUIRE(!(p.guidance_rescale > 0.f) || use_cfg, "dual denoise: guidance_rescale %g needs cfg_scale > 1 (got %g)", (double)p.guidance_rescale,
                (double)p.cfg_scale);
    const int steps = p.n_sigmas - 1;
    for (int i = 0; i < steps; ++i) LTX_REQUIRE(p.sigmas[i] > 0.f, "dual denoise: sigmas[%d] = %g must be positive", i, (double)p.sigmas[i]);
    const int C = m->cfg.in_channels, Ca = kAudioChannels * kAudioMelBins;
    LTX_REQUIRE(m->cfg.out_channels == C && C % 4 == 0, "dual denoise: video in / out channels differ");
    LTX_REQUIRE(m->cfg.audio_in_channels == Ca && m->cfg.audio_out_channels == Ca, "dual denoise: the audio stream must have %d channels", Ca);
    if (p.cond_latent) LTX_REQUIRE(p.F >= 2, "dual denoise: image-to-video needs at least two latent frames (F=%d)", p.F);
    LTX_REQUIRE(p.video_form >= 0 && p.video_form <= 1, "dual denoise: video_form=%d (0 .. 1)", p.video_form);
}

DualDenoiseState dual_denoise_state(ltx_ctx* ctx, const DualDenoiseParams& p) {
    const Plan q = make_plan(ctx->dual_model, p);
    ctx->dual_dn.ensure(q.bytes);
    char* base = (char*)ctx->dual_dn.p;
    DualDenoiseState s;
    s.xv = (float*)(base + q.o_xv); s.xa = (float*)(base + q.o_xa);
    s.tok_v = (bf16_t*)(base + q.o_tv); s.tok_a = (bf16_t*)(base + q.o_ta);
    return s;
}

void dual_denoise_run(ltx_ctx* ctx, const DualDenoiseParams& p) {
    dual_denoise_check(ctx, p);
    DualModel* m = ctx->dual_model;
    const Plan q = make_plan(m, p);
    const bool use_cfg = q.use_cfg, i2v = q.i2v, renoise = q.renoise;
    const int steps = q.steps, C = q.C, Tv = q.Tv, Ta = q.Ta, B = q.B, HW = q.HW, G = q.G, n_noise = q.n_noise;
    const long nv = q.nv, na = q.na, nk = q.nk;
    const bool entry = (p.phases & DUAL_DN_ENTRY) != 0;
    hipStream_t st = ctx->stream;

    ctx->dual_dn.ensure(q.bytes);
    char* base = (char*)ctx->dual_dn.p;
    float *xv = (float*)(base + q.o_xv), *xa = (float*)(base + q.o_xa), *vel_v = (float*)(base + q.o_vv), *vel_a = (float*)(base + q.o_va),
          *vg = (float*)(base + q.o_vg), *ts = (float*)(base + q.o_ts), *rs = (float*)(base + q.o_rs), *ss = (float*)(base + q.o_ss);
    bf16_t *tok_v = (bf16_t*)(base + q.o_tv), *tok_a = (bf16_t*)(base + q.o_ta);
    int32_t* rmap = (int32_t*)(base + q.o_map);
    float *keep_c = (float*)(base + q.o_kc), *keep_n = (float*)(base + q.o_kn);

    const bf16_t* actx = p.audio_context ? p.audio_context : p.video_context;  // audioEncoding ?? videoEncoding

    if (i2v) {  // :1261-1274, and step 0's re-noising (:1289-1294) while the latent is still in the caller's layout
        if (entry)
            launch_set_frame0(p.video_latent, p.cond_latent, renoise ? p.cond_noise : nullptr, p.image_cond_noise_scale, p.sigmas[0] * p.sigmas[0], C,
                              p.F, HW, st);
        launch_i2v_rowmap(rmap, B, Tv, HW, G, st);
        if (renoise && n_noise > 0) {  // [C][HW] -> [HW][C], every slice in one launch
            launch_unpatchify_f32(p.cond_latent, keep_c, 1, HW, C, st);
            launch_unpatchify_f32(p.cond_noise + nk, keep_n, n_noise, HW, C, st);
        }
    }
    if (entry) {  // token layout, first tokens, the text side
        launch_unpatchify_f32(p.video_latent, xv, 1, Tv, C, st);  // [C][Tv] -> [Tv][C]: the transpose with the roles of C and T exchanged
        pack_audio(p.audio_latent, xa, Ta, false, st);
        launch_cast_f32_bf16(xv, tok_v, nv, st);
        launch_cast_f32_bf16(xa, tok_a, na, st);
        if (B == 2) {
            HIP_CHECK(hipMemcpyAsync(tok_v + nv, tok_v, (size_t)nv * 2, hipMemcpyDeviceToDevice, st));
            HIP_CHECK(hipMemcpyAsync(tok_a + na, tok_a, (size_t)na * 2, hipMemcpyDeviceToDevice, st));
        }
        if (p.text_cache) dual_model_prepare_text(ctx, m, p.video_context, actx, p.mask, p.mask, B, p.S);
    }

    for (int step = 0; step < steps && (p.phases & DUAL_DN_LOOP); ++step) {
        const float sigma = p.sigmas[step], sigma_next = p.sigmas[step + 1];
        if (p.progress) p.progress(p.progress_first + step, p.progress_total > 0 ? p.progress_total : steps, sigma, p.user);  // before the forward (:1285-1287)
        if (i2v) launch_i2v_timesteps(ts, B, G, sigma, st);       // [video B][G] = {sigma, 0}, [audio B]
        else launch_fill_const_f32(ts, 4, sigma, st);            // [video B][audio B]
        DualModelForwardArgs f;
        f.video_latent = tok_v; f.audio_latent = tok_a;
        f.video_timesteps = ts; f.audio_timesteps = i2v ? ts + B * G : ts + 2;
        if (i2v) {
            f.n_groups = G;
            f.video_row_map = rmap;
        }
        f.B = B; f.F = p.F; f.H = p.H; f.W = p.W; f.T_a = Ta; f.S = p.S;
        f.video_velocity = vel_v; f.audio_velocity = vel_a;
        f.text_cache = p.text_cache;
        if (!p.text_cache) {
            f.video_context = p.video_context; f.audio_context = actx;
            f.video_mask = p.mask; f.audio_mask = p.mask;  // one mask, both streams (:1322-1323)
        }
        dual_model_forward(ctx, m, f);

        // batch order [negative, positive]
        DualStepJob jv, ja;
        jv.latent = xv; jv.v_cond = vel_v + (B - 1) * nv; jv.v_uncond = use_cfg ? vel_v : nullptr; jv.cfg_scale = p.cfg_scale;
        jv.form = p.video_form; jv.tokens = tok_v; jv.copies = B; jv.n = nv;
        jv.n_keep = nk;  // frame 0 is not stepped (:1383-1393); re-noised for the next step's forward, which is where the reference does it
        if (renoise && step + 1 < steps) {
            jv.keep_src = keep_c; jv.keep_noise = keep_n + (long)step * nk; jv.keep_scale = p.image_cond_noise_scale;
        }
        ja.latent = xa; ja.v_cond = vel_a + (B - 1) * na; ja.v_uncond = use_cfg ? vel_a : nullptr; ja.cfg_scale = p.cfg_scale;
        ja.form = 1; ja.tokens = tok_a; ja.copies = B; ja.n = na;
        if (p.guidance_rescale > 0.f) {  // video only (:1352-1359); the step then takes the guided velocity as it is
            launch_cfg_combine(jv.v_uncond, jv.v_cond, p.cfg_scale, vg, nv, st);
            launch_mean_var(vg, nv, 1, rs, st);
            launch_mean_var(jv.v_cond, nv, 1, rs + 2, st);
            launch_guidance_rescale(vg, rs, rs + 2, p.guidance_rescale, nv, 1, st);
            jv.v_cond = vg;
            jv.v_uncond = nullptr;
        }
        if (p.step_stats) {  // the guided velocities, in place of the conditional ones
            jv.v_out = (float*)jv.v_cond;
            ja.v_out = (float*)ja.v_cond;
        }
        launch_dual_step(jv, ja, sigma, sigma_next, st);
        if (p.step_stats) {  // the diagnostics of :1407-1413
            float* s8 = ss + 8 * step;
            launch_mean_var(jv.v_out, nv, 1, s8, st);
            launch_mean_var(xv, nv, 1, s8 + 2, st);
            launch_mean_var(ja.v_out, na, 1, s8 + 4, st);
            launch_mean_var(xa, na, 1, s8 + 6, st);
        }
    }

    // exit: back to the caller's layouts
    if (p.phases & DUAL_DN_EXIT_VIDEO) launch_unpatchify_f32(xv, p.video_latent, 1, C, Tv, st);
    if (p.phases & DUAL_DN_EXIT_AUDIO) pack_audio(p.audio_latent, xa, Ta, true, st);
    if (p.step_stats && (p.phases & DUAL_DN_LOOP)) {
        HIP_CHECK(hipMemcpyAsync(p.step_stats, ss, (size_t)steps * 32, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        for (int i = 0; i < 4 * steps; ++i) p.step_stats[2 * i + 1] = sqrtf(p.step_stats[2 * i + 1]);  // variance -> standard deviation
    }
}
