// dual_two_stage.cpp - see dual_two_stage.h.
#include "dual_two_stage.h"

#include <algorithm>

#include "dual_denoise.h"
#include "dual_model.h"
#include "elementwise.h"
#include "hostmath.h"
#include "upscaler.h"
#include "vae.h"

namespace {
struct Stages {
    DualDenoiseParams s1, s2;
    const float* sigmas2 = nullptr;
    int n_sigmas2 = 0;
};

// both loops' parameters; s1.video_latent is filled in by the caller once the working buffer exists
Stages make_stages(const DualTwoStageParams& p) {
    Stages g;
    g.sigmas2 = p.sigmas2 ? p.sigmas2 : kStage2DistilledSigmas;
    g.n_sigmas2 = p.sigmas2 ? p.n_sigmas2 : 4;
    const int steps1 = p.n_sigmas1 - 1, steps2 = g.n_sigmas2 - 1;
    for (DualDenoiseParams* d : {&g.s1, &g.s2}) {
        d->F = p.F; d->T_a = p.T_a; d->S = p.S;
        d->audio_latent = p.audio_latent;
        d->video_context = p.video_context; d->audio_context = p.audio_context; d->mask = p.mask;
        d->text_cache = 1;
        d->image_cond_noise_scale = p.image_cond_noise_scale;
        d->progress = p.progress; d->user = p.user;
        d->progress_total = steps1 + steps2;
        // one carving for both stages: stage 2's token count, the longer schedule, the re-noising slices if either stage has them
        d->reserve_Tv = (long)p.F * (2 * p.H) * (2 * p.W);
        d->reserve_steps = std::max(steps1, steps2);
        d->reserve_renoise = p.image_cond_noise_scale > 0.f && (p.cond_noise1 || p.cond_noise2);
    }
    g.s1.H = p.H; g.s1.W = p.W;
    g.s1.sigmas = p.sigmas1; g.s1.n_sigmas = p.n_sigmas1;
    g.s1.cond_latent = p.cond_latent1; g.s1.cond_noise = p.cond_noise1;
    g.s1.video_form = 0;  // LTXScheduler.step (:1666-1677)
    g.s1.phases = DUAL_DN_ENTRY | DUAL_DN_LOOP | DUAL_DN_EXIT_VIDEO;
    g.s1.progress_total = steps1;  // stage 1 reports its own count (:1623)
    g.s2.H = 2 * p.H; g.s2.W = 2 * p.W;
    g.s2.sigmas = g.sigmas2; g.s2.n_sigmas = g.n_sigmas2;
    g.s2.cond_latent = p.cond_latent2; g.s2.cond_noise = p.cond_noise2;
    g.s2.video_latent = p.video_latent_out;
    g.s2.video_form = 1;  // x + dt * v for the video latent too (:1799-1811)
    g.s2.phases = DUAL_DN_LOOP | DUAL_DN_EXIT_VIDEO | DUAL_DN_EXIT_AUDIO;
    g.s2.progress_first = steps1;
    return g;
}
}  // namespace

void dual_two_stage_check(ltx_ctx* ctx, const DualTwoStageParams& p) {
    if (!ctx->dual_model) LTX_THROW(LTXS_MODEL_NOT_LOADED, "Model not loaded: dual transformer model not loaded");
    if (!ctx->upscaler) LTX_THROW(LTXS_MODEL_NOT_LOADED, "Model component not loaded: spatial upscaler");
    if (!ctx->vae) LTX_THROW(LTXS_MODEL_NOT_LOADED, "Model component not loaded: vaeDecoder");
    LTX_REQUIRE(p.video_latent_in && p.video_latent_out && p.audio_latent && p.video_noise2 && p.audio_noise2 && p.video_context && p.sigmas1,
                "dual two-stage: null latent, noise, context or sigma pointer");
    LTX_REQUIRE(p.F >= 1 && p.H >= 1 && p.W >= 1 && p.H <= 1024 && p.W <= 1024, "dual two-stage: bad shapes F=%d H=%d W=%d", p.F, p.H, p.W);
    LTX_REQUIRE(!p.sigmas2 || p.n_sigmas2 >= 2, "dual two-stage: %d stage-2 sigmas (at least 2)", p.n_sigmas2);
    LTX_REQUIRE((p.cond_latent1 != nullptr) == (p.cond_latent2 != nullptr),
                "dual two-stage: image-to-video needs the image latent at both resolutions (cond_latent1 and cond_latent2), or neither");
    LTX_REQUIRE(ctx->dual_model->cfg.in_channels % 32 == 0 && ctx->upscaler->in_channels == ctx->dual_model->cfg.in_channels,
                "dual two-stage: the model's %d latent channels do not fit the upscaler / the restage launch", ctx->dual_model->cfg.in_channels);
    Stages g = make_stages(p);
    g.s1.video_latent = p.video_latent_out;  // any non-null pointer: the working buffer does not exist yet
    dual_denoise_check(ctx, g.s1);
    dual_denoise_check(ctx, g.s2);
}

void dual_two_stage_run(ltx_ctx* ctx, const DualTwoStageParams& p) {
    dual_two_stage_check(ctx, p);
    Stages g = make_stages(p);
    DualModel* m = ctx->dual_model;
    hipStream_t st = ctx->stream;
    const int C = m->cfg.in_channels;
    const long T1 = (long)p.F * p.H * p.W, T2 = 4 * T1, HW2 = 4L * p.H * p.W;
    // working memory: the stage-1 latent in the caller's layout (the caller's stage1_out serves when given), then both statistics
    const size_t lat_bytes = ((size_t)T1 * C * 4 + 255) & ~(size_t)255;
    ctx->dual_ts.ensure(lat_bytes + (size_t)4 * C * 4);
    float* s1 = p.stage1_out ? p.stage1_out : ctx->dual_ts.as<float>();
    float* stats = (float*)((char*)ctx->dual_ts.p + lat_bytes);

    // stage 1 (:1613-1685)
    HIP_CHECK(hipMemcpyAsync(s1, p.video_latent_in, (size_t)T1 * C * 4, hipMemcpyDeviceToDevice, st));
    g.s1.video_latent = s1;
    dual_denoise_run(ctx, g.s1);

    // upscale (:1690-1710): the caller's output buffer holds the upscaled latent until the stage-2 exit overwrites it
    upscaler_forward(ctx, ctx->upscaler, s1, p.F, p.H, p.W, ctx->vae->mean, ctx->vae->std_, p.video_latent_out);
    launch_mean_var(p.video_latent_out, T2, C, stats, st);
    launch_mean_var(s1, T1, C, stats + 2 * C, st);

    // the bridge (:1712-1752, and step 0's :1765-1769), into the state stage 2 starts from
    const DualDenoiseState z = dual_denoise_state(ctx, g.s2);
    const float s = g.sigmas2[0];
    DualRestageJob jv, ja;
    jv.x = p.video_latent_out; jv.latent = z.xv; jv.tokens = z.tok_v; jv.C = C; jv.T = T2;
    jv.noise = p.video_noise2; jv.noise_scale = s; jv.renoise = 1;
    jv.stats = stats; jv.stats_ref = stats + 2 * C;
    if (p.cond_latent2) {
        jv.HW = HW2; jv.cond = p.cond_latent2;
        if (p.image_cond_noise_scale > 0.f && p.cond_noise2) {
            jv.cond_noise = p.cond_noise2; jv.cond_scale = p.image_cond_noise_scale; jv.cond_sigma2 = s * s;
        }
    }
    ja.latent = z.xa; ja.tokens = z.tok_a; ja.C = 128; ja.T = p.T_a;
    ja.noise = p.audio_noise2; ja.noise_scale = s; ja.renoise = 1;
    launch_dual_restage(jv, ja, st);

    // stage 2 (:1754-1816)
    dual_denoise_run(ctx, g.s2);
}
