// dual_generate.cpp - see dual_generate.h.
#include "dual_generate.h"

#include <vector>

#include "dual_denoise.h"
#include "dual_model.h"
#include "dual_two_stage.h"
#include "hostmath.h"
#include "noise.h"

namespace {
constexpr long kSlotAlign = 64;  // floats: workspace slots start on 256-byte lines

bool has_renoise(const ltx_dual_generate_args& a) {
    return a.image_cond_noise_scale > 0.f && a.cond_latent1 && (!a.two_stage || a.cond_latent2);
}

// the loop's parameters on the plan's pointers; `ws` and the latents may be placeholders when only the checks run
struct Wiring {
    float* video1 = nullptr;       // where draw 0 goes
    const float* cond1 = nullptr;  // the first slice of each COND role, or null
    const float* video2 = nullptr;
    const float* audio2 = nullptr;
    const float* cond2 = nullptr;
};
Wiring wire(const ltx_dual_generate_args& a, const std::vector<ltx_noise_draw>& plan, float* ws) {
    Wiring w;
    for (const ltx_noise_draw& d : plan) {
        float* at = d.offset >= 0 ? ws + d.offset : nullptr;
        if (d.role == LTX_NOISE_VIDEO1) w.video1 = at ? at : a.video_latent;
        if (d.role == LTX_NOISE_COND1 && d.step == 0) w.cond1 = at;
        if (d.role == LTX_NOISE_VIDEO2) w.video2 = at;
        if (d.role == LTX_NOISE_AUDIO2) w.audio2 = at;
        if (d.role == LTX_NOISE_COND2 && d.step == 0) w.cond2 = at;
    }
    return w;
}
DualDenoiseParams one_stage_params(const ltx_dual_generate_args& a, const Wiring& w, ltx_progress_cb cb, void* user) {
    DualDenoiseParams p;
    p.F = a.F; p.H = a.H; p.W = a.W; p.T_a = a.T_a; p.S = a.S;
    p.video_latent = a.video_latent; p.audio_latent = a.audio_latent;
    p.sigmas = a.sigmas1; p.n_sigmas = a.n_sigmas1;
    p.video_context = a.video_context; p.audio_context = a.audio_context; p.mask = a.mask;
    p.cfg_scale = a.cfg_scale; p.guidance_rescale = a.guidance_rescale;
    p.cond_latent = a.cond_latent1; p.image_cond_noise_scale = a.image_cond_noise_scale; p.cond_noise = w.cond1;
    p.progress = cb; p.user = user;
    return p;
}
DualTwoStageParams two_stage_params(const ltx_dual_generate_args& a, const Wiring& w, ltx_progress_cb cb, void* user) {
    DualTwoStageParams p;
    p.F = a.F; p.H = a.H; p.W = a.W; p.T_a = a.T_a; p.S = a.S;
    p.video_latent_in = w.video1; p.video_latent_out = a.video_latent; p.audio_latent = a.audio_latent;
    p.sigmas1 = a.sigmas1; p.n_sigmas1 = a.n_sigmas1; p.sigmas2 = a.sigmas2; p.n_sigmas2 = a.n_sigmas2;
    p.video_noise2 = w.video2; p.audio_noise2 = w.audio2;
    p.video_context = a.video_context; p.audio_context = a.audio_context; p.mask = a.mask;
    p.stage1_out = a.stage1_out;
    p.cond_latent1 = a.cond_latent1; p.cond_latent2 = a.cond_latent2; p.image_cond_noise_scale = a.image_cond_noise_scale;
    p.cond_noise1 = w.cond1; p.cond_noise2 = w.cond2;
    p.progress = cb; p.user = user;
    return p;
}
std::vector<ltx_noise_draw> plan_of(const ltx_dual_generate_args& a, long* total) {
    const int n = dual_noise_plan(a, nullptr, 0, total);
    std::vector<ltx_noise_draw> plan((size_t)n);
    dual_noise_plan(a, plan.data(), n, total);
    return plan;
}
// the plan's checks and the wrapped loop's, on whatever non-null pointer stands in for the workspace
void check_with(ltx_ctx* ctx, const ltx_dual_generate_args& a, const std::vector<ltx_noise_draw>& plan, float* ws) {
    DualModel* m = ctx->dual_model;
    if (!m) LTX_THROW(LTXS_MODEL_NOT_LOADED, "Model not loaded: dual transformer model not loaded");
    LTX_REQUIRE(a.channels == m->cfg.in_channels, "dual generate: channels=%d, the loaded model has %d latent channels", a.channels, m->cfg.in_channels);
    LTX_REQUIRE(a.video_latent && a.audio_latent, "dual generate: null output latent");
    const Wiring w = wire(a, plan, ws);
    if (a.two_stage) {
        LTX_REQUIRE(!(a.cfg_scale > 1.0f) && !(a.guidance_rescale > 0.f), "dual generate: the two-stage path is distilled (no CFG, no guidance rescale)");
        dual_two_stage_check(ctx, two_stage_params(a, w, nullptr, nullptr));
    } else {
        dual_denoise_check(ctx, one_stage_params(a, w, nullptr, nullptr));
    }
}
}  // namespace

int dual_noise_plan(const ltx_dual_generate_args& a, ltx_noise_draw* out, int cap, long* total_floats) {
    LTX_REQUIRE(cap >= 0 && (out || cap == 0), "dual noise plan: cap=%d, or a null array", cap);
    LTX_REQUIRE(a.channels >= 1 && a.F >= 1 && a.H >= 1 && a.W >= 1 && a.T_a >= 1, "dual noise plan: bad shapes channels=%d F=%d H=%d W=%d T_a=%d",
                a.channels, a.F, a.H, a.W, a.T_a);
    LTX_REQUIRE(a.n_sigmas1 >= 2 && a.sigmas1, "dual noise plan: %d sigmas (at least 2)", a.n_sigmas1);
    LTX_REQUIRE(!a.two_stage || !a.sigmas2 || a.n_sigmas2 >= 2, "dual noise plan: %d stage-2 sigmas (at least 2)", a.n_sigmas2);
    LTX_REQUIRE(!a.two_stage || (a.cond_latent1 != nullptr) == (a.cond_latent2 != nullptr),
                "dual noise plan: image-to-video needs the image latent at both resolutions (cond_latent1 and cond_latent2), or neither");
    const long frame = (long)a.channels * a.H * a.W, audio = 128L * a.T_a;
    const long limit = 1L << 31;  // the counters of a draw are 32 bit
    LTX_REQUIRE(frame < limit / 4 / a.F && audio < limit, "dual noise plan: a draw of 2^31 values or more (F=%d H=%d W=%d T_a=%d)", a.F, a.H, a.W, a.T_a);
    const bool renoise = has_renoise(a);
    const int steps1 = a.n_sigmas1 - 1, steps2 = a.two_stage ? (a.sigmas2 ? a.n_sigmas2 : 4) - 1 : 0;
    int n = 0;
    long off = 0;
    auto put = [&](int role, int step, long numel, float scale, bool in_workspace, bool contiguous) {
        ltx_noise_draw d;
        d.draw_index = n; d.role = role; d.step = step; d.numel = numel; d.scale = scale; d.offset = -1;
        if (in_workspace) {
            if (!contiguous) off = (off + kSlotAlign - 1) / kSlotAlign * kSlotAlign;
            d.offset = off;
            off += numel;
        }
        if (n < cap) out[n] = d;
        ++n;
    };
    put(LTX_NOISE_VIDEO1, 0, frame * a.F, a.sigmas1[0], a.two_stage != 0, false);
    put(LTX_NOISE_AUDIO1, 0, audio, a.sigmas1[0], false, false);
    if (renoise)
        for (int s = 0; s < steps1; ++s) put(LTX_NOISE_COND1, s, frame, 1.0f, true, s > 0);
    if (a.two_stage) {
        put(LTX_NOISE_VIDEO2, 0, 4 * frame * a.F, 1.0f, true, false);
        put(LTX_NOISE_AUDIO2, 0, audio, 1.0f, true, false);
        if (renoise)
            for (int s = 0; s < steps2; ++s) put(LTX_NOISE_COND2, s, 4 * frame, 1.0f, true, s > 0);
    }
    if (total_floats) *total_floats = (off + kSlotAlign - 1) / kSlotAlign * kSlotAlign;
    return n;
}

void dual_generate_check(ltx_ctx* ctx, const ltx_dual_generate_args& a) {
    long total = 0;
    const std::vector<ltx_noise_draw> plan = plan_of(a, &total);
    check_with(ctx, a, plan, a.video_latent);  // any pointer: nothing is read through it
}

int dual_generate_run(ltx_ctx* ctx, const ltx_dual_generate_args& a, ltx_progress_cb cb, void* user) {
    long total = 0;
    const std::vector<ltx_noise_draw> plan = plan_of(a, &total);
    check_with(ctx, a, plan, a.video_latent);
    float* ws = a.noise_workspace;
    if (!ws && total > 0) {
        ctx->dual_noise.ensure((size_t)total * 4);
        ws = ctx->dual_noise.as<float>();
    }
    const Wiring w = wire(a, plan, ws);
    std::vector<ltx_noise_job> jobs(plan.size());
    for (size_t i = 0; i < plan.size(); ++i) {
        const ltx_noise_draw& d = plan[i];
        ltx_noise_job& j = jobs[i];
        mlx_draw_key(a.seed, d.draw_index, j.key);
        j.dst = d.offset >= 0 ? ws + d.offset : d.role == LTX_NOISE_VIDEO1 ? a.video_latent : a.audio_latent;
        j.n = d.numel; j.scale = d.scale; j.raw_bits = 0;
    }
    const int launches = launch_mlx_normal_group(jobs.data(), (int)jobs.size(), ctx->stream);
    if (a.two_stage)
        dual_two_stage_run(ctx, two_stage_params(a, w, cb, user));
    else
        dual_denoise_run(ctx, one_stage_params(a, w, cb, user));
    return launches;
}
