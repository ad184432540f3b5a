// dual_two_stage.h - the two denoise loops of generateVideoWithAudioTwoStage and what lies between them (LTXPipeline.swift:1613-1817),
// with both latents on the device from the first noise to the final latents. The graph:
//   stage 1   dual_denoise_run, entry + loop + the video exit: the text cache filled ONCE (stage 2 has the same B and S and reads it),
//             video form 0, audio form 1, image-to-video groups at (F, H, W). The audio latent stays in token layout in the loop's
//             allocation; the video latent goes back to the caller's layout: the AdaIN reference (:1688) and the upscaler's input
//   bridge    upscaler_forward with the VAE's statistics (:1696-1710) into the caller's output buffer; two launch_mean_var; ONE
//             launch_dual_restage = AdaIN + the re-noise of both streams + frame 0 + token layout + the first bf16 tokens (:1712-1752)
//   stage 2   dual_denoise_run, loop + exit, from that token state: BOTH streams in form 1 (:1799-1811), groups at (F, 2H, 2W)
// The loop's allocation is carved once for stage 2's shape (DualDenoiseParams::reserve_*), so stage 1 and stage 2 agree on every
// offset and nothing moves between them. Distilled: one forward per step, no CFG (:1646, :1783). Every check - this file's and both
// loops' - comes before the first launch. Noise drawing, sharding, the decode legs and the CLI are not here.
#pragma once
#include "../../include/ltxhip.h"
#include "runtime.h"

struct DualTwoStageParams {
    int F = 0, H = 0, W = 0, T_a = 0, S = 0;  // stage-1 latent dims; stage 2 is F, 2H, 2W
    const float* video_latent_in = nullptr;   // device [1][C][F][H][W] f32, scaled by sigmas1[0]
    float* video_latent_out = nullptr;        // device [1][C][F][2H][2W] f32
    float* audio_latent = nullptr;            // device [1][8][T_a][16] f32, in / out
    const float* sigmas1 = nullptr;           // host
    int n_sigmas1 = 0;
    const float* sigmas2 = nullptr;           // host; null = kStage2DistilledSigmas
    int n_sigmas2 = 0;
    const float* video_noise2 = nullptr;      // device [1][C][F][2H][2W] f32
    const float* audio_noise2 = nullptr;      // device [T_a][128] f32 (the packed shape, :1734)
    const bf16_t* video_context = nullptr;    // device [1][S][caption_channels] bf16
    const bf16_t* audio_context = nullptr;    // null = the video context
    const int32_t* mask = nullptr;            // device [1][S] or null
    float* stage1_out = nullptr;              // device [1][C][F][H][W] f32 or null
    const float* cond_latent1 = nullptr;      // device [1][C][1][H][W] f32 or null; both image latents or neither
    const float* cond_latent2 = nullptr;      // device [1][C][1][2H][2W] f32 or null
    float image_cond_noise_scale = 0.0f;
    const float* cond_noise1 = nullptr;       // device [n_sigmas1 - 1][C][1][H][W] f32 or null
    const float* cond_noise2 = nullptr;       // device [n_sigmas2 - 1][C][1][2H][2W] f32 or null
    ltx_progress_cb progress = nullptr;       // stage 1: (step, steps1); stage 2: (steps1 + step, steps1 + steps2) (:1623, :1760)
    void* user = nullptr;
};
// the checks alone (the host entry refuses before it stages); dual_two_stage_run repeats them
void dual_two_stage_check(ltx_ctx* ctx, const DualTwoStageParams& p);
void dual_two_stage_run(ltx_ctx* ctx, const DualTwoStageParams& p);
