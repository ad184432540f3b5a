// dual_denoise.h - the denoise loop of generateVideoWithAudio (LTXPipeline.swift:1276-1417), text-to-video+audio and image-to-video+audio,
// around the dual model (dual_model.h). One schedule for both streams. The graph:
//   entry     video [C][Tv] f32 -> token layout [Tv][C] (launch_unpatchify_f32 with the roles of C and T exchanged); audio (8, T_a, 16) ->
//             (T_a, 128) (packAudioLatents, :540-544: eight strided 2-D copies); two launch_cast_f32_bf16 write the first tokens;
//             dual_model_prepare_text once (text_cache)
//   per step  progress callback; both timestep vectors = sigma; ONE dual_model_forward (B = 2 on duplicated tokens and contexts
//             [negative, positive] with CFG, else B = 1); with guidance_rescale > 0 launch_cfg_combine + 2 x launch_mean_var +
//             launch_guidance_rescale on the VIDEO velocity (:1352-1359); ONE launch_dual_step (video: the scheduler's form, audio: the
//             plain form) = CFG, both Euler steps and the next forward's tokens; with step_stats four launch_mean_var
//   exit      the inverse transposes into the caller's buffers
// Both latents stay in token layout for the whole loop, which is what makes the step elementwise: the per-step patchify, unpatchify,
// cast and copy passes of denoise_run (pipeline.cpp) have no counterpart here. No new rounding point: the step is f32, every operation
// rounded on its own as the reference's array ops are (elementwise.h, DualStepJob); the tokens are the one bf16 rounding of :1306-1307.
// Image-to-video (cond_latent set, :1261-1274, :1289-1303, :1383-1399; F >= 2):
//   entry     frame 0 of the caller's latent = cond (+ (scale * noise[0]) * sigmas[0]^2 with re-noising: launch_set_frame0); the row map
//             of two timestep groups per batch element (launch_i2v_rowmap: frame-0 tokens group 1, the rest group 0); cond and the noise
//             slices of steps 1 .. to token layout, once, with the entry transpose
//   per step  video timesteps {sigma, 0} per batch element, audio sigma (ONE launch_i2v_timesteps in place of the fill); the groups
//             forward; ONE launch_dual_step whose video job freezes the first H*W*C elements (frame 0 in token layout) and, with
//             re-noising, writes them as the NEXT step must see them: cond + (scale * noise[step + 1]) * sigma_next^2. The reference
//             re-noises at the start of a step (:1289-1294), where that step's sigma is this step's sigma_next; the last step re-noises
//             nothing, so the final frame 0 is the last noised one, or cond itself without noise. No other launch per step.
// Text-to-video (cond_latent null) runs the launches it ran before the image-to-video path existed, with the same bits.
// Every check comes before the first launch: a refused call leaves both latents untouched. STG, GE and sharding are not implemented.
// The run is entry, loop and exit (DualDenoiseParams::phases). The two-stage path (dual_two_stage.h) runs stage 1 as entry + loop + the
// video exit, and stage 2 as loop + exit from the token-layout state its restage launch wrote into the same allocation: the allocation
// is carved ONCE for the larger stage (reserve_*), so no offset moves and the audio latent stays where stage 1 left it.
#pragma once
#include "../../include/ltxhip.h"
#include "runtime.h"

// the parts of a run (DualDenoiseParams::phases)
enum { DUAL_DN_ENTRY = 1, DUAL_DN_LOOP = 2, DUAL_DN_EXIT_VIDEO = 4, DUAL_DN_EXIT_AUDIO = 8, DUAL_DN_ALL = 15 };
struct DualDenoiseParams {
    int F = 0, H = 0, W = 0, T_a = 0, S = 0;
    float* video_latent = nullptr;          // device [1][C][F][H][W] f32, in / out, scaled by sigmas[0]
    float* audio_latent = nullptr;          // device [1][8][T_a][16] f32, in / out
    const float* sigmas = nullptr;          // host [n_sigmas]
    int n_sigmas = 0;
    const bf16_t* video_context = nullptr;  // device [nb][S][caption_channels] bf16, nb = 2 ([negative, positive]) iff cfg_scale > 1
    const bf16_t* audio_context = nullptr;  // the same shape; null = the video context
    const int32_t* mask = nullptr;          // device [nb][S] or null; both streams
    float cfg_scale = 1.0f;
    float guidance_rescale = 0.0f;          // video velocity only
    int text_cache = 1;
    float* step_stats = nullptr;            // host [n_sigmas - 1][8] or null: mean, std of video velocity, video latent, audio velocity, audio latent
    ltx_progress_cb progress = nullptr;
    void* user = nullptr;
    // image-to-video, as ltx_denoise_options has them (device pointers)
    const float* cond_latent = nullptr;     // [1][C][1][H][W] f32 or null (text-to-video)
    float image_cond_noise_scale = 0.0f;
    const float* cond_noise = nullptr;      // [n_sigmas - 1][C][1][H][W] f32 or null (no re-noising)
    // what the two-stage path adds; the defaults are ltx_dual_denoise
    int video_form = 0;                     // the video stream's Euler form (DualStepJob::form): 0 the scheduler's, 1 the plain one (stage 2, :1799-1811)
    int phases = DUAL_DN_ALL;               // which parts run. Without DUAL_DN_ENTRY the latents, their tokens and frame 0 are taken as they
                                            // stand in the allocation (token layout), and the text cache as it is
    int progress_first = 0, progress_total = 0;  // the callback gets (progress_first + step, progress_total, or this run's steps when 0)
    long reserve_Tv = 0;                    // carve the allocation for at least this many video tokens, ...
    int reserve_steps = 0;                  // ... this many steps ...
    bool reserve_renoise = false;           // ... and the re-noising slices, so that two runs of different shapes share every offset
};
// where the token-layout state of a run lives in ctx->dual_dn (valid until the allocation grows)
struct DualDenoiseState {
    float* xv = nullptr;      // [Tv][C] f32
    float* xa = nullptr;      // [T_a][128] f32
    bf16_t* tok_v = nullptr;  // [B][Tv][C] bf16
    bf16_t* tok_a = nullptr;  // [B][T_a][128] bf16
};
// every check of dual_denoise_run and nothing else: for a caller that must refuse before a launch of its own
void dual_denoise_check(ltx_ctx* ctx, const DualDenoiseParams& p);
// sizes the allocation for `p` (growing it if needed) and returns the state pointers
DualDenoiseState dual_denoise_state(ltx_ctx* ctx, const DualDenoiseParams& p);
void dual_denoise_run(ltx_ctx* ctx, const DualDenoiseParams& p);
