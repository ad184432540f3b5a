// dual_generate.h - generateVideoWithAudio (LTXPipeline.swift:1222-1417) and generateVideoWithAudioTwoStage (:1570-1817) from a seed to
// the final latents: the draw plan of a run, ONE launch that makes every draw on the device (noise.h), then dual_denoise_run or
// dual_two_stage_run on pointers into the noise workspace. The reference draws every tensor of a run from one seeded key sequence in a
// fixed order; the plan is that order:
//   draw 0      VIDEO1  [1][C][F][H][W], times sigmas1[0]                       (:1229, :1243 / :1576, :1597)
//   draw 1      AUDIO1  [1][8][T_a][16], times sigmas1[0]                       (:1233, :1244 / :1580, :1598)
//   then        COND1   one [1][C][1][H][W] slice per step of the (first) loop  (:1291 / :1629)   image latent and scale > 0 only
//   two-stage   VIDEO2  [1][C][F][2H][2W]                                       (:1730)
//               AUDIO2  [T_a][128], the packed shape                            (:1734)
//               COND2   one [1][C][1][2H][2W] slice per stage-2 step            (:1766)          image latents and scale > 0 only
// A draw that the loop takes in place goes straight into the latent buffer and has no slot in the workspace (offset -1): AUDIO1 always,
// VIDEO1 in the one-stage run; the two-stage run reads VIDEO1 from the workspace (its stage-1 latent is a buffer of its own). The other
// slots start at multiples of 64 floats, except that the slices of one COND role are contiguous: the loops take them as one array.
// This file adds no numerics: the result is the wrapped loop's on these draws. Every check - the plan's and the loop's - comes before
// the first launch. Sharding of the joint loop, the decode legs and the CLI are not here.
#pragma once
#include "../../include/ltxhip.h"
#include "runtime.h"

// `a` with every field present (the ABI layer has copied what struct_size covers). Returns the number of draws and writes at most `cap`
// of them; throws invalidConfiguration on what ltx_dual_noise_plan refuses.
int dual_noise_plan(const ltx_dual_generate_args& a, ltx_noise_draw* out, int cap, long* total_floats);
// the checks alone (the host entry refuses before it stages)
void dual_generate_check(ltx_ctx* ctx, const ltx_dual_generate_args& a);
// device pointers; a.noise_workspace null = ctx->dual_noise. Returns the noise launches made (1, or more past 64 draws).
int dual_generate_run(ltx_ctx* ctx, const ltx_dual_generate_args& a, ltx_progress_cb cb, void* user);
