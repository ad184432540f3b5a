// elementwise.h - HBM-bound helper kernels around the GEMM/attention cores (elementwise.hip).
// Every kernel is vectorised (16 B per lane where the layout allows) and fuses the full chain of pointwise work
// between two matrix products, so each activation tensor is read once and written once.
#pragma once
#include "common.h"

enum { LTX_NORM_RMS = 0, LTX_NORM_LAYER = 1 };

// y = norm(x) * (1 + scale[b]) + shift[b]  -> bf16            (adaLN: LTXTransformerBlock.swift:72-83;
//                                                              final head: LTXTransformer.swift:208-224)
struct NormModArgs {
    const float* x = nullptr;          // [rows][ldx] f32, D valid columns
    long ldx = 0;
    const float* scale = nullptr;      // [B][mod_bstride] f32 rows; scale and shift null together: plain norm
    const float* shift = nullptr;
    long mod_bstride = 0;
    int rows_per_batch = 1;            // modulation row b = row / rows_per_batch ...
    const int32_t* row_map = nullptr;  // ... or row_map[row] (per-token timestep groups: image-to-video)
    bf16_t* out = nullptr;             // [rows][ldo] bf16
    long ldo = 0;
    int rows = 0, D = 0;
    int norm_kind = LTX_NORM_RMS;
    float eps = 1e-6f;
    // round norm(x) to bf16 before the modulation (block 0 sees a bf16 residual stream in the reference, so MLXFast.rmsNorm returns
    // bf16 there - SURVEY R10 dtype column)
    int round_norm_bf16 = 0;
};
void launch_norm_mod(const NormModArgs& args, hipStream_t stream);

// The cross-modal norms of the dual video + audio block (LTX2TransformerBlock.swift:246-263): audio_to_video_norm(x_v) and
// video_to_audio_norm(x_a) are each computed ONCE and modulated twice - a2v query / v2a key rows of the video stream, a2v key / v2a
// query rows of the audio stream. One launch, two jobs (video rows at Dv, audio rows at Da; rows == 0: the job is empty): every f32 row
// is read once, RMS-normed once and written twice as bf16, out0 = norm * (1 + scale0[b]) + shift0[b] and out1 likewise with
// (scale1, shift1), b = row_map ? row_map[row] : row / rows_per_batch. A null (scale, shift) pair writes the plain norm. D % 4 == 0 up to 8192, ldx / ldo >= D
// and multiples of 4. Reduction order of norm_mod_kernel (wave sums added in wave order): each output is bit-equal to the
// launch_norm_mod call (LTX_NORM_RMS, round_norm_bf16 = 0, the same row map) it replaces. Every check comes before the launch.
struct NormMod2Job {
    const float* x = nullptr;       // [rows][ldx] f32
    long ldx = 0;
    const float* scale0 = nullptr;  // [B][mod_bstride] f32 rows, D valid columns
    const float* shift0 = nullptr;
    const float* scale1 = nullptr;
    const float* shift1 = nullptr;
    long mod_bstride = 0;
    int rows_per_batch = 1;
    bf16_t* out0 = nullptr;         // [rows][ldo] bf16
    bf16_t* out1 = nullptr;
    long ldo = 0;
    int rows = 0, D = 0;
    const int32_t* row_map = nullptr;  // device [rows] or null: b = row_map[row] (per-token timestep groups, as NormModArgs::row_map)
};
void launch_norm_mod2(const NormMod2Job& video, const NormMod2Job& audio, float eps, hipStream_t stream);

// q/k RMSNorm across ALL heads with learnable weight, then split-RoPE per head (LTXAttention.swift:179-189,
// LTXRoPE.swift:84-149). One launch runs one job or two: q and k of a fused projection share strides, tables and rows (job[1].x ==
// nullptr: a one-job launch). The cross-modal q and k come from different inputs, token counts and tables: two one-job launches.
struct QkNormRopeArgs {
    struct Job {
        const void* x = nullptr;   // [rows][ldx] f32, or bf16 (x_bf16) with ldx counted in bf16 elements; D valid columns
        const float* w = nullptr;  // [D] f32 norm weight
        bf16_t* out = nullptr;     // [rows][ldo] bf16
        // multiplier applied to the normed + rotated row before its single rounding to bf16. The DiT folds the softmax scale and log2(e)
        // into the query's (kAttnQueryPrescale), so that the attention kernel's scores arrive as base-2 exponents: one rounding of q as
        // before, and 48 multiplies per key tile less in the kernel (AttnArgs::q_prescaled).
        float out_scale = 1.0f;
    };
    Job job[2];
    long ldx = 0, ldo = 0;
    const float* cos = nullptr;  // f32 [T][D/2] indexed by (row % T); both null: no RoPE (cross-attention)
    const float* sin = nullptr;
    int T = 1, rows = 0, D = 0;
    float eps = 1e-6f;
    bool x_bf16 = false;
    // 128, or 64 for the audio / cross-modal attention at 32 heads x 64: head h is columns h*head_dim .., rotated as its two halves with
    // columns h*head_dim/2 .. of the cos/sin row
    int head_dim = 128;
};
void launch_qknorm_rope(const QkNormRopeArgs& args, hipStream_t stream);

// sequence-parallel self-attention: gathered V^T blocks [N][D][Tn] -> one V^T [D][ld] with rank r's keys at columns r*Tn ..
void launch_sp_vt_interleave(const bf16_t* gathered, bf16_t* vt, int N, int D, int Tn, long ld, hipStream_t stream);

void launch_cast_f32_bf16(const float* x, bf16_t* out, long n, hipStream_t stream);
void launch_cast_bf16_f32(const bf16_t* x, float* out, long n, hipStream_t stream);

// Sinusoidal timestep embedding [cos(t f_i), sin(t f_i)], f_i = exp(-ln(10000) i/128), t = sigma*mult
// (LTXTimestepEmbedding.swift:17-54). ts: f32 [n], out: f32 [n][256].
void launch_timestep_embedding(const float* ts, float mult, float* out, int n, int dim, hipStream_t stream);

// mod[b][l][j][d] = table[l][j][d] + ada[b][j][d]   (getAdaValues, LTXTransformerBlock.swift:163-185)
void launch_make_mod(const float* tables, const float* ada, float* mod, int B, int L, int J, int D, hipStream_t stream);

// int mask -> additive f32 bias (1-m)*-10000 (LTXTransformer.swift:141-156)
void launch_mask_to_bias(const int32_t* mask, float* bias, long n, hipStream_t stream);

// latent f32 [B][C][F*H*W] -> tokens bf16 [B][T][C] (patchify + .asType(.bfloat16): LatentUtils.swift:20-34,
// LTXPipeline.swift:815) and the inverse in f32 (LatentUtils.swift:42-54).
void launch_patchify_bf16(const float* latent, bf16_t* tokens, int B, int C, int T, hipStream_t stream);
void launch_unpatchify_f32(const float* tokens, float* latent, int B, int C, int T, hipStream_t stream);

// Euler flow-matching update (LTXScheduler.swift:305-327): den = x - s*v; x' = s_next>0 ? den + s_next*(x-den)/s : den
void launch_euler_step(float* latent, const float* velocity, float sigma, float sigma_next, long n, hipStream_t stream,
                       int skip_hw = 0, int frames = 1);
// image-to-video helpers (LTXPipeline.swift:2092-2094, :2225-2252)
void launch_set_frame0(float* latent, const float* cond, const float* noise, float scale, float sigma2, int C, int F, int HW,
                       hipStream_t stream);
void launch_i2v_rowmap(int32_t* row_map, int B, int T, int first, int G, hipStream_t stream);
// the joint loop's timesteps of one image-to-video step in one launch: ts[b][g] = g == 0 ? sigma : 0 ([B][G], the groups of
// launch_i2v_rowmap), followed by B audio timesteps = sigma. B * G + B <= 64.
void launch_i2v_timesteps(float* ts, int B, int G, float sigma, hipStream_t stream);
// Everything between two forwards of the joint video + audio loop (generateVideoWithAudio, LTXPipeline.swift:1276-1417) in ONE launch:
// CFG, the Euler step and the next forward's bf16 operand, for both streams. Two jobs share one grid (video, audio; n == 0: the job is
// empty). Per element, every operation rounded on its own as the reference's separate array ops round (no contraction, correctly
// rounded division), so the f32 outputs are bit-equal to a numpy float32 replay:
//   v  = v_uncond ? v_cond + (cfg_scale - 1) * (v_cond - v_uncond) : v_cond                    (LatentUtils.swift:131-141)
//   form 0 (the scheduler's, LTXScheduler.swift:305-327): den = x - sigma * v; x' = sigma_next > 0 ? den + sigma_next * (x - den) / sigma : den
//   form 1 (the audio line, LTXPipeline.swift:1402):      x' = x + (sigma_next - sigma) * v
//   tokens[c] = bf16(x'), c < copies (round to nearest even, :1306-1307): a B = 2 CFG forward reads both copies, no copy launch
// The two forms are NOT one formula: they differ in about half of the f32 results. Latents stay in TOKEN layout [T][C], which is what
// makes the step elementwise. n % 4 == 0, copies 1 .. 2, form 0 .. 1, sigma > 0; every check comes before the launch.
struct DualStepJob {
    float* latent = nullptr;          // [n] f32, in / out
    const float* v_cond = nullptr;    // [n] f32
    const float* v_uncond = nullptr;  // [n] f32 or null (no CFG)
    float cfg_scale = 1.0f;
    int form = 0;
    bf16_t* tokens = nullptr;         // [copies][n] bf16
    int copies = 1;
    float* v_out = nullptr;           // [n] f32 or null: the guided velocity; may alias v_cond
    long n = 0;
    // frozen prefix (image-to-video: in token layout frame 0 is the first H*W*C elements). Elements i < n_keep skip the Euler form:
    //   keep_noise set:  x' = keep_src + (keep_scale * keep_noise) * (sigma_next * sigma_next)   - frame 0 as the NEXT forward must see it
    //                    (LTXPipeline.swift:1289-1294; four separately rounded f32 operations, as set_frame0_kernel's)
    //   keep_noise null: x' = x
    // tokens (both copies) and v_out are written for the whole job either way. n_keep % 4 == 0, 0 <= n_keep <= n, keep_noise needs
    // keep_src; n_keep = 0 is the kernel without a prefix, bit for bit.
    long n_keep = 0;
    const float* keep_src = nullptr;    // [n_keep] f32
    const float* keep_noise = nullptr;  // [n_keep] f32 or null
    float keep_scale = 0.0f;
};
void launch_dual_step(const DualStepJob& video, const DualStepJob& audio, float sigma, float sigma_next, hipStream_t stream);
// The bridge between the two stages of generateVideoWithAudioTwoStage (LTXPipeline.swift:1712-1752, and step 0's :1765-1769) in ONE
// launch: two jobs share one grid (video, audio; T == 0: the job is empty). Per element, every operation rounded on its own as the
// reference's separate array ops round (no contraction, correctly rounded division and square root):
//   video (x set): reads the upscaled latent and the noise in the caller's layout [C][T], writes the stage-2 start latent and its bf16
//     tokens in TOKEN layout [T][C] through a padded 32x33 LDS tile (reads coalesced along t, 16-byte f32 / 8-byte bf16 stores along c)
//       y = ((x - mu) / (sqrt(var) + 1e-8f)) * sqrt(var_ref) + mu_ref        AdaIN at factor 1 (LatentUtils.swift:201-227)
//       z = s * noise + (1.0f - s) * y                                        (:1730-1731; 1.0f - s is one f32 scalar)
//       t < HW with cond: z = cond, or cond + (cond_scale * cond_noise) * cond_sigma2 (:1744, :1765-1769; set_frame0_kernel's three ops);
//       no AdaIN or re-noise result survives there
//   audio (x null): in place on the packed latent [T][C]: z = s * noise + (1.0f - s) * x (:1734-1735), and its bf16 tokens
// stats / stats_ref are launch_mean_var's {mean, var} pairs per channel. C % 32 == 0, HW <= T, noise exactly when renoise is set; every
// check comes before the launch (dual_restage_check: the checks alone, for a caller that has launches of its own to make first).
struct DualRestageJob {
    const float* x = nullptr;           // video: [C][T] f32; null: the audio job
    float* latent = nullptr;            // [T][C] f32: out (video), in / out (audio)
    bf16_t* tokens = nullptr;           // [T][C] bf16
    int C = 0;
    long T = 0;
    const float* noise = nullptr;       // video [C][T], audio [T][C]; set exactly when renoise is
    float noise_scale = 0.0f;           // s
    int renoise = 0;
    const float* stats = nullptr;       // video: [C][2] {mean, var} of x
    const float* stats_ref = nullptr;   // video: [C][2] {mean, var} of the stage-1 output
    long HW = 0;                        // video: tokens of frame 0; read with cond
    const float* cond = nullptr;        // video: [C][HW] f32 or null
    const float* cond_noise = nullptr;  // video: [C][HW] f32 or null
    float cond_scale = 0.0f;
    float cond_sigma2 = 0.0f;
};
void dual_restage_check(const DualRestageJob& video, const DualRestageJob& audio);
void launch_dual_restage(const DualRestageJob& video, const DualRestageJob& audio, hipStream_t stream);
// CFG combine v = cond + (scale-1)*(cond-uncond) (LatentUtils.swift:131-141)
void launch_cfg_combine(const float* uncond, const float* cond, float scale, float* out, long n, hipStream_t stream);
// out = a + s*(a - b)   (STG: LTXPipeline.swift:920) ; out = g*(a-b)+b (GE: :924-927) share one kernel
void launch_axpby(const float* a, const float* b, float ca, float cb, float* out, long n, hipStream_t stream);
// GE momentum: out = g*(a - b) + b (LTXPipeline.swift:924-927)
void launch_ge(const float* a, const float* b, float g, float* out, long n, hipStream_t stream);
// per-batch population mean/variance over n elements -> stats[b] = {mean, var}
void launch_mean_var(const float* x, long n_per_batch, int B, float* stats, hipStream_t stream);
// guidance rescale (LatentUtils.swift:164-183): out = phi*cfg*(std_cond/std_cfg) + (1-phi)*cfg
void launch_guidance_rescale(float* cfg, const float* stats_cfg, const float* stats_cond, float phi, long n_per_batch,
                             int B, hipStream_t stream);
// AdaIN (LatentUtils.swift:201-227): per (b,c) over F*H*W; x <- (x-mu)/(sd+1e-8)*sd_ref + mu_ref, blended by factor
void launch_adain(float* x, const float* stats_x, const float* stats_ref, float factor, long n_per_chan, int BC,
                  hipStream_t stream);
void launch_scale_inplace(float* x, float s, long n, hipStream_t stream);
// out = ca*a + cb*b
void launch_lincomb(const float* a, const float* b, float ca, float cb, float* out, long n, hipStream_t stream);

// ---- VAE decoder helpers (channels-last f32 stream [P][C]) ----
// latent [C][P] f32 (+ optional noise blend) * std + mean -> channels-last bf16 [P][C] (VideoDecoder.swift:366-381)
// latent/noise element (c,p) lives at [c*chan_stride + p] (lets a temporal tile be a strided view of the full latent)
void launch_vae_prepare(const float* latent, long chan_stride, const float* noise, float noise_scale, const float* mean,
                        const float* std_, bf16_t* out, int C, long P, hipStream_t stream);
// VAE modulation tables, up to 24 in one launch: out[r][c] = table[r][c] + (te ? te[r][c] : 0) + (r odd ? 1 : 0), rows
// shift, scale+1[, shift2, scale2+1] (VAEResBlock3d modulation, VideoDecoder.swift:93-113; final norm :421-434)
struct VaeModsJob {
    const float* table;
    const float* te;
    float* out;
    int rows, C;
};
struct VaeModsBatch {
    static constexpr int MAX_JOBS = 24;
    VaeModsJob job[MAX_JOBS];
    int n = 0;
};
void launch_vae_make_mods_batch(const VaeModsBatch& b, hipStream_t stream);
// temporal-tile blend (VideoDecoder.swift:561-592): r[i] = r[i]*(1-i/n) + nx[i]*(i/n) for frame i < n
void launch_blend_frames(float* r, const float* nx, int n_frames, long frame_elems, hipStream_t stream);
void launch_clip01(float* x, long n, hipStream_t stream);
// pixel-norm over channels (eps 1e-8) * scale + shift -> SiLU -> bf16 (VideoDecoder.swift:29-32,118-127,419-436).
// scale already contains the +1. x: f32 [P][C].
void launch_pixelnorm_silu(const float* x, const float* scale, const float* shift, bf16_t* out, long P, int C,
                           hipStream_t stream);
// conv_out [F*H*W][ldx] f32 (48 valid channels) -> frames (F, 4H, 4W, 3) f32 = clip((x+1)/2, 0, 1)
// (unpatchify VideoDecoder.swift:257-275 + decodeVideo :501-505). When blend_w >= 0 nothing is blended here;
// temporal-tile blending is done by launch_blend_frames on the (F,H,W,3) tensors.

// ---- latent upscaler helpers (SpatialUpscaler.swift) ----
// GroupNorm statistics over (all positions, C/G channels) per group, population variance: stats[g] = {mean, rstd}
// with rstd = 1/sqrt(var + eps) (UpscalerGroupNorm3D, SpatialUpscaler.swift:14-58). x: f32 [P][C].
void launch_groupnorm_stats(const float* x, long P, int C, int G, float eps, float* stats, hipStream_t stream);
// y = (x - mean_g) * rstd_g * w[c] + b[c]; if resid: y += resid; y = SiLU(y) when act; writes f32 and/or bf16
void launch_groupnorm_apply(const float* x, const float* stats, const float* w, const float* b, const float* resid,
                            int act_silu, float* out_f32, bf16_t* out_bf16, long P, int C, int G, hipStream_t stream);
// x [P][C] f32 -> out [C][P] f32 with (x - mean[c]) / std[c]  (upsampleLatents renormalisation, SpatialUpscaler.swift:352-379)
void launch_upscaler_finish(const float* x, const float* mean, const float* std_, float* out, long P, int C, hipStream_t stream);

// ---- text-embedding connector (LTXTextEncoder.swift:62-122, :428-470) ----
// masked (sum, min, max) over the valid tokens of every (state, batch) plane of hidden [states][B][T][D]; partials per chunk,
// then mean and 8/(range+eps) per plane -> stats[(l*B+b)*2 + {0,1}]
void launch_fe_stats(const bf16_t* hidden, const int32_t* mask, int states, int B, int T, int D, int padding_right, float eps,
                     float* partials, float* stats, hipStream_t stream);
// out[b][t][d*states + l] = valid ? bf16(8*(x-mean)/(range+eps)) : 0
long fe_stats_partials_floats(int states, int B, int T, int D);
void launch_fe_norm_concat(const bf16_t* hidden, const int32_t* mask, const float* stats, int states, int B, int T, int D,
                           int padding_right, float eps, bf16_t* out, hipStream_t stream);
// src[b][p] = token index whose row lands at position p, or -1 for a learnable register (valid tokens first, in order;
// position p keeps a token where reverse(valid)[p] is set)
void launch_register_plan(const int32_t* mask, int B, int T, int32_t* src, hipStream_t stream);
// x[b][p][:] = src >= 0 ? enc[b][src][:] : registers[p % R][:]   (f32 stream)
void launch_register_gather(const bf16_t* enc, const float* registers, const int32_t* src, int B, int T, int D, int R, float* x,
                            hipStream_t stream);
void launch_fill_const_i32(int32_t* p, long n, int32_t v, hipStream_t stream);

// ---- VAE encoder (VideoEncoder.swift) ----
void launch_enc_patchify(const float* pixels, bf16_t* out, int T, int H, int W, hipStream_t stream);
void launch_enc_s2d_residual(const float* conv, int Cc, const float* x, int Cx, float* out, int Cout, int T, int H, int W, int ft,
                             int fh, int fw, hipStream_t stream);
void launch_enc_finish(const float* z, long ldz, const float* mean, const float* stdv, float* out, int C, long P, hipStream_t stream);

// ---- Gemma-3 text encoder row passes (Gemma3Model.swift: Gemma.RMSNorm, Gemma3Attention, Gemma3MLP, Gemma3InnerModel) ----
// Every stream is bf16, as MLX stores it; statistics and arithmetic in f32. A norm weight arrives as the file's w (f32 container of a
// bf16 value); the kernels form g = bf16(1 + w), rounded once, as Gemma.RMSNorm forms 1.0 + weight in the weight's dtype. The mean
// square of a row is order-independent: exact f32 squares, summed in f64, rounded to f32 once (a host replay matches it bit for bit).
//   x == null:  h = bf16(rmsnorm(r) * g)                                   (layer 0's input norm)
//   x != null:  h = bf16(x + bf16(rmsnorm(r) * g))                         (post-norm + Gemma.clipResidual, Gemma3Model.swift:161-166)
//   w2 != null: n = bf16(rmsnorm(h) * g2) in the same pass                 (the next pre-norm, or model.norm after the last layer)
//   n_only:     h is not written (the raw output of the last layer is not exported; n = model.norm(h) is)
// One workgroup per row, D % 8 == 0 up to 8192, leading dims multiples of 8. x may alias h (each row is read before it is written).
struct GemmaNormArgs {
    const bf16_t* r = nullptr;  // [rows][ldr]
    long ldr = 0;
    const float* w = nullptr;   // [D]
    const bf16_t* x = nullptr;  // [rows][ldx] or null
    long ldx = 0;
    bf16_t* h = nullptr;        // [rows][ldh]
    long ldh = 0;
    const float* w2 = nullptr;  // [D] or null
    bf16_t* n = nullptr;        // [rows][ldn]
    long ldn = 0;
    int n_only = 0;
    int rows = 0, D = 0;
    float eps = 1e-6f;
};
void launch_gemma_norm(const GemmaNormArgs& args, hipStream_t stream);

// q_norm / k_norm per head of 256 and the non-traditional RoPE (Gemma3Model.swift:88-96), q and k in ONE launch: job j is `heads` heads
// of 256 at columns 0 .. of its row. y = bf16(rmsnorm(head) * bf16(1 + w)), then element i < 128 pairs with i + 128:
// out[i] = bf16(y[i] cos - y[i+128] sin), out[i+128] = bf16(y[i] sin + y[i+128] cos), cos / sin = f32 [T][128] rows indexed by
// row % T (launch_gemma_rope_tables: position p, frequency base^(-i/128)). In place when out == x. Half a wave per head.
struct GemmaQkArgs {
    struct Job {
        const bf16_t* x = nullptr;  // [rows][ldx]
        long ldx = 0;
        const float* w = nullptr;   // [256]
        bf16_t* out = nullptr;      // [rows][ldo]
        long ldo = 0;
        int heads = 0;              // 0: an empty job
    };
    Job job[2];
    const float* cos = nullptr;
    const float* sin = nullptr;
    int T = 1, rows = 0;
    float eps = 1e-6f;
};
void launch_gemma_qknorm_rope(const GemmaQkArgs& args, hipStream_t stream);
// cos / sin [T][128] f32 of positions 0 .. T-1 for one base, made on the device: angle = p * base^(-i / 128), evaluated in f64 and
// rounded to f32 once
void launch_gemma_rope_tables(float* cos_t, float* sin_t, int T, float base, hipStream_t stream);

// out = bf16(bf16(gelu_tanh(g)) * u) over the halves g = gu[:, :I], u = gu[:, I:] of a fused gate|up output (Gemma3Model.swift:128)
struct GegluArgs {
    const bf16_t* gu = nullptr;  // [rows][ldgu]
    long ldgu = 0;
    bf16_t* out = nullptr;       // [rows][ldo]
    long ldo = 0;
    int rows = 0, I = 0;         // I % 8 == 0
};
void launch_geglu(const GegluArgs& args, hipStream_t stream);

// out[r][:] = bf16(table[id[r]][:] * scale), scale = bf16(sqrt(hidden)) (Gemma3Model.swift:209-211). Ids outside [0, vocab) are
// CLAMPED here: a device-side caller has no host to report to (the host-pointer entry rejects them before the launch).
struct GemmaEmbedArgs {
    const int32_t* ids = nullptr;   // [rows]
    const bf16_t* table = nullptr;  // [vocab][D]
    bf16_t* out = nullptr;          // [rows][D]
    int rows = 0, D = 0, vocab = 0;
    float scale = 1.0f;
};
void launch_gemma_embed(const GemmaEmbedArgs& args, hipStream_t stream);

// Greedy token pick on the device (Gemma3Model.swift:438-467): the repetition penalty, then argmax, so a generated token costs the
// host one 4-byte read. hist holds the tokens generated so far; the penalty goes to every DISTINCT id among its last
// min(context, n_gen) entries: l > 0 ? l / penalty (IEEE division) : l * penalty. Nothing is applied while n_gen == 0 or when
// penalty == 1; ids outside [0, vocab) are passed over. The penalised values are written back into `logits` (the reference makes a
// penalised copy; the buffer is refilled by the next step). Argmax ties go to the LOWEST index. The logits are finite by construction
// (a bf16 dot product of finite values); what a NaN does to the pick is unspecified. The token goes to *out and, when hist is
// given, to hist[n_gen] - where the next step's embedding reads it. One workgroup of 1024 threads; logits 16-byte aligned.
struct LmPickArgs {
    float* logits = nullptr;   // [vocab]
    int vocab = 0;
    int32_t* hist = nullptr;   // [>= n_gen + 1] or null (then n_gen must be 0)
    int n_gen = 0, context = 0;
    float penalty = 1.0f;
    int32_t* out = nullptr;    // [1]
};
void launch_lm_pick(const LmPickArgs& args, hipStream_t stream);

// Left-padded mask 0..0 1..1 -> key_start[b] = index of the first 1; status[b] = 1 when row b is of that form with at least one 1
// (values 0 / 1 only), else 0. One workgroup per batch element.
void launch_gemma_mask_scan(const int32_t* mask, int B, int T, int32_t* key_start, int32_t* status, hipStream_t stream);
