/* ltxhip.h - C ABI of libltxhip.so: the MI355X-native LTX-2 denoise + VAE-decode path.
 *
 * This is the drop-in boundary for the hot path of VincentGourbin/ltx-video-swift-mlx. The reference has no FFI of
 * its own (it is a Swift library calling MLX directly); each entry point below replaces the Swift seam named in
 * its comment (file:line in the reference tree), so that a Swift `LTXPipeline` can keep its public surface and call
 * HIP through this header (see INTEGRATION.md for the module map and the Swift wrapper).
 *
 * Conventions
 *   - plain C types only; bf16 tensors are `uint16_t` bit patterns; all tensors are dense row-major.
 *   - every function returns an `ltx_status` (0 = ok). Codes mirror the reference's `LTXError` cases
 *     (LTXVideo.swift:66-141); `ltx_last_error(ctx)` returns the message the Swift wrapper re-throws.
 *   - ownership: the caller owns every buffer it passes; `ltx_ctx` owns all device memory. Entry points without a
 *     `_dev` suffix take HOST pointers and stage through HBM; `_dev` variants take DEVICE pointers valid on the
 *     context's GPU and run asynchronously on the context's stream (`ltx_ctx_set_stream`).
 *   - threading: one in-flight call per `ltx_ctx` (the reference's `LTXPipeline` is an actor; its models are not
 *     re-entrant: LTXTransformer.swift:30-31, LTXTransformerBlock.swift:117-123, LTXScheduler.swift:49-55).
 *   - the library fails loudly: there is no CPU fallback behind any of these calls.
 */
#ifndef LTXHIP_H
#define LTXHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ltx_ctx ltx_ctx;

/* LTXError (LTXVideo.swift:66-141) -> status code */
typedef enum ltx_status {
    LTX_OK = 0,
    LTX_ERR_MODEL_NOT_LOADED = 1,      /* .modelNotLoaded */
    LTX_ERR_INVALID_CONFIGURATION = 2, /* .invalidConfiguration */
    LTX_ERR_INSUFFICIENT_MEMORY = 3,   /* .insufficientMemory */
    LTX_ERR_WEIGHT_LOADING_FAILED = 4, /* .weightLoadingFailed */
    LTX_ERR_GENERATION_FAILED = 5,     /* .generationFailed */
    LTX_ERR_GENERATION_CANCELLED = 6,  /* .generationCancelled */
    LTX_ERR_INVALID_FRAME_COUNT = 7,   /* .invalidFrameCount */
    LTX_ERR_INVALID_DIMENSIONS = 8,    /* .invalidDimensions */
    LTX_ERR_FILE_NOT_FOUND = 9,        /* .fileNotFound */
    LTX_ERR_INVALID_LORA = 10,         /* .invalidLoRA */
    LTX_ERR_HIP = 11                   /* device/runtime failure (no reference counterpart) */
} ltx_status;

/* LTXTransformerConfig (LTXConfig.swift:83-177) */
typedef struct ltx_transformer_config {
    int num_layers;                  /* 48 */
    int num_attention_heads;         /* 32 */
    int attention_head_dim;          /* 128 */
    int in_channels;                 /* 128 */
    int out_channels;                /* 128 */
    int cross_attention_dim;         /* 4096 */
    int caption_channels;            /* 3840 */
    float rope_theta;                /* 10000 */
    int max_pos[3];                  /* 20, 2048, 2048 */
    float timestep_scale_multiplier; /* 1000 */
    float norm_eps;                  /* 1e-6 */
} ltx_transformer_config;

/* ------------------------------------------------------------------------------------------------------------
 * Library / context
 * ---------------------------------------------------------------------------------------------------------- */
/* LTXVideo.version (LTXVideo.swift, asserted by Tests/LTXVideoTests/LTXVideoTests.swift:9-11) */
const char* ltx_version(void);
/* Revision of THIS header's binary interface (struct layouts, entry-point signatures); also the library's soname suffix
 * (libltxhip.so.2). ltx_version() mirrors the reference's framework version and does not move with it.
 *   1  rounds 1-4      2  round 5: ltx_denoise_options.struct_size first, ltx_ctx_set_option / ltx_ctx_get_option, no environment hooks */
#define LTX_ABI_VERSION 2
int ltx_abi_version(void);
/* "gfx950;experiments=0|1": whether this build carries the measured-but-not-selected kernels (-DLTX_EXPERIMENTS; the product does not). */
const char* ltx_build_info(void);
/* Filled with the reference defaults (LTXConfig.swift:83-177). */
void ltx_transformer_config_default(ltx_transformer_config* cfg);
/* Replaces `LTXPipeline.init` device/bookkeeping (LTXPipeline.swift:189-200). Fails with LTX_ERR_HIP when no
 * gfx950 device is usable. */
int ltx_ctx_create(int device, ltx_ctx** out);
void ltx_ctx_destroy(ltx_ctx* ctx);
const char* ltx_last_error(const ltx_ctx* ctx);
/* Run all work of this context on an existing HIP stream (hipStream_t passed as void*). The handle is used as given:
 * NULL selects the default (null) stream. A new context starts on a private non-blocking stream. */
int ltx_ctx_set_stream(ltx_ctx* ctx, void* hip_stream);
int ltx_ctx_synchronize(ltx_ctx* ctx);
/* Tuning / A-B switches of the kernel launchers (csrc/options.h holds the table; `ltx_option_info` enumerates it). The library NEVER
 * reads the environment (the -DLTX_EXPERIMENTS build of tools/ seeds the same table from LTX_<NAME>): this call is the only way to move
 * a switch, so a host's numerics do not depend on who launched it. Switches flagged `numerics` move results by rounding or accumulation
 * order only - e.g. "qk_f32" = 1 and "split_f32" = 1 remove the two roundings this path has beyond the reference's;
 * the others are bit-neutral. The table is process-wide (launchers are shared by all contexts); `ctx` receives the error message.
 * Unknown key or out-of-range value: LTX_ERR_INVALID_CONFIGURATION. No reference counterpart (MLX has no such switches). */
int ltx_ctx_set_option(ltx_ctx* ctx, const char* key, int value);
int ltx_ctx_get_option(const ltx_ctx* ctx, const char* key, int* value);
/* index 0 .. n-1 -> name / default / range / numerics flag / one-line description; returns the number of options (any pointer may be
 * NULL; index out of range: only the count is returned). */
int ltx_option_info(int index, const char** name, int* default_value, int* min_value, int* max_value, int* numerics, const char** doc);
/* Counts of the last load call: tensors applied / model parameters absent from the file (left at the reference's
 * initial values) / mapped file keys with no parameter (dropped), as logged at ModelDownloader.swift:992-1017. */
int ltx_load_report(const ltx_ctx* ctx, int* n_loaded, int* n_missing, int* n_unmatched);

/* ------------------------------------------------------------------------------------------------------------
 * Pure host logic (no GPU needed): shapes, schedules, tables, key mapping
 * ---------------------------------------------------------------------------------------------------------- */
/* LTXVideoGenerationConfig.validate (LTXConfig.swift:310-353) + two-stage %64 rule (LTXPipeline.swift:2443).
 * On failure writes the reference's message into msg (if non-NULL). */
int ltx_validate_generation_config(int width, int height, int num_frames, int num_steps, float cfg_scale,
                                   int two_stage, char* msg, int msg_cap);
/* latentFrames/Height/Width (LTXConfig.swift:356-361; VideoLatentShape.fromPixelDimensions :95-111) */
int ltx_latent_shape(int width, int height, int num_frames, int* latent_frames, int* latent_height,
                     int* latent_width);
/* LTXScheduler.setTimesteps (LTXScheduler.swift:74-182). token_count <= 0 means "not provided".
 * Writes up to cap values, returns the number of sigmas (9 for distilled, num_steps+1 for dev) or <0 on error. */
int ltx_sigmas(int distilled, int num_steps, int token_count, float* out, int cap);
/* STAGE_2_DISTILLED_SIGMA_VALUES (LTXScheduler.swift:31-36); returns 4. */
int ltx_stage2_sigmas(float* out, int cap);
/* createPositionGrid + precomputeFreqsCis(doublePrecision:true) (LTXRoPE.swift:552-610,375-527).
 * cos_out/sin_out: [F*H*W][inner_dim/2] f32; head h owns columns h*64..h*64+63 (the reference's [B,H,T,64]). */
int ltx_rope_tables(const ltx_transformer_config* cfg, int F, int H, int W, float* cos_out, float* sin_out);
/* decodeWithTemporalTiling's tile walk and blended frame count (VideoDecoder.swift:517-592).
 * Returns the number of tiles (<= cap written) or <0 on error. */
int ltx_vae_tile_plan(int latent_frames, int tile, int overlap, int* starts, int* ends, int cap, int* out_frames);
/* mapTransformerKey + loadTransformerWeights filters (ModelDownloader.swift:605-639,756-803). Returns 1 and writes
 * the module key, 0 when the file key is skipped, <0 when out is too small. */
int ltx_map_transformer_key(const char* file_key, char* out, int cap);
/* mapVAEWeights (ModelDownloader.swift:808-899). */
int ltx_map_vae_key(const char* file_key, char* out, int cap);
/* LoRAKeyMapper.loraKeyToModelKey (LoRALoader.swift:209-243). */
int ltx_map_lora_key(const char* lora_key, char* out, int cap);

/* safetensors file access for host tools (the CLI reads PrecomputedEmbeddings / noise tensors through these).
 * ltx_st_info: shape of `key` (up to 8 dims), returns ndim or <0. ltx_st_read: converts to `dtype` (0 f32, 1 bf16 bits,
 * 2 int32) into out (capacity in elements), returns the element count or <0. */
int ltx_st_info(const char* path, const char* key, long* shape8);
long ltx_st_read(const char* path, const char* key, int dtype, void* out, long cap);

/* ------------------------------------------------------------------------------------------------------------
 * DiT (LTXTransformer)
 * ---------------------------------------------------------------------------------------------------------- */
/* Replaces LTXTransformer(config:) + LTXWeightLoader.loadTransformerWeights/applyTransformerWeights
 * (LTXPipeline.swift:293-314, ModelDownloader.swift:605-639,972-1019). cfg NULL = reference defaults.
 * quant_bits: 16 (bf16), 8 (qint8) or 4 (int4) = LTXQuantizationConfig.transformer (LTXQuantizationConfig.swift:19-62):
 * after loading, every Linear weight is affine-quantised per 64-wide group along `in` (LTXPipeline.swift:323-333) and
 * kept as its de-quantised bf16 value (HBM capacity is not the constraint here; the MFMA path stays bf16). */
int ltx_dit_load(ltx_ctx* ctx, const char* safetensors_path, const ltx_transformer_config* cfg, int quant_bits,
                 int group_size);
/* Random-init weights of the given architecture, generated on device (bench / property tests). */
int ltx_dit_init_synthetic(ltx_ctx* ctx, const ltx_transformer_config* cfg, uint64_t seed);
/* quantize(model:groupSize:bits:) applied to an already loaded / synthetic model (LTXPipeline.swift:329). */
int ltx_dit_quantize(ltx_ctx* ctx, int bits, int group_size);
/* Device memory the resident transformer holds, by arena (what MLX's memory statistics would show the host, LTXPipeline.swift:3176-3187
 * estimateMemory): the bf16 Linear weights (0 once quantised: ltx_dit_quantize RELEASES them, as MLXNN.quantize replaces the
 * modules), the codes + group scales / biases, the one de-quantisation scratch matrix, and everything else (biases, norm weights,
 * tables). Any pointer may be NULL. */
int ltx_dit_memory_info(ltx_ctx* ctx, long* bf16_weight_bytes, long* quantised_weight_bytes, long* scratch_bytes, long* other_bytes);
/* Reads one parameter of the resident model back to the HOST as f32 (bf16 values widened; of a quantised model the de-quantised
 * value the GEMMs use). module_key: the reference's module path, e.g. "transformer_blocks.3.attn1.to_q.weight".
 * Returns the element count (written only if <= cap; out NULL = query) or <0. Parity tests use it to hand the on-device
 * synthetic weights of ltx_dit_init_synthetic to the CPU oracle at the reference's full width. */
long ltx_dit_export_param(ltx_ctx* ctx, const char* module_key, float* out, long cap);
/* Replaces LTXPipeline.fuseLoRA(from:scale:) -> Module.fuseLoRA (LTXPipeline.swift:3134-3153, LoRAAdapter.swift:64-166):
 * W' = W + cast(scale * (alpha/rank | 1) * (up @ down)) for every LoRA layer whose mapped key (ltx_map_lora_key) names a
 * Linear weight; on a quantised model dequant -> merge -> requant. *n_fused = number of fused layers. */
int ltx_dit_fuse_lora(ltx_ctx* ctx, const char* lora_path, float scale, int* n_fused);
/* `transformer = nil` (LTXPipeline.swift:989-999) */
int ltx_dit_unload(ltx_ctx* ctx);
/* Replaces transformer(latent:context:timesteps:contextMask:latentShape:) (LTXTransformer.swift:235).
 *   latent   [B][T][in_channels] bf16, T = F*H*W, token t = (f*H+h)*W+w
 *   context  [B][S][caption_channels] bf16
 *   timesteps[B] f32 (sigma; scaled by timestep_scale_multiplier inside)
 *   mask     [B][S] int32 (1 attend, 0 pad) or NULL
 *   velocity [B][T][out_channels] f32 (out)
 * HOST pointers. */
int ltx_dit_forward(ltx_ctx* ctx, const uint16_t* latent, const uint16_t* context, const float* timesteps,
                    const int32_t* mask, int B, int F, int H, int W, int S, float* velocity);
/* Same with DEVICE pointers, asynchronous on the context stream. ctx_version: non-zero value that changes whenever
 * the context/mask contents change (lets the library keep the projected caption and cross-attention K/V resident
 * across denoise steps - output-identical to recomputing them); 0 = recompute every call.
 * mask_all_ones: caller asserts the mask is all ones (connector output, LTXTextEncoder.swift:622-626). */
int ltx_dit_forward_dev(ltx_ctx* ctx, const uint16_t* latent, const uint16_t* context, const float* timesteps,
                        const int32_t* mask, int mask_all_ones, int B, int F, int H, int W, int S,
                        uint64_t ctx_version, float* velocity);
/* Sequence-parallel forward of ONE sample over sp_world ranks, one process per GPU (no counterpart in the single-device reference;
 * SURVEY 8(e) "single video on 8 GPUs", 8(f) item 4). Rank sp_rank owns tokens [sp_rank*Tn, (sp_rank+1)*Tn) of the F*H*W grid,
 * Tn = F*H*W / sp_world (must divide, Tn % 8 == 0): `latent` is [1][Tn][in_channels] and `velocity` [1][Tn][out_channels], that
 * rank's rows only; context, timestep and mask are the full ones on every rank. Everything per-token is local; each block's
 * self-attention all-gathers its K rows and V^T block through `gather`, called 2 x num_layers times per forward:
 *   gather(user, send, recv, bytes): all-gather `bytes` from every rank into recv = [sp_world][bytes] in rank order. DEVICE pointers.
 *   It must either enqueue the collective on the context's stream (RCCL on the stream given to ltx_ctx_set_stream) or finish it
 *   before returning (then synchronise that stream first), and return 0; any other value aborts the forward with
 *   LTX_ERR_GENERATION_FAILED (the kernels behind a failed gather would read unfilled buffers). Every rank must call the forward
 *   with the same arguments. gather NULL = the context's own transport (ltx_dist_init: RCCL; ltx_dist_set_transport: host
 *   callback), whose rank/world must equal sp_rank/sp_world.
 * DEVICE pointers, asynchronous on the context stream when the transport is. */
typedef int (*ltx_allgather_fn)(void* user, const void* send, void* recv, long bytes);
int ltx_dit_forward_sp_dev(ltx_ctx* ctx, const uint16_t* latent, const uint16_t* context, const float* timesteps,
                           const int32_t* mask, int mask_all_ones, int F, int H, int W, int S, uint64_t ctx_version,
                           int sp_rank, int sp_world, ltx_allgather_fn gather, void* user, float* velocity);
/* setCrossAttentionScale (LTXTransformer.swift:497); block range inclusive, (0,-1) = all blocks. */
int ltx_dit_set_cross_attn_scale(ltx_ctx* ctx, float scale, int first_block, int last_block);
/* setSTGSkipFlags / clearSTGSkipFlags (LTXTransformer.swift:512-526) */
int ltx_dit_set_stg(ltx_ctx* ctx, const int* blocks, int n_blocks, int skip_self_attention, int skip_feed_forward);
int ltx_dit_clear_stg(ltx_ctx* ctx);

/* ------------------------------------------------------------------------------------------------------------
 * Video VAE decoder
 * ---------------------------------------------------------------------------------------------------------- */
/* Replaces VideoDecoder() + LTXWeightLoader.loadVAEWeights/applyVAEWeights + parseVAEConfig
 * (LTXPipeline.swift:338-346, ModelDownloader.swift:583-594,648-658,808-899,1022-1064). config_json NULL = look for
 * `config.json` next to the weights; its "timestep_conditioning" flag selects the conditioned decode. */
int ltx_vae_load(ltx_ctx* ctx, const char* safetensors_path, const char* config_json);
/* Random-init decoder of the reference architecture, generated on device (bench / property tests). */
int ltx_vae_init_synthetic(ltx_ctx* ctx, uint64_t seed, int timestep_conditioning);
int ltx_vae_unload(ltx_ctx* ctx);
/* VideoDecoder.timestepConditioning (VideoDecoder.swift:299) of the loaded model: 1/0, <0 on error. */
int ltx_vae_timestep_conditioning(const ltx_ctx* ctx);
/* Replaces decodeVideo(latent:decoder:timestep:temporalTileSize:temporalTileOverlap:) (VideoDecoder.swift:466).
 *   latent  [1][128][F][H][W] f32 (normalised latent, as the denoise loop leaves it)
 *   has_timestep/timestep: pass (1, 0.05) iff the model is timestep-conditioned (LTXPipeline.swift:1004); then
 *           `noise` (same shape as latent, N(0,1)) is REQUIRED - the reference draws it from the global MLX RNG
 *           (VideoDecoder.swift:369), here every noise tensor is an explicit input.
 *   tile/overlap: MemoryOptimizationConfig.vaeTemporalTileSize/Overlap (0 = untiled)
 *   frames_out (n_frames, 32H, 32W, 3) f32 in [0,1]; frames_cap = capacity in floats; *n_frames_out = frames written
 *           (8(F-1)+1 untiled; see ltx_vae_tile_plan for tiled counts, e.g. 26 latent frames, tile 8 -> 180).
 * HOST pointers. */
int ltx_vae_decode(ltx_ctx* ctx, const float* latent, int F, int H, int W, int has_timestep, float timestep,
                   const float* noise, int tile, int overlap, float* frames_out, long frames_cap, int* n_frames_out);
/* Same with DEVICE pointers (n_frames_out stays a host pointer); asynchronous on the context stream. */
int ltx_vae_decode_dev(ltx_ctx* ctx, const float* latent, int F, int H, int W, int has_timestep, float timestep,
                       const float* noise, int tile, int overlap, float* frames_out, long frames_cap,
                       int* n_frames_out);
/* One Conv3dFull (VideoConvolution.swift:202-348) on a channels-last tensor, exposed for parity tests:
 * x [F][H][W][Cin] bf16 (device), w [Cout][27][Cin] bf16 (tap = (kt*3+kh)*3+kw), bias [Cout] f32 -> out [F][H][W][Cout] f32.
 * causal: 0 replicate-pad T on both sides, 1 repeat the first frame twice. */
int ltx_op_conv3d(ltx_ctx* ctx, const uint16_t* x, int F, int H, int W, int Cin, const uint16_t* w, const float* bias,
                  int Cout, int causal, float* out);

/* ------------------------------------------------------------------------------------------------------------
 * Two-stage generation glue (generateVideoTwoStage, LTXPipeline.swift:2420-2741)
 * ---------------------------------------------------------------------------------------------------------- */
/* Replaces loadSpatialUpscaler(from:) (SpatialUpscaler.swift:271-349); mid_channels is detected from the file. */
int ltx_upscaler_load(ltx_ctx* ctx, const char* safetensors_path);
int ltx_upscaler_unload(ltx_ctx* ctx);
/* Replaces upsampleLatents(_:upscaler:latentMean:latentStd:) (SpatialUpscaler.swift:352-379; call site
 * LTXPipeline.swift:2595-2618): denormalise with the VAE's mean_of_means/std_of_means (the VAE must be loaded),
 * SpatialUpscaler forward, renormalise. latent [1][128][F][H][W] f32 -> out [1][128][F][2H][2W] f32. HOST pointers. */
int ltx_upscale_latent(ltx_ctx* ctx, const float* latent, int F, int H, int W, float* out);
int ltx_upscale_latent_dev(ltx_ctx* ctx, const float* latent, int F, int H, int W, float* out);
/* adainFilterLatent (LatentUtils.swift:201-227): per-channel mean/std of `latent` [1][C][n] matched to those of
 * `reference` [1][C][n_ref] (population variance, +1e-8 on the std), blended by factor. In place. HOST pointers. */
int ltx_adain_filter_latent(ltx_ctx* ctx, float* latent, long n_per_channel, const float* reference,
                            long n_ref_per_channel, int channels, float factor);
int ltx_adain_filter_latent_dev(ltx_ctx* ctx, float* latent, long n_per_channel, const float* reference,
                                long n_ref_per_channel, int channels, float factor);
/* Stage-2 re-noise (LTXPipeline.swift:2644-2647): latent = sigma*noise + (1-sigma)*latent. DEVICE pointers. */
int ltx_renoise_dev(ltx_ctx* ctx, float* latent, const float* noise, float sigma, long n);

/* One forward with PER-TOKEN timesteps (image-to-video; LTXTransformer.prepareTimestep, LTXTransformer.swift:105-124):
 * token_timesteps [B][T] f32 sigmas. The adaLN path is evaluated once per distinct value of a batch row (at most 8 distinct
 * (batch, value) pairs in total - I2V has two per row: 0 for frame 0 and sigma elsewhere). Other arguments as
 * ltx_dit_forward. HOST pointers. */
int ltx_dit_forward_tokens(ltx_ctx* ctx, const uint16_t* latent, const uint16_t* context, const float* token_timesteps,
                           const int32_t* mask, int B, int F, int H, int W, int S, float* velocity);

/* ------------------------------------------------------------------------------------------------------------
 * Frame export helpers (the part that is verifiable here; VideoExporter.swift:563-580). Pure host code.
 * ---------------------------------------------------------------------------------------------------------- */
/* MLX-compatible initial noise (replaces generateNoise, LatentUtils.swift:69-83 = MLXRandom.seed(seed) then
 * MLXRandom.normal(shape, float32)): writes the `draw_index`-th keyless normal draw after seeding (0 = the first) as n f32
 * values. mlx-swift is not part of the reference tree: the generator is restated from MLX's published algorithm (threefry2x32-20
 * counter hash, key split per draw, uniform -> sqrt(2)*erfinv). The hash is pinned by the Random123 known-answer vectors
 * (ltx_threefry2x32); the bits -> normal pipeline could not be checked against an MLX run. Pure host code. */
int ltx_mlx_random_normal(uint64_t seed, int draw_index, float* out, long n);
void ltx_threefry2x32(const uint32_t key[2], const uint32_t ctr[2], uint32_t out[2]);
/* The key of the `draw_index`-th keyless draw after MLXRandom.seed(seed): draw_index + 1 key splits (KeySequence::next). The host
 * generator above and the device generator below share it. draw_index < 0 or a NULL key_out: LTX_ERR_INVALID_CONFIGURATION. Pure host. */
int ltx_mlx_draw_key(uint64_t seed, int draw_index, uint32_t key_out[2]);
/* One draw of ltx_op_mlx_normal_group: n values from `key` into dst (DEVICE), each multiplied by `scale` in one more f32 multiply after
 * sqrt(2) * erfinv(u) - the reference's separate `noise * sigmas[0]` (LTXPipeline.swift:1243, :1597-1598); scale = 1 leaves the bits of
 * the draw. raw_bits != 0: dst receives the n uint32 words of the hash instead (the integer half of the pipeline, for tests). */
typedef struct ltx_noise_job {
    uint32_t key[2];
    float* dst;
    long n;
    float scale;
    int raw_bits;
} ltx_noise_job;
/* The MLX-compatible normal draws of a run on the device, in ONE launch for up to 64 jobs (more are sent 64 at a time): replaces the
 * MLXRandom.normal / generateNoise calls of a generation (LTXPipeline.swift:1225-1236, :1291, :1572-1581, :1629, :1730-1734, :1766),
 * which ltx_mlx_random_normal makes on one host thread. One thread per counter pair of mlx_random_bits; the bits -> normal tail is the
 * host's operation by operation (correctly rounded division, separate multiply and add, fmaf, logf), so a value differs from
 * ltx_mlx_random_normal only where the device's logf and the host's differ in the last place. jobs is a HOST array, every dst a
 * DEVICE pointer; asynchronous on the context stream. n_jobs < 0, n < 0, n >= 2^31 (the counters are 32 bit) or a NULL dst with n > 0:
 * LTX_ERR_INVALID_CONFIGURATION before any launch, nothing written. Empty jobs and n_jobs == 0 are valid and do nothing. */
int ltx_op_mlx_normal_group(ltx_ctx* ctx, const ltx_noise_job* jobs, int n_jobs);
/* ltx_mlx_random_normal into DEVICE memory, times scale: ltx_mlx_draw_key and one job of ltx_op_mlx_normal_group. */
int ltx_mlx_random_normal_dev(ltx_ctx* ctx, uint64_t seed, int draw_index, float* out_dev, long n, float scale);

/* tensorToImages' pixel conversion: out = uint8(clip(x, 0, 1) * 255), f32 multiply then truncation toward zero. */
int ltx_frames_to_u8(const float* frames, long n, uint8_t* out);
/* Writes one (H, W, 3) uint8 frame as a PNG (8-bit RGB, stored/uncompressed deflate blocks - no external codec). The
 * reference hands CGImages to AVAssetWriter (Apple-only); an MP4 muxer is outside this library. */
int ltx_write_png(const char* path, const uint8_t* rgb, int width, int height);

/* ------------------------------------------------------------------------------------------------------------
 * VAE encoder (VideoEncoder.swift:211-312, call site encodeImage LTXPipeline.swift:1902-1932): turns the
 * image-to-video conditioning image into the latent that ltx_denoise_options.cond_latent takes.
 * ---------------------------------------------------------------------------------------------------------- */
/* Replaces loadVAEEncoder (LTXPipeline.swift:1871-1885): reads the `encoder.*` tensors of the VAE file (key rules
 * ModelDownloader.swift:1222-1283). channel_base 0 = reference (128 -> 128..2048 channels). */
int ltx_vae_encoder_load(ltx_ctx* ctx, const char* safetensors_path, int channel_base);
int ltx_vae_encoder_init_synthetic(ltx_ctx* ctx, int channel_base, unsigned long seed);
int ltx_vae_encoder_unload(ltx_ctx* ctx);
/* pixels [1][3][T][H][W] f32 (the reference feeds images scaled to [-1,1]; image loading/resizing stays with the caller) ->
 * latent [1][128][T'][H/32][W/32] f32, T' = ltx_vae_encoder_latent_frames(T). normalize != 0 applies
 * (latent - mean_of_means) / std_of_means with the loaded decoder's statistics (LTXPipeline.swift:1920-1927; the decoder must
 * be loaded). HOST pointers. */
int ltx_vae_encode(ltx_ctx* ctx, const float* pixels, int T, int H, int W, int normalize, float* latent);
/* Same with DEVICE pointers, asynchronous on the context stream. */
int ltx_vae_encode_dev(ltx_ctx* ctx, const float* pixels, int T, int H, int W, int normalize, float* latent);
int ltx_vae_encoder_latent_frames(int T);
/* mapVAEEncoderWeights (ModelDownloader.swift:1222-1283): length of the module key, 0 if the key is not an encoder tensor. */
int ltx_map_vae_encoder_key(const char* file_key, char* out, int cap);

/* ------------------------------------------------------------------------------------------------------------
 * Audio decode leg (decodeAudio, Vocoder.swift:325-361): audio latent -> AudioVAE.decode -> stereo mel -> LTX2Vocoder -> 24 kHz
 * stereo waveform. The dual (video + audio) transformer that PRODUCES the audio latent is "Dual video + audio model" below, and
 * ltx_dual_denoise is the joint loop around it: its audio latent is this leg's input. Precision: weights rounded to bf16 at load, bf16 conv operands, f32 accumulation, f32 residual streams.
 * ---------------------------------------------------------------------------------------------------------- */
/* Replaces AudioVAE() + loadAudioVAEWeights / applyAudioVAEWeights (ModelDownloader.swift:1116-1158): keeps `decoder.*`, `latents_mean`
 * and `latents_std`, drops everything else; Conv2d weights are PyTorch (out, in, kh, kw) under `...conv.weight`. Channel counts come
 * from the tensor shapes (multiples of 32). Kept tensors that are no parameter (or have the wrong rank) count as unmatched, absent
 * biases / statistics as missing (ltx_load_report); an absent convolution weight fails with LTX_ERR_WEIGHT_LOADING_FAILED. */
int ltx_audio_vae_load(ltx_ctx* ctx, const char* safetensors_path);
/* Random-init decoder of the reference architecture (AudioVAE.swift:265-323); base_channels 0 = 128. */
int ltx_audio_vae_init_synthetic(ltx_ctx* ctx, int base_channels, uint64_t seed);
int ltx_audio_vae_unload(ltx_ctx* ctx);
/* Replaces LTX2Vocoder() + loadVocoderWeights / applyVocoderWeights (ModelDownloader.swift:1160-1194, Vocoder.swift:273-311): Conv1d
 * weights are (out, in, k), `upsamplers.N.weight` is (in, out, k). Reporting as above. */
int ltx_vocoder_load(ltx_ctx* ctx, const char* safetensors_path);
/* Random-init vocoder (Vocoder.swift:144-211); hidden_channels 0 = 1024. */
int ltx_vocoder_init_synthetic(ltx_ctx* ctx, int hidden_channels, uint64_t seed);
int ltx_vocoder_unload(ltx_ctx* ctx);
/* Replaces AudioVAE.decode (AudioVAE.swift:407-456): latent [8][T][16] f32 (normalised, as the denoise loop leaves it) ->
 * mel [2][max(4T-3, 1)][64] f32. HOST pointers. */
int ltx_audio_vae_decode(ltx_ctx* ctx, const float* latent, int T, float* mel);
/* Same with DEVICE pointers, asynchronous on the context stream. */
int ltx_audio_vae_decode_dev(ltx_ctx* ctx, const float* latent, int T, float* mel);
/* Replaces LTX2Vocoder.callAsFunction (Vocoder.swift:217-266): mel [2][T_mel][64] f32 -> waveform [2][240 * T_mel] f32 in (-1, 1).
 * HOST pointers. */
int ltx_vocoder_forward(ltx_ctx* ctx, const float* mel, int T_mel, float* waveform);
int ltx_vocoder_forward_dev(ltx_ctx* ctx, const float* mel, int T_mel, float* waveform);
/* Replaces decodeAudio(latents:audioVAE:vocoder:) (Vocoder.swift:325-361): the two chained, the mel never leaves the device.
 * latent [8][T][16] f32 -> waveform [2][ltx_audio_sample_count(T)] f32. HOST pointers. */
int ltx_audio_decode(ltx_ctx* ctx, const float* latent, int T, float* waveform);
int ltx_audio_decode_dev(ltx_ctx* ctx, const float* latent, int T, float* waveform);
/* computeAudioLatentFrames (LTXPipeline.swift:530-534): round(f32(video_frames / fps) * f32(16000 / 160 / 4)). Pure host code. */
int ltx_audio_latent_frames(int video_frames, float fps);
/* max(4T - 3, 1) (AudioVAE.swift:413) and 240 times that (Vocoder.swift:130); the vocoder's output rate, 24000 (Vocoder.swift:153). */
int ltx_audio_mel_frames(int T);
long ltx_audio_sample_count(int T);
int ltx_audio_sample_rate(void);
/* AudioExporter.exportToWAV (AudioExporter.swift:19-92): waveform [2][n] f32 -> gain, clamp to [-1, 1], int16 by truncation toward
 * zero of x * 32767.0f, interleaved L/R behind the 44-byte PCM header. Pure host code. */
int ltx_write_wav(const char* path, const float* waveform, long n, int sample_rate, float gain);

/* ------------------------------------------------------------------------------------------------------------
 * Audio / cross-modal attention: LTXAttention at 32 heads x 64 (LTXConfig.swift:134-135), the module the dual video + audio block
 * adds four times to the video block - audio self-attention, audio text cross-attention, a2v and v2a cross-modal attention
 * (LTX2TransformerBlock.swift:133-163,207-270) - with the RoPE tables of its real-valued 1-D positions. A context holds up to four
 * modules, addressed by index 0 .. 3. The block wiring is "Dual video + audio transformer blocks" below; the audio stream's adaLN
 * embedders and the cross-modal scale-shift embedders are "Dual video + audio model", the joint denoise loop is ltx_dual_denoise.
 * ---------------------------------------------------------------------------------------------------------- */
/* createAudioPositionGrid (LTXRoPE.swift:627-655; hop 160, rate 16000, scale 4, causal offset 1, f32 arithmetic): out[i] = seconds of
 * the middle of audio latent frame i, i < T_a (0.005, 0.03, 0.07, ...). Pure host code. */
int ltx_audio_positions(int T_a, float* out);
/* The temporal coordinate of every video token in token order: row 0 of createPositionGrid (LTXRoPE.swift:552-610), which the
 * cross-modal RoPE uses alone (LTX2Transformer.swift:205-209). out [F*H*W]. Pure host code. */
int ltx_video_temporal_positions(int F, int H, int W, float fps, float* out);
/* precomputeFreqsCis, f64 path, for ONE position dimension (LTXRoPE.swift:375-490 as LTX2Transformer.swift:176-184,210-233 call it):
 * dim/2 frequencies theta^(i/(n-1)) * pi/2 times 2 * positions[t] / max_pos - 1 (max_pos 20 in the dual model); cos/sin [T][dim/2] f32,
 * no padding slots. Head h of a 64-wide head owns columns 32h .. 32h+31. Pure host code. */
int ltx_rope_tables_positions(const float* positions, int T, int dim, float theta, int max_pos, float* cos_out, float* sin_out);
/* Random-init module (LTXAttention.init, LTXAttention.swift:130-158): to_q [heads*64][query_dim], to_k / to_v [heads*64][context_dim],
 * to_out [query_dim][heads*64], biases, q_norm / k_norm [heads*64]. context_dim 0 = query_dim. Dims are multiples of 64. */
int ltx_attn_module_init_synthetic(ltx_ctx* ctx, int index, int query_dim, int context_dim, int heads, uint64_t seed);
/* Reads `<key_prefix>to_q.weight` ... from a safetensors file, e.g. key_prefix "transformer_blocks.0.audio_to_video_attn." (module
 * names to_out / q_norm / k_norm or the checkpoint's to_out.0 / norm_q / norm_k, ModelDownloader.swift:756-803). query_dim and
 * context_dim come from the file; heads * 64 must be the file's inner dim (LTX_ERR_INVALID_CONFIGURATION otherwise). */
int ltx_attn_module_load(ltx_ctx* ctx, int index, const char* safetensors_path, const char* key_prefix, int heads);
int ltx_attn_module_unload(ltx_ctx* ctx, int index);
/* One resident parameter of module `index` as f32 ("to_q.weight", "to_q.bias", ..., "q_norm.weight", "k_norm.weight"): returns its
 * element count (out NULL: the count only), or a negative ltx_status. Test seam, as ltx_dit_export_param. */
long ltx_attn_module_export_param(ltx_ctx* ctx, int index, const char* name, float* out, long cap);
/* Replaces LTXAttention.callAsFunction (LTXAttention.swift:160-218) at head dim 64. x [B][Tq][query_dim] f32; context
 * [B][Tk][context_dim] f32, or bf16 with context_bf16 != 0 (the text context: K / V then round to bf16 as the reference's bf16
 * Linears do), or NULL = self-attention (Tk == Tq). q_cos / q_sin [q_table_rows][heads*32] f32 rotate q; k_cos / k_sin
 * [k_table_rows][heads*32] rotate k; with only the q tables given k is rotated with them (the reference's `kPe ?? pe`); all NULL = no
 * RoPE. key_bias [B][Tk] f32 additive in the reference's units ((1 - mask) * -10000) or NULL. out [B][Tq][query_dim] f32. DEVICE
 * pointers, asynchronous on the context stream. An empty index is LTX_ERR_MODEL_NOT_LOADED; tables with fewer rows than tokens are
 * LTX_ERR_INVALID_CONFIGURATION; both are reported before any launch. */
int ltx_attn_module_forward_dev(ltx_ctx* ctx, int index, const float* x, const void* context, int context_bf16, int B, int Tq, int Tk,
                                const float* q_cos, const float* q_sin, int q_table_rows, const float* k_cos, const float* k_sin,
                                int k_table_rows, const float* key_bias, float* out);

/* ------------------------------------------------------------------------------------------------------------
 * Dual video + audio transformer blocks: LTX2TransformerBlock (LTX2TransformerBlock.swift:174-297) as a loadable stack of L blocks
 * with a forward of its own. It takes what LTX2Transformer.callAsFunction hands its blocks and returns both residual streams. The
 * embedders that make the modulation rows (audio_adaln_single, av_ca_*), the patchify / output heads and the caption projections are
 * "Dual video + audio model" below, which owns a stack of its own; the joint denoise loop is ltx_dual_denoise; the CLI's --audio path
 * is not part of this library yet. The audio modulation rows are one per batch element. The video modulation rows are one per (batch
 * element, timestep group): n_groups and video_row_map, as ltx_dit_forward_tokens groups them - the reference's per-token form
 * (image-to-video, LTX2Transformer.swift:285-312) with each distinct row built once. A context holds one stack.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct ltx_dual_block_config {
    int num_layers;         /* 48 */
    int video_heads;        /* 32 heads x 128 */
    int video_dim;          /* 4096 = video_heads * 128 */
    int audio_heads;        /* 32 heads x 64 */
    int audio_dim;          /* 2048 = audio_heads * 64 */
    int video_context_dim;  /* width of the video text context (videoCrossAttentionDim, 4096); a multiple of 64 */
    int audio_context_dim;  /* width of the audio text context (audioCrossAttentionDim, 2048); a multiple of 64 */
    float rope_theta;       /* 10000 */
    int max_pos[3];         /* video 3-D RoPE: {20, 2048, 2048} */
    int audio_max_pos;      /* audio and cross-modal 1-D RoPE: 20 */
    float fps;              /* 24: temporal coordinates of the video tokens */
    float norm_eps;         /* 1e-6 */
} ltx_dual_block_config;
/* Filled with the reference defaults (LTXConfig.swift:83-177 and its audio fields :126-140). */
void ltx_dual_block_config_default(ltx_dual_block_config* cfg);
/* Random-init stack (LTX2TransformerBlock.init, LTX2TransformerBlock.swift:98-170): Linear weights N(0, 0.02^2), biases N(0, 0.01^2),
 * q / k norm weights 1 + N(0, 0.02^2), the four scale-shift tables N(0, 0.02^2), all bf16 values. video_dim != video_heads * 128 or
 * audio_dim != audio_heads * 64: LTX_ERR_INVALID_CONFIGURATION. */
int ltx_dual_blocks_init_synthetic(ltx_ctx* ctx, const ltx_dual_block_config* cfg, uint64_t seed);
/* Replaces the block part of loadTransformerWeights(includeAudio: true) (ModelDownloader.swift:605-639): tensors under
 * `transformer_blocks.{first_block + i}.` fill block i, i < num_blocks (cfg->num_layers is ignored). Keys in the module's spelling or
 * the checkpoint's (to_out.0, norm_q / norm_k, ff.net.0.proj / ff.net.2, mapped as mapTransformerKey does, ModelDownloader.swift:
 * 756-803; scale_shift_table_a2v_ca_video / _audio are spelled alike on both sides). ltx_load_report: tensors applied / 0 / tensors of
 * those blocks that are no parameter (the RMSNorm weights: none is applied). A parameter the file lacks: LTX_ERR_WEIGHT_LOADING_FAILED,
 * and the context holds no stack. */
int ltx_dual_blocks_load(ltx_ctx* ctx, const char* safetensors_path, const ltx_dual_block_config* cfg, int first_block, int num_blocks);
int ltx_dual_blocks_unload(ltx_ctx* ctx);
/* One resident parameter as f32 by its module key with blocks numbered from 0 ("transformer_blocks.0.audio_attn1.to_q.weight",
 * "transformer_blocks.1.scale_shift_table_a2v_ca_audio", ...): its element count (out NULL: the count only) or a negative ltx_status.
 * Test seam, as ltx_dit_export_param. */
long ltx_dual_blocks_export_param(ltx_ctx* ctx, const char* name, float* out, long cap);
/* Arguments of ltx_dual_blocks_forward_dev; starts with its own size as ltx_denoise_options does (LTX_DUAL_FORWARD_ARGS_INIT). All
 * pointers are DEVICE pointers. */
typedef struct ltx_dual_forward_args {
    uint32_t struct_size;          /* sizeof(ltx_dual_forward_args) in the caller's translation unit */
    int B, F, H, W;                /* batch; latent frames / height / width: F*H*W video tokens in (f, h, w) order */
    int T_a;                       /* audio tokens */
    int S;                         /* text tokens of both contexts */
    float* x_video;                /* [B][F*H*W][video_dim] f32, updated in place (TransformerArgs.x) */
    float* x_audio;                /* [B][T_a][audio_dim] f32, updated in place (AudioTransformerArgs.x) */
    const uint16_t* context_video; /* [B][S][video_context_dim] bf16 (TransformerArgs.context) */
    const uint16_t* context_audio; /* [B][S][audio_context_dim] bf16 */
    const float* key_bias_video;   /* [B][S] f32 additive, (1 - mask) * -10000, or NULL (contextMask) */
    const float* key_bias_audio;
    const float* temb_video;       /* [B*n_groups][6][video_dim] f32 (TransformerArgs.timesteps) */
    const float* temb_audio;       /* [B][6][audio_dim] f32 */
    const float* cross_video_ss;   /* [B*n_groups][5][video_dim] f32 (crossVideoScaleShift) */
    const float* cross_audio_ss;   /* [B][5][audio_dim] f32 (crossAudioScaleShift) */
    uint32_t phase_mask;           /* 0: all eight phases. Else bit p-1 runs phase p of every block alone - a measurement seam */
    int n_groups;                  /* timestep groups of the video stream per batch element (1); B * n_groups <= 8. Read when struct_size
                                      covers it, else 1 */
    const int32_t* video_row_map;  /* [B*F*H*W] int32: video token b*F*H*W + t reads modulation row video_row_map[..] = b*n_groups +
                                      group(b, t); entries are the caller's contract. NULL with n_groups == 1: row b */
} ltx_dual_forward_args;
#define LTX_DUAL_FORWARD_ARGS_INIT {sizeof(ltx_dual_forward_args), 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0}
/* Replaces the block loop of LTX2Transformer.callAsFunction: L x LTX2TransformerBlock.callAsFunction (LTX2TransformerBlock.swift:
 * 174-297) on both streams in place. The four RoPE table sets (LTX2Transformer.swift:136-236) are made inside from (F, H, W) and T_a and
 * cached. Asynchronous on the context stream. No stack: LTX_ERR_MODEL_NOT_LOADED; a struct_size that does not cover the fields up to
 * cross_audio_ss, B outside 1 .. 8, a dimension < 1 or a NULL stream / context / modulation pointer: LTX_ERR_INVALID_CONFIGURATION; so are
 * n_groups < 1, B * n_groups > 8 and n_groups > 1 without a map. Every check comes before the first launch: a refused call writes nothing. */
int ltx_dual_blocks_forward_dev(ltx_ctx* ctx, const ltx_dual_forward_args* args);
/* One job of ltx_op_norm_mod2: rows f32 [rows][ldx] -> two bf16 outputs [rows][ldo]. */
typedef struct ltx_norm_mod2_job {
    const float* x;
    long ldx;
    const float* scale0; /* [B][mod_bstride] f32, row b = row_map ? row_map[row] : row / rows_per_batch; NULL with shift0 NULL: the plain norm */
    const float* shift0;
    const float* scale1;
    const float* shift1;
    long mod_bstride;
    int rows_per_batch;
    uint16_t* out0;
    uint16_t* out1;
    long ldo;
    int rows; /* 0: the job is empty */
    int D;    /* D % 4 == 0, <= 8192 */
    const int32_t* row_map; /* DEVICE [rows] int32 or NULL: the modulation row of each row (per-token timestep groups) */
} ltx_norm_mod2_job;
/* Kernel hook: the cross-modal norms of the dual block in one launch (audioToVideoNorm / videoToAudioNorm and their four modulations,
 * LTX2TransformerBlock.swift:246-263). out0 = rmsnorm(x) * (1 + scale0) + shift0, out1 likewise with (scale1, shift1); each bit-equal
 * to ltx_op_norm_mod_ex with the same operands and the same row map. Either job may be NULL or empty. Bad arguments are refused before the launch. */
int ltx_op_norm_mod2(ltx_ctx* ctx, const ltx_norm_mod2_job* video, const ltx_norm_mod2_job* audio, float eps);

/* ------------------------------------------------------------------------------------------------------------
 * Dual video + audio model: LTX2Transformer.callAsFunction (LTX2Transformer.swift:254-392) - two latents, two text contexts and two
 * timestep vectors in, two velocities out. The model owns a block stack of its own (as "Dual video + audio transformer blocks" above)
 * and the top-level modules of LTX2Transformer.swift:28-48: the two patchify Linears, the six AdaLayerNormSingle embedders, the two
 * caption projections, the two output tables and the two output Linears. A context holds one model, in a slot of its own: loading it
 * does not disturb the ltx_dual_blocks_* stack, and the reverse. Timesteps are one value per batch element and stream in
 * ltx_dual_model_forward_dev; ltx_dual_model_forward_groups_dev takes video timesteps per (batch element, timestep group) and a token ->
 * group map, which is the reference's per-token form (image-to-video, LTX2Transformer.swift:285-312). The CLI's --audio path is not
 * part of this library yet. Within one prompt the text side of a forward does not change: ltx_dual_model_prepare_text_dev computes it once (both
 * caption projections, both mask biases and, for every block, the normed K and the V^T of the two text cross-attentions) and a forward
 * with text_cache != 0 reads it. The joint denoise loop is ltx_dual_denoise below.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct ltx_dual_model_config {
    ltx_dual_block_config blocks;     /* video_context_dim == video_dim, audio_context_dim == audio_dim */
    int in_channels;                  /* 128 */
    int out_channels;                 /* 128 */
    int audio_in_channels;            /* 128 */
    int audio_out_channels;           /* 128 */
    int caption_channels;             /* 3840 */
    float timestep_scale_multiplier;  /* 1000 */
} ltx_dual_model_config;
/* Filled with the reference defaults (LTXConfig.swift:83-177). */
void ltx_dual_model_config_default(ltx_dual_model_config* cfg);
/* Random-init model (LTX2Transformer.init, LTX2Transformer.swift:59-121) with the distributions of ltx_dual_blocks_init_synthetic for
 * the blocks and the top-level parameters alike (the output tables N(0, 0.02^2) rather than the reference's zeros, so that a test sees
 * them). A bad configuration: LTX_ERR_INVALID_CONFIGURATION. */
int ltx_dual_model_init_synthetic(ltx_ctx* ctx, const ltx_dual_model_config* cfg, uint64_t seed);
/* Replaces loadTransformerWeights(includeAudio: true) (ModelDownloader.swift:605-639). Keys in the module's spelling or in any spelling
 * mapTransformerKey(includeAudio: true) maps onto it (ModelDownloader.swift:756-803): proj_in., time_embed.emb.timestep_embedder.,
 * time_embed.linear., the general .emb.timestep_embedder. flattening, and the block spellings of ltx_dual_blocks_load.
 * ltx_load_report: tensors applied / 0 / tensors that are no parameter. A parameter the file lacks: LTX_ERR_WEIGHT_LOADING_FAILED, and
 * the context holds no model. */
int ltx_dual_model_load(ltx_ctx* ctx, const char* safetensors_path, const ltx_dual_model_config* cfg);
int ltx_dual_model_unload(ltx_ctx* ctx);
/* One resident parameter as f32 by its module key ("adaln_single.emb.linear_1.weight", "audio_scale_shift_table", ...; block
 * parameters under "transformer_blocks.{i}." as ltx_dual_blocks_export_param names them): its element count (out NULL: the count only)
 * or a negative ltx_status. Test seam, as ltx_dit_export_param. */
long ltx_dual_model_export_param(ltx_ctx* ctx, const char* name, float* out, long cap);
/* quantize(model: ltx2, groupSize: 64, bits: 8 | 4) on the resident dual model (LTXPipeline.swift:487-492, the audio path's use of
 * LTXQuantizationConfig.memoryEfficient / .minimal, LTXQuantizationConfig.swift:19-62): every Linear weight of the model and of its
 * blocks becomes codes + bf16 group scale / bias (group 64 along `in`) and the bf16 weights are RELEASED, as ltx_dit_quantize does
 * for the DiT. Forwards, the joint loop and the two-stage driver run unchanged on the quantised model; ltx_dual_model_export_param
 * then returns the de-quantised value bf16(q * scale + bias). The text cache is dropped (ltx_dual_model_prepare_text_dev fills it
 * again). bits outside {8, 4}, group_size != 64 or an already quantised model: LTX_ERR_INVALID_CONFIGURATION, nothing changed. */
int ltx_dual_model_quantize(ltx_ctx* ctx, int bits, int group_size);
/* ltx_dit_memory_info for the dual model (what MLX's memory statistics would show the host, LTXPipeline.swift:3176-3187): the bf16
 * Linear weights (0 once quantised), the codes + group scales / biases, the one de-quantisation scratch matrix, and everything else
 * the model keeps (biases, norm weights, tables; the text cache). All zero when no dual model is loaded. Any pointer may be NULL. */
int ltx_dual_model_memory_info(ltx_ctx* ctx, long* bf16_weight_bytes, long* quantised_weight_bytes, long* scratch_bytes, long* other_bytes);
/* Arguments of ltx_dual_model_forward_dev; starts with its own size (LTX_DUAL_MODEL_FORWARD_ARGS_INIT). All pointers are DEVICE
 * pointers. */
typedef struct ltx_dual_model_forward_args {
    uint32_t struct_size;            /* sizeof(ltx_dual_model_forward_args) in the caller's translation unit */
    int B, F, H, W;                  /* batch; latent frames / height / width: F*H*W video tokens in (f, h, w) order */
    int T_a;                         /* audio tokens */
    int S;                           /* text tokens of both contexts */
    const uint16_t* video_latent;    /* [B][F*H*W][in_channels] bf16 */
    const uint16_t* audio_latent;    /* [B][T_a][audio_in_channels] bf16 */
    const uint16_t* video_context;   /* [B][S][caption_channels] bf16 */
    const uint16_t* audio_context;   /* [B][S][caption_channels] bf16 */
    const float* video_timesteps;    /* [B] f32, sigma (unscaled) */
    const float* audio_timesteps;    /* [B] f32 */
    const int32_t* video_mask;       /* [B][S] int32 or NULL (videoContextMask) */
    const int32_t* audio_mask;       /* [B][S] int32 or NULL */
    float* video_velocity;           /* [B][F*H*W][out_channels] f32 */
    float* audio_velocity;           /* [B][T_a][audio_out_channels] f32 */
    int ungrouped;                   /* measurement seam: non-zero runs the timestep path as 18 ltx_op_gemv_f32-style launches instead of
                                        three grouped ones; the same bits. On a quantised model 1 = 18 one-job launches of the grouped
                                        kernel on codes, 2 = per Linear de-quantise + ltx_op_gemv_f32 (the same bits again) */
    int text_cache;                  /* non-zero: read the text side from the cache ltx_dual_model_prepare_text_dev filled; the context
                                        and mask pointers are not read (they may be NULL). The same bits as 0, which recomputes it */
} ltx_dual_model_forward_args;
#define LTX_DUAL_MODEL_FORWARD_ARGS_INIT {sizeof(ltx_dual_model_forward_args), 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}
/* Replaces LTX2Transformer.callAsFunction (LTX2Transformer.swift:254-392). Asynchronous on the context stream. No model:
 * LTX_ERR_MODEL_NOT_LOADED; a struct_size that does not cover the fields up to audio_velocity, B outside 1 .. 8, a dimension < 1 or a
 * NULL latent / context / timestep / velocity pointer: LTX_ERR_INVALID_CONFIGURATION. text_cache (read only when struct_size covers
 * it) without a cache of this call's (B, S): LTX_ERR_INVALID_CONFIGURATION. Every check comes before the first launch: a refused call
 * writes nothing. */
int ltx_dual_model_forward_dev(ltx_ctx* ctx, const ltx_dual_model_forward_args* args);
/* The same forward with timestep GROUPS on the video stream (image-to-video: frame-0 tokens at 0, the rest at sigma): the tokens of
 * batch element b are partitioned into n_groups groups, args->video_timesteps is read as [B][n_groups], and video_row_map (DEVICE,
 * [B*F*H*W] int32) holds b*n_groups + group(b, t) for token t of batch element b; entries are the caller's contract, as in
 * ltx_dit_forward_dev. Every video modulation row - adaLN, both cross-modal embedders (av_ca_video_scale_shift, av_ca_a2v_gate) and the
 * output head - is built once per (b, group) and picked per token through the map; audio timesteps stay [B]. n_groups == 1 with a NULL
 * map IS ltx_dual_model_forward_dev. n_groups < 1, B * n_groups > 8 or n_groups > 1 without a map: LTX_ERR_INVALID_CONFIGURATION before
 * the first launch, nothing written. Works with text_cache 0 and 1. */
int ltx_dual_model_forward_groups_dev(ltx_ctx* ctx, const ltx_dual_model_forward_args* args, int n_groups, const int32_t* video_row_map);
/* The timestep path of the forward alone (LTX2Transformer.swift:272-312), into caller buffers: temb_v [B][6][video_dim], temb_a
 * [B][6][audio_dim], cross_v [B][5][video_dim], cross_a [B][5][audio_dim] (rows 0-3 from the scale-shift embedder, row 4 from the
 * gate embedder), embts_v [B][video_dim], embts_a [B][audio_dim] (the embedded timesteps of the output heads), all f32 DEVICE
 * pointers; video_timesteps / audio_timesteps [B] f32. `ungrouped` as in the forward. Test and measurement seam, as
 * ltx_dit_export_param is one. B outside 1 .. 8 or a NULL pointer: LTX_ERR_INVALID_CONFIGURATION, nothing written. */
int ltx_dual_model_embed_dev(ltx_ctx* ctx, const float* video_timesteps, const float* audio_timesteps, int B, int ungrouped,
                             float* temb_v, float* temb_a, float* cross_v, float* cross_a, float* embts_v, float* embts_a);
/* The text side of a forward, once per prompt: caption_projection / audio_caption_projection of the two contexts [B][S][caption_channels]
 * bf16, the two mask biases (a NULL mask is a null bias, as in the forward) and, for every block, K (normed) and V^T of attn2 and
 * audio_attn2 - the same launches with the same operands as a forward with text_cache = 0 runs, so the cached operands carry the same
 * bits. The cache is ONE allocation of L * B * (S + ceil64(S)) * (video_dim + audio_dim) * 2 bytes (2.4 GB at L 48, B 2, S 1024), owned
 * by the model; ltx_dual_model_load / _init_synthetic / _unload drop it. DEVICE pointers, asynchronous on the context stream. */
int ltx_dual_model_prepare_text_dev(ltx_ctx* ctx, const uint16_t* video_context, const uint16_t* audio_context, const int32_t* video_mask,
                                    const int32_t* audio_mask, int B, int S);
/* What the text cache holds: its (B, S) (0, 0: none), its bytes, and how many times prepare_text has filled it since the model was
 * loaded. Any output pointer may be NULL. */
int ltx_dual_model_text_cache_info(ltx_ctx* ctx, int* B, int* S, long* bytes, long* builds);

/* One job of ltx_op_dual_step: one stream's share of the work between two forwards of the joint loop. */
typedef struct ltx_dual_step_job {
    float* latent;         /* [n] f32, in / out, TOKEN layout [T][C] */
    const float* v_cond;   /* [n] f32 */
    const float* v_uncond; /* [n] f32, or NULL: no CFG */
    float cfg_scale;
    int form;              /* 0: the scheduler's Euler form (LTXScheduler.swift:305-327); 1: x + (sigma_next - sigma) * v (LTXPipeline.swift:1402) */
    uint16_t* tokens;      /* [copies][n] bf16: the next forward's operand */
    int copies;            /* 1 or 2 (a B = 2 CFG forward reads the same tokens twice) */
    float* v_out;          /* [n] f32 or NULL: the guided velocity; may alias v_cond */
    long n;                /* elements; n % 4 == 0; 0: the job is empty */
    long n_keep;           /* frozen prefix (image-to-video: frame 0 in token layout): elements i < n_keep skip the Euler form. 0: none */
    const float* keep_src; /* [n_keep] f32: the conditioning latent in token layout; needed with keep_noise */
    const float* keep_noise; /* [n_keep] f32: x' = keep_src + (keep_scale * keep_noise) * (sigma_next * sigma_next), four separately
                                rounded f32 operations - the prefix as the NEXT forward must see it (LTXPipeline.swift:1289-1294). NULL: x' = x */
    float keep_scale;
} ltx_dual_step_job;
/* Kernel hook: CFG (LatentUtils.swift:131-141), the Euler step and the bf16 cast of both streams in one launch. Every operation is
 * rounded on its own (no fused multiply-add, correctly rounded division), as the reference's separate array ops are: latent and v_out
 * are bit-equal to a float32 replay of those ops. Either job may be NULL or empty. n % 4 != 0, copies outside 1 .. 2, form outside
 * 0 .. 1, a NULL latent / v_cond / tokens with n > 0, or sigma <= 0: LTX_ERR_INVALID_CONFIGURATION before the launch, nothing written.
 * With a frozen prefix the tokens (both copies) and v_out are still written for the whole job. n_keep % 4 != 0, n_keep outside 0 .. n or
 * keep_noise without keep_src are refused the same way; n_keep = 0 is the step without a prefix, bit for bit. */
int ltx_op_dual_step(ltx_ctx* ctx, const ltx_dual_step_job* video, const ltx_dual_step_job* audio, float sigma, float sigma_next);

/* One job of ltx_op_dual_restage: one stream's share of the bridge between the two stages of generateVideoWithAudioTwoStage
 * (LTXPipeline.swift:1712-1752). The video job has x set and transposes; the audio job has x NULL and works in place. */
typedef struct ltx_dual_restage_job {
    const float* x;          /* video: [C][T] f32, the upscaled and renormalised latent (ltx_upscale_latent_dev's output); audio: NULL */
    float* latent;           /* [T][C] f32, TOKEN layout: the stage-2 start latent. video: out; audio: in / out (the packed latent) */
    uint16_t* tokens;        /* [T][C] bf16: the first stage-2 forward's operand */
    int C;                   /* channels, a multiple of 32 (128) */
    long T;                  /* tokens; 0: the job is empty */
    const float* noise;      /* video [C][T], audio [T][C] (the reference draws it with the PACKED shape, :1734); NULL iff renoise == 0 */
    float noise_scale;       /* s: z = s * noise + (1.0f - s) * y (:1730-1731, :1735); 0 is valid */
    int renoise;             /* non-zero: a noise scale is given, noise must be set; 0: noise must be NULL and the blend is skipped */
    const float* stats;      /* video: [C][2] f32 {mean, variance} of x per channel, or NULL: computed from x */
    const float* stats_ref;  /* video: [C][2] f32 {mean, variance} of the stage-1 output, or NULL: computed from ref. Both or neither */
    const float* ref;        /* video: [C][T_ref] f32, the stage-1 output (the AdaIN reference); needed when stats are NULL */
    long T_ref;
    float* stats_out;        /* video: [4 * C] f32 or NULL: receives stats then stats_ref, as the kernel used them */
    long HW;                 /* video: tokens of frame 0 (t < HW), 1 .. T; read with cond */
    const float* cond;       /* video: [C][HW] f32, the full-resolution image latent, or NULL (text-to-video) */
    const float* cond_noise; /* video: [C][HW] f32, the first re-noise slice, or NULL: frame 0 = cond */
    float cond_scale;        /* frame 0 = cond + (cond_scale * cond_noise) * cond_sigma2 (:1765-1769), three separately rounded f32 ops */
    float cond_sigma2;       /* sigmas2[0] * sigmas2[0], the caller's f32 product */
} ltx_dual_restage_job;
/* Kernel hook: AdaIN at factor 1 against the stage-1 output (LatentUtils.swift:201-227), the re-noise of both streams (:1730-1735),
 * frame 0 of an image-to-video run (:1744, :1765-1769), the transpose to token layout and the bf16 cast, in one launch. Every operation
 * is rounded on its own (no fused multiply-add, correctly rounded division and square root): latent and tokens are bit-equal to a
 * float32 replay of those ops from the statistics in stats_out. No AdaIN or re-noise result survives for frame-0 tokens. Either job may be
 * NULL or empty. C % 32 != 0, a NULL x / latent / tokens with T > 0, HW outside 1 .. T with cond, cond_noise without cond, noise without
 * renoise or renoise without noise, only one of stats / stats_ref, neither statistics nor ref, or an audio job with a video-only
 * pointer set: LTX_ERR_INVALID_CONFIGURATION before any launch, nothing written. DEVICE pointers, asynchronous on the context stream. */
int ltx_op_dual_restage(ltx_ctx* ctx, const ltx_dual_restage_job* video, const ltx_dual_restage_job* audio);

/* ------------------------------------------------------------------------------------------------------------
 * Text-embedding connector (VideoGemmaTextEncoderModel.encodeFromHiddenStates,
 * LTXTextEncoder.swift:574-643 - call site LTXPipeline.swift:640-700): from the 49 Gemma-3 hidden states to the
 * [B,T,3840] bf16 context + all-ones mask that ltx_denoise / ltx_dit_forward take. The language model itself is not
 * part of this library: its hidden states are the input.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct ltx_connector_config {
    int dim;        /* 3840 = heads x 128 */
    int heads;      /* 30 */
    int layers;     /* 2 */
    int registers;  /* 128 learnable registers */
    int states;     /* 49 hidden states (embedding + 48 layers) */
    float theta;    /* 10000 */
    int max_pos;    /* 4096 */
} ltx_connector_config;
void ltx_connector_config_default(ltx_connector_config* cfg);
/* Replaces the connector part of loadModels (LTXPipeline.swift:420-540, key rules ModelDownloader.swift:911-968): reads
 * `text_embedding_projection.*` / `video_embeddings_connector.*` from a unified checkpoint, or `text_proj_in.*` /
 * `video_connector.*` from a standalone connector file. cfg NULL = reference architecture. */
int ltx_connector_load(ltx_ctx* ctx, const char* safetensors_path, const ltx_connector_config* cfg);
int ltx_connector_init_synthetic(ltx_ctx* ctx, const ltx_connector_config* cfg, unsigned long seed);
int ltx_connector_unload(ltx_ctx* ctx);
/* hidden [states][B][T][dim] bf16, attention_mask [B][T] int32 0/1 (padding_right: 0 = left padding, the reference's
 * default) -> context [B][T][dim] bf16 and out_mask [B][T] int32 (all ones; may be NULL). T must be a multiple of
 * `registers` (the reference aborts otherwise). DEVICE pointers. */
int ltx_connector_encode_dev(ltx_ctx* ctx, const uint16_t* hidden, const int32_t* attention_mask, int B, int T,
                             int padding_right, uint16_t* context, int32_t* out_mask);
/* HOST-pointer variant of the same call. */
int ltx_connector_encode(ltx_ctx* ctx, const uint16_t* hidden, const int32_t* attention_mask, int B, int T,
                         int padding_right, uint16_t* context, int32_t* out_mask);
/* Parity taps (DEVICE pointers, any may be NULL): the normalised concat [B][T][dim*states] bf16, the feature-extractor
 * output [B][T][dim] bf16 and the stream after register replacement [B][T][dim] f32. */
int ltx_connector_encode_taps_dev(ltx_ctx* ctx, const uint16_t* hidden, const int32_t* attention_mask, int B, int T,
                                  int padding_right, uint16_t* context, uint16_t* norm_concat, uint16_t* fe_out,
                                  float* after_registers);
/* The audio text context (VideoGemmaTextEncoderModel.encodeFromHiddenStates / callAsFunction, LTXTextEncoder.swift:628-636, :705-713; fed
 * to the audio stream at LTXPipeline.swift:1173): the feature extractor ONCE, then the video Embeddings1DConnector and a second,
 * independently weighted one (`audio_embeddings_connector.*` / `audio_connector.*`, key rules ModelDownloader.swift:930-941) on its
 * output. ltx_connector_load reads the audio set when the file has it; ltx_connector_init_synthetic makes one from a seed of its own.
 * video_context, audio_context [B][T][dim] bf16, out_mask [B][T] int32 (all ones; may be NULL). The video context and the mask are
 * ltx_connector_encode(_dev)'s, bit for bit. No audio set loaded: LTX_ERR_MODEL_NOT_LOADED before any launch (callers then hand the
 * video context to the audio stream, `audioEncoding ?? videoEncoding`). DEVICE pointers. */
int ltx_connector_encode_av_dev(ltx_ctx* ctx, const uint16_t* hidden, const int32_t* attention_mask, int B, int T, int padding_right,
                                uint16_t* video_context, uint16_t* audio_context, int32_t* out_mask);
/* HOST-pointer variant of the same call. */
int ltx_connector_encode_av(ltx_ctx* ctx, const uint16_t* hidden, const int32_t* attention_mask, int B, int T, int padding_right,
                            uint16_t* video_context, uint16_t* audio_context, int32_t* out_mask);
/* 1 when the loaded connector has an audio set, 0 otherwise (also without a connector or a context). */
int ltx_connector_has_audio(ltx_ctx* ctx);
/* mapTextEncoderWeights (ModelDownloader.swift:911-968): returns the length of the module key, 0 if the key is dropped. */
int ltx_map_text_encoder_key(const char* file_key, char* out, int cap);
/* Connector RoPE tables (positions 0..T-1, one axis, f64 math): cos/sin [T][dim/2] f32, before the cast to bf16. */
int ltx_rope_tables_1d(int T, int dim, float theta, int max_pos, float* cos_out, float* sin_out);

/* ------------------------------------------------------------------------------------------------------------
 * Denoising loop
 * ---------------------------------------------------------------------------------------------------------- */
/* GenerationProgressCallback (LTXPipeline.swift:50-72): invoked synchronously on the calling thread once per step,
 * before that step's forward (LTXPipeline.swift:805-810). */
typedef void (*ltx_progress_cb)(int current_step, int total_steps, float sigma, void* user);

/* LTXVideoGenerationConfig's sampling knobs (LTXConfig.swift:216-300) for one denoise run.
 * ABI revision 2: the struct starts with its own size as the CALLER compiled it. The library reads a field only when struct_size covers
 * it, so a host built against an older header (a shorter struct) stays safe when fields are appended; struct_size == 0 or smaller than
 * the revision-2 core (everything up to and including `shard`) is rejected with LTX_ERR_INVALID_CONFIGURATION. Initialise with
 * LTX_DENOISE_OPTIONS_INIT (C / C++) or MemoryLayout<ltx_denoise_options>.size (Swift). */
typedef struct ltx_denoise_options {
    uint32_t struct_size;   /* sizeof(ltx_denoise_options) in the caller's translation unit */
    float cfg_scale;        /* > 1 enables CFG; context batch is then [negative, positive] (LatentUtils.swift:104-117) */
    float guidance_rescale; /* phi (LatentUtils.swift:164-183) */
    float stg_scale;        /* STG (LTXPipeline.swift:897-921) */
    const int* stg_blocks;  /* default [29] */
    int n_stg_blocks;
    float ge_gamma;         /* GE momentum (LTXPipeline.swift:924-927) */
    /* Image-to-video (denoise(...) with conditioningMask / conditionedLatent, LTXPipeline.swift:2191-2401).
     * cond_latent: the encoded conditioning image [1][C][1][H][W] f32, in the same memory space as `latent` (NULL = text-to-video).
     * The VAE encoder is outside this library, so the image latent is an input. Frame 0 of `latent` is set to it (:2092-2094),
     * its tokens run at timestep 0 (:2237-2252) and the Euler step leaves it untouched (:2344-2357).
     * cond_noise: optional N(0,1) draws [n_sigmas-1][C][1][H][W] for the per-step re-noising of frame 0,
     * frame0 = cond + image_cond_noise_scale * cond_noise[step] * sigma^2 (:2225-2229); NULL = no re-noising. */
    const float* cond_latent;
    float image_cond_noise_scale;
    const float* cond_noise;
    /* Multi-GPU sharding of the loop over the ranks of this context's group (ltx_dist_init / ltx_dist_set_transport; the reference is
     * single-device - SURVEY 8(e)). Every rank calls ltx_denoise(_dev) with the same arguments and ends with the same latent, bit
     * for bit: CFG / rescale / STG / GE / Euler run redundantly on every rank with the library's own kernels.
     *   LTX_SHARD_NONE     (0) this context evaluates everything.
     *   LTX_SHARD_CFG      (1) the CFG pair is split: rank 0 = negative branch, rank 1 = positive branch (the two B=1 forwards of
     *                          LTXPipeline.swift:829-848 / the B=2 forward of :2236-2264), rank 2 of a three-rank group = the STG
     *                          pass; ONE all-gather of the [C*T] f32 velocities per step. Needs cfg_scale > 1 and 2 (or 3) ranks.
     *   LTX_SHARD_SEQUENCE (2) one sample's tokens are split into equal contiguous slices (F*H*W divisible by the group size into
     *                          multiples of 8): per transformer block one all-gather of K rows and one of V^T, per forward one
     *                          all-gather of the velocity slices. */
    int shard;
    /* Per-step diagnostics, optional: a HOST array of 4 * (n_sigmas - 1) floats that receives, for every step, the mean and the
     * (population) standard deviation of the guided velocity and of the latent after the Euler update - the numbers the reference logs
     * under --profile ("Step i: ... vel mean=, std=, latent mean=, std=", LTXPipeline.swift:945-951). With it the call ends with a
     * stream synchronisation (the device entry point is otherwise asynchronous). NULL = none. A maintainer with the reference on a Mac
     * can compare these lines for the same weights, embeddings and noise without touching the reference's code. */
    float* step_stats;
} ltx_denoise_options;
/* size set, CFG / rescale / STG / GE off, text-to-video, no sharding, no diagnostics */
#define LTX_DENOISE_OPTIONS_INIT {(uint32_t)sizeof(ltx_denoise_options), 1.0f, 0.0f, 0.0f, NULL, 0, 0.0f, NULL, 0.0f, NULL, 0, NULL}
enum { LTX_SHARD_NONE = 0, LTX_SHARD_CFG = 1, LTX_SHARD_SEQUENCE = 2 };

/* Replaces the denoise loop of generateVideo (LTXPipeline.swift:800-956) / denoise(...) (:2191-2401), T2V.
 *   latent  [1][C][F][H][W] f32, in/out; must already be scaled by sigmas[0] (LTXPipeline.swift:793)
 *   sigmas  HOST array of n_sigmas values (n_sigmas-1 Euler steps), e.g. from ltx_sigmas
 *   context [nb][S][caption_channels] bf16, mask [nb][S] int32 or NULL; nb = 2 ([neg,pos]) iff cfg_scale > 1
 * HOST pointers for latent/context/mask. */
int ltx_denoise(ltx_ctx* ctx, float* latent, int F, int H, int W, const float* sigmas, int n_sigmas,
                const uint16_t* context, const int32_t* mask, int S, const ltx_denoise_options* opt,
                ltx_progress_cb cb, void* user);
/* Same with DEVICE pointers for latent/context/mask (sigmas stays a host array); asynchronous on the context
 * stream. ctx_version / mask_all_ones as in ltx_dit_forward_dev. */
int ltx_denoise_dev(ltx_ctx* ctx, float* latent, int F, int H, int W, const float* sigmas, int n_sigmas,
                    const uint16_t* context, const int32_t* mask, int mask_all_ones, int S, uint64_t ctx_version,
                    const ltx_denoise_options* opt, ltx_progress_cb cb, void* user);

/* Arguments of ltx_dual_denoise(_dev); starts with its own size (LTX_DUAL_DENOISE_ARGS_INIT). */
typedef struct ltx_dual_denoise_args {
    uint32_t struct_size;          /* sizeof(ltx_dual_denoise_args) in the caller's translation unit */
    int F, H, W;                   /* latent frames / height / width */
    int T_a;                       /* audio latent frames */
    int S;                         /* text tokens */
    float* video_latent;           /* [1][in_channels][F][H][W] f32, in / out, already scaled by sigmas[0]: ltx_denoise's and ltx_vae_decode's layout */
    float* audio_latent;           /* [1][8][T_a][16] f32, in / out, scaled: the layout ltx_audio_decode takes */
    const float* sigmas;           /* HOST, n_sigmas values: one schedule for both streams (the reference builds two identical schedulers) */
    int n_sigmas;
    const uint16_t* video_context; /* [nb][S][caption_channels] bf16, nb = 2 ([negative, positive]) iff cfg_scale > 1 */
    const uint16_t* audio_context; /* the same shape, or NULL: the video context (audioEncoding ?? videoEncoding) */
    const int32_t* mask;           /* [nb][S] int32 or NULL; both streams use it (LTXPipeline.swift:1322-1323) */
    float cfg_scale;
    float guidance_rescale;        /* > 0 (needs cfg_scale > 1): applied to the VIDEO velocity only (LTXPipeline.swift:1352-1359) */
    int text_cache;                /* non-zero (default): the text side is computed once; 0 recomputes it every step. The same bits */
    float* step_stats;             /* HOST, 8 * (n_sigmas - 1) floats or NULL: per step mean and std of the video velocity, the video
                                      latent, the audio velocity and the audio latent. Non-NULL makes the _dev call synchronous */
    /* image-to-video, with the meanings, layouts and memory space of the same fields of ltx_denoise_options; read when struct_size covers them */
    const float* cond_latent;      /* [1][in_channels][1][H][W] f32 or NULL (text-to-video): the encoded image; needs F >= 2 */
    float image_cond_noise_scale;  /* > 0 with cond_noise: frame 0 is re-noised at the start of every step (LTXPipeline.swift:1289-1294) */
    const float* cond_noise;       /* [n_sigmas - 1][in_channels][1][H][W] f32 or NULL: the caller's draws, one slice per step */
} ltx_dual_denoise_args;
#define LTX_DUAL_DENOISE_ARGS_INIT {(uint32_t)sizeof(ltx_dual_denoise_args), 0, 0, 0, 0, 0, NULL, NULL, NULL, 0, NULL, NULL, NULL, 1.0f, 0.0f, 1, NULL, NULL, 0.0f, NULL}
/* Replaces the denoise loop of generateVideoWithAudio (LTXPipeline.swift:1276-1417), text-to-video+audio and (cond_latent set)
 * image-to-video+audio: per step the progress
 * callback, ONE dual-model forward (B = 2 on [negative, positive] with CFG), optional guidance rescale of the video velocity, and ONE
 * launch for CFG + both Euler steps + the next forward's tokens (ltx_op_dual_step; video form 0, audio form 1). Both latents are held in
 * token layout for the whole loop and transposed once at entry and once at exit. Noise is the caller's (video first, then audio,
 * :1229-1236). Image-to-video (:1261-1274, :1289-1303, :1383-1399): frame 0 of the latent is set to cond_latent at entry, its tokens run
 * at timestep 0 (two timestep groups, ltx_dual_model_forward_groups_dev), it is never stepped, and with re-noising it holds cond +
 * (scale * noise[step]) * sigma^2 during step `step` - written by the step launch of the step before, so no launch is added per step;
 * the result's frame 0 is the last step's noised frame, or cond_latent itself without re-noising. F < 2 with cond_latent:
 * LTX_ERR_INVALID_CONFIGURATION. STG, GE and sharding are not implemented here; the two-stage path is ltx_dual_two_stage below. DEVICE pointers except sigmas and
 * step_stats; asynchronous on the context stream unless step_stats is set. No dual model: LTX_ERR_MODEL_NOT_LOADED; a short struct_size,
 * n_sigmas < 2, a dimension < 1, a NULL latent / sigmas / video_context, a sigma <= 0 before the last, or guidance_rescale > 0 without
 * CFG: LTX_ERR_INVALID_CONFIGURATION. Every check comes before the first launch: a refused call leaves both latents untouched. */
int ltx_dual_denoise_dev(ltx_ctx* ctx, const ltx_dual_denoise_args* args, ltx_progress_cb cb, void* user);
/* The same with HOST pointers throughout; staged through the context's staging buffers, synchronous. */
int ltx_dual_denoise(ltx_ctx* ctx, const ltx_dual_denoise_args* args, ltx_progress_cb cb, void* user);

/* Arguments of ltx_dual_two_stage(_dev); starts with its own size (LTX_DUAL_TWO_STAGE_ARGS_INIT). */
typedef struct ltx_dual_two_stage_args {
    uint32_t struct_size;          /* sizeof(ltx_dual_two_stage_args) in the caller's translation unit */
    int F, H, W;                   /* STAGE-1 latent frames / height / width; stage 2 runs at F, 2H, 2W */
    int T_a;                       /* audio latent frames */
    int S;                         /* text tokens */
    const float* video_latent_in;  /* [1][128][F][H][W] f32: the stage-1 noise, already scaled by sigmas1[0] (:1597); not written */
    float* video_latent_out;       /* [1][128][F][2H][2W] f32: the final video latent */
    float* audio_latent;           /* [1][8][T_a][16] f32, in / out, scaled by sigmas1[0] (:1598) */
    const float* sigmas1;          /* HOST, n_sigmas1 values: the stage-1 schedule (:1587-1593) */
    int n_sigmas1;
    const float* sigmas2;          /* HOST, n_sigmas2 values, or NULL: ltx_stage2_sigmas (STAGE_2_DISTILLED_SIGMA_VALUES, :1727) */
    int n_sigmas2;
    const float* video_noise2;     /* [1][128][F][2H][2W] f32: the stage-2 video noise (:1730) */
    const float* audio_noise2;     /* [T_a][128] f32: the stage-2 audio noise, drawn with the PACKED shape (:1734) */
    const uint16_t* video_context; /* [1][S][caption_channels] bf16 */
    const uint16_t* audio_context; /* the same shape, or NULL: the video context */
    const int32_t* mask;           /* [1][S] int32 or NULL; both streams, both stages */
    float* stage1_out;             /* [1][128][F][H][W] f32 or NULL: receives the stage-1 video latent (the AdaIN reference, :1688) */
    /* image-to-video (:1600-1610, :1737-1751): both latents or neither; needs F >= 2 */
    const float* cond_latent1;     /* [1][128][1][H][W] f32: the image encoded at the stage-1 resolution, or NULL */
    const float* cond_latent2;     /* [1][128][1][2H][2W] f32: the image encoded at the stage-2 resolution, or NULL */
    float image_cond_noise_scale;  /* > 0 with the noise of a stage: frame 0 is re-noised at the start of every step of it (:1628-1632, :1765-1769) */
    const float* cond_noise1;      /* [n_sigmas1 - 1][128][1][H][W] f32 or NULL */
    const float* cond_noise2;      /* [n_sigmas2 - 1][128][1][2H][2W] f32 or NULL */
} ltx_dual_two_stage_args;
#define LTX_DUAL_TWO_STAGE_ARGS_INIT {(uint32_t)sizeof(ltx_dual_two_stage_args), 0, 0, 0, 0, 0, NULL, NULL, NULL, NULL, 0, NULL, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0.0f, NULL, NULL}
/* Replaces the two denoise loops of generateVideoWithAudioTwoStage and what lies between them (LTXPipeline.swift:1613-1817); both latents
 * stay on the device from the first noise to the final latents:
 *   1. the text side of the dual model once, for both stages (the same B and S)
 *   2. stage 1 as ltx_dual_denoise runs it: the video by the scheduler's Euler form, the audio by the plain form (:1666-1678),
 *      image-to-video with two timestep groups
 *   3. the stage-1 video latent back to the caller's layout: the AdaIN reference (:1688) and the upscaler's input (stage1_out)
 *   4. the latent upscaler with the VAE's per-channel statistics (:1696-1710)
 *   5. the per-channel statistics of the upscaled latent and of the stage-1 output
 *   6. ONE launch (ltx_op_dual_restage): AdaIN (:1712), the re-noise of both streams by sigmas2[0] (:1730-1735), frame 0 of stage 2
 *      (:1744, and step 0's :1765-1769), token layout and the first bf16 tokens
 *   7. stage 2 from that token state: BOTH streams by the plain form x + (sigma_next - sigma) * v (:1799-1811), which is not the
 *      scheduler's form bit for bit; image-to-video groups at the stage-2 shape
 *   8. the final latents back to the caller's layouts
 * The path is distilled: one forward per step and no CFG (:1646, :1783), no STG, no GE. The progress callback reports stage 1 as
 * (step, n_sigmas1 - 1) and stage 2 as (n_sigmas1 - 1 + step, n_sigmas1 - 1 + n_sigmas2 - 1) (:1623, :1760). Noise is the caller's, in
 * the reference's order of drawing: (1) the stage-1 video noise, (2) the audio noise [1][8][T_a][16], (3) one frame-0 slice per stage-1
 * step, (4) the stage-2 video noise, (5) the packed audio noise [T_a][128], (6) one frame-0 slice per stage-2 step. The VAE and audio
 * decode legs follow through ltx_vae_decode and ltx_audio_decode. No dual model, upscaler or VAE (statistics): LTX_ERR_MODEL_NOT_LOADED;
 * a short struct_size, a NULL required pointer, a dimension < 1, fewer than 2 sigmas, a sigma <= 0 before the last of either schedule,
 * only one of the two image latents, or F < 2 with them: LTX_ERR_INVALID_CONFIGURATION. Every check comes before the first launch: a
 * refused call leaves both latents untouched. DEVICE pointers except the sigmas; asynchronous on the context stream. */
int ltx_dual_two_stage_dev(ltx_ctx* ctx, const ltx_dual_two_stage_args* args, ltx_progress_cb cb, void* user);
/* The same with HOST pointers throughout; staged through the context's staging buffers, synchronous. */
int ltx_dual_two_stage(ltx_ctx* ctx, const ltx_dual_two_stage_args* args, ltx_progress_cb cb, void* user);

/* Arguments of ltx_dual_generate(_dev) and ltx_dual_noise_plan; starts with its own size (LTX_DUAL_GENERATE_ARGS_INIT). A generation
 * from a seed alone: the noise of ltx_dual_denoise / ltx_dual_two_stage drawn by the library, on the device, in the reference's order. */
typedef struct ltx_dual_generate_args {
    uint32_t struct_size;          /* sizeof(ltx_dual_generate_args) in the caller's translation unit */
    int two_stage;                 /* 0: generateVideoWithAudio (ltx_dual_denoise); non-zero: generateVideoWithAudioTwoStage (ltx_dual_two_stage) */
    uint64_t seed;                 /* MLXRandom.seed(seed) (LTXPipeline.swift:1224-1226, :1571-1573) */
    int channels;                  /* latent channels (128): must be the loaded model's in_channels */
    int F, H, W;                   /* latent frames / height / width; of STAGE 1 with two_stage (stage 2 runs at F, 2H, 2W) */
    int T_a;                       /* audio latent frames (ltx_audio_latent_frames) */
    int S;                         /* text tokens */
    float* video_latent;           /* OUT [1][channels][F][H][W] f32, or [1][channels][F][2H][2W] with two_stage */
    float* audio_latent;           /* OUT [1][8][T_a][16] f32 */
    const float* sigmas1;          /* HOST, n_sigmas1 values: the only schedule, or stage 1's */
    int n_sigmas1;
    const float* sigmas2;          /* HOST, two_stage only: n_sigmas2 values, or NULL = ltx_stage2_sigmas */
    int n_sigmas2;
    const uint16_t* video_context; /* [nb][S][caption_channels] bf16, nb = 2 ([negative, positive]) iff cfg_scale > 1 */
    const uint16_t* audio_context; /* the same shape, or NULL: the video context (audioEncoding ?? videoEncoding) */
    const int32_t* mask;           /* [nb][S] int32 or NULL */
    float cfg_scale;               /* one-stage only; the two-stage path is distilled (must be <= 1 there) */
    float guidance_rescale;        /* one-stage only */
    const float* cond_latent1;     /* image-to-video: [1][channels][1][H][W] f32 or NULL */
    const float* cond_latent2;     /* two_stage image-to-video: [1][channels][1][2H][2W] f32; both or neither */
    float image_cond_noise_scale;  /* > 0 with an image latent: one frame-0 slice is drawn per step and frame 0 re-noised with it */
    float* noise_workspace;        /* total_floats of ltx_dual_noise_plan, or NULL: the library keeps one of its own. DEVICE memory for
                                      ltx_dual_generate_dev; for ltx_dual_generate HOST memory that receives a copy of the draws */
    float* stage1_out;             /* two_stage only: [1][channels][F][H][W] f32 or NULL, as ltx_dual_two_stage_args.stage1_out */
} ltx_dual_generate_args;
#define LTX_DUAL_GENERATE_ARGS_INIT {(uint32_t)sizeof(ltx_dual_generate_args), 0, 0, 128, 0, 0, 0, 0, 0, NULL, NULL, NULL, 0, NULL, 0, NULL, NULL, NULL, 1.0f, 0.0f, NULL, NULL, 0.0f, NULL, NULL}

/* One draw of a generation. The roles, in the reference's order of drawing:
 *   LTX_NOISE_VIDEO1  draw 0, [1][channels][F][H][W], times sigmas1[0] (LTXPipeline.swift:1229, :1243 / :1576, :1597)
 *   LTX_NOISE_AUDIO1  draw 1, [1][8][T_a][16], times sigmas1[0] (:1233-1235, :1244 / :1580-1582, :1598)
 *   LTX_NOISE_COND1   one [1][channels][1][H][W] slice per step of the (first) loop, unscaled (:1291 / :1629)
 *   LTX_NOISE_VIDEO2  two_stage: [1][channels][F][2H][2W], unscaled (:1730)
 *   LTX_NOISE_AUDIO2  two_stage: the packed shape [T_a][128], unscaled (:1734)
 *   LTX_NOISE_COND2   two_stage: one [1][channels][1][2H][2W] slice per stage-2 step, unscaled (:1766)
 * COND1 / COND2 exist only with an image latent and image_cond_noise_scale > 0. The reference skips a step's slice when its sigma
 * is 0 (:1290); ltx_dual_denoise refuses a sigma <= 0 before the last, so every step draws. */
enum { LTX_NOISE_VIDEO1 = 0, LTX_NOISE_AUDIO1 = 1, LTX_NOISE_COND1 = 2, LTX_NOISE_VIDEO2 = 3, LTX_NOISE_AUDIO2 = 4, LTX_NOISE_COND2 = 5 };
typedef struct ltx_noise_draw {
    int draw_index;  /* which keyless draw after seeding (the argument of ltx_mlx_random_normal) */
    int role;        /* LTX_NOISE_* */
    int step;        /* COND1 / COND2: the step of its loop; 0 otherwise */
    long numel;
    long offset;     /* in floats into the noise workspace, a multiple of 64 - except that the slices of one COND role follow each
                        other without gaps (the loops take them as one array). -1: the draw is not in the workspace, because the loop
                        takes it in place in a latent buffer: AUDIO1 always (audio_latent), VIDEO1 without two_stage (video_latent) */
    float scale;
} ltx_noise_draw;
/* The draws of ltx_dual_generate(_dev) for these arguments, in drawing order, and the floats of the workspace that holds them. Reads
 * two_stage, channels, F, H, W, T_a, the schedules' lengths, sigmas1[0], the image latents (as flags) and image_cond_noise_scale. Returns the number of draws -
 * the number needed when cap is too small, in which case out is not written (total_floats is) - or -LTX_ERR_INVALID_CONFIGURATION for
 * NULL args, a short struct_size, a dimension or channels < 1, a draw of 2^31 values or more, n_sigmas1 < 2 or NULL sigmas1, n_sigmas2 < 2
 * with sigmas2, only one of the two image latents with two_stage, cap < 0 or a NULL out with cap > 0. The VAE decoder's own noise
 * (ltx_vae_decode's seed) is not part of the plan. Pure host code. */
int ltx_dual_noise_plan(const ltx_dual_generate_args* args, ltx_noise_draw* out, int cap, long* total_floats);
/* Replaces generateVideoWithAudio (LTXPipeline.swift:1222-1417) and generateVideoWithAudioTwoStage (:1570-1817) from the noise to the
 * final latents: builds the plan, fills every draw in ONE ltx_op_mlx_normal_group launch - VIDEO1 and AUDIO1 straight into the latent
 * buffers where the loop takes them in place - and runs ltx_dual_denoise_dev or ltx_dual_two_stage_dev on pointers into the workspace.
 * It adds no numerics of its own: the result is that loop's on those draws, bit for bit. The refusals of the plan and of the loop it
 * wraps, channels != the model's in_channels, and cfg_scale > 1 or guidance_rescale > 0 with two_stage: all before the first launch, so
 * a refused call leaves the outputs and the workspace untouched. DEVICE pointers except the sigmas; asynchronous on the context stream.
 * The decode legs follow through ltx_vae_decode and ltx_audio_decode. Sharding of the joint loop is not implemented. */
int ltx_dual_generate_dev(ltx_ctx* ctx, const ltx_dual_generate_args* args, ltx_progress_cb cb, void* user);
/* The same with HOST pointers throughout (noise_workspace: see the struct); synchronous. */
int ltx_dual_generate(ltx_ctx* ctx, const ltx_dual_generate_args* args, ltx_progress_cb cb, void* user);

/* ------------------------------------------------------------------------------------------------------------
 * Multi-GPU: one process per GPU, one ltx_ctx per process, RCCL over xGMI called by the library itself (librccl is loaded
 * on the first ltx_dist_* call; no PyTorch on this path). The reference is a single-device program: this section has no Swift
 * counterpart, it shards what SURVEY 8(e) says shards - the CFG pair (LTXPipeline.swift:820-865, :2235-2283), one sample's
 * tokens, the VAE's temporal tiles (VideoDecoder.swift:517-592). Independent samples need nothing from here (replicas).
 * ---------------------------------------------------------------------------------------------------------- */
#define LTX_DIST_ID_BYTES 128
/* ncclGetUniqueId: called on ONE rank; the host carries the 128 bytes to the other ranks of the group (any channel: MPI, a TCP
 * store, a file) and every rank passes them to ltx_dist_init. */
int ltx_dist_unique_id(void* id_out);
/* ncclCommInitRank on the context's device; collective over the group's ranks. A group is whatever set of contexts shares one
 * id: the CFG pair of one sample (2 ranks), the ranks decoding one video's tiles, all 8 GPUs of one sequence-parallel sample. */
int ltx_dist_init(ltx_ctx* ctx, int rank, int world, const void* id);
/* The same group membership with a caller-supplied all-gather instead of RCCL (contract as ltx_allgather_fn above). For hosts
 * that already own a transport, and for world-size-2 tests where RCCL cannot run (two processes on one GPU). */
int ltx_dist_set_transport(ltx_ctx* ctx, int rank, int world, ltx_allgather_fn gather, void* user);
int ltx_dist_shutdown(ltx_ctx* ctx);
/* rank / world of the context's group (0 / 1 without one); *native = 1 when the transport is RCCL; *n_collectives = collectives
 * enqueued so far. Any pointer may be NULL. */
int ltx_dist_info(const ltx_ctx* ctx, int* rank, int* world, int* native_transport, long* n_collectives);
/* Collectives on the context's stream for the host's own exchanges (the one-time broadcast of the text context).
 * DEVICE pointers. recv = [world][bytes] in rank order. */
int ltx_dist_allgather_dev(ltx_ctx* ctx, const void* send, void* recv, long bytes);
int ltx_dist_broadcast_dev(ltx_ctx* ctx, void* buf, long bytes, int root);

/* Tiled VAE decode as building blocks (decodeWithTemporalTiling, VideoDecoder.swift:517-602), for hosts that place tiles on GPUs
 * themselves. ltx_vae_decode_tile_dev: the RAW frames - before blending and before the (x+1)/2 clip of :501-505 - of tile
 * `tile_index` of the plan (tile, overlap) over `latent` [1][128][F][H][W] -> tile_out (n, 32H, 32W, 3) f32, n = 8(len-1)+1.
 * Blending clipped tiles is not the reference: raw frames are what travels between GPUs. DEVICE pointers. */
int ltx_vae_decode_tile_dev(ltx_ctx* ctx, const float* latent, int F, int H, int W, int has_timestep, float timestep,
                            const float* noise, int tile, int overlap, int tile_index, float* tile_out, long tile_cap,
                            int* n_frames_out);
/* One VAEResBlock3d of the loaded decoder (VideoDecoder.swift:75-131: PixelNorm -> scale/shift -> SiLU -> conv1 -> PixelNorm ->
 * scale/shift -> SiLU -> conv2 -> + x; no timestep conditioning) applied in place to a channels-last f32 stream x [F][H][W][C],
 * C = channels of up-block group `group` (0..3: 1024, 512, 256, 128), block 0..4. Runs the very kernels and fused epilogues of the
 * decode, so a host (or a parity test) can check one stage at full resolution without a full-size reference decode. DEVICE pointer. */
int ltx_vae_res_block_dev(ltx_ctx* ctx, int group, int block, float* x, int F, int H, int W);
/* One VAEDepthToSpaceUpsample3d of the loaded decoder (VideoDecoder.swift:201-251: conv C -> 4C, depth-to-space (2,2,2), drop the first
 * frame, + the channel-tiled depth-to-space of the input) - the stage behind up-block group `group` (0..2: 1024, 512, 256 channels in,
 * half of that out) - on a caller-supplied channels-last f32 stream x [F][H][W][C] -> out [2F-1][2H][2W][C/2]. Runs the decode's own
 * conv kernel and fused depth-to-space epilogue, so one upsampler can be checked at full resolution. DEVICE pointers. */
int ltx_vae_upsample_dev(ltx_ctx* ctx, int group, const float* x, int F, int H, int W, float* out);
/* Blend raw tiles in tile order over 8*overlap frames (VideoDecoder.swift:561-592), then clip((x+1)/2, 0, 1) (:501-505).
 * tiles: HOST array of n_tiles DEVICE pointers, tile_frames their frame counts; tiles[0] may be frames_out. */
int ltx_vae_blend_tiles_dev(ltx_ctx* ctx, const float* const* tiles, const int* tile_frames, int n_tiles, int overlap, int H,
                            int W, float* frames_out, long frames_cap, int* n_frames_out);
/* ltx_vae_decode_dev with the tiles decoded round-robin by the ranks of the context's group (tile i on rank i % world), each raw
 * tile broadcast from its owner, and the blend + clip done on every rank: every rank returns the full frames, bit-identical to
 * the single-GPU ltx_vae_decode_dev. Every rank must call it with the same arguments. */
int ltx_vae_decode_sharded_dev(ltx_ctx* ctx, const float* latent, int F, int H, int W, int has_timestep, float timestep,
                               const float* noise, int tile, int overlap, float* frames_out, long frames_cap,
                               int* n_frames_out);
/* The gather form of the same: every raw tile travels ONCE, from its owner to rank `root` (ncclSend / ncclRecv over xGMI), and only
 * `root` blends, clips and fills frames_out (bit-identical to ltx_vae_decode_dev); the other ranks pass frames_out = NULL and get the
 * frame count. This is what a host that exports one video wants (decodeVideo returns ONE tensor, VideoDecoder.swift:466-507): with
 * the 4 tiles of 768x512x201 (tile 8, overlap 1 - the plan is fixed by VideoDecoder.swift:534-548 and must not be changed to fill
 * more GPUs: it decides the blended frames) on 8 ranks, 0.8 GB reach one rank instead of 1 GB reaching all eight. Every rank of the
 * group must call it with the same arguments. */
int ltx_vae_decode_gathered_dev(ltx_ctx* ctx, const float* latent, int F, int H, int W, int has_timestep, float timestep,
                                const float* noise, int tile, int overlap, int root, float* frames_out, long frames_cap,
                                int* n_frames_out);

/* ------------------------------------------------------------------------------------------------------------
 * Live kernel timing (replaces the reference's wall-clock GenerationTimings, LTXVideo.swift:255-297, with HIP
 * events recorded on the launch stream around every launch of a kernel family). kind: 0 GEMM, 1 attention,
 * 2 conv3d, 3 elementwise. work = algorithmic FLOPs of the timed launches.
 * ---------------------------------------------------------------------------------------------------------- */
int ltx_prof_enable(ltx_ctx* ctx, int on);
/* Synchronises the stream, folds finished events into the totals and returns them; reset != 0 clears afterwards. */
int ltx_prof_collect(ltx_ctx* ctx, int kind, double* total_ms, long* launches, double* work, int reset);

/* ------------------------------------------------------------------------------------------------------------
 * Kernel-level entry points (DEVICE pointers). These expose the individual gfx950 kernels so that parity tests can
 * pin each one against the oracle; they are not needed by a pipeline caller.
 * ---------------------------------------------------------------------------------------------------------- */
/* C[M,N] = A[M,K] . B[N,K]^T (+bias[N]) ; act: 0 none, 1 gelu-tanh, 2 silu; tile_cfg: -1 auto, else a forced tile configuration
 * (0,1,3,4: two-stage 4-wave tiles; 21,23,25: 8-wave LDS-ring tiles; 75: 192x256 one-wave-per-SIMD tile; 41,42,71-74,90
 * only in the experiments build; S*100 + ring cfg: the
 * same with an S-way deterministic split of the K reduction, as the VAE's 1024-channel convolutions use).
 * Exactly one of out_f32/out_bf16 may be NULL. */
int ltx_op_gemm_bf16(ltx_ctx* ctx, const uint16_t* A, long lda, const uint16_t* B, long ldb, const float* bias, int M,
                     int N, int K, int act, int tile_cfg, float* out_f32, long ld_f32, uint16_t* out_bf16,
                     long ld_bf16);
/* out = A . dequant(codes)^T + bias for a few-row launch (M <= 256) on an affine-quantised Linear as MLX's QuantizedLinear holds it
 * (LTXQuantizationConfig.swift:19-62): 8-bit codes [N][K], bf16 scale / bias per 64-wide group [N][K/64], w' = bf16(q * scale + bias).
 * via_scratch = 0: the codes are de-quantised in the GEMM's B stage (what a quantised DiT does at few tokens, e.g. 256x256x9);
 * via_scratch = 1: codes -> bf16 scratch matrix -> the same kernel (what every other launch does). Same bits either way.
 * split_k >= 1: deterministic split of the K reduction. tile_cfg: 30 = the few-row kernel (M <= 128; operand rings of their own, codes
 * staged 15 K-tiles ahead), 29 = the 128x64 ring kernel. */
int ltx_op_gemm_q8(ltx_ctx* ctx, const uint16_t* A, long lda, const uint8_t* codes, const uint16_t* scales, const uint16_t* biases,
                   const float* bias, int M, int N, int K, int split_k, int via_scratch, int tile_cfg, float* out_f32, long ld_f32);
/* vt[n][t] = bf16(sum_k X[t][k] W[n][k] + bias[n]): the value projection in the transposed layout the attention op takes
 * (to_v of LTXAttention.swift:100-104 followed by the head split; columns t >= tokens of vt are left untouched), ldvt % 4 == 0 */
int ltx_op_value_projection_t(ltx_ctx* ctx, const uint16_t* X, long ldx, int tokens, const uint16_t* W, const float* bias, int out_features,
                              int in_features, uint16_t* vt, long ldvt);
/* The self-attention projections of a DiT block from the same rows X[rows][K]: qk_out[m][n] = bf16(X[m] . Wqk[n] + bqk[n]) for the
 * fused to_q|to_k Linear Wqk [2 D][K], and V^T per batch element b = m / rows_per_batch in the layout the attention op takes:
 * vt_out[(b * D + d) * ldvt + m % rows_per_batch] = bf16(X[m] . Wv[d] + bv[d]), Wv [D][K]; everything else of vt_out / qk_out is left
 * untouched. fused != 0: ONE launch of 192 x 384 tiles (an error unless rows and rows_per_batch are multiples of 192, D of 128, K of
 * 64, ldx and ld_qk of 8, ldvt of 4); fused == 0: the q|k Linear and one V^T launch per batch element. Both give the same bits. */
int ltx_op_qkv_projection(ltx_ctx* ctx, const uint16_t* X, long ldx, int rows, int rows_per_batch, const uint16_t* Wqk, const float* bqk,
                          const uint16_t* Wv, const float* bv, int D, int K, uint16_t* qk_out, long ld_qk, uint16_t* vt_out, long ldvt,
                          int fused);
/* x[m][n] += gate[n] * (A.B^T + bias) in place on an f32 stream, optional bf16 mirror of the result */
int ltx_op_gemm_bf16_gated_residual(ltx_ctx* ctx, const uint16_t* A, long lda, const uint16_t* B, long ldb,
                                    const float* bias, const float* gate, float gate_scalar, int M, int N, int K,
                                    float* x, long ldx, uint16_t* mirror_bf16, long ld_mirror);
/* the same update followed by the adaLN pass over the updated rows: xn[m][:] = bf16(rms_norm(x[m][:]) * (1 + scale) + shift)
 * (LTXTransformerBlock.swift:72-92: a block's last residual update and the next block's first norm-modulate). fused != 0: the way the
 * DiT graph launches the pair (the norm rides on the GEMM's split-K finish pass where the launch has one); fused == 0: two launches.
 * Both give the same bits. */
int ltx_op_gemm_bf16_gated_residual_norm(ltx_ctx* ctx, const uint16_t* A, long lda, const uint16_t* B, long ldb,
                                         const float* bias, const float* gate, float gate_scalar, int M, int N, int K,
                                         float* x, long ldx, const float* scale, const float* shift, float eps,
                                         uint16_t* xn, long ldxn, int fused);
/* One launch of the 192 x 256 (tile_cfg 75) or the 384 x 256 (tile_cfg 76) GEMM kernel with any epilogue it has, for the tests that pin
 * every form of their store: v = act(A.B^T + bias_n[n] + bias_m[m]), rounded through bf16 when round_bf16; stored to out_f32 and / or
 * out_bf16, or, with resid, out_f32[m][n] = (resid_src ? resid_src : out_f32)[m][n] + gate(m, n) * v (and its bf16 copy), gate(m, n) =
 * gate ? gate[(gate_rowmap ? gate_rowmap[m] : m / rows_per_batch) * gate_bstride + n] : gate_scalar. split_k > 1 (tile_cfg 75): that many
 * K ranges through the context's workspace, as f32 or (split_bf16) bf16 partial tiles, and the finish pass. An error for a launch the
 * kernel does not take (whole tiles, K % 64 == 0, leading dimensions % 8 == 0; 76: plain stores only). */
typedef struct ltx_gemm_tile_launch {
    uint32_t struct_size; /* sizeof(ltx_gemm_tile_launch) */
    int tile_cfg;
    const uint16_t* A; /* [M][lda] bf16 */
    long lda;
    const uint16_t* B; /* [N][ldb] bf16 */
    long ldb;
    int M, N, K;
    int split_k;       /* >= 1 */
    int split_bf16;
    int act;           /* 0 none, 1 gelu-tanh, 2 silu */
    int round_bf16;
    int resid;
    const float* bias_n; /* [N] or NULL */
    const float* bias_m; /* [M] or NULL */
    float* out_f32;      /* [M][ld_f32] or NULL */
    long ld_f32;
    uint16_t* out_bf16;  /* [M][ld_bf16] or NULL */
    long ld_bf16;
    const float* resid_src; /* [M][ld_resid] or NULL: in place on out_f32 */
    long ld_resid;
    const float* gate;      /* or NULL: gate_scalar */
    long gate_bstride;
    const int32_t* gate_rowmap; /* [M] or NULL */
    int rows_per_batch;     /* 0: M */
    float gate_scalar;
} ltx_gemm_tile_launch;
int ltx_op_gemm_tile(ltx_ctx* ctx, const ltx_gemm_tile_launch* launch);
/* out[m][n] = sum_k in_act(a[m][k]) W[n][k] + bias[n], f32 x bf16 -> f32, M <= 8 */
int ltx_op_gemv_f32(ltx_ctx* ctx, const float* a, long lda, const uint16_t* W, long ldw, const float* bias, float* out,
                    long ldo, int M, int N, int K, int in_act);
/* One job of ltx_op_gemv_group: the operands of ltx_op_gemv_f32 without M. */
typedef struct ltx_gemv_job {
    const float* a; /* [M][lda] f32 */
    long lda;       /* lda % 4 == 0 */
    const uint16_t* W; /* [N][ldw] bf16 */
    long ldw;       /* ldw % 8 == 0 */
    const float* bias; /* [N] f32 or NULL */
    float* out;     /* [M][ldo] f32; may point into the middle of a wider row */
    long ldo;
    int N;          /* 0: the job is skipped */
    int K;          /* K % 8 == 0 */
    int in_act;     /* 0 none, 2 SiLU on the activations */
} ltx_gemv_job;
/* Up to 8 ltx_op_gemv_f32 jobs that share M in ONE launch, as the dual model's timestep path runs the six AdaLayerNormSingle embedders
 * of LTX2Transformer.swift:272-312 (one launch per stage). Jobs may differ in N, K and activation. Every job is bit-equal to
 * ltx_op_gemv_f32 on its operands. n_jobs outside 1 .. 8, M outside 1 .. 8, a K / lda / ldw that ltx_op_gemv_f32 refuses, or a NULL
 * a / W / out with N > 0: LTX_ERR_INVALID_CONFIGURATION. Every check comes before the launch: a refused call writes nothing. */
int ltx_op_gemv_group(ltx_ctx* ctx, const ltx_gemv_job* jobs, int n_jobs, int M);
/* One job of ltx_op_gemv_group_q: ltx_gemv_job with W as affine-quantised codes (MLX QuantizedLinear's layout, group 64 along K). */
typedef struct ltx_gemv_job_q {
    const float* a;         /* [M][lda] f32 */
    long lda;               /* lda % 4 == 0 */
    const uint8_t* codes;   /* [N][K * bits / 8]: 8 bits one code per byte; 4 bits two per byte, the even element in the low nibble */
    const uint16_t* scales; /* [N][K / 64] bf16 */
    const uint16_t* biases; /* [N][K / 64] bf16 */
    const float* bias;      /* [N] f32 or NULL */
    float* out;             /* [M][ldo] f32; may point into the middle of a wider row */
    long ldo;
    int N;                  /* 0: the job is skipped */
    int K;                  /* K % 64 == 0 */
    int in_act;             /* 0 none, 2 SiLU on the activations */
} ltx_gemv_job_q;
/* ltx_op_gemv_group on quantised weights, as a quantised dual model runs its timestep path (LTX2Transformer.swift:272-312 on the
 * QuantizedLinear modules quantize(model:) leaves, LTXPipeline.swift:487-492): every job is bit-equal to ltx_op_gemv_f32 on
 * W = bf16(q * scale + bias). bits is 8 or 4, one value per launch. n_jobs outside 1 .. 8, M outside 1 .. 8, other bits, K % 64 != 0,
 * lda % 4 != 0 or a NULL a / codes / scales / biases / out with N > 0: LTX_ERR_INVALID_CONFIGURATION before the launch, nothing
 * written. */
int ltx_op_gemv_group_q(ltx_ctx* ctx, const ltx_gemv_job_q* jobs, int n_jobs, int M, int bits);
/* O = softmax(Q K^T * scale + bias) V ; Q [B][Tq][H*128], K [B][Tk][H*128], Vt [B][H*128][ldvt] (keys contiguous,
 * ldvt >= roundup(Tk,64)), bias [B][Tk] f32 or NULL, O [B][Tq][H*128] ; all bf16. scale <= 0: Q already carries
 * (1/sqrt(128)) * log2(e) - what the DiT's q-norm + RoPE pass writes, one rounding to bf16 - and the scores are base-2 exponents:
 * O = softmax_2(Q K^T + bias * log2(e)) V: the bias is in the reference's units (added after the scale) in both modes.
 * Columns Tk..ldvt-1 of Vt are read and must hold finite values (they are multiplied by P = 0); here and in ltx_op_attention_hd. */
int ltx_op_attention(ltx_ctx* ctx, const uint16_t* Q, const uint16_t* K, const uint16_t* Vt, long ldvt,
                     const float* bias, int B, int H, int Tq, int Tk, float scale, uint16_t* O);
/* Number of key ranges the attention launcher divides a launch of this shape into when it has a workspace (1 = it does not): few
 * queries against many keys - the cross-attention of a 128-token clip is 32 workgroups walking 16 key tiles each - run one workgroup
 * per (query block, head, key range) and a combine pass (attention.h, AttnArgs::split_ws). ltx_op_attention and the DiT forward
 * both lend that workspace. No reference counterpart: MLXFast.scaledDotProductAttention (LTXAttention.swift:209) is one call. */
int ltx_attention_key_splits(int B, int H, int Tq, int Tk);
/* ltx_op_attention with a head dim (64 or 128): at 128 it IS ltx_op_attention; at 64 (LTXAttention at 32 heads x 64,
 * LTXAttention.swift:192-214) the layouts are Q / K / O [B][T][H*64], Vt [B][H*64][ldvt], and scale <= 0 means Q carries
 * (1/sqrt(64)) * log2(e). Launches at head dim 64 are never key-split. */
int ltx_op_attention_hd(ltx_ctx* ctx, const uint16_t* Q, const uint16_t* K, const uint16_t* Vt, long ldvt, const float* bias, int B, int H,
                        int Tq, int Tk, int head_dim, float scale, uint16_t* O);
/* Test seam: queries per workgroup the launcher picks for a head-dim-64 launch of this shape, 256, 128 or 64 by grid fill (0: not head
 * dim 64), so that the tests can show they reach every instance of the kernel. No reference counterpart, as ltx_attention_key_splits. */
int ltx_attention_hd_workgroup_queries(int B, int H, int Tq, int head_dim);
/* adaLN: out = norm(x) * (1+scale) + shift -> bf16 ; norm_kind 0 RMS, 1 LayerNorm; scale/shift [D] or NULL */
int ltx_op_norm_mod(ltx_ctx* ctx, const float* x, const float* scale, const float* shift, int rows, int D,
                    int norm_kind, float eps, int round_norm_bf16, uint16_t* out);
/* q/k RMSNorm (weight w[D]) + split RoPE (cos/sin [T][D/2] or NULL) -> bf16 */
int ltx_op_qknorm_rope(ltx_ctx* ctx, const float* x, long ldx, const float* w, const float* cos_t, const float* sin_t,
                       int T, int rows, int D, float eps, uint16_t* out);
/* ltx_op_qknorm_rope with a head dim (64 or 128) and the folded output scale: head h of a row is columns h*head_dim .., rotated as its
 * two halves with columns h*head_dim/2 .. of the cos/sin row [T][D/2] (applySplitRotaryEmb, LTXRoPE.swift:84-149); the norm is across
 * the whole row (LTXAttention.swift:145-149,179-180); out_scale multiplies the row before its one rounding to bf16. */
int ltx_op_qknorm_rope_hd(ltx_ctx* ctx, const float* x, long ldx, const float* w, const float* cos_t, const float* sin_t, int T, int rows,
                          int D, int head_dim, float out_scale, float eps, uint16_t* out);
/* ltx_op_norm_mod with every argument of the launcher (test seam: the shapes and strides the DiT passes select kernels the call above
 * cannot reach): x [rows][ldx] f32, out [rows][ldo] bf16, the modulation row of output row r is scale/shift + b * mod_bstride with
 * b = row_map ? row_map[r] : r / rows_per_batch (row_map: device int32 [rows] or NULL; per-token timestep groups of image-to-video). */
int ltx_op_norm_mod_ex(ltx_ctx* ctx, const float* x, long ldx, const float* scale, const float* shift, long mod_bstride,
                       int rows_per_batch, const int32_t* row_map, int rows, int D, int norm_kind, float eps,
                       int round_norm_bf16, uint16_t* out, long ldo);
/* ltx_op_qknorm_rope for the q and k of a fused projection in ONE launch, as the DiT's self-attention runs it (test seam): job 0
 * (x0, w0, out0) and job 1 (x1 == NULL: one job) share ldx, ldo and the tables; rows are f32, or bf16 at the same element offsets
 * with x_bf16 != 0 (ldx counts elements of that type); out_scale0 multiplies job 0's row before its one rounding to bf16 (the folded
 * softmax scale), job 1's is 1. */
int ltx_op_qknorm_rope_pair(ltx_ctx* ctx, const void* x0, const float* w0, uint16_t* out0, const void* x1, const float* w1,
                            uint16_t* out1, long ldx, long ldo, const float* cos_t, const float* sin_t, int T, int rows, int D,
                            float eps, float out_scale0, int x_bf16);
/* 1 when the VAE decoder's upsampler conv C -> 4C at (F, H, W) carries the next stage's first PixelNorm in its epilogue (the conv
 * launcher's own rule, which the decoder asks; options "conv_halo" and the 32-bit offset limits of the halo-staged kernels enter it),
 * 0 when that PixelNorm runs as a row pass. Host-side, no device. */
int ltx_conv_takes_d2s_pn(int F, int H, int W, int C);
/* The tile configuration the GEMM launcher picks for a dense launch C[M][N] = A[M][K] . B[N][K]^T (+ bias_n, activation `act`)
 * without split-K on a device of `ncu` CUs: 21 = 192x128 ring, 1 = 192x128 two-stage, 75 = 192x256, 76 = 384x256, ... flags: 1 f32
 * output, 2 bf16 output, 4 gated residual, 8 transposed bf16 output, 16 per-row bias. Reads option "gemm_tall". -1 on a shape no
 * launch takes. Host-side, no device. */
int ltx_gemm_dense_tile_cfg(int M, int N, int K, int act, int flags, int ncu);
/* The audio leg's convolutions (csrc/audio_conv.hip), one launch family: x channels-last bf16, f32 accumulation. tile: -1 auto, else
 * the instance by output-channel width (128, 64, 32). Cin must be a multiple of 32. Epilogue arguments as the launcher takes them:
 * resid f32 (same layout as out_f32) is added; f32_act 0 none / 2 tanh; transposed != 0 stores out_f32 as [Cout][rows]; out_bf16
 * [rows][Cout] receives act(v) with bf16_act 0 none / 1 LeakyReLU(slope). Either output may be NULL, not both.
 * ltx_op_conv1d: Conv1d with "same" padding (Vocoder.swift:34-51): x [L][Cin], w [Cout][k][Cin] (tap-major), odd k <= 16. */
int ltx_op_conv1d(ltx_ctx* ctx, const uint16_t* x, int L, int Cin, const uint16_t* w, const float* bias, int Cout, int k, int dilation,
                  int tile, const float* resid, int f32_act, int transposed, float* out_f32, int bf16_act, float slope,
                  uint16_t* out_bf16);
/* ConvTransposed1d (Vocoder.swift:81-102) as `stride` phase launches: x [L][Cin], w in the PyTorch layout [Cin][Cout][k],
 * padding == (k - stride) / 2 -> out [stride * L][Cout]. */
int ltx_op_conv_transpose1d(ltx_ctx* ctx, const uint16_t* x, int L, int Cin, const uint16_t* w, const float* bias, int Cout, int k,
                            int stride, int padding, int tile, float* out_f32, int bf16_act, float slope, uint16_t* out_bf16);
/* AudioCausalConv2d (AudioVAE.swift:37-104), ksize 3 or 1: x [H][W][Cin], w [Cout][ksize*ksize][Cin] (tap = kh*ksize + kw); output row
 * h sees input rows h-2 .. h only -> out [H][W][Cout]. */
int ltx_op_conv2d_causal(ltx_ctx* ctx, const uint16_t* x, int H, int W, int Cin, const uint16_t* w, const float* bias, int Cout, int ksize,
                         int tile, const float* resid, int transposed, float* out_f32, uint16_t* out_bf16);
/* deterministic device fills used by bench.py to create synthetic inputs */
int ltx_op_fill_normal_bf16(ltx_ctx* ctx, uint16_t* p, long n, uint64_t seed, float mean, float stddev);
int ltx_op_fill_normal_f32(ltx_ctx* ctx, float* p, long n, uint64_t seed, float mean, float stddev);

/* ---- Gemma-3 text encoder (csrc/gemma.h): token ids + attention mask -> the hidden states ltx_connector_encode* consumes ----
 * Reference: Gemma3Model.swift (Gemma3Attention, Gemma3MLP, Gemma3DecoderLayer, Gemma3InnerModel.callAsFunction), Gemma3Config.swift,
 * Gemma3WeightLoader.swift; call sites LTXPipeline.swift:1155-1170 and :3194-3277. Only the hidden-state extraction with an attention
 * mask: no tokenizer (token ids are inputs), no sliding-window masking (T <= sliding_window). Token generation on a KV cache is the
 * ltx_lm_ section below. */
typedef struct ltx_gemma_config {
    int hidden_size;             /* 3840 */
    int num_hidden_layers;       /* 48 */
    int intermediate_size;       /* 15360 */
    int num_attention_heads;     /* 16 */
    int head_dim;                /* 256; nothing else is accepted */
    int num_key_value_heads;     /* 8 */
    int vocab_size;              /* 262208 */
    float rms_norm_eps;          /* 1e-6 */
    float rope_theta;            /* 1e6: global layers, (i + 1) % sliding_window_pattern == 0 */
    float rope_local_base_freq;  /* 1e4: sliding layers */
    float query_pre_attn_scalar; /* 256: softmax scale = its inverse square root */
    int sliding_window;          /* 1024: the longest sequence encoded */
    int sliding_window_pattern;  /* 6 */
} ltx_gemma_config;
void ltx_gemma_config_default(ltx_gemma_config* cfg);
/* paths: the n_paths safetensors shards of one checkpoint. Module keys of the reference (model.embed_tokens, model.layers.N.self_attn.
 * {q,k,v,o}_proj / q_norm / k_norm, the four layer norms, mlp.{gate,up,down}_proj, model.norm), with or without the language_model.
 * prefix; lm_head* is ignored. A weight may be bf16 / f16 / f32 (rounded to bf16) or MLX affine-quantised (weight as packed uint32 +
 * scales + biases, group size 64, 4 or 8 bits; the three tensors of one Linear in the same shard), which is de-quantised to bf16 once,
 * here. A missing parameter is weightLoadingFailed
 * and named in the message. cfg NULL = the reference's defaults. */
int ltx_gemma_load(ltx_ctx* ctx, const char* const* paths, int n_paths, const ltx_gemma_config* cfg);
int ltx_gemma_init_synthetic(ltx_ctx* ctx, const ltx_gemma_config* cfg, unsigned long seed);
int ltx_gemma_unload(ltx_ctx* ctx);
/* device bytes the encoder holds now: parameters (+ RoPE tables), and activation workspaces; both 0 without a model */
int ltx_gemma_memory_info(ltx_ctx* ctx, long* weight_bytes, long* workspace_bytes);
/* token_ids, attention_mask [B][T] int32; hidden [num_hidden_layers + 1][B][T][hidden_size] bf16 - slot 0 the scaled embedding, slot
 * i + 1 the output of layer i, the last slot model.norm of the last layer: the connector's input. The mask must be left-padded
 * (0..0 1..1, at least one 1 per row) and T <= sliding_window, else invalidConfiguration. DEVICE pointers; ids outside [0, vocab) are
 * clamped. Waits for the stream once (the mask check) before the layers are queued. */
int ltx_gemma_encode_dev(ltx_ctx* ctx, const int32_t* token_ids, const int32_t* attention_mask, int B, int T, uint16_t* hidden);
/* HOST-pointer variant; ids outside [0, vocab) are invalidConfiguration. */
int ltx_gemma_encode(ltx_ctx* ctx, const int32_t* token_ids, const int32_t* attention_mask, int B, int T, uint16_t* hidden);
/* ltx_gemma_encode_dev into a buffer of the encoder's, then ltx_connector_encode_dev (left padding) on it: token ids -> the context
 * [B][T][dim] and all-ones mask the denoise entries take. Bit-equal to the two calls in turn. DEVICE pointers. */
int ltx_text_encode_dev(ltx_ctx* ctx, const int32_t* token_ids, const int32_t* attention_mask, int B, int T, uint16_t* context,
                        int32_t* out_mask);
/* HOST-pointer variant of ltx_text_encode_dev: only the ids, the mask and the context cross the bus; the hidden states (385 MB per
 * batch element at 49 x 1024 x 3840) stay on the device. Ids outside [0, vocab) are invalidConfiguration. out_mask may be NULL. */
int ltx_text_encode(ltx_ctx* ctx, const int32_t* token_ids, const int32_t* attention_mask, int B, int T, uint16_t* context, int32_t* out_mask);
/* The same two wrappers over ltx_connector_encode_av_dev: token ids -> the video context, the audio context and the mask
 * (LTXTextEncoder.swift:705-713). No audio set: LTX_ERR_MODEL_NOT_LOADED before the encoder runs. DEVICE pointers. */
int ltx_text_av_encode_dev(ltx_ctx* ctx, const int32_t* token_ids, const int32_t* attention_mask, int B, int T, uint16_t* video_context,
                           uint16_t* audio_context, int32_t* out_mask);
/* HOST-pointer variant. */
int ltx_text_av_encode(ltx_ctx* ctx, const int32_t* token_ids, const int32_t* attention_mask, int B, int T, uint16_t* video_context,
                       uint16_t* audio_context, int32_t* out_mask);
/* Test seams of the encoder's kernels (DEVICE pointers).
 * ltx_op_attention_causal: causal grouped-query attention over left-padded keys. Q / O [B][T][Hq*head_dim], K [B][T][Hkv*head_dim],
 * Vt [B][Hkv*head_dim][ldvt] bf16, key_start int32 [B] or NULL; query i attends keys key_start[b] <= j <= i, rows i < key_start[b] of O
 * are zeros. Only head_dim == 256; anything else is invalidConfiguration. ldvt >= T rounded up to 64 (and a multiple of 8); columns
 * T..ldvt-1 of Vt, and the K / V rows below key_start, are read and must hold FINITE values: they are multiplied by P = 0, so an Inf
 * or NaN there would come out as NaN. */
int ltx_op_attention_causal(ltx_ctx* ctx, const uint16_t* Q, const uint16_t* K, const uint16_t* Vt, long ldvt, const int32_t* key_start,
                            int B, int Hq, int Hkv, int T, int head_dim, float scale, uint16_t* O);
/* The same launch with every stride of the launcher (elements): row strides ldq / ldk / ldo, Vt row stride ldvt and the four batch
 * strides, so an operand may be a view into a longer buffer - the encoder reads Q and K out of one fused [B*T][(Hq+Hkv)*256] row buffer
 * and Vt out of a workspace of row stride roundup(T, 64). The Vt columns from T to ldvt-1 are read (those below roundup(T, 64)) and must be finite.
 * ltx_op_attention_causal is this call with dense operands. No product path calls it. */
int ltx_op_attention_causal_ld(ltx_ctx* ctx, const uint16_t* Q, long ldq, long q_bstride, const uint16_t* K, long ldk, long k_bstride,
                               const uint16_t* Vt, long ldvt, long vt_bstride, const int32_t* key_start, int B, int Hq, int Hkv, int T,
                               int head_dim, float scale, uint16_t* O, long ldo, long o_bstride);
/* r, x, h, n dense [rows][D] bf16; w, w2 [D] f32 (the stored weights; the kernel forms bf16(1 + w)). x NULL: h = norm(r); else
 * h = x + norm(r). w2 and n together: n = norm2(h) too. h NULL (with w2, n): only n is written. */
int ltx_op_gemma_norm(ltx_ctx* ctx, const uint16_t* r, const float* w, const uint16_t* x, const float* w2, int rows, int D, float eps,
                      uint16_t* h, uint16_t* n);
/* qk [rows][ld] bf16, in place: q_heads heads of 256 at column 0 (weight wq [256]), k_heads at column q_heads*256 (wk). Per head RMS
 * norm with bf16(1 + w), then half-split RoPE from cos / sin [T][128] f32 at position row % T. */
int ltx_op_gemma_qknorm_rope(ltx_ctx* ctx, uint16_t* qk, long ld, const float* wq, const float* wk, int q_heads, int k_heads,
                             const float* cos_t, const float* sin_t, int T, int rows, float eps);
/* cos / sin [T][128] f32 of positions 0 .. T-1, frequencies base^(-i/128), computed on the device */
int ltx_op_gemma_rope_tables(ltx_ctx* ctx, int T, float base, float* cos_t, float* sin_t);
/* gu [rows][2*I] bf16 (gate | up) -> out [rows][I] = bf16(bf16(gelu_tanh(gate)) * up) */
int ltx_op_geglu(ltx_ctx* ctx, const uint16_t* gu, int rows, int I, uint16_t* out);
/* out [rows][D] = bf16(table[ids[row]] * bf16(sqrt(D))); ids are clamped to [0, vocab) */
int ltx_op_gemma_embed(ltx_ctx* ctx, const int32_t* ids, const uint16_t* table, int rows, int D, int vocab, uint16_t* out);

/* ---- Gemma-3 token generation on a KV cache: prompt enhancement (csrc/gemma.h, csrc/gemma_generate.cpp) ----
 * Reference: Gemma3TextModel.generateTokens (Gemma3Model.swift:375-492) and the cache: path of Gemma3Attention (:73-110); the stage
 * config.enhancePrompt of LTXPipeline.swift. Runs on the model ltx_gemma_load / ltx_gemma_init_synthetic loaded (without one:
 * LTX_ERR_MODEL_NOT_LOADED). Batch 1; the tokenizer and the chat template stay outside: token ids in, token ids out. A session
 * (ltx_lm_begin .. ltx_lm_end) holds the per-layer K and V^T caches of `capacity` positions (capacity x 393 KB at the reference's
 * size), RoPE tables of that many positions and every buffer a step touches; nothing is allocated per token. The decode attention
 * covers ALL cached keys on every layer - the reference decodes with mask: .none on a KVCacheSimple - and the prefill, which builds no
 * window mask, refuses prompts longer than sliding_window (as ltx_gemma_encode does). Every refusal comes before the first launch. */
typedef struct ltx_lm_params {
    uint32_t struct_size;      /* sizeof(ltx_lm_params): set by ltx_lm_params_default */
    int max_new_tokens;        /* 512 */
    float temperature;         /* 0.7; <= 0: greedy, picked on the device (4 bytes per token cross the bus) */
    float top_p;               /* 0.95 */
    float repetition_penalty;  /* 1.1 */
    int repetition_context;    /* 64 */
    uint64_t seed;             /* the sampler's threefry key sequence: ltx_mlx_draw_key(seed, step) */
    int n_eos;                 /* 1; up to 8 */
    int32_t eos_ids[8];        /* {1} */
} ltx_lm_params;
void ltx_lm_params_default(ltx_lm_params* p);
/* Replaces a session the context already holds. */
int ltx_lm_begin(ltx_ctx* ctx, int capacity);
/* freed_bytes (may be NULL): what ltx_lm_memory_info reported, cache + workspace; 0 without a session. */
int ltx_lm_end(ltx_ctx* ctx, long* freed_bytes);
/* Device bytes the session holds: the K / V^T caches, and everything else it allocated at begin (tables, hidden slots, step rows,
 * logits, history, split workspace); zeros with a model and no session. The activation workspaces the prefill shares with the encoder
 * (T rows of every intermediate) are the model's and are reported by ltx_gemma_memory_info. */
int ltx_lm_memory_info(ltx_ctx* ctx, long* cache_bytes, long* workspace_bytes);
/* Resets the session and fills cache positions 0 .. T-1 from ids [T]. logits [vocab] f32 of the last position, or NULL. The logits
 * hold bf16-rounded values (the reference's asLinear on bf16 operands yields a bf16 array). DEVICE pointers; ids are clamped. */
int ltx_lm_prefill_dev(ltx_ctx* ctx, const int32_t* ids, int T, float* logits);
/* HOST pointers; ids outside [0, vocab) are invalidConfiguration. */
int ltx_lm_prefill(ltx_ctx* ctx, const int32_t* ids, int T, float* logits);
/* One token at the next position: token int32 [1] and logits [vocab] or NULL, DEVICE pointers. */
int ltx_lm_step_dev(ltx_ctx* ctx, const int32_t* token, float* logits);
/* HOST variant: the token by value, logits a host array or NULL. */
int ltx_lm_step(ltx_ctx* ctx, int32_t token, float* logits);
/* Debug seams (HOST pointers): model.norm of the newest position [hidden_size] bf16 - the logits projection's input; and rows
 * 0 .. rows-1 of a layer's K cache, [rows][num_key_value_heads * 256] bf16; and columns 0 .. cols-1 of every row of a layer's V^T
 * cache, [num_key_value_heads * 256][cols] bf16, 1 <= cols <= the padded width roundup(capacity, 64) - the columns past the filled
 * positions are the session's own and zero since ltx_lm_begin. */
int ltx_lm_last_state(ltx_ctx* ctx, uint16_t* state);
int ltx_lm_cache_k(ltx_ctx* ctx, int layer, int rows, uint16_t* k);
int ltx_lm_cache_vt(ltx_ctx* ctx, int layer, int cols, uint16_t* vt);
/* Prefill + the generate loop: pick, stop-id check, append, step. ids HOST [T]; out_tokens HOST [max_new_tokens]; *n_out tokens are
 * written (a stop id ends the run and is not written). T + max_new_tokens must fit the session's capacity. params NULL: defaults. */
int ltx_lm_generate(ltx_ctx* ctx, const int32_t* ids, int T, const ltx_lm_params* params, int32_t* out_tokens, int* n_out);
/* The sampler of temperature > 0, pure host code (no context, no device) and THIS library's own definition: the
 * repetition penalty in place on logits - every distinct id among the last min(context, n_generated) of `generated`:
 * l > 0 ? l / penalty : l * penalty -, softmax of l / temperature in f64, the nucleus = the fewest tokens in decreasing probability
 * (ties: the lower id) whose mass reaches top_p, one inverse-CDF draw with the uniform (w >> 8) * 2^-24, w = word 0 of
 * threefry2x32(ltx_mlx_draw_key(seed, step), {0, 0}). temperature <= 0: argmax, ties to the lowest id. */
int ltx_lm_sample_host(float* logits, int vocab, const int32_t* generated, int n_generated, int context, float penalty, float temperature,
                       float top_p, uint64_t seed, int step, int32_t* token);
/* Test seams of the generation kernels (DEVICE pointers).
 * ltx_op_gemv_bf16: out[n] = sum_k x[k] W[n][k], bf16 x bf16, f32 accumulation, one rounding at the store; M must be 1. epilogue 0:
 * out_bf16[n * out_stride] = bf16(sum); 1: out_f32[n] = the bf16-rounded sum as f32; 2 (GeGLU): W is [2N][ldw], gate rows then up
 * rows, out_bf16[n * out_stride] = bf16(bf16(gelu_tanh(bf16(g))) * bf16(u)). Any N; K % 8 == 0, K <= 16384; ldw % 8 == 0. */
int ltx_op_gemv_bf16(ltx_ctx* ctx, const uint16_t* x, const uint16_t* W, long ldw, int M, int N, int K, int epilogue, uint16_t* out_bf16,
                     long out_stride, float* out_f32);
/* output rows per workgroup of that launch (8 or 16): tests place rows on both sides of its multiples. Host-side. */
int ltx_gemv_bf16_rows_per_workgroup(int N, int epilogue);
/* ltx_op_attention_decode: one query q [Hq*256] against the first n_keys rows of K [cap][ldk] and columns of Vt [Hkv*256][ldvt]
 * (ldvt >= n_keys rounded up to 64), O [Hq*256], all bf16; query head h reads K/V head h / (Hq / Hkv), up to 4 per K/V head. K rows and
 * Vt columns at or past n_keys never influence O, whatever they hold. The split workspace is the context's. */
int ltx_op_attention_decode(ltx_ctx* ctx, const uint16_t* q, const uint16_t* K, long ldk, const uint16_t* Vt, long ldvt, int Hq, int Hkv,
                            int n_keys, float scale, uint16_t* O);
/* ltx_op_lm_pick: repetition penalty (ltx_lm_sample_host's rule, over hist [n_gen] int32; the penalised values are written back to
 * logits [vocab] f32), then argmax with ties to the lowest index; the token goes to out [1] and to hist[n_gen] (hist NULL: n_gen
 * must be 0). Logits are finite by construction; what a NaN does to the pick is unspecified. */
int ltx_op_lm_pick(ltx_ctx* ctx, float* logits, int vocab, int32_t* hist, int n_gen, int context, float penalty, int32_t* out);

/* Test seams of the helper passes around the matrix cores: guidance, scheduler, VAE, latent upscaler and connector. DEVICE pointers
 * throughout; each call is one launch on the context's stream and returns without waiting. A null required pointer or an empty shape
 * is invalidConfiguration. No model has to be loaded, and no product path goes through these.
 * stats[b] = {mean, population variance} of the n_per_batch f32 values of segment b (two passes: the mean, then the deviations) */
int ltx_op_mean_var(ltx_ctx* ctx, const float* x, long n_per_batch, int B, float* stats);
/* cfg [B][n_per_batch] f32, in place: cfg = phi * cfg * (std_cond / std_cfg) + (1 - phi) * cfg, std = sqrt(var + 1e-8) of the
 * ltx_op_mean_var pairs stats_cfg / stats_cond [B][2] (LatentUtils.swift:164-183) */
int ltx_op_guidance_rescale(ltx_ctx* ctx, float* cfg, const float* stats_cfg, const float* stats_cond, float phi, long n_per_batch, int B);
/* x [BC][n_per_chan] f32, in place: y = (x - mean) / (sqrt(var) + 1e-8) * sqrt(var_ref) + mean_ref per channel;
 * x = factor >= 1 ? y : factor * y + (1 - factor) * x (LatentUtils.swift:201-227). stats_x / stats_ref [BC][2] {mean, var}. */
int ltx_op_adain(ltx_ctx* ctx, float* x, const float* stats_x, const float* stats_ref, float factor, long n_per_chan, int BC);
/* GroupNorm over channels-last x [P][C] f32 with G groups of C / G adjacent channels (SpatialUpscaler.swift:14-58):
 * stats[g] = {mean, 1 / sqrt(population variance + eps)} over all positions of the group's channels */
int ltx_op_groupnorm_stats(ltx_ctx* ctx, const float* x, long P, int C, int G, float eps, float* stats);
/* y = (x - mean_g) * rstd_g * w[c] + b[c]; resid [P][C] f32 (or NULL) is added, then SiLU when act_silu. Written as f32 [P][C]
 * and / or bf16 [P][C] (either may be NULL, not both); out_f32 may alias resid. */
int ltx_op_groupnorm_apply(ltx_ctx* ctx, const float* x, const float* stats, const float* w, const float* b, const float* resid,
                           int act_silu, float* out_f32, uint16_t* out_bf16, long P, int C, int G);
/* x [P][C] f32 -> out [P][C] bf16 = SiLU(x / sqrt(mean_c(x^2) + 1e-8) * scale[c] + shift[c]); scale and shift [C] f32 or both NULL
 * (scale 1, shift 0). scale already holds the + 1. C % 4 == 0, C <= 2048 (VideoDecoder.swift:29-32, :118-127). */
int ltx_op_pixelnorm_silu(ltx_ctx* ctx, const float* x, const float* scale, const float* shift, uint16_t* out, long P, int C);
/* latent element (c, p) at [c * chan_stride + p], f32 (chan_stride >= P: a temporal tile is a view of a longer latent); noise, when
 * not NULL, in the same layout: v = noise * noise_scale + (1 - noise_scale) * latent. out [P][C] bf16 = v * std[c] + mean[c]
 * (VideoDecoder.swift:366-381). */
int ltx_op_vae_prepare(ltx_ctx* ctx, const float* latent, long chan_stride, const float* noise, float noise_scale, const float* mean,
                       const float* std_, uint16_t* out, int C, long P);
/* x [P][C] f32 -> out [C][P] f32 = (x - mean[c]) / std[c] (SpatialUpscaler.swift:352-379) */
int ltx_op_upscaler_finish(ltx_ctx* ctx, const float* x, const float* mean, const float* std_, float* out, long P, int C);
/* r, nx [n_frames][frame_elems] f32; r[i] = r[i] * (1 - i / n_frames) + nx[i] * (i / n_frames), in place (VideoDecoder.swift:561-592) */
int ltx_op_blend_frames(ltx_ctx* ctx, float* r, const float* nx, int n_frames, long frame_elems);
/* latent [B][C][T] f32 -> tokens [B][T][C] bf16 (LatentUtils.swift:20-34), and tokens [B][T][C] f32 -> latent [B][C][T] f32 (:42-54) */
int ltx_op_patchify_bf16(ltx_ctx* ctx, const float* latent, uint16_t* tokens, int B, int C, int T);
int ltx_op_unpatchify_f32(ltx_ctx* ctx, const float* tokens, float* latent, int B, int C, int T);
/* latent, velocity [n] f32: den = x - sigma * v; x = sigma_next > 0 ? den + sigma_next * (x - den) / sigma : den, in place
 * (LTXScheduler.swift:305-327). skip_hw > 0: the latent is [C][frames][skip_hw] and frame 0 of every channel is left as it is. */
int ltx_op_euler_step(ltx_ctx* ctx, float* latent, const float* velocity, float sigma, float sigma_next, long n, int skip_hw, int frames);
/* latent [C][F][HW] f32: frame 0 of every channel = cond [C][HW], or cond + (scale * noise) * sigma2 with noise [C][HW] (three
 * separately rounded f32 operations); frames >= 1 are not touched (LTXPipeline.swift:2092-2094, :2225-2229) */
int ltx_op_set_frame0(ltx_ctx* ctx, float* latent, const float* cond, const float* noise, float scale, float sigma2, int C, int F, int HW);
/* mod [B][L][J][D] = tables [L][J][D] + ada [B][J][D], f32 (LTXTransformerBlock.swift:163-185) */
int ltx_op_make_mod(ltx_ctx* ctx, const float* tables, const float* ada, float* mod, int B, int L, int J, int D);
/* The connector's feature statistics (LTXTextEncoder.swift:62-122). hidden [states][B][T][D] bf16, mask [B][T] int32; the valid
 * tokens of row b are its last n_b (first n_b with padding_right), n_b = the number of non-zero mask entries. stats[(l*B + b)*2] =
 * {sum over valid tokens / (n_b * D + eps), (max - min over valid tokens) + eps}. partials: scratch of
 * ltx_fe_stats_partials_floats(states, B, T, D) floats (0 for an empty shape). D % 8 == 0. */
long ltx_fe_stats_partials_floats(int states, int B, int T, int D);
int ltx_op_fe_stats(ltx_ctx* ctx, const uint16_t* hidden, const int32_t* mask, int states, int B, int T, int D, int padding_right,
                    float eps, float* partials, float* stats);
/* out [B][T][D * states] bf16: out[b][t][d * states + l] = bf16(8 * (x - mean) / (range + eps)) with the ltx_op_fe_stats pair of plane
 * (l, b) for a valid token, zero for a padded one */
int ltx_op_fe_norm_concat(ltx_ctx* ctx, const uint16_t* hidden, const int32_t* mask, const float* stats, int states, int B, int T, int D,
                          int padding_right, float eps, uint16_t* out);

/* Test seams of the remaining helper passes: the guidance combines, the casts, the timestep embedding, the connector's registers, the
 * VAE encoder's passes and the audio row passes. Same rules as above: DEVICE pointers, one launch on the context's stream, a null
 * required pointer, an empty shape or a shape the launcher does not take is invalidConfiguration before anything is launched.
 * out = cond + (scale - 1) * (cond - uncond) (LatentUtils.swift:131-141) */
int ltx_op_cfg_combine(ltx_ctx* ctx, const float* uncond, const float* cond, float scale, float* out, long n);
/* out = ca * a + cb * b */
int ltx_op_lincomb(ltx_ctx* ctx, const float* a, const float* b, float ca, float cb, float* out, long n);
/* out = cb * a + ca * (a - b) (STG, LTXPipeline.swift:920) */
int ltx_op_axpby(ltx_ctx* ctx, const float* a, const float* b, float ca, float cb, float* out, long n);
/* out = g * (a - b) + b (GE momentum, LTXPipeline.swift:924-927) */
int ltx_op_ge(ltx_ctx* ctx, const float* a, const float* b, float g, float* out, long n);
/* x *= s, in place */
int ltx_op_scale_inplace(ltx_ctx* ctx, float* x, float s, long n);
/* x = min(max((x + 1) / 2, 0), 1), in place (VideoDecoder.swift:501-505) */
int ltx_op_clip01(ltx_ctx* ctx, float* x, long n);
/* bias = (1 - mask) * -10000 as f32: exactly -10000 for 0 and +0 for 1 (LTXTransformer.swift:141-156) */
int ltx_op_mask_to_bias(ltx_ctx* ctx, const int32_t* mask, float* bias, long n);
/* f32 -> bf16, round to nearest even, and bf16 -> f32 */
int ltx_op_cast_f32_bf16(ltx_ctx* ctx, const float* x, uint16_t* out, long n);
int ltx_op_cast_bf16_f32(ltx_ctx* ctx, const uint16_t* x, float* out, long n);
/* out [n][dim] f32: row r = [cos(t f_k) | sin(t f_k)], k < dim / 2, t = ts[r] * mult, f_k = exp(-ln(10000) * k / (dim / 2))
 * (LTXTimestepEmbedding.swift:17-54). dim even. */
int ltx_op_timestep_embedding(ltx_ctx* ctx, const float* ts, float mult, float* out, int n, int dim);
/* The VAE's modulation tables, n jobs (1 .. ltx_vae_mods_max_jobs()) in one launch: out [rows][C] = table [rows][C] + (te ? te : 0) +
 * (row odd ? 1 : 0) (VideoDecoder.swift:93-113). te may be NULL. */
typedef struct ltx_vae_mods_job {
    const float* table;
    const float* te;
    float* out;
    int rows, C;
} ltx_vae_mods_job;
int ltx_vae_mods_max_jobs(void);
int ltx_op_vae_make_mods_batch(ltx_ctx* ctx, const ltx_vae_mods_job* jobs, int n);
/* gathered [N][D][Tn] bf16 -> vt [D][ld] bf16 with rank r's keys at columns r * Tn ..; columns N * Tn .. ld-1 are not written.
 * Tn % 8 == 0, ld % 8 == 0, ld >= N * Tn. */
int ltx_op_sp_vt_interleave(ltx_ctx* ctx, const uint16_t* gathered, uint16_t* vt, int N, int D, int Tn, long ld);
/* mask [B][T] int32 -> src [B][T] int32: position p keeps a token where mask[T-1-p] != 0 and then holds the index of the p-th entry
 * of (the valid tokens in order, then the padded ones); elsewhere -1, a learnable register (LTXTextEncoder.swift:428-470) */
int ltx_op_register_plan(ltx_ctx* ctx, const int32_t* mask, int B, int T, int32_t* src);
/* x [B][T][D] f32: row (b, p) = src[b][p] >= 0 ? enc[b][src[b][p]] (bf16 [B][T][D]) : registers[p % R] (f32 [R][D]). R >= 1. */
int ltx_op_register_gather(ltx_ctx* ctx, const uint16_t* enc, const float* registers, const int32_t* src, int B, int T, int D, int R,
                           float* x);
/* pixels [3][T][H][W] f32 -> out [T][H/4][W/4][64] bf16, channel c * 16 + pw * 4 + ph, channels 48 .. 63 zero (VideoEncoder.swift:25-31).
 * H % 4 == 0, W % 4 == 0. */
int ltx_op_enc_patchify(ltx_ctx* ctx, const float* pixels, uint16_t* out, int T, int H, int W);
/* conv [T][H][W][Cc], x [T][H][W][Cx] f32 -> out [T2][H/fh][W/fw][Cout] f32 = s2d(conv) + mean over groups of G = Cx * S / Cout
 * adjacent channels of s2d(x), S = ft * fh * fw; s2d channel c * S + (it * fh + ih) * fw + iw; T is padded in FRONT with copies of
 * frame 0 to a multiple of ft (VideoEncoder.swift:146-167). Cc * S == Cout, (Cx * S) % Cout == 0, H % fh == 0, W % fw == 0. */
int ltx_op_enc_s2d_residual(ltx_ctx* ctx, const float* conv, int Cc, const float* x, int Cx, float* out, int Cout, int T, int H, int W,
                            int ft, int fh, int fw);
/* z [P][ldz] f32 (first C columns) -> out [C][P] f32 = mean ? (z - mean[c]) / std_[c] : z; mean and std_ both or neither
 * (LTXPipeline.swift:1920-1927). ldz >= C. */
int ltx_op_enc_finish(ltx_ctx* ctx, const float* z, long ldz, const float* mean, const float* std_, float* out, int C, long P);
/* row_map [B][T] int32 = b * G + (t < first ? 1 : 0): the timestep group of every token of an image-to-video forward. 0 <= first <= T. */
int ltx_op_i2v_rowmap(ltx_ctx* ctx, int32_t* row_map, int B, int T, int first, int G);
/* ts [B * G + B] f32: ts[b * G + g] = g == 0 ? sigma : 0, then B audio timesteps = sigma. B * G + B <= 64. */
int ltx_op_i2v_timesteps(ltx_ctx* ctx, float* ts, int B, int G, float sigma);
/* p [n] int32 = v */
int ltx_op_fill_const_i32(ltx_ctx* ctx, int32_t* p, long n, int32_t v);
/* mask [B][T] int32 -> key_start[b] = index of the first 1 (T without one); status[b] = 1 when row b is 0..0 1..1 with at least one 1
 * and no value other than 0 and 1, else 0 */
int ltx_op_gemma_mask_scan(ltx_ctx* ctx, const int32_t* mask, int B, int T, int32_t* key_start, int32_t* status);
/* The audio row passes (AudioVAE.swift, Vocoder.swift). Each writes ONLY the interior of its haloed bf16 operand.
 * x [H][W][C] f32 -> out [(H+3)][W+2][C] at (h + 2, w + 1): mode 0 SiLU(x / sqrt(mean_c(x^2) + 1e-6)), mode 1 the plain cast */
int ltx_op_audio_pn_pad(ltx_ctx* ctx, const float* x, int H, int W, int C, int mode, uint16_t* out);
/* x [H][W][C] f32, nearest-2x -> out [(2H+2)][2W+2][C] at (u + 1, v + 1). C % 4 == 0. */
int ltx_op_audio_upsample_pad(ltx_ctx* ctx, const float* x, int H, int W, int C, uint16_t* out);
/* latent [Cl][T][Wl] f32 * std_[c * Wl + w] + mean[c * Wl + w] -> out [(T+3)][Wl+2][Cpad] at (t + 2, w + 1), channels < Cl only */
int ltx_op_audio_denorm_pad(ltx_ctx* ctx, const float* latent, const float* mean, const float* std_, int Cl, int T, int Wl, int Cpad,
                            uint16_t* out);
/* mel [2][T][M] f32 -> out [T][2 * M] bf16, column c * M + m */
int ltx_op_audio_mel_pack(ltx_ctx* ctx, const float* mel, int T, int M, uint16_t* out);
/* a, b, c [rows][C] f32 -> out [rows][ldb] bf16, columns < C: leaky((a + b + c) / 3, slope). C % 4 == 0, ldb % 4 == 0, ldb >= C. */
int ltx_op_audio_mean3_act(ltx_ctx* ctx, const float* a, const float* b, const float* c, long rows, int C, float slope, uint16_t* out,
                           long ldb);

#ifdef __cplusplus
}
#endif
#endif /* LTXHIP_H */
