// dual_model.h - LTX2Transformer.callAsFunction (LTX2Transformer.swift:254-392): the dual video + audio model above its blocks, as a
// host graph over the kernels dit_forward and dual_forward already run. Two latents, two text contexts and two timestep vectors in,
// two velocities out. A DualModel owns a DualStack (dual_block.h, the L blocks, filled at first_block = 0) and the top-level
// parameters of LTX2Transformer.swift:28-48: patchify_proj / audio_patchify_proj, the six AdaLayerNormSingle embedders (each
// emb.linear_1, emb.linear_2, linear), caption_projection / audio_caption_projection (linear_1, linear_2), scale_shift_table [2][Dv] /
// audio_scale_shift_table [2][Da], proj_out / audio_proj_out. norm_out / audio_norm_out are LayerNorm(affine: false): no weight.
// The joint denoise loop is dual_denoise.h; the CLI's --audio path is not here.
//
// Quantised storage (dual_model_quantize, the reference's quantize(model: ltx2, groupSize: 64, bits: 8 | 4), LTXPipeline.swift:487-492):
// every Linear of the model and of its blocks is held as codes + bf16 group scale / bias in ONE arena and the bf16 weights are
// released, as dit_quantize does for the DiT. The forward is the same graph: gemm_linear / gemm_vt hand a Linear without `w` to the
// few-row GEMM as codes (8 bits, M <= 256: every audio-stream GEMM of a block) or de-quantise it into the model's one scratch matrix,
// and the timestep path reads the codes in launch_gemv_group_q - each job bit-equal to the gemv on the de-quantised matrix. With
// option "qb_off" = 1 a quantised model's forward therefore equals, bit for bit, the bf16 model holding bf16(q * scale + bias).
//
// The text side of a forward (step 3 below and the K / V^T of the blocks' text cross-attentions) does not change within a prompt:
// dual_model_prepare_text runs it once into model-owned buffers and the stack's DualTextCache, and a forward with text_cache set reads
// those instead. Same launches, same operands, same bits as the forward that recomputes them.
//
// Audio timesteps are one value per batch element (audio_timesteps [B], sigma unscaled; the reference's audioTimestep is always
// [sigma]). Video timesteps are one value per (batch element, timestep GROUP): video_timesteps [B][n_groups] with video_row_map[b*Tv + t]
// = b*n_groups + group(b, t), as dit_forward groups them. That is the reference's per-token form (image-to-video,
// LTX2Transformer.swift:285-312) with each distinct timestep embedded once: the three video embedders run at M = B * n_groups rows and
// the three audio embedders at M = B, two launch_gemv_group launches per stage (a grouped launch shares one M); the video head builds
// its modulation for B * n_groups rows and picks them through the map. n_groups = 1 with no map keeps the single launch per stage and
// every launch of the forward as it was, with the same bits. B * n_groups <= 8 (the grouped gemv's limit on M).
//
// The graph, in the reference's order:
//   1. patchify: x_v = patchify_proj(video_latent), x_a = audio_patchify_proj(audio_latent) -> the two f32 residual streams
//   2. timestep path: two launch_timestep_embedding (sigma * timestep_scale_multiplier -> [B][256]), then the six embedders
//      (adaln_single 6 x Dv, audio_adaln_single 6 x Da, av_ca_video_scale_shift 4 x Dv, av_ca_a2v_gate 1 x Dv,
//      av_ca_audio_scale_shift 4 x Da, av_ca_v2a_gate 1 x Da) as THREE launch_gemv_group launches of six jobs: stage 1 256 -> D,
//      stage 2 D -> D with SiLU in, stage 3 D -> n x D with SiLU in. Stage 3 writes temb_v [B][6][Dv], temb_a [B][6][Da],
//      cross_video_ss [B][5][Dv] and cross_audio_ss [B][5][Da] in place: rows 0-3 of the last two from the scale-shift embedder, row 4
//      from the gate embedder (the reference's concatenation, :298-312). Video embedders read the video timestep, audio embedders
//      the audio timestep. The stage-2 outputs of adaln_single / audio_adaln_single are the embedded timesteps of the heads.
//      `ungrouped` runs the same 18 Linears as 18 launch_gemv_f32 launches: bit-equal, a measurement seam. On a quantised model
//      the same three grouping modes call launch_gemv_group_q on the codes (ungrouped = one job per launch of the same kernel);
//      ungrouped == 2 is the composed alternative that kernel replaces, per Linear launch_dequant into the scratch matrix +
//      launch_gemv_f32 (36 launches, bit-equal, a measurement seam; on a bf16 model it is `ungrouped`).
//   3. text: caption_projection / audio_caption_projection (Linear, GELU-tanh, Linear) -> the stack's two bf16 contexts; int32 masks
//      [B][S] -> additive biases (launch_mask_to_bias); a null mask is a null bias
//   4. blocks: dual_forward on the owned stack, unchanged
//   5. heads: LayerNorm(x) * (1 + table[1] + embedded_ts) + table[0] + embedded_ts -> proj_out, per stream, f32 velocities
// Launches above the blocks: 2 patchify GEMMs + 2 embeddings + 3 grouped gemv + 4 caption GEMMs + up to 2 mask passes + per head
// 1 modulation add, 1 norm, 1 GEMM = 19 (34 with `ungrouped`), plus split-K finish passes where a GEMM launcher chooses them.
//
// Rounding points above the blocks (the reference runs these Linears in the dtype of their input):
//   1. The latents and text contexts arrive as bf16. patchify_proj / audio_patchify_proj accumulate in f32 and the residual streams
//      start as the bf16-ROUNDED value held in f32, as dit_forward rounds its patchify output: the reference's patchify Linear is
//      bf16 x bf16 -> bf16. (dit_forward also rounds block 0's norm to bf16 for that reason; dual_forward, which stays unchanged,
//      does not.)
//   2. The whole timestep path is f32 activations x bf16 weights -> f32 (launch_gemv_f32's promotion): no rounding.
//   3. Caption projections: f32 accumulation, GELU-tanh on the f32 value, ONE rounding to bf16 for the hidden activation, one for
//      the projected context (the DiT's prepare_context).
//   4. Heads: the modulated LayerNorm row is computed in f32 and rounded to bf16 once, as the proj_out GEMM's operand; the
//      velocities are the GEMM's f32 accumulators + bias.
// Scratch grows to the largest shape seen; nothing is allocated per call after that. Every argument check comes before the first
// launch: a refused forward writes nothing.
#pragma once
#include <map>
#include <string>

#include "dual_block.h"

struct DualModelConfig {
    DualBlockConfig blocks;  // video_context_dim == video_dim and audio_context_dim == audio_dim: the caption projections' widths
    int in_channels = 128, out_channels = 128;
    int audio_in_channels = 128, audio_out_channels = 128;
    int caption_channels = 3840;
    float timestep_scale_multiplier = 1000.0f;
};

// one AdaLayerNormSingle (LTXTimestepEmbedding.swift:62-124): emb.linear_1 256 -> D, emb.linear_2 D -> D, linear D -> n x D
struct DualEmbedder {
    const char* name = nullptr;
    LinearW l1, l2, lin;
    int n = 0;           // numEmbeddings
    bool audio = false;  // reads the audio timestep, width Da
};
constexpr int kDualEmbedders = 6;

struct DualModel {
    DualModelConfig cfg;
    int Dv = 0, Da = 0;
    DualStack* stack = nullptr;
    LinearW patchify, audio_patchify, cap1, cap2, acap1, acap2, proj_out, audio_proj_out;
    DualEmbedder emb[kDualEmbedders];  // adaln_single, audio_adaln_single, av_ca_video_scale_shift, av_ca_a2v_gate, av_ca_audio_scale_shift, av_ca_v2a_gate
    float* sst_out_v = nullptr;  // [2][Dv]: row 0 shift, row 1 scale
    float* sst_out_a = nullptr;  // [2][Da]
    DeviceArena qarena;  // after dual_model_quantize: codes + group scales / biases of every Linear, the blocks' included
    DequantScratch dq;   // one scratch matrix for the whole model, sized by its largest Linear (adaln_single.linear: 24576 x 4096 at full width)
    int quant_bits = 16; // 16 (bf16), 8 or 4
    ParamTable params;  // the top-level parameters by module key (arena: biases and the two output tables; warena: Linear weights); the blocks' are stack->params

    // scratch
    DevBuf ws_xv, ws_xa;                              // f32 residual streams
    DevBuf ws_ctx_v, ws_ctx_a, ws_cap_h;              // projected contexts and the caption hidden activation (bf16, [B*S][max(Dv, Da)])
    DevBuf ws_bias_v, ws_bias_a;                      // [B][S] f32
    DevBuf ws_emb256, ws_h1, ws_h2;                   // [2][B][256]; stage-1 / stage-2 outputs of the six embedders, end to end
    DevBuf ws_temb_v, ws_temb_a, ws_cross_v, ws_cross_a;
    DevBuf ws_modout_v, ws_modout_a;                  // [B][2][D]
    DevBuf ws_xn;                                     // head operand (bf16)
    DevBuf ws_splitk;
    // what dual_model_prepare_text keeps for the cached forwards (never the per-forward scratch above): the projected contexts it
    // built the stack's K / V^T from, and the mask biases
    DevBuf tc_ctx_v, tc_ctx_a, tc_bias_v, tc_bias_a;
    bool tc_has_bias_v = false, tc_has_bias_a = false;

    ~DualModel();
};

DualModel* dual_model_create(const DualModelConfig& cfg);
void dual_model_destroy(DualModel* m);
// the distributions of dual_init_synthetic, for the blocks and the top-level parameters alike
void dual_model_init_synthetic(ltx_ctx* ctx, DualModel* m, uint64_t seed);
// Replaces loadTransformerWeights(includeAudio: true) (ModelDownloader.swift:605-639). Keys in the module's spelling or any spelling
// mapTransformerKey(includeAudio: true) maps onto it (ModelDownloader.swift:756-803): proj_in., time_embed.emb.timestep_embedder.,
// time_embed.linear., .emb.timestep_embedder. and the block spellings of dual_load. Fills the load report (tensors applied / missing
// / tensors that are no parameter); a parameter the file lacks is weightLoadingFailed.
void dual_model_load(ltx_ctx* ctx, DualModel* m, const std::string& path);
// a parameter by module key, top-level or "transformer_blocks.{i}."; null when there is none
const ParamSlot* dual_model_find(const DualModel* m, const std::string& name);
// MLXNN.quantize(model: ltx2, groupSize:bits:) (LTXPipeline.swift:487-492; LTXQuantizationConfig.swift:19-62): every Linear - both patchify
// Linears, the 18 embedder Linears, the four caption-projection Linears, both heads, and per block the six attention modules' to_q /
// to_k / to_v / to_out (a fused q|k matrix as one [2 inner][Dq] Linear, so that its row views stay row offsets) and the four FFN
// Linears - becomes codes + bf16 group scale / bias (group 64 along `in`), and every bf16 weight arena is released. The text cache is
// dropped: its K / V^T came from the bf16 weights. bits outside {8, 4}, group != 64 or an already quantised model: refused as
// dit_quantize refuses them, nothing changed.
void dual_model_quantize(ltx_ctx* ctx, DualModel* m, int bits, int group);
// device bytes by kind (ltx_dit_memory_info's meaning): bf16 weight arenas, the code arena, the scratch matrix, and everything else the
// model holds as parameters or per prompt (f32 parameter arenas of the model, the stack and its modules; the text cache)
void dual_model_memory_info(const DualModel* m, long* bf16_weights, long* quantised, long* scratch, long* other);

// outputs of the timestep path (device, f32)
struct DualEmbedOut {
    float* temb_v = nullptr;   // [B][6][Dv]
    float* temb_a = nullptr;   // [B][6][Da]
    float* cross_v = nullptr;  // [B][5][Dv]
    float* cross_a = nullptr;  // [B][5][Da]
    float* embts_v = nullptr;  // [B][Dv]
    float* embts_a = nullptr;  // [B][Da]
};
// the timestep path alone, into caller buffers (test and measurement seam)
void dual_model_embed(ltx_ctx* ctx, DualModel* m, const float* video_ts, const float* audio_ts, int B, int ungrouped, const DualEmbedOut& out);

struct DualModelForwardArgs {
    const bf16_t* video_latent = nullptr;   // [B][F*H*W][in_channels] bf16
    const bf16_t* audio_latent = nullptr;   // [B][T_a][audio_in_channels] bf16
    const bf16_t* video_context = nullptr;  // [B][S][caption_channels] bf16
    const bf16_t* audio_context = nullptr;
    const float* video_timesteps = nullptr; // [B][n_groups] f32, sigma unscaled
    const float* audio_timesteps = nullptr; // [B]
    const int32_t* video_mask = nullptr;    // [B][S] int32 or null
    const int32_t* audio_mask = nullptr;
    int B = 1, F = 0, H = 0, W = 0, T_a = 0, S = 0;
    float* video_velocity = nullptr;        // [B][F*H*W][out_channels] f32
    float* audio_velocity = nullptr;        // [B][T_a][audio_out_channels] f32
    int ungrouped = 0;                      // non-zero: 18 launch_gemv_f32 launches instead of the three grouped ones (bit-equal); the
                                            // grouped path is the default because it measured faster (profiles/dual_model_bench.txt)
    int text_cache = 0;                     // non-zero: the text side comes from dual_model_prepare_text; contexts and masks are not read
    int n_groups = 1;                       // timestep groups of the video stream: video_timesteps is [B][n_groups]
    const int32_t* video_row_map = nullptr; // device [B*F*H*W] int32, entries in [0, B*n_groups) (the caller's contract); null with one group
};
void dual_model_forward(ltx_ctx* ctx, DualModel* m, const DualModelForwardArgs& a);
// Both caption projections and both launch_mask_to_bias passes (a null mask is a null bias) into model-owned buffers, then
// dual_prepare_text on the owned stack. Contexts [B][S][caption_channels] bf16, masks [B][S] int32 or null; device pointers.
void dual_model_prepare_text(ltx_ctx* ctx, DualModel* m, const bf16_t* video_context, const bf16_t* audio_context, const int32_t* video_mask,
                             const int32_t* audio_mask, int B, int S);
