// gemma.h - the Gemma-3 text encoder: token ids + attention mask -> the 49 hidden states the text-embedding connector consumes.
// Reference: Models/TextEncoder/Gemma3/Gemma3Model.swift - Gemma3Attention (:14-111), Gemma3MLP (:115-130), Gemma3DecoderLayer
// (:134-168), Gemma3InnerModel.callAsFunction (:203-303); Gemma3Config.swift (defaults :42-80); Gemma3WeightLoader.swift (sanitize,
// MLX affine quantisation); the call sites LTXPipeline.swift:1155-1170 and :3194-3277. Only the hidden-state extraction WITH an
// attention mask is built - the only way the pipeline calls the model. Token generation, KV caches, the tokenizer and the no-mask path
// with a true sliding window stay out.
// The graph re-uses the bf16 GEMMs; new are the causal grouped-query attention at head dim 256 (attention.hip, attn256_causal_kernel)
// and four row passes (elementwise.hip: gemma_norm, gemma_qknorm_rope, geglu, gemma_embed). DESIGN.md 6i lists the rounding points.
#pragma once
#include <string>
#include <vector>

#include "dit.h"
#include "params.h"
#include "runtime.h"

struct GemmaConfig {  // Gemma3Config.swift:42-60
    int hidden = 3840, layers = 48, intermediate = 15360, heads = 16, head_dim = 256, kv_heads = 8, vocab = 262208;
    float rms_eps = 1e-6f;
    float rope_theta = 1000000.0f, rope_local_base = 10000.0f;
    float query_pre_attn_scalar = 256.0f;
    int sliding_window = 1024, sliding_window_pattern = 6;
};
// layer i runs the global RoPE base iff (i + 1) % pattern == 0 (Gemma3Model.swift:53); with a mask that is all the layer kind decides
inline bool gemma_layer_is_global(const GemmaConfig& c, int layer) { return (layer + 1) % c.sliding_window_pattern == 0; }

struct GemmaLayer {
    LinearW qk, v, o, gu, down;  // q_proj|k_proj fused [(Hq+Hkv)*256][hidden], gate_proj|up_proj fused [2I][hidden]; no biases
    float* qn = nullptr;         // [256] norm weights w as stored (the kernels form bf16(1 + w))
    float* kn = nullptr;
    float* in_norm = nullptr;    // [hidden]
    float* post_attn = nullptr;
    float* pre_ff = nullptr;
    float* post_ff = nullptr;
};

struct GemmaModel {
    GemmaConfig cfg;
    ParamTable params;
    bf16_t* embed = nullptr;  // [vocab][hidden]
    float* final_norm = nullptr;
    std::vector<GemmaLayer> layers;
    size_t weight_bytes = 0;
    DevBuf rope;  // cos_local | sin_local | cos_global | sin_global, each [sliding_window][128] f32, made on the device at creation
    DevBuf ws_hidden;  // ltx_text_encode_dev: the hidden states between the encoder and the connector
    DevBuf ws_ks, ws_xn, ws_qk, ws_vt, ws_ao, ws_r, ws_h, ws_gu, ws_ff;  // ws_ks: key_start[B] | status[B]
};

GemmaModel* gemma_create(ltx_ctx* ctx, const GemmaConfig& cfg);
void gemma_destroy(GemmaModel* m);
// shards: every file of the checkpoint. Keys as the reference's modules (model.embed_tokens, model.layers.N..., model.norm), with or
// without the language_model. prefix; lm_head* ignored. A weight is bf16 / f16 / f32 (rounded to bf16, as sanitize does) or MLX
// affine-quantised (weight U32 [rows][cols * bits / 32] + scales + biases [rows][cols / 64], group 64, 4 or 8 bits: de-quantised to
// bf16 here, once; the scales and biases must sit in the same shard as their weight, as mx.save_safetensors writes them). Throws
// weightLoadingFailed naming the first missing key.
void gemma_load_safetensors(ltx_ctx* ctx, GemmaModel* m, const std::vector<std::string>& shards);
void gemma_init_synthetic(ltx_ctx* ctx, GemmaModel* m, uint64_t seed);
size_t gemma_resident_bytes(const GemmaModel* m);  // weights + tables + workspaces now held

struct GemmaArgs {
    const int32_t* ids = nullptr;   // device [B][T]; out-of-range ids are clamped (elementwise.h, GemmaEmbedArgs)
    const int32_t* mask = nullptr;  // device [B][T] 0/1, left-padded 0..0 1..1 with at least one 1 per row
    int B = 1, T = 0;
    bf16_t* hidden = nullptr;       // device [layers+1][B][T][hidden] bf16: ConnectorArgs::hidden
};
// Slot 0 = the scaled embedding, slot i+1 = the raw output of layer i < L-1, the last slot = model.norm(last layer). Rows of padded
// positions hold finite values nothing downstream reads (their attention output is zero here, a uniform average in the reference).
// Waits for the mask check (one small device-to-host copy) before the layers are launched.
void gemma_encode(ltx_ctx* ctx, GemmaModel* m, const GemmaArgs& a);
