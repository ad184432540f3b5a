// gemma.h - the Gemma-3 text encoder: token ids + attention mask -> the 49 hidden states the text-embedding connector consumes.
// Reference: Models/TextEncoder/Gemma3/Gemma3Model.swift - Gemma3Attention (:14-111), Gemma3MLP (:115-130), Gemma3DecoderLayer
// (:134-168), Gemma3InnerModel.callAsFunction (:203-303); Gemma3Config.swift (defaults :42-80); Gemma3WeightLoader.swift (sanitize,
// MLX affine quantisation); the call sites LTXPipeline.swift:1155-1170 and :3194-3277. Only the hidden-state extraction WITH an
// attention mask is built for the encoder - the only way the pipeline calls it. The tokenizer and the no-mask path with a true
// sliding window stay out. Token generation for prompt enhancement (generateTokens, :375-492, and the cache: path of Gemma3Attention,
// :73-110) is the second half of this header: GemmaLm, gemma_lm_*; csrc/gemma_generate.cpp. DESIGN.md 6l.
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

// A token-generation session (gemma_lm_begin .. gemma_lm_end): the KV cache of `cap` positions and everything a step touches, all
// allocated at begin - the generate loop allocates nothing.
struct GemmaLm {
    int cap = 0, len = 0;  // capacity in positions; positions filled so far (0: not prefilled)
    long ldvt = 0;         // roundup(cap, 64)
    DevBuf kc;             // [layers][cap][Hkv*256] bf16: K after q/k norm + RoPE, row = position
    DevBuf vt;             // [layers][Hkv*256][ldvt] bf16: V^T, column = position; zero-initialised (the prefill kernel reads pad columns)
    DevBuf rope;           // cos_local | sin_local | cos_global | sin_global, each [cap][128] f32 (the encoder's tables stay untouched)
    DevBuf hid;            // prefill: two ping-pong hidden slots [min(cap, sliding_window)][hidden] bf16
    DevBuf sb;             // step rows: x[2][hidden] | xn[hidden] | qk[(Hq+Hkv)*256] | ao[Hq*256] | r[hidden] | h[hidden] | ff[I] | fin[hidden]
    DevBuf logits;         // [vocab] f32
    DevBuf hist;           // [cap + 2] int32: the generated tokens (lm_pick reads the recent ones and appends; the prompt is staged here first) | one staged token | the pick
    DevBuf dec_ws;         // attn_decode_ws_bytes(Hq, cap)
    size_t cache_bytes() const { return kc.bytes + vt.bytes; }
    size_t workspace_bytes() const { return rope.bytes + hid.bytes + sb.bytes + logits.bytes + hist.bytes + dec_ws.bytes; }
};

struct GemmaModel {
    GemmaConfig cfg;
    GemmaLm* lm = nullptr;  // the generation session, or null
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

// The layer loop that gemma_encode and the generation prefill share: what differs between the two around the same launches.
struct GemmaStackRun {
    int B = 1, T = 0;
    const int32_t* key_start = nullptr;  // device [B] or null (no padding)
    const float* rope = nullptr;         // cos_local | sin_local | cos_global | sin_global, each `tab` floats
    size_t tab = 0;
    bf16_t* hidden = nullptr;            // slots of [B*T][hidden]; slot 0 holds the scaled embedding on entry
    int ping_pong = 0;                   // 0: layer l reads slot l and writes slot l + 1; 1: two slots, l & 1 and (l + 1) & 1
    bf16_t* kcache = nullptr;            // null: K stays in the q|k row buffer; else layer l's rows go to kcache + l * k_stride, [T][Hkv*256]
    size_t k_stride = 0;
    bf16_t* vtcache = nullptr;           // null: V^T in the workspace, ld roundup(T, 64); else vtcache + l * vt_stride, [Hkv*256][ldvt] (B == 1)
    size_t vt_stride = 0;
    long ldvt = 0;
    bf16_t* final_out = nullptr;         // null: model.norm of every row into the last slot; else of the LAST row only, into [hidden] here
};
void gemma_run_layers(ltx_ctx* ctx, GemmaModel* m, const GemmaStackRun& s);

// ---- token generation on a KV cache (Gemma3Model.swift:375-492; batch 1, ids in, ids out) ----
// The decode attention covers ALL pos + 1 cached keys on every layer, sliding ones included: the reference decodes with mask: .none
// on a KVCacheSimple (:481-484). That is the reference's behaviour, not a shortcut. The prefill builds no window mask either and
// therefore refuses prompts longer than sliding_window, exactly as gemma_encode does.
struct GemmaLmParams {  // defaults: generateTokens' (:390-398)
    int max_new = 512;
    float temperature = 0.7f;  // <= 0: greedy, picked on the device (lm_pick_kernel)
    float top_p = 0.95f;
    float penalty = 1.1f;
    int context = 64;
    uint64_t seed = 0;
    int n_eos = 1;
    int32_t eos[8] = {1, 0, 0, 0, 0, 0, 0, 0};
};
void gemma_lm_begin(ltx_ctx* ctx, GemmaModel* m, int capacity);  // replaces a session the model already holds
size_t gemma_lm_end(ltx_ctx* ctx, GemmaModel* m);                // bytes released (0 without a session)
// ids: device [T]. Resets the session, fills cache positions 0 .. T-1, leaves model.norm of the last row in the step rows' `fin` and
// its logits in lm->logits. Throws before the first launch without a session, on T < 1, T > sliding_window or T > cap.
void gemma_lm_prefill(ltx_ctx* ctx, GemmaModel* m, const int32_t* ids, int T);
// token: device [1] (clamped to the vocabulary by the embedding). Appends position len, leaves `fin` and the logits as above.
// Throws before the first launch without a prefilled session or with the cache full.
void gemma_lm_step(ltx_ctx* ctx, GemmaModel* m, const int32_t* token);
bf16_t* gemma_lm_state(GemmaModel* m);  // device [hidden]: model.norm of the newest position (the logits gemv's input)
// ids: HOST [T]. Returns the number of tokens written to out (capacity p.max_new); a stop id ends the run and is not written.
// Throws before the first launch when T + max_new exceeds the capacity (and whatever gemma_lm_prefill refuses).
int gemma_lm_generate(ltx_ctx* ctx, GemmaModel* m, const int32_t* ids, int T, const GemmaLmParams& p, int32_t* out);
// The sampler at temperature > 0, pure host code, OURS (the reference's live sampler is outside its tree): the
// repetition penalty in place on `logits` (lm_pick's rule over the last min(context, n_generated) entries of `generated`), softmax of
// l / temperature in f64, the nucleus = the fewest tokens in decreasing probability (ties: lower id) whose mass reaches top_p, one
// inverse-CDF draw with u = (w >> 8) * 2^-24, w = word 0 of threefry2x32(mlx_draw_key(seed, step), {0, 0}). temperature <= 0: argmax,
// ties to the lowest id.
// scratch: the two vocabulary-sized arrays of the nucleus search. The generate loop reserves them once before its first token; a
// stand-alone call (null) allocates its own.
struct LmSampleScratch {
    std::vector<double> w;
    std::vector<int32_t> order;
    void reserve(int vocab) {
        if ((int)w.size() != vocab) w.resize(vocab);
        if ((int)order.size() != vocab) order.resize(vocab);
    }
};
int32_t lm_sample_host(float* logits, int vocab, const int32_t* generated, int n_generated, int context, float penalty, float temperature,
                       float top_p, uint64_t seed, int step, LmSampleScratch* scratch = nullptr);
