// abi_models.cpp - extern "C" surface of libltxhip.so (include/ltxhip.h), part 2 of 3: the model entry points. Per component:
// *_load / *_init_synthetic / *_unload over one model slot of the context (abi_internal.h: replace_model / unload_model / need),
// then the *_dev entry point on device pointers and its host-pointer twin, which stages through stage_in / stage_out around the same
// body. Also the denoise loop and the multi-GPU group.
#include <algorithm>
#include <vector>

#include "abi_internal.h"
#include "audio.h"
#include "attn_module.h"
#include "dual_block.h"
#include "dual_denoise.h"
#include "dual_generate.h"
#include "dual_model.h"
#include "dual_two_stage.h"
#include "connector.h"
#include "gemma.h"
#include "dist.h"
#include "elementwise.h"
#include "pipeline.h"
#include "upscaler.h"
#include "vae.h"
#include "vae_encoder.h"

namespace {

// FNV-1a over 8-byte words: cheap change detector for host-pointer context buffers
uint64_t hash_bytes(const void* p, size_t n, uint64_t h) {
    const uint8_t* b = (const uint8_t*)p;
    size_t i = 0;
    for (; i + 8 <= n; i += 8) {
        uint64_t w;
        memcpy(&w, b + i, 8);
        h = (h ^ w) * 0x100000001B3ull;
        h ^= h >> 29;
    }
    for (; i < n; ++i) h = (h ^ b[i]) * 0x100000001B3ull;
    return h ? h : 1;
}

// What a host-pointer entry point knows about its text context: `version` names the bytes of context (+ mask) for the DiT's context
// cache (never 0, which means "do not cache"), `all_ones` says that no key is masked. A null `context` asks for the mask scan alone
// and gives version 0.
struct ContextSignature {
    uint64_t version = 0;
    int all_ones = 1;
};
ContextSignature context_signature(const void* context, size_t context_bytes, const int32_t* mask, long mask_elems) {
    ContextSignature s;
    if (context) s.version = hash_bytes(context, context_bytes, 0xCBF29CE484222325ull);
    if (mask) {
        if (context) s.version = hash_bytes(mask, (size_t)mask_elems * 4, s.version);
        for (long i = 0; i < mask_elems; ++i)
            if (mask[i] != 1) { s.all_ones = 0; break; }
    }
    return s;
}

DiTForwardArgs dit_args(const uint16_t* latent, const uint16_t* context, const float* timesteps, const int32_t* mask, int mask_all_ones,
                        int B, int F, int H, int W, int S, uint64_t ctx_version, float* velocity) {
    DiTForwardArgs a;
    a.latent = latent;
    a.context = context;
    a.timesteps = timesteps;
    a.mask = mask;
    a.mask_all_ones = mask_all_ones;
    a.B = B; a.F = F; a.H = H; a.W = W; a.S = S;
    a.ctx_version = ctx_version;
    a.velocity = velocity;
    return a;
}

VaeDecodeArgs vae_args(const float* latent, int F, int H, int W, int has_timestep, float timestep, const float* noise, int tile,
                       int overlap, float* frames, long frames_cap, int* n_frames_out) {
    VaeDecodeArgs a;
    a.latent = latent; a.F = F; a.H = H; a.W = W;
    a.has_timestep = has_timestep; a.timestep = timestep; a.noise = noise;
    a.tile = tile; a.overlap = overlap;
    a.frames = frames; a.frames_cap = frames_cap; a.n_frames_out = n_frames_out;
    return a;
}

GemmaConfig to_gemma_cfg(const ltx_gemma_config* c) {
    GemmaConfig g;
    if (!c) return g;
    g.hidden = c->hidden_size; g.layers = c->num_hidden_layers; g.intermediate = c->intermediate_size;
    g.heads = c->num_attention_heads; g.head_dim = c->head_dim; g.kv_heads = c->num_key_value_heads; g.vocab = c->vocab_size;
    g.rms_eps = c->rms_norm_eps; g.rope_theta = c->rope_theta; g.rope_local_base = c->rope_local_base_freq;
    g.query_pre_attn_scalar = c->query_pre_attn_scalar; g.sliding_window = c->sliding_window;
    g.sliding_window_pattern = c->sliding_window_pattern;
    return g;
}

ConnectorConfig to_conn_cfg(const ltx_connector_config* c) {
    ConnectorConfig k;
    if (c) {
        k.dim = c->dim; k.heads = c->heads; k.layers = c->layers; k.registers = c->registers; k.states = c->states;
        k.theta = c->theta; k.max_pos = c->max_pos;
    }
    return k;
}

// ---- bodies shared by a *_dev entry point and its host-pointer twin (all pointers are device pointers) ----
void upscale_body(ltx_ctx* ctx, const float* latent, int F, int H, int W, float* out) {
    UpscalerModel* u = need(ctx->upscaler, kNoUpscaler);
    VaeModel* v = need(ctx->vae, kNoVae);  // per-channel statistics come from the VAE (LTXPipeline.swift:2598-2599)
    upscaler_forward(ctx, u, latent, F, H, W, v->mean, v->std_, out);
}

void adain_body(ltx_ctx* ctx, float* latent, long n, const float* reference, long n_ref, int channels, float factor) {
    ctx->dn_stats.ensure((size_t)channels * 4 * 4 + 64);
    float* sx = ctx->dn_stats.as<float>();
    float* sr = sx + 2 * channels;
    launch_mean_var(latent, n, channels, sx, ctx->stream);
    launch_mean_var(reference, n_ref, channels, sr, ctx->stream);
    launch_adain(latent, sx, sr, factor, n, channels, ctx->stream);
}

void encode_body(ltx_ctx* ctx, const float* pixels, int T, int H, int W, int normalize, float* latent) {
    VaeEncoderModel* m = need(ctx->vae_encoder, kNoVaeEncoder);
    const float* mean = nullptr;
    const float* stdv = nullptr;
    if (normalize) {
        const VaeModel* v = need(ctx->vae, kNoVaeStats);
        mean = v->mean;
        stdv = v->std_;
    }
    vae_encoder_encode(ctx, m, pixels, T, H, W, mean, stdv, latent, nullptr);
}

void audio_decode_body(ltx_ctx* ctx, const float* latent, int T, float* wave) {
    AudioVaeModel* v = need(ctx->audio_vae, kNoAudioVae);
    VocoderModel* g = need(ctx->vocoder, kNoVocoder);
    LTX_REQUIRE(latent && wave && T >= 1, "ltx_audio_decode: bad arguments");
    const int Tm = audio_mel_frames(T);
    ctx->audio_mel.ensure((size_t)2 * Tm * 64 * 4);
    audio_vae_decode(ctx, v, latent, T, ctx->audio_mel.as<float>());
    vocoder_forward(ctx, g, ctx->audio_mel.as<float>(), Tm, wave);
}

// host-pointer side of the three audio entry points: one f32 input, one f32 output, through H2D_IN / H2D_OUT
const float* audio_stage_in(ltx_ctx* ctx, const float* in, size_t n_in, float* out, size_t n_out) {
    LTX_REQUIRE(in && out, "audio: null host pointer");
    ctx->h2d[H2D_IN].ensure(n_in * 4);
    ctx->h2d[H2D_OUT].ensure(n_out * 4);
    stage_in(ctx, ctx->h2d[H2D_IN], in, n_in * 4);
    return ctx->h2d[H2D_IN].as<float>();
}
void audio_stage_out(ltx_ctx* ctx, float* out, size_t n_out) {
    stage_out(ctx, out, ctx->h2d[H2D_OUT], n_out * 4);
    stage_sync(ctx);
}

void fill_params(DenoiseParams& p, const ltx_denoise_options* o) {
    if (!o) return;
    // ABI revision 2: the caller declares how much of the struct it knows; nothing past that is read (round-4 advice: a host compiled
    // against the older, shorter struct must not have `step_stats` read past its end)
    const size_t sz = o->struct_size;
    LTX_REQUIRE(sz >= offsetof(ltx_denoise_options, shard) + sizeof(o->shard) && sz <= 4096,
                "ltx_denoise_options.struct_size = %zu: set it to sizeof(ltx_denoise_options) (LTX_DENOISE_OPTIONS_INIT); this library is ABI revision %d",
                sz, LTX_ABI_VERSION);
    p.cfg_scale = o->cfg_scale;
    p.guidance_rescale = o->guidance_rescale;
    p.stg_scale = o->stg_scale;
    p.stg_blocks = o->stg_blocks;
    p.n_stg = o->n_stg_blocks;
    p.ge_gamma = o->ge_gamma;
    p.cond_latent = o->cond_latent;  // device variant: used as given; host variant: replaced by staged copies below
    p.image_cond_noise_scale = o->image_cond_noise_scale;
    p.cond_noise = o->cond_noise;
    p.shard = o->shard;
    if (sz >= offsetof(ltx_denoise_options, step_stats) + sizeof(o->step_stats)) p.step_stats = o->step_stats;
}

// the context's slot of attention module `index` (attn_module.h)
AttnModule** attn_slot(ltx_ctx* ctx, int index) {
    LTX_REQUIRE(index >= 0 && index < kAttnModuleSlots, "attention module index %d outside 0 .. %d", index, kAttnModuleSlots - 1);
    return &ctx->attn_modules[index];
}

DualBlockConfig to_dual_cfg(const ltx_dual_block_config* c) {
    DualBlockConfig t;
    if (!c) return t;
    t.num_layers = c->num_layers;
    t.video_heads = c->video_heads;
    t.video_dim = c->video_dim;
    t.audio_heads = c->audio_heads;
    t.audio_dim = c->audio_dim;
    t.video_context_dim = c->video_context_dim;
    t.audio_context_dim = c->audio_context_dim;
    t.rope_theta = c->rope_theta;
    for (int i = 0; i < 3; ++i) t.max_pos[i] = c->max_pos[i];
    t.audio_max_pos = c->audio_max_pos;
    t.fps = c->fps;
    t.norm_eps = c->norm_eps;
    return t;
}

DualModelConfig to_dual_model_cfg(const ltx_dual_model_config* c) {
    DualModelConfig t;
    if (!c) return t;
    t.blocks = to_dual_cfg(&c->blocks);
    t.in_channels = c->in_channels;
    t.out_channels = c->out_channels;
    t.audio_in_channels = c->audio_in_channels;
    t.audio_out_channels = c->audio_out_channels;
    t.caption_channels = c->caption_channels;
    t.timestep_scale_multiplier = c->timestep_scale_multiplier;
    return t;
}

}  // namespace

extern "C" {

// ---- DiT ----
int ltx_dit_load(ltx_ctx* ctx, const char* path, const ltx_transformer_config* cfg, int quant_bits, int group_size) {
    if (!ctx || !path) return LTX_ERR_INVALID_CONFIGURATION;
    return guarded(ctx, [&] {
        LTX_REQUIRE(quant_bits == 16 || quant_bits == 0 || quant_bits == 8 || quant_bits == 4,
                    "transformer quantization must be bf16 (16), qint8 (8) or int4 (4); got %d bits", quant_bits);
        LTX_REQUIRE(quant_bits == 16 || quant_bits == 0 || group_size == 64, "quantization group size must be 64, got %d", group_size);
        replace_model(ctx, &ctx->dit, [&] { return dit_create(to_cfg(cfg)); },
                      [&](DiTModel* m) {
                          dit_load_safetensors(ctx, m, path);
                          if (quant_bits == 8 || quant_bits == 4) dit_quantize(ctx, m, quant_bits, 64);
                      },
                      dit_destroy);
    });
}

int ltx_dit_init_synthetic(ltx_ctx* ctx, const ltx_transformer_config* cfg, uint64_t seed) {
    return with_ctx(ctx, [&] {
        replace_model(ctx, &ctx->dit, [&] { return dit_create(to_cfg(cfg)); }, [&](DiTModel* m) { dit_init_synthetic(ctx, m, seed); },
                      dit_destroy);
    });
}

int ltx_dit_quantize(ltx_ctx* ctx, int bits, int group_size) {
    return with_ctx(ctx, [&] { dit_quantize(ctx, need(ctx->dit, kNoDit), bits, group_size); });
}

int ltx_dit_memory_info(ltx_ctx* ctx, long* bf16_weight_bytes, long* quantised_weight_bytes, long* scratch_bytes, long* other_bytes) {
    return with_ctx(ctx, [&] {
        DiTModel* m = need(ctx->dit, kNoDit);
        if (bf16_weight_bytes) *bf16_weight_bytes = m->params.warena.buf.p ? (long)m->params.warena.buf.bytes : 0;
        if (quantised_weight_bytes) *quantised_weight_bytes = m->qarena.buf.p ? (long)m->qarena.buf.bytes : 0;
        if (scratch_bytes) *scratch_bytes = m->dq.buf.p ? (long)m->dq.buf.bytes : 0;
        if (other_bytes) *other_bytes = m->params.arena.buf.p ? (long)m->params.arena.buf.bytes : 0;
    });
}

int ltx_dit_fuse_lora(ltx_ctx* ctx, const char* path, float scale, int* n_fused) {
    if (!ctx || !path) return LTX_ERR_INVALID_CONFIGURATION;
    return guarded(ctx, [&] {
        const int n = dit_fuse_lora(ctx, need(ctx->dit, kNoDitLora), path, scale);
        if (n_fused) *n_fused = n;
    });
}

int ltx_dit_unload(ltx_ctx* ctx) {
    return with_ctx(ctx, [&] { unload_model(ctx, &ctx->dit, dit_destroy); });
}

int ltx_dit_forward_dev(ltx_ctx* ctx, const uint16_t* latent, const uint16_t* context, const float* timesteps,
                        const int32_t* mask, int mask_all_ones, int B, int F, int H, int W, int S,
                        uint64_t ctx_version, float* velocity) {
    return with_ctx(ctx, [&] {
        DiTModel* m = need(ctx->dit, kNoDit);
        dit_forward(ctx, m, dit_args(latent, context, timesteps, mask, mask_all_ones, B, F, H, W, S, ctx_version, velocity));
    });
}

int ltx_dit_forward_sp_dev(ltx_ctx* ctx, const uint16_t* latent, const uint16_t* context, const float* timesteps,
                           const int32_t* mask, int mask_all_ones, int F, int H, int W, int S, uint64_t ctx_version,
                           int sp_rank, int sp_world, ltx_allgather_fn gather, void* user, float* velocity) {
    return with_ctx(ctx, [&] {
        DiTModel* m = need(ctx->dit, kNoDit);
        LTX_REQUIRE(sp_world >= 1 && (sp_world == 1 || gather || ctx->dist), "ltx_dit_forward_sp_dev: %d ranks need a gather callback or ltx_dist_init", sp_world);
        DiTForwardArgs a = dit_args(latent, context, timesteps, mask, mask_all_ones, 1, F, H, W, S, ctx_version, velocity);
        a.sp_rank = sp_rank;
        a.sp_world = sp_world;
        a.sp_gather = gather;
        a.sp_user = user;
        dit_forward(ctx, m, a);
    });
}

int ltx_dit_forward(ltx_ctx* ctx, const uint16_t* latent, const uint16_t* context, const float* timesteps,
                    const int32_t* mask, int B, int F, int H, int W, int S, float* velocity) {
    return with_ctx(ctx, [&] {
        DiTModel* m = need(ctx->dit, kNoDit);
        LTX_REQUIRE(latent && context && timesteps && velocity && B >= 1 && F >= 1 && H >= 1 && W >= 1 && S >= 1, "ltx_dit_forward: bad arguments");
        const long T = (long)F * H * W;
        const size_t n_lat = (size_t)B * T * m->cfg.in_channels * 2;
        const size_t n_ctx = (size_t)B * S * m->cfg.caption_channels * 2;
        const size_t n_mask = (size_t)B * S * 4;
        const size_t n_vel = (size_t)B * T * m->cfg.out_channels * 4;
        DevBuf &d_lat = ctx->h2d[H2D_DIT_LATENT], &d_ctx = ctx->h2d[H2D_DIT_CONTEXT], &d_ts = ctx->h2d[H2D_DIT_TIMESTEPS],
               &d_mask = ctx->h2d[H2D_DIT_MASK], &d_vel = ctx->h2d[H2D_DIT_VELOCITY];
        d_ctx.ensure(n_ctx);
        d_mask.ensure(n_mask);
        d_vel.ensure(n_vel);
        // the context is constant across denoise steps: upload + re-project it only when its bytes change
        const ContextSignature sig = context_signature(context, n_ctx, mask, (long)B * S);
        stage_in(ctx, d_lat, latent, n_lat);
        bool cached = false;
        for (auto* e : m->ctx_cache) cached = cached || (e->version == sig.version && e->kind == 0 && e->B == B && e->S == S);
        if (!cached) {
            stage_in(ctx, d_ctx, context, n_ctx);
            if (mask) stage_in(ctx, d_mask, mask, n_mask);
        }
        stage_in(ctx, d_ts, timesteps, (size_t)B * 4);
        dit_forward(ctx, m, dit_args(d_lat.as<bf16_t>(), d_ctx.as<bf16_t>(), d_ts.as<float>(), mask ? d_mask.as<int32_t>() : nullptr,
                                     sig.all_ones, B, F, H, W, S, sig.version, d_vel.as<float>()));
        stage_out(ctx, velocity, d_vel, n_vel);
        stage_sync(ctx);
    });
}

int ltx_dit_forward_tokens(ltx_ctx* ctx, const uint16_t* latent, const uint16_t* context, const float* token_timesteps,
                           const int32_t* mask, int B, int F, int H, int W, int S, float* velocity) {
    return with_ctx(ctx, [&] {
        DiTModel* m = need(ctx->dit, kNoDit);
        LTX_REQUIRE(latent && context && token_timesteps && velocity && B >= 1 && F >= 1 && H >= 1 && W >= 1 && S >= 1,
                    "ltx_dit_forward_tokens: bad arguments");
        const long T = (long)F * H * W;
        // distinct timestep values per batch row -> groups (order of first appearance); G = the largest count
        std::vector<std::vector<float>> uniq(B);
        std::vector<int32_t> rowmap((size_t)B * T);
        int G = 1;
        for (int b = 0; b < B; ++b) {
            for (long t = 0; t < T; ++t) {
                const float v = token_timesteps[(size_t)b * T + t];
                size_t g = 0;
                while (g < uniq[b].size() && uniq[b][g] != v) ++g;
                if (g == uniq[b].size()) uniq[b].push_back(v);
                rowmap[(size_t)b * T + t] = (int32_t)g;
                LTX_REQUIRE(uniq[b].size() <= 8, "ltx_dit_forward_tokens: more than 8 distinct timesteps in batch row %d", b);
            }
            G = std::max(G, (int)uniq[b].size());
        }
        LTX_REQUIRE(B * G <= 8, "ltx_dit_forward_tokens: batch x distinct timesteps = %d exceeds 8", B * G);
        std::vector<float> ts((size_t)B * G);
        for (int b = 0; b < B; ++b)
            for (int g = 0; g < G; ++g) ts[(size_t)b * G + g] = uniq[b][g < (int)uniq[b].size() ? g : 0];
        for (int b = 0; b < B; ++b)
            for (long t = 0; t < T; ++t) rowmap[(size_t)b * T + t] += b * G;
        const size_t n_lat = (size_t)B * T * m->cfg.in_channels * 2;
        const size_t n_ctx = (size_t)B * S * m->cfg.caption_channels * 2;
        const size_t n_mask = (size_t)B * S * 4;
        const size_t n_vel = (size_t)B * T * m->cfg.out_channels * 4;
        DevBuf &d_lat = ctx->h2d[H2D_DIT_LATENT], &d_ctx = ctx->h2d[H2D_DIT_CONTEXT], &d_ts = ctx->h2d[H2D_DIT_TIMESTEPS],
               &d_mask = ctx->h2d[H2D_DIT_MASK], &d_vel = ctx->h2d[H2D_DIT_VELOCITY];
        d_ts.ensure(8 * 4);
        d_mask.ensure(n_mask);
        d_vel.ensure(n_vel);
        ctx->dn_rowmap.ensure(std::max((size_t)B * T * 4, (size_t)2 * T * 4));
        // per-token timesteps are not cached by context version (0): only the mask scan is wanted
        const ContextSignature sig = context_signature(nullptr, 0, mask, (long)B * S);
        stage_in(ctx, d_lat, latent, n_lat);
        stage_in(ctx, d_ctx, context, n_ctx);
        if (mask) stage_in(ctx, d_mask, mask, n_mask);
        stage_in(ctx, d_ts, ts.data(), ts.size() * 4);
        stage_in(ctx, ctx->dn_rowmap, rowmap.data(), rowmap.size() * 4);
        DiTForwardArgs a = dit_args(d_lat.as<bf16_t>(), d_ctx.as<bf16_t>(), d_ts.as<float>(), mask ? d_mask.as<int32_t>() : nullptr,
                                    sig.all_ones, B, F, H, W, S, sig.version, d_vel.as<float>());
        a.n_groups = G;
        a.row_map = ctx->dn_rowmap.as<int32_t>();
        dit_forward(ctx, m, a);
        stage_out(ctx, velocity, d_vel, n_vel);
        stage_sync(ctx);  // also keeps ts / rowmap alive until the copies are done
    });
}

int ltx_dit_set_cross_attn_scale(ltx_ctx* ctx, float scale, int first_block, int last_block) {
    return with_ctx(ctx, [&] {
        DiTModel* m = need(ctx->dit, kNoDit);
        if (last_block < 0) last_block = m->L - 1;
        for (int i = first_block; i <= last_block; ++i)
            if (i >= 0 && i < m->L) m->blocks[i].cross_scale = scale;
    });
}

int ltx_dit_set_stg(ltx_ctx* ctx, const int* blocks, int n_blocks, int skip_attn, int skip_ff) {
    return with_ctx(ctx, [&] {
        DiTModel* m = need(ctx->dit, kNoDit);
        for (int j = 0; j < n_blocks; ++j) {
            const int i = blocks[j];
            if (i < 0 || i >= m->L) continue;
            m->blocks[i].skip_attn = skip_attn != 0;
            m->blocks[i].skip_ff = skip_ff != 0;
        }
    });
}

int ltx_dit_clear_stg(ltx_ctx* ctx) {
    return with_ctx(ctx, [&] {
        DiTModel* m = need(ctx->dit, kNoDit);
        for (auto& b : m->blocks) b.skip_attn = b.skip_ff = false;
    });
}

// ---- VAE ----
int ltx_vae_load(ltx_ctx* ctx, const char* path, const char* config_json) {
    if (!ctx || !path) return LTX_ERR_INVALID_CONFIGURATION;
    return guarded(ctx, [&] {
        replace_model(ctx, &ctx->vae, vae_create,
                      [&](VaeModel* m) { vae_load_safetensors(ctx, m, path, config_json ? config_json : ""); }, vae_destroy);
    });
}

int ltx_vae_init_synthetic(ltx_ctx* ctx, uint64_t seed, int timestep_conditioning) {
    return with_ctx(ctx, [&] {
        replace_model(ctx, &ctx->vae, vae_create, [&](VaeModel* m) { vae_init_synthetic(ctx, m, seed, timestep_conditioning != 0); },
                      vae_destroy);
    });
}

int ltx_vae_unload(ltx_ctx* ctx) {
    return with_ctx(ctx, [&] { unload_model(ctx, &ctx->vae, vae_destroy); });
}

int ltx_vae_timestep_conditioning(const ltx_ctx* ctx) {
    if (!ctx || !ctx->vae) return -LTX_ERR_MODEL_NOT_LOADED;
    return ctx->vae->timestep_conditioning ? 1 : 0;
}

int ltx_vae_decode_dev(ltx_ctx* ctx, const float* latent, int F, int H, int W, int has_timestep, float timestep,
                       const float* noise, int tile, int overlap, float* frames_out, long frames_cap,
                       int* n_frames_out) {
    return with_ctx(ctx, [&] {
        VaeModel* m = need(ctx->vae, kNoVae);
        vae_decode(ctx, m, vae_args(latent, F, H, W, has_timestep, timestep, noise, tile, overlap, frames_out, frames_cap, n_frames_out));
    });
}

int ltx_vae_decode_sharded_dev(ltx_ctx* ctx, const float* latent, int F, int H, int W, int has_timestep, float timestep,
                               const float* noise, int tile, int overlap, float* frames_out, long frames_cap,
                               int* n_frames_out) {
    return with_ctx(ctx, [&] {
        VaeModel* m = need(ctx->vae, kNoVae);
        LTX_REQUIRE(ctx->dist, "ltx_vae_decode_sharded_dev: no group on this context (ltx_dist_init / ltx_dist_set_transport)");
        VaeDecodeArgs a = vae_args(latent, F, H, W, has_timestep, timestep, noise, tile, overlap, frames_out, frames_cap, n_frames_out);
        a.shard = 1;
        vae_decode(ctx, m, a);
    });
}

int ltx_vae_decode_gathered_dev(ltx_ctx* ctx, const float* latent, int F, int H, int W, int has_timestep, float timestep,
                                const float* noise, int tile, int overlap, int root, float* frames_out, long frames_cap,
                                int* n_frames_out) {
    return with_ctx(ctx, [&] {
        VaeModel* m = need(ctx->vae, kNoVae);
        LTX_REQUIRE(ctx->dist, "ltx_vae_decode_gathered_dev: no group on this context (ltx_dist_init / ltx_dist_set_transport)");
        VaeDecodeArgs a = vae_args(latent, F, H, W, has_timestep, timestep, noise, tile, overlap, frames_out, frames_cap, n_frames_out);
        a.shard = 2;
        a.root = root;
        vae_decode(ctx, m, a);
    });
}

int ltx_vae_decode_tile_dev(ltx_ctx* ctx, const float* latent, int F, int H, int W, int has_timestep, float timestep,
                            const float* noise, int tile, int overlap, int tile_index, float* tile_out, long tile_cap,
                            int* n_frames_out) {
    return with_ctx(ctx, [&] {
        VaeModel* m = need(ctx->vae, kNoVae);
        vae_decode_tile(ctx, m, vae_args(latent, F, H, W, has_timestep, timestep, noise, tile, overlap, tile_out, tile_cap, n_frames_out),
                        tile_index);
    });
}

int ltx_vae_res_block_dev(ltx_ctx* ctx, int group, int block, float* x, int F, int H, int W) {
    return with_ctx(ctx, [&] { vae_res_block(ctx, need(ctx->vae, kNoVae), group, block, x, F, H, W); });
}

int ltx_vae_upsample_dev(ltx_ctx* ctx, int group, const float* x, int F, int H, int W, float* out) {
    return with_ctx(ctx, [&] { vae_upsample(ctx, need(ctx->vae, kNoVae), group, x, F, H, W, out); });
}

int ltx_vae_blend_tiles_dev(ltx_ctx* ctx, const float* const* tiles, const int* tile_frames, int n_tiles, int overlap, int H,
                            int W, float* frames_out, long frames_cap, int* n_frames_out) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(H >= 1 && W >= 1, "ltx_vae_blend_tiles_dev: bad latent size");
        const int n = vae_blend_tiles(ctx, tiles, tile_frames, n_tiles, overlap, H, W, frames_out, frames_cap);
        if (n_frames_out) *n_frames_out = n;
    });
}

int ltx_vae_decode(ltx_ctx* ctx, const float* latent, int F, int H, int W, int has_timestep, float timestep,
                   const float* noise, int tile, int overlap, float* frames_out, long frames_cap, int* n_frames_out) {
    return with_ctx(ctx, [&] {
        VaeModel* m = need(ctx->vae, kNoVae);
        LTX_REQUIRE(latent && frames_out && F >= 1 && H >= 1 && W >= 1, "ltx_vae_decode: bad arguments");
        const size_t n_lat = (size_t)128 * F * H * W * 4;
        DevBuf dl, dn, df;  // per call, freed on return: the frame buffer is far too large to keep resident
        const bool noisy = has_timestep && noise;
        stage_in(ctx, dl, latent, n_lat);
        if (noisy) stage_in(ctx, dn, noise, n_lat);
        df.ensure((size_t)frames_cap * 4);
        int nf = 0;
        vae_decode(ctx, m, vae_args(dl.as<float>(), F, H, W, has_timestep, timestep, noisy ? dn.as<float>() : nullptr, tile, overlap,
                                    df.as<float>(), frames_cap, &nf));
        stage_out(ctx, frames_out, df, (size_t)nf * H * 32 * W * 32 * 3 * 4);
        stage_sync(ctx);
        if (n_frames_out) *n_frames_out = nf;
    });
}

// ---- two-stage glue ----
int ltx_upscaler_load(ltx_ctx* ctx, const char* path) {
    if (!ctx || !path) return LTX_ERR_INVALID_CONFIGURATION;
    return guarded(ctx, [&] {
        // upscaler_load sizes the model from the file and returns it filled (or throws with nothing left behind)
        replace_model(ctx, &ctx->upscaler, [&] { return upscaler_load(ctx, path); }, [](UpscalerModel*) {}, upscaler_destroy);
    });
}

int ltx_upscaler_unload(ltx_ctx* ctx) {
    return with_ctx(ctx, [&] { unload_model(ctx, &ctx->upscaler, upscaler_destroy); });
}

int ltx_upscale_latent_dev(ltx_ctx* ctx, const float* latent, int F, int H, int W, float* out) {
    return with_ctx(ctx, [&] { upscale_body(ctx, latent, F, H, W, out); });
}

int ltx_upscale_latent(ltx_ctx* ctx, const float* latent, int F, int H, int W, float* out) {
    return with_ctx(ctx, [&] {
        need(ctx->upscaler, kNoUpscaler);  // a missing model is reported before a bad argument
        need(ctx->vae, kNoVae);
        LTX_REQUIRE(latent && out && F >= 1 && H >= 1 && W >= 1, "ltx_upscale_latent: bad arguments");
        const size_t n_in = (size_t)128 * F * H * W * 4;
        DevBuf di, dout;  // per call, freed on return
        di.ensure(n_in);
        dout.ensure(n_in * 4);
        stage_in(ctx, di, latent, n_in);
        upscale_body(ctx, di.as<float>(), F, H, W, dout.as<float>());
        stage_out(ctx, out, dout, n_in * 4);
        stage_sync(ctx);
    });
}

int ltx_adain_filter_latent_dev(ltx_ctx* ctx, float* latent, long n, const float* reference, long n_ref, int channels,
                                float factor) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(latent && reference && n > 0 && n_ref > 0 && channels > 0, "adain: bad arguments");
        if (factor <= 0.f) return;
        adain_body(ctx, latent, n, reference, n_ref, channels, factor);
    });
}

int ltx_adain_filter_latent(ltx_ctx* ctx, float* latent, long n, const float* reference, long n_ref, int channels,
                            float factor) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(latent && reference && n > 0 && n_ref > 0 && channels > 0, "adain: bad arguments");
        if (factor <= 0.f) return;
        const size_t n_lat = (size_t)n * channels * 4, n_reference = (size_t)n_ref * channels * 4;
        DevBuf dl, dr;  // per call, freed on return
        dl.ensure(n_lat);
        dr.ensure(n_reference);
        stage_in(ctx, dl, latent, n_lat);
        stage_in(ctx, dr, reference, n_reference);
        adain_body(ctx, dl.as<float>(), n, dr.as<float>(), n_ref, channels, factor);
        stage_out(ctx, latent, dl, n_lat);
        stage_sync(ctx);
    });
}

int ltx_renoise_dev(ltx_ctx* ctx, float* latent, const float* noise, float sigma, long n) {
    return with_ctx(ctx, [&] { launch_lincomb(noise, latent, sigma, 1.0f - sigma, latent, n, ctx->stream); });
}

// ---- denoise loop ----
int ltx_denoise_dev(ltx_ctx* ctx, float* latent, int F, int H, int W, const float* sigmas, int n_sigmas,
                    const uint16_t* context, const int32_t* mask, int mask_all_ones, int S, uint64_t ctx_version,
                    const ltx_denoise_options* opt, ltx_progress_cb cb, void* user) {
    return with_ctx(ctx, [&] {
        DenoiseParams p;
        p.latent = latent; p.F = F; p.H = H; p.W = W;
        p.sigmas = sigmas; p.n_sigmas = n_sigmas;
        p.context = context; p.mask = mask; p.mask_all_ones = mask_all_ones; p.S = S;
        p.ctx_version = ctx_version;
        fill_params(p, opt);
        p.progress = cb; p.user = user;
        denoise_run(ctx, p);
    });
}

int ltx_denoise(ltx_ctx* ctx, float* latent, int F, int H, int W, const float* sigmas, int n_sigmas,
                const uint16_t* context, const int32_t* mask, int S, const ltx_denoise_options* opt,
                ltx_progress_cb cb, void* user) {
    return with_ctx(ctx, [&] {
        DiTModel* m = need(ctx->dit, kNoDit);
        LTX_REQUIRE(latent && sigmas && context && F >= 1 && H >= 1 && W >= 1 && S >= 1 && n_sigmas >= 2, "ltx_denoise: bad arguments");
        const int nb = (opt && opt->cfg_scale > 1.0f) ? 2 : 1;
        const size_t n_lat = (size_t)m->cfg.in_channels * F * H * W * 4;
        const size_t n_ctx = (size_t)nb * S * m->cfg.caption_channels * 2;
        const size_t n_mask = (size_t)nb * S * 4;
        DevBuf &d_lat = ctx->h2d[H2D_DENOISE_LATENT], &d_ctx = ctx->h2d[H2D_DENOISE_CONTEXT], &d_mask = ctx->h2d[H2D_DENOISE_MASK];
        d_ctx.ensure(n_ctx);
        d_mask.ensure(n_mask);
        stage_in(ctx, d_lat, latent, n_lat);
        stage_in(ctx, d_ctx, context, n_ctx);
        if (mask) stage_in(ctx, d_mask, mask, n_mask);
        const ContextSignature sig = context_signature(context, n_ctx, mask, (long)nb * S);
        DenoiseParams p;
        p.latent = d_lat.as<float>(); p.F = F; p.H = H; p.W = W;
        p.sigmas = sigmas; p.n_sigmas = n_sigmas;
        p.context = d_ctx.as<bf16_t>();
        p.mask = mask ? d_mask.as<int32_t>() : nullptr;
        p.mask_all_ones = sig.all_ones; p.S = S;
        p.ctx_version = sig.version;
        fill_params(p, opt);
        if (opt && opt->cond_latent) {  // image-to-video: stage the image latent (and the re-noising draws) on the device
            const size_t n_c = (size_t)m->cfg.in_channels * H * W * 4;
            stage_in(ctx, ctx->i2v_cond, opt->cond_latent, n_c);
            p.cond_latent = ctx->i2v_cond.as<float>();
            if (opt->cond_noise) {
                stage_in(ctx, ctx->i2v_noise, opt->cond_noise, n_c * (n_sigmas - 1));
                p.cond_noise = ctx->i2v_noise.as<float>();
            }
        }
        p.progress = cb; p.user = user;
        denoise_run(ctx, p);
        stage_out(ctx, latent, d_lat, n_lat);
        stage_sync(ctx);
    });
}

// ---- multi-GPU ----
int ltx_dist_unique_id(void* id_out) {
    if (!id_out) return LTX_ERR_INVALID_CONFIGURATION;
    return guarded(nullptr, [&] { dist_unique_id(id_out); });
}

int ltx_dist_init(ltx_ctx* ctx, int rank, int world, const void* id) {
    return with_ctx(ctx, [&] { dist_init_native(ctx, rank, world, id); });
}

int ltx_dist_set_transport(ltx_ctx* ctx, int rank, int world, ltx_allgather_fn gather, void* user) {
    return with_ctx(ctx, [&] { dist_set_transport(ctx, rank, world, gather, user); });
}

int ltx_dist_shutdown(ltx_ctx* ctx) {
    return with_ctx(ctx, [&] { dist_shutdown(ctx); });
}

int ltx_dist_info(const ltx_ctx* ctx, int* rank, int* world, int* native_transport, long* n_collectives) {
    if (!ctx) return LTX_ERR_INVALID_CONFIGURATION;
    if (rank) *rank = dist_rank(ctx);
    if (world) *world = dist_world(ctx);
    if (native_transport) *native_transport = (ctx->dist && ctx->dist->comm) ? 1 : 0;
    if (n_collectives) *n_collectives = ctx->dist ? ctx->dist->n_collectives : 0;
    return LTX_OK;
}

int ltx_dist_allgather_dev(ltx_ctx* ctx, const void* send, void* recv, long bytes) {
    return with_ctx(ctx, [&] { dist_allgather(ctx, send, recv, bytes); });
}

int ltx_dist_broadcast_dev(ltx_ctx* ctx, void* buf, long bytes, int root) {
    return with_ctx(ctx, [&] { dist_broadcast(ctx, buf, bytes, root); });
}

/* ---- text-embedding connector ---- */
int ltx_connector_load(ltx_ctx* ctx, const char* path, const ltx_connector_config* cfg) {
    if (!ctx || !path) return LTX_ERR_INVALID_CONFIGURATION;
    return guarded(ctx, [&] {
        replace_model(ctx, &ctx->connector, [&] { return connector_create(to_conn_cfg(cfg)); },
                      [&](ConnectorModel* m) { connector_load_safetensors(ctx, m, path); }, connector_destroy);
    });
}

int ltx_connector_init_synthetic(ltx_ctx* ctx, const ltx_connector_config* cfg, unsigned long seed) {
    return with_ctx(ctx, [&] {
        replace_model(ctx, &ctx->connector, [&] { return connector_create(to_conn_cfg(cfg)); },
                      [&](ConnectorModel* m) { connector_init_synthetic(ctx, m, seed); }, connector_destroy);
    });
}

int ltx_connector_unload(ltx_ctx* ctx) {
    return with_ctx(ctx, [&] { unload_model(ctx, &ctx->connector, connector_destroy); });
}

int ltx_connector_encode_taps_dev(ltx_ctx* ctx, const uint16_t* hidden, const int32_t* attention_mask, int B, int T,
                                  int padding_right, uint16_t* context, uint16_t* norm_concat, uint16_t* fe_out,
                                  float* after_registers) {
    return with_ctx(ctx, [&] {
        ConnectorModel* m = need(ctx->connector, kNoConnector);
        ConnectorArgs a;
        a.hidden = hidden; a.mask = attention_mask; a.B = B; a.T = T; a.padding_right = padding_right;
        a.out = context; a.dbg_nc = norm_concat; a.dbg_fe = fe_out; a.dbg_reg = after_registers;
        connector_encode(ctx, m, a);
    });
}

namespace {
// ltx_connector_encode_dev and ltx_connector_encode_av_dev: `av` asks for the audio set's context too
void connector_encode_dev_body(ltx_ctx* ctx, const uint16_t* hidden, const int32_t* attention_mask, int B, int T, int padding_right,
                               uint16_t* context, bool av, uint16_t* audio_context, int32_t* out_mask) {
    ConnectorModel* m = need(ctx->connector, kNoConnector);
    if (av) {
        need(m->audio, kNoAudioConnector);
        LTX_REQUIRE(audio_context, "connector_encode_av: null audio context");
    }
    ConnectorArgs a;
    a.hidden = hidden; a.mask = attention_mask; a.B = B; a.T = T; a.padding_right = padding_right;
    a.out = context; a.out_audio = av ? audio_context : nullptr; a.out_mask = out_mask;
    connector_encode(ctx, m, a);
}
void connector_encode_host_body(ltx_ctx* ctx, const uint16_t* hidden, const int32_t* attention_mask, int B, int T, int padding_right,
                                uint16_t* context, bool av, uint16_t* audio_context, int32_t* out_mask) {
    ConnectorModel* m = need(ctx->connector, kNoConnector);
    if (av) need(m->audio, kNoAudioConnector);
    LTX_REQUIRE(hidden && attention_mask && context && (!av || audio_context) && B >= 1 && T >= 1, "connector_encode: bad arguments");
    const ConnectorConfig& c = m->cfg;
    const size_t hb = (size_t)c.states * B * T * c.dim * 2, mb = (size_t)B * T * 4, ob = (size_t)B * T * c.dim * 2;
    DevBuf &d_hidden = ctx->h2d[H2D_CONN_HIDDEN], &d_mask = ctx->h2d[H2D_CONN_MASK], &d_context = ctx->h2d[H2D_CONN_CONTEXT],
           &d_out_mask = ctx->h2d[H2D_CONN_OUT_MASK];
    DevBuf d_audio;  // freed on return, after the synchronisation
    d_context.ensure(ob);
    d_out_mask.ensure(mb);
    if (av) d_audio.ensure(ob);
    stage_in(ctx, d_hidden, hidden, hb);
    stage_in(ctx, d_mask, attention_mask, mb);
    connector_encode_dev_body(ctx, d_hidden.as<uint16_t>(), d_mask.as<int32_t>(), B, T, padding_right, d_context.as<uint16_t>(), av,
                              d_audio.as<uint16_t>(), d_out_mask.as<int32_t>());
    stage_out(ctx, context, d_context, ob);
    if (av) stage_out(ctx, audio_context, d_audio, ob);
    if (out_mask) stage_out(ctx, out_mask, d_out_mask, mb);
    stage_sync(ctx);
}
}  // namespace

int ltx_connector_encode_dev(ltx_ctx* ctx, const uint16_t* hidden, const int32_t* attention_mask, int B, int T,
                             int padding_right, uint16_t* context, int32_t* out_mask) {
    return with_ctx(ctx, [&] { connector_encode_dev_body(ctx, hidden, attention_mask, B, T, padding_right, context, false, nullptr, out_mask); });
}

int ltx_connector_encode(ltx_ctx* ctx, const uint16_t* hidden, const int32_t* attention_mask, int B, int T,
                         int padding_right, uint16_t* context, int32_t* out_mask) {
    return with_ctx(ctx, [&] { connector_encode_host_body(ctx, hidden, attention_mask, B, T, padding_right, context, false, nullptr, out_mask); });
}

int ltx_connector_encode_av_dev(ltx_ctx* ctx, const uint16_t* hidden, const int32_t* attention_mask, int B, int T, int padding_right,
                                uint16_t* video_context, uint16_t* audio_context, int32_t* out_mask) {
    return with_ctx(ctx, [&] {
        connector_encode_dev_body(ctx, hidden, attention_mask, B, T, padding_right, video_context, true, audio_context, out_mask);
    });
}

int ltx_connector_encode_av(ltx_ctx* ctx, const uint16_t* hidden, const int32_t* attention_mask, int B, int T, int padding_right,
                            uint16_t* video_context, uint16_t* audio_context, int32_t* out_mask) {
    return with_ctx(ctx, [&] {
        connector_encode_host_body(ctx, hidden, attention_mask, B, T, padding_right, video_context, true, audio_context, out_mask);
    });
}

int ltx_connector_has_audio(ltx_ctx* ctx) { return ctx && ctx->connector && ctx->connector->audio ? 1 : 0; }

/* ---- Gemma-3 text encoder ---- */
int ltx_gemma_load(ltx_ctx* ctx, const char* const* paths, int n_paths, const ltx_gemma_config* cfg) {
    if (!ctx || !paths || n_paths < 1) return LTX_ERR_INVALID_CONFIGURATION;
    return guarded(ctx, [&] {
        std::vector<std::string> shards;
        for (int i = 0; i < n_paths; ++i) {
            LTX_REQUIRE(paths[i], "ltx_gemma_load: null path");
            shards.push_back(paths[i]);
        }
        replace_model(ctx, &ctx->gemma, [&] { return gemma_create(ctx, to_gemma_cfg(cfg)); },
                      [&](GemmaModel* m) { gemma_load_safetensors(ctx, m, shards); }, gemma_destroy);
    });
}

int ltx_gemma_init_synthetic(ltx_ctx* ctx, const ltx_gemma_config* cfg, unsigned long seed) {
    return with_ctx(ctx, [&] {
        replace_model(ctx, &ctx->gemma, [&] { return gemma_create(ctx, to_gemma_cfg(cfg)); },
                      [&](GemmaModel* m) { gemma_init_synthetic(ctx, m, seed); }, gemma_destroy);
    });
}

int ltx_gemma_unload(ltx_ctx* ctx) {
    return with_ctx(ctx, [&] { unload_model(ctx, &ctx->gemma, gemma_destroy); });
}

int ltx_gemma_memory_info(ltx_ctx* ctx, long* weight_bytes, long* workspace_bytes) {
    return with_ctx(ctx, [&] {
        const GemmaModel* m = ctx->gemma;
        const size_t w = m ? m->params.arena.buf.bytes + m->rope.bytes : 0;
        if (weight_bytes) *weight_bytes = (long)w;
        if (workspace_bytes) *workspace_bytes = m ? (long)(gemma_resident_bytes(m) - w) : 0;
    });
}

int ltx_gemma_encode_dev(ltx_ctx* ctx, const int32_t* token_ids, const int32_t* attention_mask, int B, int T, uint16_t* hidden) {
    return with_ctx(ctx, [&] {
        GemmaModel* m = need(ctx->gemma, kNoGemma);
        GemmaArgs a;
        a.ids = token_ids; a.mask = attention_mask; a.B = B; a.T = T; a.hidden = hidden;
        gemma_encode(ctx, m, a);
    });
}

int ltx_gemma_encode(ltx_ctx* ctx, const int32_t* token_ids, const int32_t* attention_mask, int B, int T, uint16_t* hidden) {
    return with_ctx(ctx, [&] {
        GemmaModel* m = need(ctx->gemma, kNoGemma);
        LTX_REQUIRE(token_ids && attention_mask && hidden && B >= 1 && T >= 1, "gemma_encode: bad arguments");
        const GemmaConfig& c = m->cfg;
        for (long i = 0; i < (long)B * T; ++i)
            LTX_REQUIRE(token_ids[i] >= 0 && token_ids[i] < c.vocab, "gemma_encode: token id %d at position %ld is outside the vocabulary of %d",
                        token_ids[i], i, c.vocab);
        const size_t ib = (size_t)B * T * 4, hb = (size_t)(c.layers + 1) * B * T * c.hidden * 2;
        DevBuf &d_ids = ctx->h2d[H2D_IN], &d_mask = ctx->h2d[H2D_CONN_MASK], &d_hidden = ctx->h2d[H2D_CONN_CONTEXT];
        d_hidden.ensure(hb);
        stage_in(ctx, d_ids, token_ids, ib);
        stage_in(ctx, d_mask, attention_mask, ib);
        GemmaArgs a;
        a.ids = d_ids.as<int32_t>(); a.mask = d_mask.as<int32_t>(); a.B = B; a.T = T; a.hidden = d_hidden.as<bf16_t>();
        gemma_encode(ctx, m, a);
        stage_out(ctx, hidden, d_hidden, hb);
        stage_sync(ctx);
    });
}

namespace {
void text_encode_body(ltx_ctx* ctx, const int32_t* token_ids, const int32_t* attention_mask, int B, int T, uint16_t* context, bool av,
                      uint16_t* audio_context, int32_t* out_mask) {
    GemmaModel* g = need(ctx->gemma, kNoGemma);
    ConnectorModel* m = need(ctx->connector, kNoConnector);
    if (av) need(m->audio, kNoAudioConnector);
    LTX_REQUIRE(B >= 1 && T >= 1 && context && (!av || audio_context), "text_encode: bad arguments");
    LTX_REQUIRE(m->cfg.states == g->cfg.layers + 1 && m->cfg.dim == g->cfg.hidden,
                "text_encode: the connector takes %d states of %d, the encoder makes %d of %d", m->cfg.states, m->cfg.dim, g->cfg.layers + 1,
                g->cfg.hidden);
    g->ws_hidden.ensure((size_t)(g->cfg.layers + 1) * B * T * g->cfg.hidden * 2);
    GemmaArgs ga;
    ga.ids = token_ids; ga.mask = attention_mask; ga.B = B; ga.T = T; ga.hidden = g->ws_hidden.as<bf16_t>();
    gemma_encode(ctx, g, ga);
    ConnectorArgs a;
    a.hidden = ga.hidden; a.mask = attention_mask; a.B = B; a.T = T; a.padding_right = 0;
    a.out = context; a.out_audio = av ? audio_context : nullptr; a.out_mask = out_mask;
    connector_encode(ctx, m, a);
}
void check_token_ids(const GemmaModel* m, const int32_t* token_ids, long n) {
    for (long i = 0; i < n; ++i)
        LTX_REQUIRE(token_ids[i] >= 0 && token_ids[i] < m->cfg.vocab, "gemma_encode: token id %d at position %ld is outside the vocabulary of %d",
                    token_ids[i], i, m->cfg.vocab);
}
}  // namespace

namespace {
void text_encode_host_body(ltx_ctx* ctx, const int32_t* token_ids, const int32_t* attention_mask, int B, int T, uint16_t* context, bool av,
                           uint16_t* audio_context, int32_t* out_mask) {
    GemmaModel* g = need(ctx->gemma, kNoGemma);
    ConnectorModel* m = need(ctx->connector, kNoConnector);
    if (av) need(m->audio, kNoAudioConnector);
    LTX_REQUIRE(token_ids && attention_mask && context && (!av || audio_context) && B >= 1 && T >= 1, "text_encode: bad arguments");
    check_token_ids(g, token_ids, (long)B * T);
    const size_t ib = (size_t)B * T * 4, ob = (size_t)B * T * m->cfg.dim * 2;
    DevBuf &d_ids = ctx->h2d[H2D_IN], &d_mask = ctx->h2d[H2D_CONN_MASK], &d_context = ctx->h2d[H2D_CONN_CONTEXT],
           &d_out_mask = ctx->h2d[H2D_CONN_OUT_MASK];
    DevBuf d_audio;  // freed on return, after the synchronisation
    d_context.ensure(ob);
    d_out_mask.ensure(ib);
    if (av) d_audio.ensure(ob);
    stage_in(ctx, d_ids, token_ids, ib);
    stage_in(ctx, d_mask, attention_mask, ib);
    text_encode_body(ctx, d_ids.as<int32_t>(), d_mask.as<int32_t>(), B, T, d_context.as<uint16_t>(), av, d_audio.as<uint16_t>(),
                     d_out_mask.as<int32_t>());
    stage_out(ctx, context, d_context, ob);
    if (av) stage_out(ctx, audio_context, d_audio, ob);
    if (out_mask) stage_out(ctx, out_mask, d_out_mask, ib);
    stage_sync(ctx);
}
}  // namespace

int ltx_text_encode_dev(ltx_ctx* ctx, const int32_t* token_ids, const int32_t* attention_mask, int B, int T, uint16_t* context,
                        int32_t* out_mask) {
    return with_ctx(ctx, [&] { text_encode_body(ctx, token_ids, attention_mask, B, T, context, false, nullptr, out_mask); });
}

int ltx_text_encode(ltx_ctx* ctx, const int32_t* token_ids, const int32_t* attention_mask, int B, int T, uint16_t* context, int32_t* out_mask) {
    return with_ctx(ctx, [&] { text_encode_host_body(ctx, token_ids, attention_mask, B, T, context, false, nullptr, out_mask); });
}

int ltx_text_av_encode_dev(ltx_ctx* ctx, const int32_t* token_ids, const int32_t* attention_mask, int B, int T, uint16_t* video_context,
                           uint16_t* audio_context, int32_t* out_mask) {
    return with_ctx(ctx, [&] { text_encode_body(ctx, token_ids, attention_mask, B, T, video_context, true, audio_context, out_mask); });
}

int ltx_text_av_encode(ltx_ctx* ctx, const int32_t* token_ids, const int32_t* attention_mask, int B, int T, uint16_t* video_context,
                       uint16_t* audio_context, int32_t* out_mask) {
    return with_ctx(ctx, [&] { text_encode_host_body(ctx, token_ids, attention_mask, B, T, video_context, true, audio_context, out_mask); });
}

/* ---- Gemma-3 token generation (prompt enhancement) ---- */
void ltx_lm_params_default(ltx_lm_params* p) {
    if (!p) return;
    const GemmaLmParams d;
    memset(p, 0, sizeof(*p));
    p->struct_size = (uint32_t)sizeof(*p);
    p->max_new_tokens = d.max_new; p->temperature = d.temperature; p->top_p = d.top_p; p->repetition_penalty = d.penalty;
    p->repetition_context = d.context; p->seed = d.seed; p->n_eos = d.n_eos;
    for (int i = 0; i < 8; ++i) p->eos_ids[i] = d.eos[i];
}

int ltx_lm_begin(ltx_ctx* ctx, int capacity) {
    return with_ctx(ctx, [&] { gemma_lm_begin(ctx, need(ctx->gemma, kNoGemma), capacity); });
}

int ltx_lm_end(ltx_ctx* ctx, long* freed_bytes) {
    return with_ctx(ctx, [&] {
        if (freed_bytes) *freed_bytes = 0;
        const size_t n = gemma_lm_end(ctx, need(ctx->gemma, kNoGemma));
        if (freed_bytes) *freed_bytes = (long)n;
    });
}

int ltx_lm_memory_info(ltx_ctx* ctx, long* cache_bytes, long* workspace_bytes) {
    return with_ctx(ctx, [&] {
        if (cache_bytes) *cache_bytes = 0;
        if (workspace_bytes) *workspace_bytes = 0;
        const GemmaLm* lm = need(ctx->gemma, kNoGemma)->lm;
        if (cache_bytes) *cache_bytes = lm ? (long)lm->cache_bytes() : 0;
        if (workspace_bytes) *workspace_bytes = lm ? (long)lm->workspace_bytes() : 0;
    });
}

namespace {
GemmaModel* need_lm(ltx_ctx* ctx, const char* who) {
    GemmaModel* m = need(ctx->gemma, kNoGemma);
    LTX_REQUIRE(m->lm != nullptr, "%s: no generation session (ltx_lm_begin)", who);
    return m;
}
void lm_logits_out(ltx_ctx* ctx, GemmaModel* m, float* logits, bool host) {
    if (!logits) return;
    HIP_CHECK(hipMemcpyAsync(logits, m->lm->logits.p, (size_t)m->cfg.vocab * 4, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, ctx->stream));
    if (host) stage_sync(ctx);
}
}  // namespace

int ltx_lm_prefill_dev(ltx_ctx* ctx, const int32_t* ids, int T, float* logits) {
    return with_ctx(ctx, [&] {
        GemmaModel* m = need_lm(ctx, "ltx_lm_prefill_dev");
        gemma_lm_prefill(ctx, m, ids, T);
        lm_logits_out(ctx, m, logits, false);
    });
}

int ltx_lm_prefill(ltx_ctx* ctx, const int32_t* ids, int T, float* logits) {
    return with_ctx(ctx, [&] {
        GemmaModel* m = need_lm(ctx, "ltx_lm_prefill");
        LTX_REQUIRE(ids && T >= 1 && T <= m->lm->cap, "ltx_lm_prefill: null ids, an empty prompt or %d tokens above the session's capacity %d", T, m->lm->cap);
        for (int i = 0; i < T; ++i)
            LTX_REQUIRE(ids[i] >= 0 && ids[i] < m->cfg.vocab, "ltx_lm_prefill: token id %d at position %d is outside the vocabulary of %d", ids[i], i, m->cfg.vocab);
        if (T > m->cfg.sliding_window) LTX_THROW(LTXS_INVALID_CONFIGURATION, "lm_prefill: %d tokens exceed the sliding window %d", T, m->cfg.sliding_window);
        int32_t* d_ids = m->lm->hist.as<int32_t>();  // the history is unused until the first pick, and holds cap + 2 entries
        HIP_CHECK(hipMemcpyAsync(d_ids, ids, (size_t)T * 4, hipMemcpyHostToDevice, ctx->stream));
        gemma_lm_prefill(ctx, m, d_ids, T);
        lm_logits_out(ctx, m, logits, true);
        stage_sync(ctx);  // ids is the caller's
    });
}

int ltx_lm_step_dev(ltx_ctx* ctx, const int32_t* token, float* logits) {
    return with_ctx(ctx, [&] {
        GemmaModel* m = need_lm(ctx, "ltx_lm_step_dev");
        gemma_lm_step(ctx, m, token);
        lm_logits_out(ctx, m, logits, false);
    });
}

int ltx_lm_step(ltx_ctx* ctx, int32_t token, float* logits) {
    return with_ctx(ctx, [&] {
        GemmaModel* m = need_lm(ctx, "ltx_lm_step");
        LTX_REQUIRE(token >= 0 && token < m->cfg.vocab, "ltx_lm_step: token id %d is outside the vocabulary of %d", token, m->cfg.vocab);
        LTX_REQUIRE(m->lm->len >= 1 && m->lm->len < m->lm->cap, "ltx_lm_step: no prompt in the session, or the cache is full (%d of %d positions)",
                    m->lm->len, m->lm->cap);
        int32_t* d_tok = m->lm->hist.as<int32_t>() + m->lm->cap;  // the staged-token entry
        HIP_CHECK(hipMemcpyAsync(d_tok, &token, 4, hipMemcpyHostToDevice, ctx->stream));
        gemma_lm_step(ctx, m, d_tok);
        lm_logits_out(ctx, m, logits, true);
        stage_sync(ctx);  // token is a parameter of this call
    });
}

int ltx_lm_last_state(ltx_ctx* ctx, uint16_t* state) {
    return with_ctx(ctx, [&] {
        GemmaModel* m = need_lm(ctx, "ltx_lm_last_state");
        LTX_REQUIRE(state && m->lm->len >= 1, "ltx_lm_last_state: null output or no prompt in the session");
        HIP_CHECK(hipMemcpyAsync(state, gemma_lm_state(m), (size_t)m->cfg.hidden * 2, hipMemcpyDeviceToHost, ctx->stream));
        stage_sync(ctx);
    });
}

int ltx_lm_cache_k(ltx_ctx* ctx, int layer, int rows, uint16_t* k) {
    return with_ctx(ctx, [&] {
        GemmaModel* m = need_lm(ctx, "ltx_lm_cache_k");
        LTX_REQUIRE(k && layer >= 0 && layer < m->cfg.layers && rows >= 1 && rows <= m->lm->len, "ltx_lm_cache_k: layer %d, %d rows of %d filled", layer, rows,
                    m->lm->len);
        const size_t Dk = (size_t)m->cfg.kv_heads * 256;
        HIP_CHECK(hipMemcpyAsync(k, m->lm->kc.as<bf16_t>() + (size_t)layer * m->lm->cap * Dk, (size_t)rows * Dk * 2, hipMemcpyDeviceToHost, ctx->stream));
        stage_sync(ctx);
    });
}

int ltx_lm_cache_vt(ltx_ctx* ctx, int layer, int cols, uint16_t* vt) {
    return with_ctx(ctx, [&] {
        GemmaModel* m = need_lm(ctx, "ltx_lm_cache_vt");
        const long ldvt = m->lm->ldvt;
        LTX_REQUIRE(vt && layer >= 0 && layer < m->cfg.layers && cols >= 1 && cols <= ldvt, "ltx_lm_cache_vt: layer %d, %d columns of %ld", layer, cols, ldvt);
        const size_t Dk = (size_t)m->cfg.kv_heads * 256;
        HIP_CHECK(hipMemcpy2DAsync(vt, (size_t)cols * 2, m->lm->vt.as<bf16_t>() + (size_t)layer * Dk * ldvt, (size_t)ldvt * 2, (size_t)cols * 2, Dk,
                                   hipMemcpyDeviceToHost, ctx->stream));
        stage_sync(ctx);
    });
}

int ltx_lm_generate(ltx_ctx* ctx, const int32_t* ids, int T, const ltx_lm_params* params, int32_t* out_tokens, int* n_out) {
    return with_ctx(ctx, [&] {
        if (n_out) *n_out = 0;
        GemmaModel* m = need_lm(ctx, "ltx_lm_generate");
        LTX_REQUIRE(n_out != nullptr, "ltx_lm_generate: null n_out");
        GemmaLmParams p;
        if (params) {
            const size_t sz = params->struct_size;
            LTX_REQUIRE(sz >= offsetof(ltx_lm_params, eos_ids) + sizeof(params->eos_ids) && sz <= 4096,
                        "ltx_lm_params.struct_size = %zu: set it to sizeof(ltx_lm_params) (ltx_lm_params_default); this library is ABI revision %d", sz,
                        LTX_ABI_VERSION);
            LTX_REQUIRE(params->n_eos >= 0 && params->n_eos <= 8, "ltx_lm_generate: %d stop ids (up to 8)", params->n_eos);
            p.max_new = params->max_new_tokens; p.temperature = params->temperature; p.top_p = params->top_p; p.penalty = params->repetition_penalty;
            p.context = params->repetition_context; p.seed = params->seed; p.n_eos = params->n_eos;
            for (int i = 0; i < 8; ++i) p.eos[i] = params->eos_ids[i];
        }
        *n_out = gemma_lm_generate(ctx, m, ids, T, p, out_tokens);
    });
}

int ltx_lm_sample_host(float* logits, int vocab, const int32_t* generated, int n_generated, int context, float penalty, float temperature,
                       float top_p, uint64_t seed, int step, int32_t* token) {
    return guarded(nullptr, [&] {
        LTX_REQUIRE(logits && token && vocab >= 1, "ltx_lm_sample_host: null logits / token or an empty vocabulary");
        LTX_REQUIRE(n_generated >= 0 && context >= 0 && (generated || n_generated == 0), "ltx_lm_sample_host: n_generated=%d context=%d need the tokens", n_generated,
                    context);
        LTX_REQUIRE(penalty > 0.f && (temperature <= 0.f || (top_p > 0.f && top_p <= 1.f)), "ltx_lm_sample_host: penalty %g must be positive, top_p %g in (0, 1]",
                    (double)penalty, (double)top_p);
        *token = lm_sample_host(logits, vocab, generated, n_generated, context, penalty, temperature, top_p, seed, step);
    });
}

/* ---- VAE encoder ---- */
int ltx_vae_encoder_load(ltx_ctx* ctx, const char* path, int channel_base) {
    if (!ctx || !path) return LTX_ERR_INVALID_CONFIGURATION;
    return guarded(ctx, [&] {
        replace_model(ctx, &ctx->vae_encoder, [&] { return vae_encoder_create(channel_base > 0 ? channel_base : 128); },
                      [&](VaeEncoderModel* m) { vae_encoder_load_safetensors(ctx, m, path); }, vae_encoder_destroy);
    });
}

int ltx_vae_encoder_init_synthetic(ltx_ctx* ctx, int channel_base, unsigned long seed) {
    return with_ctx(ctx, [&] {
        replace_model(ctx, &ctx->vae_encoder, [&] { return vae_encoder_create(channel_base > 0 ? channel_base : 128); },
                      [&](VaeEncoderModel* m) { vae_encoder_init_synthetic(ctx, m, seed); }, vae_encoder_destroy);
    });
}

int ltx_vae_encoder_unload(ltx_ctx* ctx) {
    return with_ctx(ctx, [&] { unload_model(ctx, &ctx->vae_encoder, vae_encoder_destroy); });
}

int ltx_vae_encode_dev(ltx_ctx* ctx, const float* pixels, int T, int H, int W, int normalize, float* latent) {
    return with_ctx(ctx, [&] { encode_body(ctx, pixels, T, H, W, normalize, latent); });
}

int ltx_vae_encode(ltx_ctx* ctx, const float* pixels, int T, int H, int W, int normalize, float* latent) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(pixels && latent && T >= 1 && H >= 1 && W >= 1, "ltx_vae_encode: bad arguments");
        const size_t nb_in = (size_t)3 * T * H * W * 4;
        const size_t nb_out = (size_t)128 * vae_encoder_latent_frames(T) * (H / 32) * (W / 32) * 4;
        DevBuf &d_pixels = ctx->h2d[H2D_IN], &d_latent = ctx->h2d[H2D_OUT];
        d_latent.ensure(nb_out ? nb_out : 4);
        stage_in(ctx, d_pixels, pixels, nb_in);
        encode_body(ctx, d_pixels.as<float>(), T, H, W, normalize, d_latent.as<float>());
        stage_out(ctx, latent, d_latent, nb_out);
        stage_sync(ctx);
    });
}

/* ---- audio decode leg (audio.h) ---- */
int ltx_audio_vae_load(ltx_ctx* ctx, const char* path) {
    if (!ctx || !path) return LTX_ERR_INVALID_CONFIGURATION;
    return guarded(ctx, [&] {
        replace_model(ctx, &ctx->audio_vae, audio_vae_create, [&](AudioVaeModel* m) { audio_vae_load(ctx, m, path); }, audio_vae_destroy);
    });
}
int ltx_audio_vae_init_synthetic(ltx_ctx* ctx, int base_channels, uint64_t seed) {
    return with_ctx(ctx, [&] {
        replace_model(ctx, &ctx->audio_vae, audio_vae_create,
                      [&](AudioVaeModel* m) { audio_vae_init_synthetic(ctx, m, base_channels > 0 ? base_channels : 128, seed); },
                      audio_vae_destroy);
    });
}
int ltx_audio_vae_unload(ltx_ctx* ctx) {
    return with_ctx(ctx, [&] { unload_model(ctx, &ctx->audio_vae, audio_vae_destroy); });
}
int ltx_vocoder_load(ltx_ctx* ctx, const char* path) {
    if (!ctx || !path) return LTX_ERR_INVALID_CONFIGURATION;
    return guarded(ctx, [&] {
        replace_model(ctx, &ctx->vocoder, vocoder_create, [&](VocoderModel* m) { vocoder_load(ctx, m, path); }, vocoder_destroy);
    });
}
int ltx_vocoder_init_synthetic(ltx_ctx* ctx, int hidden_channels, uint64_t seed) {
    return with_ctx(ctx, [&] {
        replace_model(ctx, &ctx->vocoder, vocoder_create,
                      [&](VocoderModel* m) { vocoder_init_synthetic(ctx, m, hidden_channels > 0 ? hidden_channels : 1024, seed); },
                      vocoder_destroy);
    });
}
int ltx_vocoder_unload(ltx_ctx* ctx) {
    return with_ctx(ctx, [&] { unload_model(ctx, &ctx->vocoder, vocoder_destroy); });
}

int ltx_audio_vae_decode_dev(ltx_ctx* ctx, const float* latent, int T, float* mel) {
    return with_ctx(ctx, [&] { audio_vae_decode(ctx, need(ctx->audio_vae, kNoAudioVae), latent, T, mel); });
}
int ltx_audio_vae_decode(ltx_ctx* ctx, const float* latent, int T, float* mel) {
    return with_ctx(ctx, [&] {
        AudioVaeModel* m = need(ctx->audio_vae, kNoAudioVae);
        LTX_REQUIRE(T >= 1 && T <= 4096, "ltx_audio_vae_decode: T=%d", T);
        const size_t n_mel = (size_t)2 * audio_mel_frames(T) * 64;
        const float* d_latent = audio_stage_in(ctx, latent, (size_t)8 * T * 16, mel, n_mel);
        audio_vae_decode(ctx, m, d_latent, T, ctx->h2d[H2D_OUT].as<float>());
        audio_stage_out(ctx, mel, n_mel);
    });
}
int ltx_vocoder_forward_dev(ltx_ctx* ctx, const float* mel, int T_mel, float* waveform) {
    return with_ctx(ctx, [&] { vocoder_forward(ctx, need(ctx->vocoder, kNoVocoder), mel, T_mel, waveform); });
}
int ltx_vocoder_forward(ltx_ctx* ctx, const float* mel, int T_mel, float* waveform) {
    return with_ctx(ctx, [&] {
        VocoderModel* m = need(ctx->vocoder, kNoVocoder);
        LTX_REQUIRE(T_mel >= 1 && T_mel <= 16384, "ltx_vocoder_forward: T_mel=%d", T_mel);
        const size_t n_wave = (size_t)2 * 240 * T_mel;
        const float* d_mel = audio_stage_in(ctx, mel, (size_t)2 * T_mel * 64, waveform, n_wave);
        vocoder_forward(ctx, m, d_mel, T_mel, ctx->h2d[H2D_OUT].as<float>());
        audio_stage_out(ctx, waveform, n_wave);
    });
}
int ltx_audio_decode_dev(ltx_ctx* ctx, const float* latent, int T, float* waveform) {
    return with_ctx(ctx, [&] { audio_decode_body(ctx, latent, T, waveform); });
}
int ltx_audio_decode(ltx_ctx* ctx, const float* latent, int T, float* waveform) {
    return with_ctx(ctx, [&] {
        need(ctx->audio_vae, kNoAudioVae);  // a missing model is reported before a bad argument
        need(ctx->vocoder, kNoVocoder);
        LTX_REQUIRE(T >= 1 && T <= 4096, "ltx_audio_decode: T=%d", T);
        const size_t n_wave = (size_t)2 * 240 * audio_mel_frames(T);
        const float* d_latent = audio_stage_in(ctx, latent, (size_t)8 * T * 16, waveform, n_wave);
        audio_decode_body(ctx, d_latent, T, ctx->h2d[H2D_OUT].as<float>());
        audio_stage_out(ctx, waveform, n_wave);
    });
}

/* ---- LTXAttention at head dim 64: the audio / cross-modal attention modules of the dual block (attn_module.h) ---- */
int ltx_attn_module_init_synthetic(ltx_ctx* ctx, int index, int query_dim, int context_dim, int heads, uint64_t seed) {
    return with_ctx(ctx, [&] {
        replace_model(ctx, attn_slot(ctx, index), [&] { return attn_module_create(query_dim, context_dim > 0 ? context_dim : query_dim, heads); },
                      [&](AttnModule* m) { attn_module_init_synthetic(ctx, m, seed); }, attn_module_destroy);
    });
}
int ltx_attn_module_load(ltx_ctx* ctx, int index, const char* path, const char* key_prefix, int heads) {
    if (!ctx || !path || !key_prefix) return LTX_ERR_INVALID_CONFIGURATION;
    return guarded(ctx, [&] {
        AttnModule** slot = attn_slot(ctx, index);
        int Dq = 0, Dc = 0, inner = 0;
        attn_module_file_shape(path, key_prefix, &Dq, &Dc, &inner);
        LTX_REQUIRE(heads >= 1 && (long)heads * 64 == inner, "ltx_attn_module_load: %d heads of 64 do not make the file's inner dim %d (%sto_q)", heads,
                    inner, key_prefix);
        replace_model(ctx, slot, [&] { return attn_module_create(Dq, Dc, heads); },
                      [&](AttnModule* m) { attn_module_load(ctx, m, path, key_prefix); }, attn_module_destroy);
    });
}
int ltx_attn_module_unload(ltx_ctx* ctx, int index) {
    return with_ctx(ctx, [&] { unload_model(ctx, attn_slot(ctx, index), attn_module_destroy); });
}
long ltx_attn_module_export_param(ltx_ctx* ctx, int index, const char* name, float* out, long cap) {
    return export_param_body(ctx, "ltx_attn_module_export_param", name, out, cap,
                             [&] { return need(*attn_slot(ctx, index), kNoAttnModule)->params.find(name); });
}
int ltx_attn_module_forward_dev(ltx_ctx* ctx, int index, const float* x, const void* context, int context_bf16, int B, int Tq, int Tk,
                                const float* q_cos, const float* q_sin, int q_table_rows, const float* k_cos, const float* k_sin,
                                int k_table_rows, const float* key_bias, float* out) {
    return with_ctx(ctx, [&] {
        AttnModule* m = need(*attn_slot(ctx, index), kNoAttnModule);
        AttnModuleArgs a;
        a.x = x; a.context = context; a.context_bf16 = context_bf16;
        a.B = B; a.Tq = Tq; a.Tk = Tk;
        a.q_cos = q_cos; a.q_sin = q_sin; a.q_rows = q_table_rows;
        a.k_cos = k_cos; a.k_sin = k_sin; a.k_rows = k_table_rows;
        a.key_bias = key_bias;
        a.out = out;
        attn_module_forward(ctx, m, a);
    });
}

/* ---- LTX2TransformerBlock x L: the dual video + audio transformer blocks (dual_block.h) ---- */
void ltx_dual_block_config_default(ltx_dual_block_config* cfg) {
    if (!cfg) return;
    const DualBlockConfig d;
    cfg->num_layers = d.num_layers;
    cfg->video_heads = d.video_heads;
    cfg->video_dim = d.video_dim;
    cfg->audio_heads = d.audio_heads;
    cfg->audio_dim = d.audio_dim;
    cfg->video_context_dim = d.video_context_dim;
    cfg->audio_context_dim = d.audio_context_dim;
    cfg->rope_theta = d.rope_theta;
    for (int i = 0; i < 3; ++i) cfg->max_pos[i] = d.max_pos[i];
    cfg->audio_max_pos = d.audio_max_pos;
    cfg->fps = d.fps;
    cfg->norm_eps = d.norm_eps;
}
int ltx_dual_blocks_init_synthetic(ltx_ctx* ctx, const ltx_dual_block_config* cfg, uint64_t seed) {
    return with_ctx(ctx, [&] {
        replace_model(ctx, &ctx->dual, [&] { return dual_create(to_dual_cfg(cfg)); }, [&](DualStack* m) { dual_init_synthetic(ctx, m, seed); },
                      dual_destroy);
    });
}
int ltx_dual_blocks_load(ltx_ctx* ctx, const char* path, const ltx_dual_block_config* cfg, int first_block, int num_blocks) {
    if (!ctx || !path) return LTX_ERR_INVALID_CONFIGURATION;
    return guarded(ctx, [&] {
        LTX_REQUIRE(first_block >= 0 && num_blocks >= 1, "ltx_dual_blocks_load: first_block %d, num_blocks %d", first_block, num_blocks);
        DualBlockConfig c = to_dual_cfg(cfg);
        c.num_layers = num_blocks;
        replace_model(ctx, &ctx->dual, [&] { return dual_create(c); }, [&](DualStack* m) { dual_load(ctx, m, path, first_block); }, dual_destroy);
    });
}
int ltx_dual_blocks_unload(ltx_ctx* ctx) {
    return with_ctx(ctx, [&] { unload_model(ctx, &ctx->dual, dual_destroy); });
}
long ltx_dual_blocks_export_param(ltx_ctx* ctx, const char* name, float* out, long cap) {
    return export_param_body(ctx, "ltx_dual_blocks_export_param", name, out, cap, [&] { return need(ctx->dual, kNoDualBlocks)->params.find(name); });
}
int ltx_dual_blocks_forward_dev(ltx_ctx* ctx, const ltx_dual_forward_args* args) {
    if (!ctx) return LTX_ERR_INVALID_CONFIGURATION;
    return guarded(ctx, [&] {
        LTX_REQUIRE(args != nullptr, "ltx_dual_blocks_forward_dev: null arguments");
        const size_t sz = args->struct_size;
        LTX_REQUIRE(sz >= offsetof(ltx_dual_forward_args, cross_audio_ss) + sizeof(args->cross_audio_ss) && sz <= 4096,
                    "ltx_dual_forward_args.struct_size = %zu: set it to sizeof(ltx_dual_forward_args) (LTX_DUAL_FORWARD_ARGS_INIT); this library is ABI revision %d",
                    sz, LTX_ABI_VERSION);
        DualStack* m = need(ctx->dual, kNoDualBlocks);
        DualForwardArgs a;
        a.B = args->B; a.F = args->F; a.H = args->H; a.W = args->W; a.T_a = args->T_a; a.S = args->S;
        a.x_video = args->x_video; a.x_audio = args->x_audio;
        a.ctx_video = args->context_video; a.ctx_audio = args->context_audio;
        a.bias_video = args->key_bias_video; a.bias_audio = args->key_bias_audio;
        a.temb_video = args->temb_video; a.temb_audio = args->temb_audio;
        a.cross_video_ss = args->cross_video_ss; a.cross_audio_ss = args->cross_audio_ss;
        if (sz >= offsetof(ltx_dual_forward_args, phase_mask) + sizeof(args->phase_mask)) a.phase_mask = args->phase_mask;
        if (sz >= offsetof(ltx_dual_forward_args, n_groups) + sizeof(args->n_groups)) a.n_groups = args->n_groups;
        if (sz >= offsetof(ltx_dual_forward_args, video_row_map) + sizeof(args->video_row_map)) a.video_row_map = args->video_row_map;
        dual_forward(ctx, m, a);
    });
}

/* ---- LTX2Transformer: the dual video + audio model (dual_model.h) ---- */
void ltx_dual_model_config_default(ltx_dual_model_config* cfg) {
    if (!cfg) return;
    const DualModelConfig d;
    ltx_dual_block_config_default(&cfg->blocks);
    cfg->in_channels = d.in_channels;
    cfg->out_channels = d.out_channels;
    cfg->audio_in_channels = d.audio_in_channels;
    cfg->audio_out_channels = d.audio_out_channels;
    cfg->caption_channels = d.caption_channels;
    cfg->timestep_scale_multiplier = d.timestep_scale_multiplier;
}
int ltx_dual_model_init_synthetic(ltx_ctx* ctx, const ltx_dual_model_config* cfg, uint64_t seed) {
    return with_ctx(ctx, [&] {
        replace_model(ctx, &ctx->dual_model, [&] { return dual_model_create(to_dual_model_cfg(cfg)); },
                      [&](DualModel* m) { dual_model_init_synthetic(ctx, m, seed); }, dual_model_destroy);
    });
}
int ltx_dual_model_load(ltx_ctx* ctx, const char* path, const ltx_dual_model_config* cfg) {
    if (!ctx || !path) return LTX_ERR_INVALID_CONFIGURATION;
    return guarded(ctx, [&] {
        replace_model(ctx, &ctx->dual_model, [&] { return dual_model_create(to_dual_model_cfg(cfg)); },
                      [&](DualModel* m) { dual_model_load(ctx, m, path); }, dual_model_destroy);
    });
}
int ltx_dual_model_unload(ltx_ctx* ctx) {
    return with_ctx(ctx, [&] { unload_model(ctx, &ctx->dual_model, dual_model_destroy); });
}
long ltx_dual_model_export_param(ltx_ctx* ctx, const char* name, float* out, long cap) {
    return export_param_body(
        ctx, "ltx_dual_model_export_param", name, out, cap, [&] { return dual_model_find(need(ctx->dual_model, kNoDualModel), name); },
        [&](const ParamSlot& s, float* o) { quant_export_slot(ctx, s, ctx->dual_model->quant_bits, o); });
}
int ltx_dual_model_quantize(ltx_ctx* ctx, int bits, int group_size) {
    return with_ctx(ctx, [&] { dual_model_quantize(ctx, need(ctx->dual_model, kNoDualModel), bits, group_size); });
}
int ltx_dual_model_memory_info(ltx_ctx* ctx, long* bf16_weight_bytes, long* quantised_weight_bytes, long* scratch_bytes, long* other_bytes) {
    return with_ctx(ctx, [&] {
        for (long* p : {bf16_weight_bytes, quantised_weight_bytes, scratch_bytes, other_bytes})
            if (p) *p = 0;
        if (ctx->dual_model) dual_model_memory_info(ctx->dual_model, bf16_weight_bytes, quantised_weight_bytes, scratch_bytes, other_bytes);
    });
}
int ltx_dual_model_forward_dev(ltx_ctx* ctx, const ltx_dual_model_forward_args* args) {
    return ltx_dual_model_forward_groups_dev(ctx, args, 1, nullptr);
}
int ltx_dual_model_forward_groups_dev(ltx_ctx* ctx, const ltx_dual_model_forward_args* args, int n_groups, const int32_t* video_row_map) {
    if (!ctx) return LTX_ERR_INVALID_CONFIGURATION;
    return guarded(ctx, [&] {
        LTX_REQUIRE(args != nullptr, "ltx_dual_model_forward_dev: null arguments");
        const size_t sz = args->struct_size;
        LTX_REQUIRE(sz >= offsetof(ltx_dual_model_forward_args, audio_velocity) + sizeof(args->audio_velocity) && sz <= 4096,
                    "ltx_dual_model_forward_args.struct_size = %zu: set it to sizeof(ltx_dual_model_forward_args) (LTX_DUAL_MODEL_FORWARD_ARGS_INIT); this library is ABI revision %d",
                    sz, LTX_ABI_VERSION);
        DualModel* m = need(ctx->dual_model, kNoDualModel);
        DualModelForwardArgs a;
        a.B = args->B; a.F = args->F; a.H = args->H; a.W = args->W; a.T_a = args->T_a; a.S = args->S;
        a.video_latent = args->video_latent; a.audio_latent = args->audio_latent;
        a.video_context = args->video_context; a.audio_context = args->audio_context;
        a.video_timesteps = args->video_timesteps; a.audio_timesteps = args->audio_timesteps;
        a.video_mask = args->video_mask; a.audio_mask = args->audio_mask;
        a.video_velocity = args->video_velocity; a.audio_velocity = args->audio_velocity;
        if (sz >= offsetof(ltx_dual_model_forward_args, ungrouped) + sizeof(args->ungrouped)) a.ungrouped = args->ungrouped;
        if (sz >= offsetof(ltx_dual_model_forward_args, text_cache) + sizeof(args->text_cache)) a.text_cache = args->text_cache;
        a.n_groups = n_groups; a.video_row_map = video_row_map;
        dual_model_forward(ctx, m, a);
    });
}
int ltx_dual_model_embed_dev(ltx_ctx* ctx, const float* video_timesteps, const float* audio_timesteps, int B, int ungrouped,
                             float* temb_v, float* temb_a, float* cross_v, float* cross_a, float* embts_v, float* embts_a) {
    return with_ctx(ctx, [&] {
        DualModel* m = need(ctx->dual_model, kNoDualModel);
        DualEmbedOut o;
        o.temb_v = temb_v; o.temb_a = temb_a; o.cross_v = cross_v; o.cross_a = cross_a; o.embts_v = embts_v; o.embts_a = embts_a;
        dual_model_embed(ctx, m, video_timesteps, audio_timesteps, B, ungrouped, o);
    });
}
int ltx_dual_model_prepare_text_dev(ltx_ctx* ctx, const uint16_t* video_context, const uint16_t* audio_context, const int32_t* video_mask,
                                    const int32_t* audio_mask, int B, int S) {
    return with_ctx(ctx, [&] {
        DualModel* m = need(ctx->dual_model, kNoDualModel);
        dual_model_prepare_text(ctx, m, video_context, audio_context, video_mask, audio_mask, B, S);
    });
}
int ltx_dual_model_text_cache_info(ltx_ctx* ctx, int* B, int* S, long* bytes, long* builds) {
    return with_ctx(ctx, [&] {
        const DualTextCache& c = need(ctx->dual_model, kNoDualModel)->stack->text_cache;
        if (B) *B = c.B;
        if (S) *S = c.S;
        if (bytes) *bytes = c.bytes;
        if (builds) *builds = c.builds;
    });
}

/* ---- the joint video + audio denoise loop (dual_denoise.h) ---- */
namespace {
void dual_denoise_params(ltx_ctx* ctx, const ltx_dual_denoise_args* args, ltx_progress_cb cb, void* user, const char* who, DualDenoiseParams& p) {
    need(ctx->dual_model, kNoDualModel);
    LTX_REQUIRE(args != nullptr, "%s: null arguments", who);
    const size_t sz = args->struct_size;
    LTX_REQUIRE(sz >= offsetof(ltx_dual_denoise_args, step_stats) + sizeof(args->step_stats) && sz <= 4096,
                "ltx_dual_denoise_args.struct_size = %zu: set it to sizeof(ltx_dual_denoise_args) (LTX_DUAL_DENOISE_ARGS_INIT); this library is ABI revision %d",
                sz, LTX_ABI_VERSION);
    p.F = args->F; p.H = args->H; p.W = args->W; p.T_a = args->T_a; p.S = args->S;
    p.video_latent = args->video_latent; p.audio_latent = args->audio_latent;
    p.sigmas = args->sigmas; p.n_sigmas = args->n_sigmas;
    p.video_context = args->video_context; p.audio_context = args->audio_context; p.mask = args->mask;
    p.cfg_scale = args->cfg_scale; p.guidance_rescale = args->guidance_rescale;
    p.text_cache = args->text_cache; p.step_stats = args->step_stats;
    p.progress = cb; p.user = user;
    if (sz >= offsetof(ltx_dual_denoise_args, cond_latent) + sizeof(args->cond_latent)) p.cond_latent = args->cond_latent;
    if (sz >= offsetof(ltx_dual_denoise_args, image_cond_noise_scale) + sizeof(args->image_cond_noise_scale))
        p.image_cond_noise_scale = args->image_cond_noise_scale;
    if (sz >= offsetof(ltx_dual_denoise_args, cond_noise) + sizeof(args->cond_noise)) p.cond_noise = args->cond_noise;
}
}  // namespace

int ltx_dual_denoise_dev(ltx_ctx* ctx, const ltx_dual_denoise_args* args, ltx_progress_cb cb, void* user) {
    return with_ctx(ctx, [&] {
        DualDenoiseParams p;
        dual_denoise_params(ctx, args, cb, user, "ltx_dual_denoise_dev", p);
        dual_denoise_run(ctx, p);
    });
}

int ltx_dual_denoise(ltx_ctx* ctx, const ltx_dual_denoise_args* args, ltx_progress_cb cb, void* user) {
    return with_ctx(ctx, [&] {
        DualDenoiseParams p;
        dual_denoise_params(ctx, args, cb, user, "ltx_dual_denoise", p);
        const DualModel* m = ctx->dual_model;
        // what staging needs; dual_denoise_run repeats these checks among its own
        LTX_REQUIRE(p.video_latent && p.audio_latent && p.video_context && p.F >= 1 && p.H >= 1 && p.W >= 1 && p.T_a >= 1 && p.S >= 1 &&
                        p.T_a <= (1 << 20) && p.S <= (1 << 20) && (long)p.F * p.H * p.W <= (1 << 20) && p.n_sigmas >= 2 && p.sigmas,
                    "ltx_dual_denoise: bad arguments");
        LTX_REQUIRE(!(p.guidance_rescale > 0.f) || p.cfg_scale > 1.0f, "ltx_dual_denoise: guidance_rescale needs cfg_scale > 1");
        for (int i = 0; i + 1 < p.n_sigmas; ++i) LTX_REQUIRE(p.sigmas[i] > 0.f, "ltx_dual_denoise: sigmas[%d] must be positive", i);
        LTX_REQUIRE(!p.cond_latent || p.F >= 2, "ltx_dual_denoise: image-to-video needs at least two latent frames (F=%d)", p.F);
        const int nb = p.cfg_scale > 1.0f ? 2 : 1;
        const size_t n_v = (size_t)m->cfg.in_channels * p.F * p.H * p.W * 4, n_a = (size_t)128 * p.T_a * 4;
        const size_t n_ctx = (size_t)nb * p.S * m->cfg.caption_channels * 2, n_mask = (size_t)nb * p.S * 4;
        DevBuf &d_v = ctx->h2d[H2D_DENOISE_LATENT], &d_a = ctx->h2d[H2D_DUAL_AUDIO_LATENT], &d_cv = ctx->h2d[H2D_DENOISE_CONTEXT],
               &d_ca = ctx->h2d[H2D_DUAL_AUDIO_CONTEXT], &d_mask = ctx->h2d[H2D_DENOISE_MASK];
        float* host_v = p.video_latent;
        float* host_a = p.audio_latent;
        stage_in(ctx, d_v, host_v, n_v);
        stage_in(ctx, d_a, host_a, n_a);
        stage_in(ctx, d_cv, p.video_context, n_ctx);
        if (p.audio_context) stage_in(ctx, d_ca, p.audio_context, n_ctx);
        if (p.mask) stage_in(ctx, d_mask, p.mask, n_mask);
        p.video_latent = d_v.as<float>(); p.audio_latent = d_a.as<float>();
        p.video_context = d_cv.as<bf16_t>();
        p.audio_context = p.audio_context ? d_ca.as<bf16_t>() : nullptr;
        p.mask = p.mask ? d_mask.as<int32_t>() : nullptr;
        if (p.cond_latent) {  // the image latent and its re-noising slices, as ltx_denoise stages them
            const size_t n_c = (size_t)m->cfg.in_channels * p.H * p.W * 4;
            DevBuf &d_c = ctx->i2v_cond, &d_n = ctx->i2v_noise;
            stage_in(ctx, d_c, p.cond_latent, n_c);
            p.cond_latent = d_c.as<float>();
            if (p.cond_noise) {
                stage_in(ctx, d_n, p.cond_noise, n_c * (size_t)(p.n_sigmas - 1));
                p.cond_noise = d_n.as<float>();
            }
        }
        dual_denoise_run(ctx, p);
        stage_out(ctx, host_v, d_v, n_v);
        stage_out(ctx, host_a, d_a, n_a);
        stage_sync(ctx);
    });
}

/* ---- the two-stage video + audio path (dual_two_stage.h) ---- */
namespace {
void dual_two_stage_params(ltx_ctx* ctx, const ltx_dual_two_stage_args* args, ltx_progress_cb cb, void* user, const char* who, DualTwoStageParams& p) {
    need(ctx->dual_model, kNoDualModel);
    need(ctx->upscaler, kNoUpscaler);
    need(ctx->vae, kNoVae);
    LTX_REQUIRE(args != nullptr, "%s: null arguments", who);
    const size_t sz = args->struct_size;
    LTX_REQUIRE(sz >= sizeof(ltx_dual_two_stage_args) && sz <= 4096,
                "ltx_dual_two_stage_args.struct_size = %zu: set it to sizeof(ltx_dual_two_stage_args) (LTX_DUAL_TWO_STAGE_ARGS_INIT); this library is ABI revision %d",
                sz, LTX_ABI_VERSION);
    p.F = args->F; p.H = args->H; p.W = args->W; p.T_a = args->T_a; p.S = args->S;
    p.video_latent_in = args->video_latent_in; p.video_latent_out = args->video_latent_out; p.audio_latent = args->audio_latent;
    p.sigmas1 = args->sigmas1; p.n_sigmas1 = args->n_sigmas1; p.sigmas2 = args->sigmas2; p.n_sigmas2 = args->n_sigmas2;
    p.video_noise2 = args->video_noise2; p.audio_noise2 = args->audio_noise2;
    p.video_context = args->video_context; p.audio_context = args->audio_context; p.mask = args->mask;
    p.stage1_out = args->stage1_out;
    p.cond_latent1 = args->cond_latent1; p.cond_latent2 = args->cond_latent2; p.image_cond_noise_scale = args->image_cond_noise_scale;
    p.cond_noise1 = args->cond_noise1; p.cond_noise2 = args->cond_noise2;
    p.progress = cb; p.user = user;
}
}  // namespace

int ltx_dual_two_stage_dev(ltx_ctx* ctx, const ltx_dual_two_stage_args* args, ltx_progress_cb cb, void* user) {
    return with_ctx(ctx, [&] {
        DualTwoStageParams p;
        dual_two_stage_params(ctx, args, cb, user, "ltx_dual_two_stage_dev", p);
        dual_two_stage_run(ctx, p);
    });
}

int ltx_dual_two_stage(ltx_ctx* ctx, const ltx_dual_two_stage_args* args, ltx_progress_cb cb, void* user) {
    return with_ctx(ctx, [&] {
        DualTwoStageParams p;
        dual_two_stage_params(ctx, args, cb, user, "ltx_dual_two_stage", p);
        dual_two_stage_check(ctx, p);  // on the host pointers: refuse before anything is staged
        const DualModel* m = ctx->dual_model;
        const int steps1 = p.n_sigmas1 - 1, steps2 = (p.sigmas2 ? p.n_sigmas2 : 4) - 1;
        const size_t n_v1 = (size_t)m->cfg.in_channels * p.F * p.H * p.W * 4, n_v2 = 4 * n_v1, n_a = (size_t)128 * p.T_a * 4;
        const size_t n_c1 = n_v1 / p.F, n_c2 = n_v2 / p.F;
        const size_t n_ctx = (size_t)p.S * m->cfg.caption_channels * 2, n_mask = (size_t)p.S * 4;
        DevBuf &d_v = ctx->h2d[H2D_DENOISE_LATENT], &d_a = ctx->h2d[H2D_DUAL_AUDIO_LATENT], &d_cv = ctx->h2d[H2D_DENOISE_CONTEXT],
               &d_ca = ctx->h2d[H2D_DUAL_AUDIO_CONTEXT], &d_mask = ctx->h2d[H2D_DENOISE_MASK], &d_nv = ctx->h2d[H2D_DUAL2_VIDEO_NOISE],
               &d_na = ctx->h2d[H2D_DUAL2_AUDIO_NOISE], &d_out = ctx->h2d[H2D_DUAL2_VIDEO_OUT];
        DevBuf d_s1, d_c2, d_n2;  // freed on return, after the synchronisation
        float *host_out = p.video_latent_out, *host_a = p.audio_latent, *host_s1 = p.stage1_out;
        stage_in(ctx, d_v, p.video_latent_in, n_v1);
        stage_in(ctx, d_a, host_a, n_a);
        stage_in(ctx, d_nv, p.video_noise2, n_v2);
        stage_in(ctx, d_na, p.audio_noise2, n_a);
        stage_in(ctx, d_cv, p.video_context, n_ctx);
        if (p.audio_context) stage_in(ctx, d_ca, p.audio_context, n_ctx);
        if (p.mask) stage_in(ctx, d_mask, p.mask, n_mask);
        d_out.ensure(n_v2);
        p.video_latent_in = d_v.as<float>(); p.video_latent_out = d_out.as<float>(); p.audio_latent = d_a.as<float>();
        p.video_noise2 = d_nv.as<float>(); p.audio_noise2 = d_na.as<float>();
        p.video_context = d_cv.as<bf16_t>();
        p.audio_context = p.audio_context ? d_ca.as<bf16_t>() : nullptr;
        p.mask = p.mask ? d_mask.as<int32_t>() : nullptr;
        if (host_s1) {
            d_s1.ensure(n_v1);
            p.stage1_out = d_s1.as<float>();
        }
        if (p.cond_latent1) {  // the image latents and their re-noising slices; stage 1's as ltx_dual_denoise stages them
            stage_in(ctx, ctx->i2v_cond, p.cond_latent1, n_c1);
            stage_in(ctx, d_c2, p.cond_latent2, n_c2);
            p.cond_latent1 = ctx->i2v_cond.as<float>(); p.cond_latent2 = d_c2.as<float>();
            if (p.cond_noise1) {
                stage_in(ctx, ctx->i2v_noise, p.cond_noise1, n_c1 * (size_t)steps1);
                p.cond_noise1 = ctx->i2v_noise.as<float>();
            }
            if (p.cond_noise2) {
                stage_in(ctx, d_n2, p.cond_noise2, n_c2 * (size_t)steps2);
                p.cond_noise2 = d_n2.as<float>();
            }
        } else {
            p.cond_noise1 = p.cond_noise2 = nullptr;
        }
        dual_two_stage_run(ctx, p);
        stage_out(ctx, host_out, d_out, n_v2);
        stage_out(ctx, host_a, d_a, n_a);
        if (host_s1) stage_out(ctx, host_s1, d_s1, n_v1);
        stage_sync(ctx);
    });
}

/* ---- a generation from a seed: the draw plan, the noise launch and the loop (dual_generate.h) ---- */
namespace {
// the caller's struct into one with every field: what struct_size covers is copied, the rest keeps LTX_DUAL_GENERATE_ARGS_INIT
void dual_generate_params(const ltx_dual_generate_args* args, const char* who, ltx_dual_generate_args& a) {
    LTX_REQUIRE(args != nullptr, "%s: null arguments", who);
    const size_t sz = args->struct_size;
    LTX_REQUIRE(sz >= offsetof(ltx_dual_generate_args, noise_workspace) + sizeof(args->noise_workspace) && sz <= 4096,
                "ltx_dual_generate_args.struct_size = %zu: set it to sizeof(ltx_dual_generate_args) (LTX_DUAL_GENERATE_ARGS_INIT); this library is ABI revision %d",
                sz, LTX_ABI_VERSION);
    const ltx_dual_generate_args init = LTX_DUAL_GENERATE_ARGS_INIT;
    a = init;
    memcpy(&a, args, sz < sizeof(a) ? sz : sizeof(a));
    a.struct_size = (uint32_t)sizeof(a);
}
}  // namespace

int ltx_dual_noise_plan(const ltx_dual_generate_args* args, ltx_noise_draw* out, int cap, long* total_floats) {
    try {  // pure host code: no context, no device
        ltx_dual_generate_args a;
        dual_generate_params(args, "ltx_dual_noise_plan", a);
        LTX_REQUIRE(cap >= 0 && (out || cap == 0), "ltx_dual_noise_plan: cap=%d, or a null array", cap);
        const int n = dual_noise_plan(a, nullptr, 0, total_floats);
        if (n <= cap) dual_noise_plan(a, out, cap, total_floats);  // too small: the count alone, `out` stays as it was
        return n;
    } catch (const LtxError& e) {
        noctx_error() = e.msg;
        return -e.code;
    }
}

int ltx_dual_generate_dev(ltx_ctx* ctx, const ltx_dual_generate_args* args, ltx_progress_cb cb, void* user) {
    return with_ctx(ctx, [&] {
        need(ctx->dual_model, kNoDualModel);
        ltx_dual_generate_args a;
        dual_generate_params(args, "ltx_dual_generate_dev", a);
        dual_generate_run(ctx, a, cb, user);
    });
}

int ltx_dual_generate(ltx_ctx* ctx, const ltx_dual_generate_args* args, ltx_progress_cb cb, void* user) {
    return with_ctx(ctx, [&] {
        const DualModel* m = need(ctx->dual_model, kNoDualModel);
        ltx_dual_generate_args a;
        dual_generate_params(args, "ltx_dual_generate", a);
        dual_generate_check(ctx, a);  // on the host pointers: refuse before anything is staged
        long total = 0;
        dual_noise_plan(a, nullptr, 0, &total);
        const int nb = a.cfg_scale > 1.0f ? 2 : 1, up = a.two_stage ? 4 : 1;
        const size_t n_v1 = (size_t)a.channels * a.F * a.H * a.W * 4, n_out = n_v1 * up, n_a = (size_t)128 * a.T_a * 4;
        const size_t n_c1 = n_v1 / a.F, n_c2 = 4 * n_c1;
        const size_t n_ctx = (size_t)nb * a.S * m->cfg.caption_channels * 2, n_mask = (size_t)nb * a.S * 4;
        DevBuf &d_v = ctx->h2d[H2D_DENOISE_LATENT], &d_a = ctx->h2d[H2D_DUAL_AUDIO_LATENT], &d_cv = ctx->h2d[H2D_DENOISE_CONTEXT],
               &d_ca = ctx->h2d[H2D_DUAL_AUDIO_CONTEXT], &d_mask = ctx->h2d[H2D_DENOISE_MASK];
        DevBuf d_s1, d_c2;  // freed on return, after the synchronisation
        float *host_v = a.video_latent, *host_a = a.audio_latent, *host_s1 = a.two_stage ? a.stage1_out : nullptr, *host_ws = a.noise_workspace;
        d_v.ensure(n_out);
        d_a.ensure(n_a);
        stage_in(ctx, d_cv, a.video_context, n_ctx);
        if (a.audio_context) stage_in(ctx, d_ca, a.audio_context, n_ctx);
        if (a.mask) stage_in(ctx, d_mask, a.mask, n_mask);
        a.video_latent = d_v.as<float>(); a.audio_latent = d_a.as<float>();
        a.video_context = d_cv.as<uint16_t>();
        a.audio_context = a.audio_context ? d_ca.as<uint16_t>() : nullptr;
        a.mask = a.mask ? d_mask.as<int32_t>() : nullptr;
        a.noise_workspace = nullptr;  // the library's own
        a.stage1_out = nullptr;
        if (host_s1) {
            d_s1.ensure(n_v1);
            a.stage1_out = d_s1.as<float>();
        }
        if (a.cond_latent1) {
            stage_in(ctx, ctx->i2v_cond, a.cond_latent1, n_c1);
            a.cond_latent1 = ctx->i2v_cond.as<float>();
            if (a.two_stage) {
                stage_in(ctx, d_c2, a.cond_latent2, n_c2);
                a.cond_latent2 = d_c2.as<float>();
            }
        }
        dual_generate_run(ctx, a, cb, user);
        stage_out(ctx, host_v, d_v, n_out);
        stage_out(ctx, host_a, d_a, n_a);
        if (host_s1) stage_out(ctx, host_s1, d_s1, n_v1);
        if (host_ws && total > 0) stage_out(ctx, host_ws, ctx->dual_noise, (size_t)total * 4);
        stage_sync(ctx);
    });
}

}  // extern "C"
