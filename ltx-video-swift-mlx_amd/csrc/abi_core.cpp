// abi_core.cpp - extern "C" surface of libltxhip.so (include/ltxhip.h), part 1 of 3: the context and its options, and everything that
// runs on the host alone - generation-config checks, sigma / RoPE / tile tables, file-key mapping, safetensors reads, noise and
// frame / audio export. The model entry points are in abi_models.cpp, the test hooks in abi_hooks.cpp.
#include <vector>

#include "abi_internal.h"
#include "attn_module.h"
#include "dual_block.h"
#include "dual_model.h"
#include "audio.h"
#include "connector.h"
#include "gemma.h"
#include "dist.h"
#include "hostmath.h"
#include "options.h"
#include "pipeline.h"
#include "upscaler.h"
#include "vae.h"
#include "vae_encoder.h"

std::string& noctx_error() {
    thread_local std::string e;
    return e;
}

long export_param_body(ltx_ctx* ctx, const char* who, const char* name, float* out, long cap, const std::function<const ParamSlot*()>& find,
                       const std::function<void(const ParamSlot&, float*)>& export_slot) {
    if (!ctx || !name) return -LTX_ERR_INVALID_CONFIGURATION;
    long n = 0;
    const int rc = guarded(ctx, [&] {
        const ParamSlot* s = find();
        LTX_REQUIRE(s != nullptr, "%s: no parameter '%s'", who, name);
        n = s->numel;
        if (!out) return;
        LTX_REQUIRE(cap >= n, "%s: buffer too small (%ld < %ld)", who, cap, n);
        if (export_slot)
            export_slot(*s, out);
        else
            param_export(ctx, *s, out);
    });
    return rc == 0 ? n : -rc;
}

extern "C" {

const char* ltx_version(void) { return "0.1.0"; }
int ltx_abi_version(void) { return LTX_ABI_VERSION; }

int ltx_ctx_set_option(ltx_ctx* ctx, const char* key, int value) {
    return guarded(ctx, [&] {
        const int i = ltx_opt_find(key);
        LTX_REQUIRE(i >= 0, "ltx_ctx_set_option: unknown option '%s' (ltx_option_info enumerates them)", key ? key : "(null)");
        const LtxOptInfo& o = ltx_opt_info(i);
        LTX_REQUIRE(ltx_opt_set(i, value), "ltx_ctx_set_option: %s = %d outside [%d, %d]", o.name, value, o.lo, o.hi);
    });
}
int ltx_ctx_get_option(const ltx_ctx* ctx, const char* key, int* value) {
    return guarded(const_cast<ltx_ctx*>(ctx), [&] {
        const int i = ltx_opt_find(key);
        LTX_REQUIRE(i >= 0 && value, "ltx_ctx_get_option: unknown option '%s'", key ? key : "(null)");
        *value = ltx_opt((LtxOpt)i);
    });
}
int ltx_option_info(int index, const char** name, int* def, int* lo, int* hi, int* numerics, const char** doc) {
    if (index >= 0 && index < OPT_COUNT) {
        const LtxOptInfo& o = ltx_opt_info(index);
        if (name) *name = o.name;
        if (def) *def = o.def;
        if (lo) *lo = o.lo;
        if (hi) *hi = o.hi;
        if (numerics) *numerics = o.numerics;
        if (doc) *doc = o.doc;
    }
    return OPT_COUNT;
}

const char* ltx_build_info(void) {
#ifdef LTX_EXPERIMENTS
    return "gfx950;experiments=1";
#else
    return "gfx950;experiments=0";
#endif
}

void ltx_transformer_config_default(ltx_transformer_config* c) {
    if (!c) return;
    TransformerConfig t;
    c->num_layers = t.num_layers;
    c->num_attention_heads = t.num_heads;
    c->attention_head_dim = t.head_dim;
    c->in_channels = t.in_channels;
    c->out_channels = t.out_channels;
    c->cross_attention_dim = t.cross_attention_dim;
    c->caption_channels = t.caption_channels;
    c->rope_theta = t.rope_theta;
    for (int i = 0; i < 3; ++i) c->max_pos[i] = t.max_pos[i];
    c->timestep_scale_multiplier = t.timestep_scale_multiplier;
    c->norm_eps = t.norm_eps;
}

void ltx_connector_config_default(ltx_connector_config* cfg) {
    if (!cfg) return;
    const ConnectorConfig k;
    cfg->dim = k.dim; cfg->heads = k.heads; cfg->layers = k.layers; cfg->registers = k.registers; cfg->states = k.states;
    cfg->theta = k.theta; cfg->max_pos = k.max_pos;
}

void ltx_gemma_config_default(ltx_gemma_config* cfg) {
    if (!cfg) return;
    const GemmaConfig k;
    cfg->hidden_size = k.hidden; cfg->num_hidden_layers = k.layers; cfg->intermediate_size = k.intermediate;
    cfg->num_attention_heads = k.heads; cfg->head_dim = k.head_dim; cfg->num_key_value_heads = k.kv_heads; cfg->vocab_size = k.vocab;
    cfg->rms_norm_eps = k.rms_eps; cfg->rope_theta = k.rope_theta; cfg->rope_local_base_freq = k.rope_local_base;
    cfg->query_pre_attn_scalar = k.query_pre_attn_scalar; cfg->sliding_window = k.sliding_window;
    cfg->sliding_window_pattern = k.sliding_window_pattern;
}

int ltx_ctx_create(int device, ltx_ctx** out) {
    if (!out) return LTX_ERR_INVALID_CONFIGURATION;
    *out = nullptr;
    ltx_ctx* ctx = nullptr;
    const int rc = guarded(nullptr, [&] {
        int n = 0;
        HIP_CHECK(hipGetDeviceCount(&n));
        if (device < 0 || device >= n) LTX_THROW(LTXS_HIP_ERROR, "no HIP device %d (found %d)", device, n);
        HIP_CHECK(hipSetDevice(device));
        hipDeviceProp_t prop;
        HIP_CHECK(hipGetDeviceProperties(&prop, device));
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            LTX_THROW(LTXS_HIP_ERROR, "libltxhip is built for gfx950 (MI355X) only; device %d is %s", device, prop.gcnArchName);
        ctx = new ltx_ctx();
        ctx->device = device;
        HIP_CHECK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
        ctx->own_stream = true;
    });
    if (rc != LTX_OK) {
        delete ctx;
        return rc;
    }
    *out = ctx;
    return LTX_OK;
}

void ltx_ctx_destroy(ltx_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    try { dist_shutdown(ctx); } catch (...) {}
    drop_model(&ctx->dit, dit_destroy);
    drop_model(&ctx->vae, vae_destroy);
    drop_model(&ctx->upscaler, upscaler_destroy);
    drop_model(&ctx->connector, connector_destroy);
    drop_model(&ctx->vae_encoder, vae_encoder_destroy);
    drop_model(&ctx->audio_vae, audio_vae_destroy);
    drop_model(&ctx->vocoder, vocoder_destroy);
    for (AttnModule*& m : ctx->attn_modules) drop_model(&m, attn_module_destroy);
    drop_model(&ctx->dual, dual_destroy);
    drop_model(&ctx->dual_model, dual_model_destroy);
    drop_model(&ctx->gemma, gemma_destroy);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char* ltx_last_error(const ltx_ctx* ctx) { return ctx ? ctx->last_error.c_str() : noctx_error().c_str(); }

int ltx_ctx_set_stream(ltx_ctx* ctx, void* hip_stream) {
    return with_ctx(ctx, [&] {
        if (ctx->stream) HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (ctx->own_stream && ctx->stream) HIP_CHECK(hipStreamDestroy(ctx->stream));
        // the handle is used as given: NULL is the (legacy) default stream, which is what torch's default stream is
        ctx->stream = (hipStream_t)hip_stream;
        ctx->own_stream = false;
    });
}

int ltx_ctx_synchronize(ltx_ctx* ctx) {
    return with_ctx(ctx, [&] { HIP_CHECK(hipStreamSynchronize(ctx->stream)); });
}

int ltx_load_report(const ltx_ctx* ctx, int* n_loaded, int* n_missing, int* n_unmatched) {
    if (!ctx) return LTX_ERR_INVALID_CONFIGURATION;
    if (n_loaded) *n_loaded = ctx->n_loaded;
    if (n_missing) *n_missing = ctx->n_missing;
    if (n_unmatched) *n_unmatched = ctx->n_unmatched;
    return LTX_OK;
}

// ---- pure host ----
int ltx_validate_generation_config(int width, int height, int num_frames, int num_steps, float cfg_scale,
                                   int two_stage, char* msg, int msg_cap) {
    std::string m;
    const int rc = validate_generation_config(width, height, num_frames, num_steps, cfg_scale, two_stage, &m);
    if (msg && msg_cap > 0) {
        strncpy(msg, m.c_str(), msg_cap - 1);
        msg[msg_cap - 1] = 0;
    }
    return rc;
}

int ltx_latent_shape(int width, int height, int num_frames, int* F, int* H, int* W) {
    if (!F || !H || !W) return LTX_ERR_INVALID_CONFIGURATION;
    latent_shape(width, height, num_frames, F, H, W);
    return LTX_OK;
}

int ltx_sigmas(int distilled, int num_steps, int token_count, float* out, int cap) {
    if (!out || (!distilled && num_steps < 1)) return -LTX_ERR_INVALID_CONFIGURATION;
    const std::vector<float> s = compute_sigmas(distilled != 0, num_steps, token_count);
    for (int i = 0; i < (int)s.size() && i < cap; ++i) out[i] = s[i];
    return (int)s.size();
}

int ltx_stage2_sigmas(float* out, int cap) {
    for (int i = 0; i < 4 && i < cap; ++i) out[i] = kStage2DistilledSigmas[i];
    return 4;
}

int ltx_rope_tables(const ltx_transformer_config* cfg, int F, int H, int W, float* cos_out, float* sin_out) {
    if (!cos_out || !sin_out || F < 1 || H < 1 || W < 1) return LTX_ERR_INVALID_CONFIGURATION;
    const TransformerConfig t = to_cfg(cfg);
    std::vector<float> c, s;
    rope_tables(t, F, H, W, 24.0f, &c, &s);
    memcpy(cos_out, c.data(), c.size() * 4);
    memcpy(sin_out, s.data(), s.size() * 4);
    return LTX_OK;
}

int ltx_rope_tables_1d(int T, int dim, float theta, int max_pos, float* cos_out, float* sin_out) {
    if (!cos_out || !sin_out || T < 1 || dim < 2 || max_pos < 1) return LTX_ERR_INVALID_CONFIGURATION;
    std::vector<float> c, s;
    rope_tables_1d(T, dim, (double)theta, max_pos, &c, &s);
    memcpy(cos_out, c.data(), c.size() * 4);
    memcpy(sin_out, s.data(), s.size() * 4);
    return LTX_OK;
}

int ltx_audio_positions(int T_a, float* out) {
    if (!out || T_a < 1) return LTX_ERR_INVALID_CONFIGURATION;
    const std::vector<float> p = audio_positions(T_a);
    memcpy(out, p.data(), p.size() * 4);
    return LTX_OK;
}

int ltx_video_temporal_positions(int F, int H, int W, float fps, float* out) {
    if (!out || F < 1 || H < 1 || W < 1 || !(fps > 0.f)) return LTX_ERR_INVALID_CONFIGURATION;
    const std::vector<float> p = video_temporal_positions(F, H, W, fps);
    memcpy(out, p.data(), p.size() * 4);
    return LTX_OK;
}

int ltx_rope_tables_positions(const float* positions, int T, int dim, float theta, int max_pos, float* cos_out, float* sin_out) {
    if (!positions || !cos_out || !sin_out || T < 1 || dim < 2 || dim % 2 != 0 || max_pos < 1 || !(theta > 1.f)) return LTX_ERR_INVALID_CONFIGURATION;
    std::vector<float> c, s;
    rope_tables_positions(positions, T, dim, (double)theta, max_pos, &c, &s);
    memcpy(cos_out, c.data(), c.size() * 4);
    memcpy(sin_out, s.data(), s.size() * 4);
    return LTX_OK;
}

int ltx_vae_tile_plan(int latent_frames, int tile, int overlap, int* starts, int* ends, int cap, int* out_frames) {
    if (latent_frames < 1) return -LTX_ERR_INVALID_CONFIGURATION;
    const TilePlan p = vae_tile_plan(latent_frames, tile, overlap);
    if (p.start.empty()) return -LTX_ERR_INVALID_CONFIGURATION;
    for (int i = 0; i < (int)p.start.size() && i < cap; ++i) {
        if (starts) starts[i] = p.start[i];
        if (ends) ends[i] = p.end[i];
    }
    if (out_frames) *out_frames = p.out_frames;
    return (int)p.start.size();
}

int ltx_vae_encoder_latent_frames(int T) { return T < 1 ? 0 : vae_encoder_latent_frames(T); }

int ltx_audio_latent_frames(int video_frames, float fps) { return video_frames < 1 || !(fps > 0) ? 0 : audio_latent_frames(video_frames, fps); }
int ltx_audio_mel_frames(int T) { return T < 1 ? 0 : audio_mel_frames(T); }
long ltx_audio_sample_count(int T) { return T < 1 ? 0 : 240L * audio_mel_frames(T); }
int ltx_audio_sample_rate(void) { return 24000; }

// ---- file key -> module key ----
int ltx_map_transformer_key(const char* file_key, char* out, int cap) {
    std::string mk;
    if (!file_key || !map_transformer_file_key(file_key, &mk)) return 0;
    return copy_str(mk, out, cap);
}
int ltx_map_vae_key(const char* file_key, char* out, int cap) {
    std::string mk;
    if (!file_key || !map_vae_file_key(file_key, &mk)) return 0;
    return copy_str(mk, out, cap);
}
int ltx_map_lora_key(const char* lora_key, char* out, int cap) {
    std::string mk;
    if (!lora_key || !map_lora_key(lora_key, &mk)) return 0;
    return copy_str(mk, out, cap);
}
int ltx_map_text_encoder_key(const char* file_key, char* out, int cap) {
    std::string mk;
    if (!file_key || !map_text_encoder_file_key(file_key, &mk)) return 0;
    return copy_str(mk, out, cap);
}
int ltx_map_vae_encoder_key(const char* file_key, char* out, int cap) {
    std::string mk;
    if (!file_key || !map_vae_encoder_file_key(file_key, &mk)) return 0;
    return copy_str(mk, out, cap);
}

// ---- safetensors ----
int ltx_st_info(const char* path, const char* key, long* shape8) {
    if (!path || !key) return -LTX_ERR_INVALID_CONFIGURATION;
    int nd = -1;
    const int rc = guarded(nullptr, [&] {
        SafeTensors st;
        st.open(path);
        auto it = st.tensors.find(key);
        if (it == st.tensors.end()) LTX_THROW(LTXS_WEIGHT_LOADING_FAILED, "Failed to load weights: no tensor '%s' in %s", key, path);
        nd = (int)it->second.shape.size();
        for (int i = 0; i < nd && i < 8; ++i)
            if (shape8) shape8[i] = it->second.shape[i];
    });
    return rc == 0 ? nd : -rc;
}

long ltx_st_read(const char* path, const char* key, int dtype, void* out, long cap) {
    if (!path || !key || !out) return -LTX_ERR_INVALID_CONFIGURATION;
    long n = -1;
    const int rc = guarded(nullptr, [&] {
        SafeTensors st;
        st.open(path);
        auto it = st.tensors.find(key);
        if (it == st.tensors.end()) LTX_THROW(LTXS_WEIGHT_LOADING_FAILED, "Failed to load weights: no tensor '%s' in %s", key, path);
        const StTensor& t = it->second;
        n = t.numel();
        LTX_REQUIRE(n <= cap, "ltx_st_read: buffer too small (%ld < %ld)", cap, n);
        if (dtype == 1) {
            st_to_bf16(st, t, (bf16_t*)out);
        } else if (dtype == 0) {
            st_to_f32(st, t, (float*)out);
        } else {
            if (t.dtype == "I32") {
                memcpy(out, st.ptr(t), (size_t)n * 4);
            } else if (t.dtype == "I64") {
                const int64_t* s64 = (const int64_t*)st.ptr(t);
                for (long i = 0; i < n; ++i) ((int32_t*)out)[i] = (int32_t)s64[i];
            } else {
                std::vector<float> f(n);
                st_to_f32(st, t, f.data());
                for (long i = 0; i < n; ++i) ((int32_t*)out)[i] = (int32_t)f[i];
            }
        }
    });
    return rc == 0 ? n : -rc;
}

/* ---- MLX-compatible noise ---- */
int ltx_mlx_random_normal(uint64_t seed, int draw_index, float* out, long n) {
    if (!out || n < 0 || draw_index < 0) return LTX_ERR_INVALID_CONFIGURATION;
    mlx_random_normal(seed, draw_index, n, out);
    return LTX_OK;
}

int ltx_mlx_draw_key(uint64_t seed, int draw_index, uint32_t key_out[2]) {
    if (!key_out || draw_index < 0) return LTX_ERR_INVALID_CONFIGURATION;
    mlx_draw_key(seed, draw_index, key_out);
    return LTX_OK;
}

void ltx_threefry2x32(const uint32_t key[2], const uint32_t ctr[2], uint32_t out[2]) { threefry2x32(key, ctr, out); }

/* ---- frame and audio export ---- */
int ltx_frames_to_u8(const float* frames, long n, uint8_t* out) {
    if (!frames || !out || n < 0) return LTX_ERR_INVALID_CONFIGURATION;
    frames_to_u8(frames, n, out);
    return LTX_OK;
}

int ltx_write_png(const char* path, const uint8_t* rgb, int width, int height) {
    return write_png_rgb8(path, rgb, width, height) ? LTX_OK : LTX_ERR_FILE_NOT_FOUND;
}

int ltx_write_wav(const char* path, const float* waveform, long n, int sample_rate, float gain) {
    if (!path || !waveform || n < 0 || sample_rate < 1 || n > (1L << 28)) return LTX_ERR_INVALID_CONFIGURATION;
    return write_wav_pcm16(path, waveform, n, sample_rate, gain) ? LTX_OK : LTX_ERR_FILE_NOT_FOUND;
}

}  // extern "C"
