// abi_internal.h - what the three extern "C" translation units share (abi_core.cpp: context, options, host math, key mapping,
// safetensors; abi_models.cpp: load / forward / decode / denoise / dist; abi_hooks.cpp: ltx_op_*, ltx_prof_*, fill and export test
// hooks). Every entry point converts C++ exceptions into an ltx_status + message; nothing here computes on the CPU on behalf of the
// GPU path.
#pragma once
#include <stddef.h>
#include <string.h>

#include <functional>
#include <string>

#include "../../include/ltxhip.h"
#include "dit.h"
#include "runtime.h"

// message of the last failed call that had no context (per thread; abi_core.cpp)
std::string& noctx_error();

template <class Fn>
int guarded(ltx_ctx* ctx, Fn&& fn) {
    try {
        if (ctx) HIP_CHECK(hipSetDevice(ctx->device));
        prof_set_current(ctx ? &ctx->prof : nullptr);
        fn();
        return LTX_OK;
    } catch (const LtxError& e) {
        (ctx ? ctx->last_error : noctx_error()) = e.msg;
        return e.code;
    } catch (const std::exception& e) {
        (ctx ? ctx->last_error : noctx_error()) = e.what();
        return LTX_ERR_GENERATION_FAILED;
    }
}

// The common case: a context is required and nothing else is checked outside the guard. Entry points that accept a null context or
// check more than the context keep the explicit form.
template <class Fn>
int with_ctx(ltx_ctx* ctx, Fn&& fn) {
    if (!ctx) return LTX_ERR_INVALID_CONFIGURATION;
    return guarded(ctx, fn);
}

inline int copy_str(const std::string& s, char* out, int cap) {
    if (!out || cap <= (int)s.size()) return -1;
    memcpy(out, s.c_str(), s.size() + 1);
    return 1;
}

inline TransformerConfig to_cfg(const ltx_transformer_config* c) {
    TransformerConfig t;
    if (!c) return t;
    t.num_layers = c->num_layers;
    t.num_heads = c->num_attention_heads;
    t.head_dim = c->attention_head_dim;
    t.in_channels = c->in_channels;
    t.out_channels = c->out_channels;
    t.cross_attention_dim = c->cross_attention_dim;
    t.caption_channels = c->caption_channels;
    t.rope_theta = c->rope_theta;
    for (int i = 0; i < 3; ++i) t.max_pos[i] = c->max_pos[i];
    t.timestep_scale_multiplier = c->timestep_scale_multiplier;
    t.norm_eps = c->norm_eps;
    return t;
}

// ---- model slots: the pointer members of ltx_ctx that hold a component (dit, vae, upscaler, connector, vae_encoder, audio_vae,
// vocoder, each attn_modules[i], dual, dual_model). A slot is either null or a fully built model; nothing else is ever published. ----

// Destroy and null. The caller has made the GPU idle (ltx_ctx_destroy, after its device-wide synchronise).
template <class M, class Destroy>
void drop_model(M** slot, Destroy destroy) {
    if (*slot) destroy(*slot);
    *slot = nullptr;
}

// Every *_unload: wait for the launches that may still read the model, then drop it.
template <class M, class Destroy>
void unload_model(ltx_ctx* ctx, M** slot, Destroy destroy) {
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    drop_model(slot, destroy);
}

// Every *_load and *_init_synthetic: unload the old model, build the new one in a local, fill it, and publish it only when the
// fill has succeeded. A throwing create or fill leaves the slot empty, so the next forward reports "not loaded".
template <class M, class Create, class Fill, class Destroy>
void replace_model(ltx_ctx* ctx, M** slot, Create create, Fill fill, Destroy destroy) {
    unload_model(ctx, slot, destroy);
    M* m = create();
    try {
        fill(m);
    } catch (...) {
        destroy(m);
        throw;
    }
    *slot = m;
}

template <class M>
M* need(M* model, const char* message) {
    if (!model) LTX_THROW(LTXS_MODEL_NOT_LOADED, "%s", message);
    return model;
}

// The body of every ltx_*_export_param: the element count, and the values when `out` is given. `find` names the model's parameter (null:
// no such parameter) and throws the model's not-loaded error itself; `export_slot` replaces param_export (the DiT's also de-quantises).
long export_param_body(ltx_ctx* ctx, const char* who, const char* name, float* out, long cap, const std::function<const ParamSlot*()>& find,
                       const std::function<void(const ParamSlot&, float*)>& export_slot = nullptr);

// the not-loaded texts; callers and the mirrors may match on them
constexpr const char* kNoDit = "Model component not loaded: transformer";
constexpr const char* kNoDitLora = "Model component not loaded: Transformer not loaded";  // ltx_dit_fuse_lora only
constexpr const char* kNoVae = "Model component not loaded: vaeDecoder";
constexpr const char* kNoUpscaler = "Model component not loaded: spatial upscaler";
constexpr const char* kNoConnector = "Model not loaded: text-embedding connector";
constexpr const char* kNoAudioConnector = "Model not loaded: audio embeddings connector (the file had no audio_embeddings_connector.* tensors)";
constexpr const char* kNoGemma = "Model not loaded: Gemma text encoder";
constexpr const char* kNoVaeEncoder = "Model not loaded: VAE encoder failed to load";
constexpr const char* kNoVaeStats = "Model not loaded: VAE decoder not loaded (needed for latent statistics)";
constexpr const char* kNoAudioVae = "Model not loaded: audio VAE not loaded";
constexpr const char* kNoVocoder = "Model not loaded: vocoder not loaded";
constexpr const char* kNoAttnModule = "Model not loaded: attention module not loaded at this index";
constexpr const char* kNoDualBlocks = "Model not loaded: dual transformer blocks not loaded";
constexpr const char* kNoDualModel = "Model not loaded: dual transformer model not loaded";

// ---- staging for host-pointer entry points: stage_in* / run the _dev body / stage_out* / stage_sync, all on the context's stream.
// The DevBuf is the caller's choice and decides what stays resident: a ctx->h2d slot (runtime.h, H2dSlot) is kept for the next call,
// a local DevBuf is freed on return. ----
inline void stage_in(ltx_ctx* ctx, DevBuf& buf, const void* host, size_t bytes) {
    buf.ensure(bytes);
    HIP_CHECK(hipMemcpyAsync(buf.p, host, bytes, hipMemcpyHostToDevice, ctx->stream));
}
inline void stage_out(ltx_ctx* ctx, void* host, DevBuf& buf, size_t bytes) {
    HIP_CHECK(hipMemcpyAsync(host, buf.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
}
inline void stage_sync(ltx_ctx* ctx) { HIP_CHECK(hipStreamSynchronize(ctx->stream)); }
