// runtime.h - context, device memory and safetensors plumbing shared by the DiT / VAE host graphs.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <map>
#include <string>
#include <vector>

#include "common.h"

// RAII device allocation that only grows (activation workspaces are sized on first use and then reused: no
// hipMalloc/hipFree inside a denoise step).
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    // returns true when (re)allocated
    bool ensure(size_t n, bool zero = false) {
        if (n <= bytes && p) return false;
        release();
        HIP_CHECK(hipMalloc(&p, n));
        bytes = n;
        if (zero) HIP_CHECK(hipMemset(p, 0, n));
        return true;
    }
    template <class T>
    T* as() const { return (T*)p; }
};

// One big allocation carved into 256-B aligned tensors (weights live here for the lifetime of a model).
struct DeviceArena {
    DevBuf buf;
    size_t used = 0;
    std::vector<size_t> pending;  // sizes requested before commit
    void reserve(size_t total) {
        buf.ensure(total);
        used = 0;
    }
    void* take(size_t n) {
        const size_t off = (used + 255) & ~(size_t)255;
        if (off + n > buf.bytes) LTX_THROW(LTXS_INSUFFICIENT_MEMORY, "arena overflow: need %zu, have %zu", off + n, buf.bytes);
        used = off + n;
        return (char*)buf.p + off;
    }
    static size_t padded(size_t n) { return (n + 255) & ~(size_t)255; }
};

// ---- safetensors (header JSON + mmap) ----
struct StTensor {
    std::string dtype;  // "BF16", "F32", "F16", "I32", ...
    std::vector<long> shape;
    size_t begin = 0, end = 0;  // byte offsets into the data section
    long numel() const {
        long n = 1;
        for (long s : shape) n *= s;
        return n;
    }
};
struct SafeTensors {
    std::map<std::string, StTensor> tensors;
    const uint8_t* data = nullptr;  // start of the data section inside the mapping
    void* map_base = nullptr;
    size_t map_len = 0;
    int fd = -1;
    SafeTensors() = default;
    SafeTensors(const SafeTensors&) = delete;
    ~SafeTensors() { close(); }
    void open(const std::string& path);  // throws LtxError (fileNotFound / weightLoadingFailed)
    void close();
    const uint8_t* ptr(const StTensor& t) const { return data + t.begin; }
};
// Convert `n` elements of a safetensors tensor to bf16 bits / f32 on the host.
void st_to_bf16(const SafeTensors& st, const StTensor& t, bf16_t* out);
void st_to_f32(const SafeTensors& st, const StTensor& t, float* out);

struct DiTModel;
struct VaeModel;
struct ConnectorModel;
struct VaeEncoderModel;
struct UpscalerModel;
struct AudioVaeModel;
struct VocoderModel;
struct AttnModule;
struct DualStack;
struct DualModel;
struct GemmaModel;
struct DistState;

// ---- live per-kernel timing (HIP events recorded on the launch stream around each launch of a kernel family) ----
// Used by bench.py for the roofline numbers: achieved = algorithmic work of the launches / their summed duration.
enum { PROF_GEMM = 0, PROF_ATTN = 1, PROF_CONV = 2, PROF_ELEM = 3, PROF_NKINDS = 4 };
struct ProfRec {
    hipEvent_t a = nullptr, b = nullptr;
    int kind = 0;
    double work = 0;  // algorithmic FLOPs (GEMM/attention/conv) or bytes (elementwise)
};
struct Profiler {
    bool on = false;
    std::vector<ProfRec> pool;
    size_t used = 0;
    double total_ms[PROF_NKINDS] = {0, 0, 0, 0};
    double total_work[PROF_NKINDS] = {0, 0, 0, 0};
    long launches[PROF_NKINDS] = {0, 0, 0, 0};
    ProfRec* begin(int kind, double work, hipStream_t s);
    void end(ProfRec* r, hipStream_t s);
    void collect();  // call after the stream is idle
    void reset();
    ~Profiler();
};
Profiler* prof_current();
void prof_set_current(Profiler* p);
struct ProfScope {
    ProfRec* r = nullptr;
    hipStream_t s;
    ProfScope(int kind, double work, hipStream_t stream) : s(stream) {
        Profiler* p = prof_current();
        if (p && p->on) r = p->begin(kind, work, stream);
    }
    ~ProfScope() {
        if (r) prof_current()->end(r, s);
    }
};

// Staging buffers of the host-pointer entry points (ltx_ctx::h2d). They grow on demand and stay resident. Every host-pointer entry
// point synchronises before it returns, so entry points may share a slot; none keeps data in one across calls (a context-cache hit
// in ltx_dit_forward reads the cached projection, not H2D_DIT_CONTEXT).
enum H2dSlot {
    // ltx_dit_forward and ltx_dit_forward_tokens
    H2D_DIT_LATENT = 0, H2D_DIT_CONTEXT = 1, H2D_DIT_TIMESTEPS = 2, H2D_DIT_MASK = 3, H2D_DIT_VELOCITY = 4,
    // ltx_denoise: slots of its own
    H2D_DENOISE_LATENT = 5, H2D_DENOISE_CONTEXT = 6, H2D_DENOISE_MASK = 7,
    // ltx_connector_encode: shares 0-3 with the DiT forwards
    H2D_CONN_HIDDEN = 0, H2D_CONN_MASK = 1, H2D_CONN_CONTEXT = 2, H2D_CONN_OUT_MASK = 3,
    // one input, one output: ltx_vae_encode, ltx_audio_vae_decode, ltx_vocoder_forward, ltx_audio_decode (share 0-1 with the above)
    H2D_IN = 0, H2D_OUT = 1,
    // ltx_dual_denoise: video latent / video context / mask in ltx_denoise's slots, the audio latent and context in 0-1
    H2D_DUAL_AUDIO_LATENT = 0, H2D_DUAL_AUDIO_CONTEXT = 1,
    // ltx_dual_two_stage: ltx_dual_denoise's slots, and the stage-2 noises and the output latent in 2-4
    H2D_DUAL2_VIDEO_NOISE = 2, H2D_DUAL2_AUDIO_NOISE = 3, H2D_DUAL2_VIDEO_OUT = 4,
    H2D_COUNT = 8
};

constexpr int kAttnModuleSlots = 4;  // attention modules a context holds: one dual block's worth

struct ltx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string last_error;
    DiTModel* dit = nullptr;
    VaeModel* vae = nullptr;
    UpscalerModel* upscaler = nullptr;
    ConnectorModel* connector = nullptr;
    VaeEncoderModel* vae_encoder = nullptr;
    DistState* dist = nullptr;  // multi-GPU state (dist.h); null = single GPU
    AudioVaeModel* audio_vae = nullptr;  // audio decode leg (audio.h)
    VocoderModel* vocoder = nullptr;
    AttnModule* attn_modules[kAttnModuleSlots] = {};  // head-dim-64 attention modules by index (attn_module.h)
    DualStack* dual = nullptr;  // dual video + audio transformer blocks (dual_block.h)
    DualModel* dual_model = nullptr;  // the dual model: its own blocks + embedders, caption projections and heads (dual_model.h)
    GemmaModel* gemma = nullptr;  // the Gemma-3 text encoder (gemma.h)
    DevBuf audio_mel, audio_op[2];  // the mel between the two audio models; haloed operands of the audio conv test hooks
    DevBuf h2d[H2D_COUNT];  // staging buffers of the host-pointer entry points, indexed by H2dSlot
    // load report of the last *_load call (mirrors the reference's "unmatched/missing" debug logs)
    int n_loaded = 0, n_missing = 0, n_unmatched = 0;
    Profiler prof;
    // denoise-loop scratch (device)
    DevBuf dn_tokens, dn_vel_tok, dn_vel, dn_vel2, dn_vel3, dn_prev, dn_ts, dn_stats, dn_lat2, dn_step_stats;
    DevBuf dn_rowmap;  // I2V token -> timestep-group map
    DevBuf dn_vel_slice;  // sequence-sharded loop: this rank's [T/N][C] velocity rows before the all-gather
    DevBuf i2v_cond, i2v_noise;  // staged image latent / re-noising draws of the host-pointer denoise entry
    DevBuf op_ws;  // split-K workspace of the kernel-level test hook
    DevBuf dual_dn;  // joint video + audio loop (dual_denoise.h): token-layout latents, velocities, tokens, timesteps, statistics
    DevBuf dual_noise;  // a generation's noise workspace when the caller gives none (dual_generate.h): the draws the loop does not take in place
    DevBuf dual_ts;  // two-stage joint path (dual_two_stage.h): the stage-1 latent in the caller's layout, the AdaIN statistics
};

// synthetic weights (bench / property tests): counter-based normal fill on device
void launch_fill_normal_bf16(bf16_t* p, long n, uint64_t seed, float mean, float stddev, hipStream_t stream);
void launch_fill_normal_f32(float* p, long n, uint64_t seed, float mean, float stddev, int round_bf16, hipStream_t stream);
void launch_fill_const_f32(float* p, long n, float v, hipStream_t stream);
