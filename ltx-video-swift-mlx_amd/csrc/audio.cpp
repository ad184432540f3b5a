// audio.cpp - host graphs of the audio decode leg: the audio VAE decoder (reference Models/AudioVAE/AudioVAE.swift:249-456) and the
// HiFi-GAN vocoder (Vocoder.swift:132-266), their safetensors loaders and the pure-host helpers (frame counts, WAV export).
// Every convolution runs through launch_audio_conv (audio_conv.hip); see audio.h for the precision contract.
#include "audio.h"

#include <math.h>
#include <stdio.h>
#include <string.h>

#include <set>

namespace {

// ---- deterministic host normal draws for the synthetic models (splitmix64 + Box-Muller) ----
struct HostRng {
    uint64_t s;
    explicit HostRng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 0x1234567ull) {}
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    double uni() { return ((double)(next() >> 11) + 0.5) * (1.0 / 9007199254740992.0); }
    float normal() { return (float)(sqrt(-2.0 * log(uni())) * cos(6.283185307179586 * uni())); }
};

AHostTensor make_normal(HostRng& rng, std::vector<long> shape, float stdv) {
    AHostTensor t;
    t.shape = shape;
    long n = 1;
    for (long s : shape) n *= s;
    t.v.resize((size_t)n);
    for (auto& x : t.v) x = rng.normal() * stdv;
    return t;
}

// ---- assembling a model from host tensors ----
struct Pending {
    void** dst;
    std::vector<uint8_t> bytes;
};
struct Assembler {
    const AHostWeights& hw;
    std::set<std::string> used;
    std::vector<Pending> pend;
    int loaded = 0, missing = 0;
    std::string first_missing;
    explicit Assembler(const AHostWeights& h) : hw(h) {}

    const AHostTensor* get(const std::string& key, int rank) {
        auto it = hw.find(key);
        if (it == hw.end() || (int)it->second.shape.size() != rank) {  // a wrong-rank tensor is no parameter: it stays unmatched
            ++missing;
            if (first_missing.empty()) first_missing = key;
            return nullptr;
        }
        used.insert(key);
        ++loaded;
        return &it->second;
    }
    bool has(const std::string& key) const { return hw.count(key) != 0; }
    void push_bf16(bf16_t** dst, const std::vector<float>& v) {
        Pending p;
        p.dst = (void**)dst;
        p.bytes.resize(v.size() * 2);
        bf16_t* o = (bf16_t*)p.bytes.data();
        for (size_t i = 0; i < v.size(); ++i) o[i] = host_f32_to_bf16(v[i]);
        pend.push_back(std::move(p));
    }
    void push_f32(float** dst, const std::vector<float>& v) {
        Pending p;
        p.dst = (void**)dst;
        p.bytes.resize(v.size() * 4);
        memcpy(p.bytes.data(), v.data(), v.size() * 4);
        pend.push_back(std::move(p));
    }
    void bias(const std::string& key, int cout, float** dst) {
        const AHostTensor* b = get(key, 1);
        std::vector<float> v((size_t)cout, 0.f);
        if (b) {
            LTX_REQUIRE((int)b->shape[0] == cout, "%s: %ld values for %d output channels", key.c_str(), b->shape[0], cout);
            v = b->v;
        }
        push_f32(dst, v);
    }
    // PyTorch conv weight (out, in, taps...) -> [out][tap][in_pad]; returns false when the weight is absent
    bool conv(const std::string& prefix, int rank, AConvW* c, int expect_cin) {
        const AHostTensor* w = get(prefix + ".weight", rank);
        if (!w) return false;
        const int cout = (int)w->shape[0], cin = (int)w->shape[1];
        int taps = 1;
        for (int d = 2; d < rank; ++d) taps *= (int)w->shape[d];
        if (rank == 4) LTX_REQUIRE(w->shape[2] == w->shape[3] && (w->shape[2] == 1 || w->shape[2] == 3), "%s: %ldx%ld kernel (1x1 or 3x3)",
                                   prefix.c_str(), w->shape[2], w->shape[3]);
        LTX_REQUIRE(expect_cin < 0 || cin == expect_cin, "%s: %d input channels, the graph carries %d", prefix.c_str(), cin, expect_cin);
        LTX_REQUIRE(taps <= ACONV_MAX_TAPS && (rank == 4 || taps % 2 == 1), "%s: %d taps", prefix.c_str(), taps);
        const int cin_pad = (cin + 31) / 32 * 32;
        std::vector<float> r((size_t)cout * taps * cin_pad, 0.f);
        for (int o = 0; o < cout; ++o)
            for (int i = 0; i < cin; ++i)
                for (int t = 0; t < taps; ++t) r[((size_t)o * taps + t) * cin_pad + i] = w->v[((size_t)o * cin + i) * taps + t];
        c->cout = cout;
        c->cin = cin;
        c->cin_pad = cin_pad;
        c->k = rank == 4 ? (int)w->shape[2] : taps;
        push_bf16(&c->w, r);
        bias(prefix + ".bias", cout, &c->b);
        return true;
    }
    void commit(ltx_ctx* ctx, DeviceArena& arena, int n_filtered_keys) {
        size_t total = 256;
        for (auto& p : pend) total += DeviceArena::padded(p.bytes.size());
        arena.reserve(total);
        for (auto& p : pend) {
            void* d = arena.take(p.bytes.size());
            HIP_CHECK(hipMemcpy(d, p.bytes.data(), p.bytes.size(), hipMemcpyHostToDevice));
            *p.dst = d;
        }
        ctx->n_loaded = loaded;
        ctx->n_missing = missing;
        ctx->n_unmatched = n_filtered_keys - (int)used.size();
    }
    void fail_if_missing_weights(ltx_ctx* ctx, int n_filtered_keys, const char* what) {
        ctx->n_loaded = loaded;
        ctx->n_missing = missing;
        ctx->n_unmatched = n_filtered_keys - (int)used.size();
        LTX_THROW(LTXS_WEIGHT_LOADING_FAILED, "Failed to load weights: %s has no usable tensor '%s'", what, first_missing.c_str());
    }
};

AHostWeights read_file(const std::string& path, bool (*keep)(const std::string&)) {
    SafeTensors st;
    st.open(path);
    AHostWeights hw;
    for (auto& kv : st.tensors) {
        if (!keep(kv.first)) continue;
        AHostTensor t;
        t.shape = kv.second.shape;
        t.v.resize((size_t)kv.second.numel());
        st_to_f32(st, kv.second, t.v.data());
        hw[kv.first] = std::move(t);
    }
    return hw;
}
// loadAudioVAEWeights' filter (ModelDownloader.swift:1116-1130): decoder.* and the two latent statistics; the encoder is dropped
bool keep_audio_vae(const std::string& k) { return k.rfind("decoder.", 0) == 0 || k == "latents_mean" || k == "latents_std"; }
bool keep_all(const std::string&) { return true; }

// ---- per-model activation workspace: named device buffers that live as long as T does not change ----
struct Workspace {
    std::map<std::string, DevBuf>* bufs;
    hipStream_t stream;
    // zero = true: a haloed operand; it is zeroed ONCE when created and only its interior is ever written afterwards
    void* get(const std::string& name, size_t bytes, bool zero) {
        DevBuf& b = (*bufs)[name];
        if (b.ensure(bytes) && zero) HIP_CHECK(hipMemsetAsync(b.p, 0, b.bytes, stream));
        return b.p;
    }
};
std::string key3(const char* what, int a, int b) {
    char s[64];
    snprintf(s, sizeof(s), "%s.%d.%d", what, a, b);
    return s;
}

}  // namespace

std::vector<int> convt_phase_taps(int k, int s, int p, int r, std::vector<int>* offs) {
    std::vector<int> js;
    offs->clear();
    for (int j = 0; j < k; ++j) {
        const int d = r + p - j;
        if (d % s != 0) continue;
        js.push_back(j);
        offs->push_back(d / s);
    }
    return js;
}

std::vector<float> convt_phase_slab(const float* w, int cin, int cout, int k, const std::vector<int>& js, int cin_pad) {
    const size_t nt = js.size();
    std::vector<float> slab((size_t)cout * nt * cin_pad, 0.f);
    for (int o = 0; o < cout; ++o)
        for (size_t t = 0; t < nt; ++t)
            for (int c = 0; c < cin; ++c) slab[((size_t)o * nt + t) * cin_pad + c] = w[((size_t)c * cout + o) * k + js[t]];
    return slab;
}

// ================================================================================================================
// Audio VAE decoder
// ================================================================================================================
AudioVaeModel* audio_vae_create() { return new AudioVaeModel(); }
void audio_vae_destroy(AudioVaeModel* m) {
    delete m;
}

static void audio_vae_assemble(ltx_ctx* ctx, AudioVaeModel* m, const AHostWeights& hw) {
    Assembler as(hw);
    const int nkeys = (int)hw.size();
    bool ok = as.conv("decoder.conv_in.conv", 4, &m->conv_in, -1);
    int ch = m->conv_in.cout;
    m->latent_ch = m->conv_in.cin;
    for (int b = 0; b < 2 && ok; ++b) {
        const std::string p = "decoder.mid.block_" + std::to_string(b + 1);
        ok = ok && as.conv(p + ".conv1.conv", 4, &m->mid[b].c1, ch) && as.conv(p + ".conv2.conv", 4, &m->mid[b].c2, ch);
    }
    for (int l = 2; l >= 0 && ok; --l) {
        for (int b = 0; b < 3 && ok; ++b) {
            const std::string p = "decoder.up." + std::to_string(l) + ".block." + std::to_string(b);
            AudioVaeModel::Res& r = m->up[l][b];
            ok = ok && as.conv(p + ".conv1.conv", 4, &r.c1, ch);
            const int co = r.c1.cout;
            ok = ok && as.conv(p + ".conv2.conv", 4, &r.c2, co);
            r.has_sc = as.has(p + ".nin_shortcut.conv.weight");
            if (r.has_sc) ok = ok && as.conv(p + ".nin_shortcut.conv", 4, &r.sc, ch);
            if (ok) LTX_REQUIRE(r.c2.cout == co && (r.has_sc ? r.sc.cout == co && r.sc.k == 1 : co == ch),
                                "%s: channel counts %d -> %d do not chain", p.c_str(), ch, co);
            ch = co;
        }
        if (l > 0) ok = ok && as.conv("decoder.up." + std::to_string(l) + ".upsample.conv.conv", 4, &m->ups[l], ch);
    }
    ok = ok && as.conv("decoder.conv_out.conv", 4, &m->conv_out, ch);
    if (!ok) as.fail_if_missing_weights(ctx, nkeys, "the audio VAE decoder");
    m->base = ch;
    m->out_ch = m->conv_out.cout;
    LTX_REQUIRE(m->out_ch == 2 && ch % 32 == 0 && m->conv_in.cout % 32 == 0 && m->conv_in.cout <= 1024,
                "audio VAE: %d -> %d channels, %d outputs (channel counts must be multiples of 32, stereo out)", m->conv_in.cout, ch, m->out_ch);
    const int nstat = m->latent_ch * 16;
    for (int which = 0; which < 2; ++which) {
        const char* key = which ? "latents_std" : "latents_mean";
        const AHostTensor* t = as.get(key, 1);
        std::vector<float> v((size_t)nstat, which ? 1.f : 0.f);  // the reference's initial values (AudioVAE.swift:399-400)
        if (t) {
            LTX_REQUIRE((int)t->shape[0] == nstat, "%s: %ld values, expected %d", key, t->shape[0], nstat);
            v = t->v;
        }
        as.push_f32(which ? &m->stdv : &m->mean, v);
    }
    as.commit(ctx, m->arena, nkeys);
}

void audio_vae_load(ltx_ctx* ctx, AudioVaeModel* m, const std::string& path) {
    audio_vae_assemble(ctx, m, read_file(path, keep_audio_vae));
}

void audio_vae_init_synthetic(ltx_ctx* ctx, AudioVaeModel* m, int base, uint64_t seed) {
    LTX_REQUIRE(base >= 32 && base % 32 == 0 && base <= 256, "audio VAE: base %d (32..256, multiple of 32)", base);
    HostRng rng(seed);
    AHostWeights hw;
    auto conv = [&](const std::string& p, int co, int ci, int k, float gain) {
        hw[p + ".weight"] = make_normal(rng, {co, ci, k, k}, gain / sqrtf((float)ci * k * k));
        hw[p + ".bias"] = make_normal(rng, {co}, 0.02f);
    };
    const int top = base * 4;
    conv("decoder.conv_in.conv", top, 8, 3, 1.f);
    auto res = [&](const std::string& p, int ci, int co) {
        conv(p + ".conv1.conv", co, ci, 3, 1.4f);
        conv(p + ".conv2.conv", co, co, 3, 0.7f);
        if (ci != co) conv(p + ".nin_shortcut.conv", co, ci, 1, 1.f);
    };
    res("decoder.mid.block_1", top, top);
    res("decoder.mid.block_2", top, top);
    int ch = top;
    const int mult[3] = {1, 2, 4};
    for (int l = 2; l >= 0; --l) {
        const int co = base * mult[l];
        for (int b = 0; b < 3; ++b) {
            res("decoder.up." + std::to_string(l) + ".block." + std::to_string(b), ch, co);
            ch = co;
        }
        if (l > 0) conv("decoder.up." + std::to_string(l) + ".upsample.conv.conv", ch, ch, 3, 1.f);
    }
    conv("decoder.conv_out.conv", 2, ch, 3, 1.f);
    hw["latents_mean"] = make_normal(rng, {128}, 0.1f);
    AHostTensor sd = make_normal(rng, {128}, 0.1f);
    for (auto& x : sd.v) x = 1.0f + fabsf(x);
    hw["latents_std"] = sd;
    audio_vae_assemble(ctx, m, hw);
}

void audio_vae_decode(ltx_ctx* ctx, AudioVaeModel* m, const float* latent, int T, float* mel) {
    LTX_REQUIRE(latent && mel && T >= 1 && T <= 4096, "audio VAE decode: T=%d (1..4096)", T);
    LTX_REQUIRE(m->conv_in.w, "audio VAE decode: model not assembled");
    hipStream_t st = ctx->stream;
    if (m->ws_T != T) {  // other geometry: the halos of the old buffers are in the wrong places
        HIP_CHECK(hipStreamSynchronize(st));
        m->ws.clear();
        m->ws_T = T;
    }
    Workspace ws{&m->ws, st};
    const int Wl = 16;
    int H[3], W[3];  // by resolution step: 0 = latent grid
    H[0] = T, W[0] = Wl;
    for (int s = 1; s < 3; ++s) H[s] = 2 * H[s - 1] - 1, W[s] = 2 * W[s - 1];
    const int cmax = m->conv_in.cout;
    size_t f32_elems = 0;
    {
        // the stream is widest either at the latent grid (top channels) or later; channels halve no faster than the grid quadruples
        int ch = cmax;
        f32_elems = (size_t)H[0] * W[0] * ch;
        f32_elems = std::max(f32_elems, (size_t)H[1] * W[1] * m->up[2][2].c2.cout);
        f32_elems = std::max(f32_elems, (size_t)H[2] * W[2] * m->up[1][2].c2.cout);
    }
    float* xa = (float*)ws.get("xa", f32_elems * 4, false);
    float* xb = (float*)ws.get("xb", f32_elems * 4, false);
    float* t1 = (float*)ws.get("t1", f32_elems * 4, false);
    auto pad = [&](const char* slot, int step, int C) {
        return (bf16_t*)ws.get(key3(slot, step, C), (size_t)(H[step] + 3) * (W[step] + 2) * C * 2, true);
    };
    // one causal conv on step `s`: operand = padded buffer, f32 output dense [H][W][Cout] (or transposed [Cout][H*W])
    auto conv2d = [&](const AConvW& c, int s, const bf16_t* in, const float* resid, float* out, bool transposed) {
        AConvArgs a;
        const int wp = W[s] + 2;
        a.x = in;
        a.ldx = c.cin_pad;
        a.w = c.w;
        a.bias = c.b;
        a.P = H[s] * wp;
        a.Cin = c.cin_pad;
        a.Cout = c.cout;
        if (c.k == 3) {
            a.ntaps = 9;
            for (int kh = 0; kh < 3; ++kh)
                for (int kw = 0; kw < 3; ++kw) a.off[kh * 3 + kw] = kh * wp + kw;
        } else {
            a.ntaps = 1;
            a.off[0] = 2 * wp + 1;
        }
        a.wp = wp;
        a.wv = W[s];
        a.opitch = W[s];
        a.resid = resid;
        a.out_f32 = out;
        a.f32_transposed = transposed ? 1 : 0;
        a.ldo = transposed ? (long)H[s] * W[s] : c.cout;
        launch_audio_conv(a, -1, st);
    };
    float* x = xa;
    float* other = xb;
    auto res_block = [&](const AudioVaeModel::Res& r, int s) {
        const int ci = r.c1.cin, co = r.c1.cout;
        bf16_t* A = pad("a", s, ci);
        launch_audio_pn_pad(x, H[s], W[s], ci, 0, A, st);
        conv2d(r.c1, s, A, nullptr, t1, false);
        bf16_t* B = pad("b", s, co);
        launch_audio_pn_pad(t1, H[s], W[s], co, 0, B, st);
        if (r.has_sc) {
            bf16_t* S = pad("s", s, ci);
            launch_audio_pn_pad(x, H[s], W[s], ci, 1, S, st);
            conv2d(r.sc, s, S, nullptr, other, false);
            conv2d(r.c2, s, B, other, other, false);
            std::swap(x, other);
        } else {
            conv2d(r.c2, s, B, x, x, false);
        }
    };
    // decode(): denormalise the packed (T, 8*16) view, unpatchify (AudioVAE.swift:415-434)
    bf16_t* in = pad("in", 0, m->conv_in.cin_pad);
    launch_audio_denorm_pad(latent, m->mean, m->stdv, m->latent_ch, T, Wl, m->conv_in.cin_pad, in, st);
    conv2d(m->conv_in, 0, in, nullptr, x, false);
    res_block(m->mid[0], 0);
    res_block(m->mid[1], 0);
    int step = 0;
    for (int l = 2; l >= 0; --l) {
        for (int b = 0; b < 3; ++b) res_block(m->up[l][b], step);
        if (l > 0) {
            // nearest 2x + causal conv with its first output row dropped (AudioVAE.swift:178-198): the upsampled rows are written one
            // padded row higher, so the dropped row is simply never computed
            const int C = m->ups[l].cin;
            bf16_t* U = pad("u", step + 1, C);
            launch_audio_upsample_pad(x, H[step], W[step], C, U, st);
            ++step;
            conv2d(m->ups[l], step, U, nullptr, other, false);
            std::swap(x, other);
        }
    }
    bf16_t* A = pad("a", 2, m->base);
    launch_audio_pn_pad(x, H[2], W[2], m->base, 0, A, st);
    // (2, 4T-3, 64): already the cropped shape of AudioVAE.swift:443-452
    conv2d(m->conv_out, 2, A, nullptr, mel, true);
}

// ================================================================================================================
// Vocoder
// ================================================================================================================
VocoderModel* vocoder_create() { return new VocoderModel(); }
void vocoder_destroy(VocoderModel* m) {
    delete m;
}

static const int kUpK[5] = {16, 15, 8, 4, 4}, kUpS[5] = {6, 5, 2, 2, 2};  // Vocoder.swift:148-149
static const int kResK[3] = {3, 7, 11}, kResD[3] = {1, 3, 5};             // Vocoder.swift:150-151

static void vocoder_assemble(ltx_ctx* ctx, VocoderModel* m, const AHostWeights& hw) {
    Assembler as(hw);
    const int nkeys = (int)hw.size();
    bool ok = as.conv("conv_in", 3, &m->conv_in, -1);
    int ch = m->conv_in.cout;
    m->in_ch = m->conv_in.cin;
    m->hidden = ch;
    for (int i = 0; i < 5 && ok; ++i) {
        VocoderModel::Up& u = m->up[i];
        const std::string p = "upsamplers." + std::to_string(i);
        const AHostTensor* w = as.get(p + ".weight", 3);  // PyTorch ConvTranspose1d: (in, out, k)
        if (!w) { ok = false; break; }
        u.cin = (int)w->shape[0], u.cout = (int)w->shape[1], u.k = (int)w->shape[2];
        u.stride = kUpS[i];
        LTX_REQUIRE(u.cin == ch && u.k == kUpK[i] && u.cout % 4 == 0, "%s: (%d, %d, %d) against %d channels, kernel %d", p.c_str(), u.cin,
                    u.cout, u.k, ch, kUpK[i]);
        u.cin_pad = (u.cin + 31) / 32 * 32;
        u.pad = (u.k - u.stride) / 2;
        u.w.assign((size_t)u.stride, nullptr);
        u.off.assign((size_t)u.stride, {});
        for (int r = 0; r < u.stride; ++r) {
            const std::vector<int> js = convt_phase_taps(u.k, u.stride, u.pad, r, &u.off[r]);
            as.push_bf16(&u.w[r], convt_phase_slab(w->v.data(), u.cin, u.cout, u.k, js, u.cin_pad));
        }
        as.bias(p + ".bias", u.cout, &u.b);
        ch = u.cout;
        for (int j = 0; j < 3 && ok; ++j) {
            VocoderModel::Res& rb = m->res[i * 3 + j];
            rb.k = kResK[j];
            for (int d = 0; d < 3 && ok; ++d) {
                const std::string q = "resnets." + std::to_string(i * 3 + j);
                ok = ok && as.conv(q + ".convs1." + std::to_string(d), 3, &rb.c1[d], ch) &&
                     as.conv(q + ".convs2." + std::to_string(d), 3, &rb.c2[d], ch);
                if (ok) LTX_REQUIRE(rb.c1[d].k == rb.k && rb.c2[d].k == rb.k && rb.c1[d].cout == ch && rb.c2[d].cout == ch,
                                    "%s: kernel %d / %d, expected %d on %d channels", q.c_str(), rb.c1[d].k, rb.c2[d].k, rb.k, ch);
            }
        }
    }
    ok = ok && as.conv("conv_out", 3, &m->conv_out, ch);
    if (!ok) as.fail_if_missing_weights(ctx, nkeys, "the vocoder");
    m->out_ch = m->conv_out.cout;
    LTX_REQUIRE(m->conv_in.k == 7 && m->conv_out.k == 7 && m->out_ch == 2 && m->in_ch % 2 == 0 && ch % 4 == 0,
                "vocoder: conv_in k=%d, conv_out k=%d -> %d channels, last stage %d channels", m->conv_in.k, m->conv_out.k, m->out_ch, ch);
    as.commit(ctx, m->arena, nkeys);
}

void vocoder_load(ltx_ctx* ctx, VocoderModel* m, const std::string& path) { vocoder_assemble(ctx, m, read_file(path, keep_all)); }

void vocoder_init_synthetic(ltx_ctx* ctx, VocoderModel* m, int hidden, uint64_t seed) {
    LTX_REQUIRE(hidden >= 128 && hidden <= 2048 && hidden % 128 == 0, "vocoder: hidden %d (128..2048, multiple of 128)", hidden);
    HostRng rng(seed);
    AHostWeights hw;
    auto conv = [&](const std::string& p, int co, int ci, int k, float gain) {
        hw[p + ".weight"] = make_normal(rng, {co, ci, k}, gain / sqrtf((float)ci * k));
        hw[p + ".bias"] = make_normal(rng, {co}, 0.02f);
    };
    conv("conv_in", hidden, 128, 7, 1.f);
    int ch = hidden;
    for (int i = 0; i < 5; ++i) {
        const int co = ch / 2;
        hw["upsamplers." + std::to_string(i) + ".weight"] =
            make_normal(rng, {ch, co, kUpK[i]}, 1.4f / sqrtf((float)ch * kUpK[i] / kUpS[i]));
        hw["upsamplers." + std::to_string(i) + ".bias"] = make_normal(rng, {co}, 0.02f);
        ch = co;
        for (int j = 0; j < 3; ++j)
            for (int d = 0; d < 3; ++d) {
                const std::string q = "resnets." + std::to_string(i * 3 + j);
                conv(q + ".convs1." + std::to_string(d), ch, ch, kResK[j], 1.4f);
                conv(q + ".convs2." + std::to_string(d), ch, ch, kResK[j], 0.5f);
            }
    }
    conv("conv_out", 2, ch, 7, 0.5f);
    vocoder_assemble(ctx, m, hw);
}

void vocoder_forward(ltx_ctx* ctx, VocoderModel* m, const float* mel, int T, float* wave) {
    LTX_REQUIRE(mel && wave && T >= 1 && T <= 16384, "vocoder: T=%d (1..16384)", T);
    LTX_REQUIRE(m->conv_in.w, "vocoder: model not assembled");
    hipStream_t st = ctx->stream;
    if (m->ws_T != T) {
        HIP_CHECK(hipStreamSynchronize(st));
        m->ws.clear();
        m->ws_T = T;
    }
    Workspace ws{&m->ws, st};
    // haloed 1-D operand of L rows x C channels; the returned pointer is row 0 of the signal
    auto cpad = [](int C) { return (C + 31) / 32 * 32; };
    auto rows = [&](const char* slot, int stage, long L, int Craw) {
        const int C = cpad(Craw);  // channels past Craw are never written: they stay zero like the halo rows
        bf16_t* base = (bf16_t*)ws.get(key3(slot, stage, C), (size_t)(L + 2 * ACONV_HALO) * C * 2, true);
        return base + (size_t)ACONV_HALO * C;
    };
    auto f32buf = [&](const char* slot, int stage, long L, int C) { return (float*)ws.get(key3(slot, stage, C), (size_t)L * C * 4, false); };
    auto conv1d = [&](const AConvW& c, int dil, long L, const bf16_t* in) {
        AConvArgs a;
        a.x = in;
        a.ldx = c.cin_pad;
        a.w = c.w;
        a.bias = c.b;
        a.P = (int)L;
        a.Cin = c.cin_pad;
        a.Cout = c.cout;
        a.ntaps = c.k;
        for (int j = 0; j < c.k; ++j) a.off[j] = (j - (c.k - 1) / 2) * dil;
        return a;
    };
    long L = T;
    const int M = m->in_ch / 2;
    bf16_t* x0 = rows("in", 0, L, m->conv_in.cin_pad);
    LTX_REQUIRE(m->conv_in.cin_pad == m->in_ch, "vocoder: %d input channels (multiple of 32)", m->in_ch);
    launch_audio_mel_pack(mel, T, M, x0, st);
    bf16_t* act = rows("act", 0, L, m->hidden);  // leaky(conv_in(x)): the first transposed conv's operand
    {
        AConvArgs a = conv1d(m->conv_in, 1, L, x0);
        a.out_bf16 = act;
        a.ldb = cpad(m->hidden);
        a.bf16_act = AACT_LEAKY;
        a.slope = 0.1f;
        launch_audio_conv(a, -1, st);
    }
    for (int i = 0; i < 5; ++i) {
        const VocoderModel::Up& u = m->up[i];
        const long Lo = L * u.stride;
        const int C = u.cout;
        float* x = f32buf("x", i, Lo, C);
        bf16_t* pinit = rows("pi", i, Lo, C);
        for (int r = 0; r < u.stride; ++r) {
            AConvArgs a;
            a.x = act;
            a.ldx = u.cin_pad;
            a.w = u.w[r];
            a.bias = u.b;
            a.P = (int)L;
            a.Cin = u.cin_pad;
            a.Cout = C;
            a.ntaps = (int)u.off[r].size();
            for (int t = 0; t < a.ntaps; ++t) a.off[t] = u.off[r][t];
            a.omul = u.stride;
            a.oadd = r;
            a.out_f32 = x;
            a.ldo = C;
            a.out_bf16 = pinit;
            a.ldb = cpad(C);
            a.bf16_act = AACT_LEAKY;
            a.slope = 0.1f;
            launch_audio_conv(a, -1, st);
        }
        bf16_t* P = rows("p", i, Lo, C);
        bf16_t* Q = rows("q", i, Lo, C);
        float* h[3];
        for (int j = 0; j < 3; ++j) {
            const VocoderModel::Res& rb = m->res[i * 3 + j];
            char slot[8];
            snprintf(slot, sizeof(slot), "h%d", j);
            h[j] = f32buf(slot, i, Lo, C);
            for (int d = 0; d < 3; ++d) {
                AConvArgs a1 = conv1d(rb.c1[d], kResD[d], Lo, d == 0 ? pinit : P);
                a1.out_bf16 = Q;
                a1.ldb = cpad(C);
                a1.bf16_act = AACT_LEAKY;
                a1.slope = 0.1f;
                launch_audio_conv(a1, -1, st);
                AConvArgs a2 = conv1d(rb.c2[d], 1, Lo, Q);
                a2.resid = d == 0 ? x : h[j];
                a2.out_f32 = h[j];
                a2.ldo = C;
                if (d < 2) {
                    a2.out_bf16 = P;
                    a2.ldb = cpad(C);
                    a2.bf16_act = AACT_LEAKY;
                    a2.slope = 0.1f;
                }
                launch_audio_conv(a2, -1, st);
            }
        }
        // mean of the three blocks + the next consumer's LeakyReLU: 0.1 before an upsampler, 0.01 before conv_out (Vocoder.swift:257-258)
        act = rows("act", i + 1, Lo, C);
        launch_audio_mean3_act(h[0], h[1], h[2], Lo, C, i == 4 ? 0.01f : 0.1f, act, cpad(C), st);
        L = Lo;
    }
    AConvArgs a = conv1d(m->conv_out, 1, L, act);
    a.out_f32 = wave;
    a.f32_transposed = 1;
    a.ldo = L;
    a.f32_act = AACT_TANH;
    launch_audio_conv(a, -1, st);
}

// ================================================================================================================
// pure host
// ================================================================================================================
int audio_latent_frames(int video_frames, float fps) {
    const float duration = (float)video_frames / fps;
    const float per_second = 16000.0f / 160.0f / 4.0f;  // sample rate / hop length / temporal compression (LTXPipeline.swift:419-423)
    return (int)round((double)(duration * per_second));
}

bool write_wav_pcm16(const char* path, const float* waveform, long n, int sample_rate, float gain) {
    FILE* f = fopen(path, "wb");
    if (!f) return false;
    const uint32_t data_size = (uint32_t)(n * 2 * 2);
    uint8_t hdr[44];
    auto u32 = [&](int at, uint32_t v) { for (int i = 0; i < 4; ++i) hdr[at + i] = (uint8_t)(v >> (8 * i)); };
    auto u16 = [&](int at, uint32_t v) { for (int i = 0; i < 2; ++i) hdr[at + i] = (uint8_t)(v >> (8 * i)); };
    memcpy(hdr, "RIFF", 4);
    u32(4, 36 + data_size);
    memcpy(hdr + 8, "WAVEfmt ", 8);
    u32(16, 16);
    u16(20, 1);
    u16(22, 2);
    u32(24, (uint32_t)sample_rate);
    u32(28, (uint32_t)sample_rate * 4);
    u16(32, 4);
    u16(34, 16);
    memcpy(hdr + 36, "data", 4);
    u32(40, data_size);
    bool ok = fwrite(hdr, 1, 44, f) == 44;
    std::vector<int16_t> pcm((size_t)n * 2);
    for (long i = 0; i < n; ++i)
        for (int c = 0; c < 2; ++c) {
            float s = waveform[(size_t)c * n + i];
            if (gain != 1.0f) s *= gain;
            s = s < -1.0f ? -1.0f : s > 1.0f ? 1.0f : s;  // NaN falls through the comparisons and converts to 0 below
            const float v = s * 32767.0f;
            pcm[(size_t)i * 2 + c] = v != v ? 0 : (int16_t)v;  // truncation toward zero
        }
    ok = ok && fwrite(pcm.data(), 2, pcm.size(), f) == pcm.size();
    return fclose(f) == 0 && ok;
}
