// gemma.cpp - see gemma.h.
#include "gemma.h"

#include <math.h>
#include <string.h>

#include "attention.h"
#include "elementwise.h"
#include "gemm.h"
#include "linear_ops.h"

namespace {
bool starts_with(const std::string& s, const char* pre) { return s.compare(0, strlen(pre), pre) == 0; }
bool ends_with(const std::string& s, const char* suf) {
    const size_t n = strlen(suf);
    return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}
}  // namespace

GemmaModel* gemma_create(ltx_ctx* ctx, const GemmaConfig& cfg) {
    if (cfg.head_dim != 256) LTX_THROW(LTXS_INVALID_CONFIGURATION, "gemma: head_dim %d is not supported (256)", cfg.head_dim);
    LTX_REQUIRE(cfg.layers >= 1 && cfg.heads >= 1 && cfg.kv_heads >= 1 && cfg.heads % cfg.kv_heads == 0, "gemma: %d query heads over %d K/V heads",
                cfg.heads, cfg.kv_heads);
    LTX_REQUIRE(cfg.hidden % 64 == 0 && cfg.hidden <= 8192 && cfg.intermediate % 64 == 0, "gemma: hidden %d / intermediate %d must be multiples of 64, hidden <= 8192",
                cfg.hidden, cfg.intermediate);
    LTX_REQUIRE(cfg.vocab >= 1 && cfg.sliding_window >= 1 && cfg.sliding_window_pattern >= 1 && cfg.query_pre_attn_scalar > 0.f, "gemma: configuration");
    GemmaModel* m = new GemmaModel();
    m->cfg = cfg;
    m->layers.resize(cfg.layers);
    const int H = cfg.hidden, I = cfg.intermediate, Dq = cfg.heads * 256, Dk = cfg.kv_heads * 256;
    ParamTable& pt = m->params;
    auto weight = [&](LinearW& l, int out, int in) {
        l.out = out;
        l.in = in;
    };
    pt.add("model.embed_tokens.weight", (void**)&m->embed, SLOT_BF16, cfg.vocab, H);
    pt.add("model.norm.weight", (void**)&m->final_norm, SLOT_F32, H, 0);
    for (int i = 0; i < cfg.layers; ++i) {
        GemmaLayer& l = m->layers[i];
        const std::string p = "model.layers." + std::to_string(i) + ".";
        weight(l.qk, Dq + Dk, H);
        pt.add_hidden((void**)&l.qk.w, SLOT_BF16, Dq + Dk, H);
        weight(l.v, Dk, H);
        pt.add(p + "self_attn.v_proj.weight", (void**)&l.v.w, SLOT_BF16, Dk, H);
        weight(l.o, H, Dq);
        pt.add(p + "self_attn.o_proj.weight", (void**)&l.o.w, SLOT_BF16, H, Dq);
        pt.add(p + "self_attn.q_norm.weight", (void**)&l.qn, SLOT_F32, 256, 0);
        pt.add(p + "self_attn.k_norm.weight", (void**)&l.kn, SLOT_F32, 256, 0);
        pt.add(p + "input_layernorm.weight", (void**)&l.in_norm, SLOT_F32, H, 0);
        pt.add(p + "post_attention_layernorm.weight", (void**)&l.post_attn, SLOT_F32, H, 0);
        pt.add(p + "pre_feedforward_layernorm.weight", (void**)&l.pre_ff, SLOT_F32, H, 0);
        pt.add(p + "post_feedforward_layernorm.weight", (void**)&l.post_ff, SLOT_F32, H, 0);
        weight(l.gu, 2 * I, H);
        pt.add_hidden((void**)&l.gu.w, SLOT_BF16, 2 * I, H);
        weight(l.down, H, I);
        pt.add(p + "mlp.down_proj.weight", (void**)&l.down.w, SLOT_BF16, H, I);
    }
    try {
        m->weight_bytes = pt.place(false);
        for (int i = 0; i < cfg.layers; ++i) {
            GemmaLayer& l = m->layers[i];
            const std::string p = "model.layers." + std::to_string(i) + ".";
            pt.view(p + "self_attn.q_proj.weight", l.qk.w, SLOT_BF16, Dq, H);
            pt.view(p + "self_attn.k_proj.weight", l.qk.w + (long)Dq * H, SLOT_BF16, Dk, H);
            pt.view(p + "mlp.gate_proj.weight", l.gu.w, SLOT_BF16, I, H);
            pt.view(p + "mlp.up_proj.weight", l.gu.w + (long)I * H, SLOT_BF16, I, H);
        }
        // RoPE tables of positions 0 .. window-1 for the two bases (no rope_scaling: Gemma3Model.swift:55-59)
        const size_t tab = (size_t)cfg.sliding_window * 128;
        m->rope.ensure(4 * tab * 4);
        float* r = m->rope.as<float>();
        launch_gemma_rope_tables(r, r + tab, cfg.sliding_window, cfg.rope_local_base, ctx->stream);
        launch_gemma_rope_tables(r + 2 * tab, r + 3 * tab, cfg.sliding_window, cfg.rope_theta, ctx->stream);
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    } catch (...) {
        delete m;
        throw;
    }
    return m;
}

void gemma_destroy(GemmaModel* m) {
    if (m) delete m->lm;
    delete m;
}

size_t gemma_resident_bytes(const GemmaModel* m) {
    size_t n = m->params.arena.buf.bytes + m->rope.bytes;
    for (const DevBuf* b : {&m->ws_hidden, &m->ws_ks, &m->ws_xn, &m->ws_qk, &m->ws_vt, &m->ws_ao, &m->ws_r, &m->ws_h, &m->ws_gu, &m->ws_ff}) n += b->bytes;
    return n;
}

void gemma_load_safetensors(ltx_ctx* ctx, GemmaModel* m, const std::vector<std::string>& shards) {
    LTX_REQUIRE(!shards.empty(), "gemma_load: no files");
    ParamTable& pt = m->params;
    ctx->n_loaded = ctx->n_missing = ctx->n_unmatched = 0;
    for (auto& kv : pt.slots) kv.second.loaded = false;
    std::vector<uint8_t> staging;
    std::vector<bf16_t> h_scales, h_biases;
    DevBuf d_codes, d_scales, d_biases;
    for (const std::string& path : shards) {
        SafeTensors st;
        st.open(path);
        for (auto& kv : st.tensors) {
            std::string key = kv.first;
            if (starts_with(key, "language_model.")) key.erase(0, 15);  // VLM conversions (sanitize, Gemma3Model.swift:350-354)
            if (starts_with(key, "lm_head")) continue;                  // :357
            if (ends_with(key, ".scales") || ends_with(key, ".biases")) continue;  // read with their .weight below
            auto it = pt.slots.find(key);
            if (it == pt.slots.end()) {
                ctx->n_unmatched++;
                continue;
            }
            ParamSlot& s = it->second;
            const StTensor& t = kv.second;
            if (t.dtype == "U32") {
                // MLX affine quantisation: 32 / bits codes per word, low bits first - byte for byte this library's code layout
                const std::string base = kv.first.substr(0, kv.first.size() - 7);  // without ".weight"
                auto is = st.tensors.find(base + ".scales"), ib = st.tensors.find(base + ".biases");
                if (!ends_with(kv.first, ".weight") || is == st.tensors.end() || ib == st.tensors.end())
                    LTX_THROW(LTXS_WEIGHT_LOADING_FAILED, "Failed to load weights: %s is packed but has no scales / biases beside it", kv.first.c_str());
                const long rows = s.rows, cols = s.cols;
                const long words = t.numel();
                const int bits = rows > 0 && cols > 0 && (words * 32) % (rows * cols) == 0 ? (int)(words * 32 / (rows * cols)) : 0;
                const bool shape_ok = t.shape.size() == 2 && t.shape[0] == rows && t.shape[1] * 32 == cols * bits;  // [rows][cols * bits / 32]
                if (s.kind != SLOT_BF16 || cols % 64 != 0 || (bits != 4 && bits != 8) || !shape_ok || (size_t)words * 4 != t.end - t.begin)
                    LTX_THROW(LTXS_WEIGHT_LOADING_FAILED, "Failed to load weights: %s is not a 4- or 8-bit packing of [%ld, %ld]", kv.first.c_str(), rows, cols);
                const long groups = rows * cols / 64;
                if (is->second.numel() != groups || ib->second.numel() != groups)
                    LTX_THROW(LTXS_WEIGHT_LOADING_FAILED, "Failed to load weights: %s needs %ld scales and biases (group size 64)", kv.first.c_str(), groups);
                h_scales.resize(groups);
                h_biases.resize(groups);
                st_to_bf16(st, is->second, h_scales.data());
                st_to_bf16(st, ib->second, h_biases.data());
                d_codes.ensure((size_t)words * 4);
                d_scales.ensure((size_t)groups * 2);
                d_biases.ensure((size_t)groups * 2);
                HIP_CHECK(hipMemcpy(d_codes.p, st.ptr(t), (size_t)words * 4, hipMemcpyHostToDevice));
                HIP_CHECK(hipMemcpy(d_scales.p, h_scales.data(), (size_t)groups * 2, hipMemcpyHostToDevice));
                HIP_CHECK(hipMemcpy(d_biases.p, h_biases.data(), (size_t)groups * 2, hipMemcpyHostToDevice));
                launch_dequant(d_codes.as<uint8_t>(), d_scales.as<bf16_t>(), d_biases.as<bf16_t>(), rows, cols, bits, (bf16_t*)s.dst, ctx->stream);
                HIP_CHECK(hipStreamSynchronize(ctx->stream));
            } else {
                param_check_shape(kv.first, t, s);
                param_upload(st, t, s, &staging);
            }
            if (!s.loaded) ctx->n_loaded++;
            s.loaded = true;
        }
    }
    std::string first_missing;
    for (auto& kv : pt.slots)
        if (!kv.second.loaded) {
            if (first_missing.empty()) first_missing = kv.first;
            ctx->n_missing++;
        }
    if (!first_missing.empty())
        LTX_THROW(LTXS_WEIGHT_LOADING_FAILED, "Failed to load weights: %s is missing (%d parameters missing)", first_missing.c_str(), ctx->n_missing);
}

void gemma_init_synthetic(ltx_ctx* ctx, GemmaModel* m, uint64_t seed) {
    // the shared fill; norm weights are the stored w of the 1 + w form, so they are drawn around 0
    param_table_fill_synthetic(ctx, m->params, seed, 0, [](const std::string&, const ParamSlot&) -> std::pair<float, float> { return {0.f, 0.02f}; });
}

void gemma_encode(ltx_ctx* ctx, GemmaModel* m, const GemmaArgs& a) {
    const GemmaConfig& c = m->cfg;
    const int B = a.B, T = a.T, H = c.hidden;
    LTX_REQUIRE(a.ids && a.mask && a.hidden, "gemma_encode: null argument");
    LTX_REQUIRE(B >= 1 && T >= 1, "gemma_encode: empty batch");
    if (T > c.sliding_window)  // window masking is not built; the tokenizer truncates to the window
        LTX_THROW(LTXS_INVALID_CONFIGURATION, "gemma_encode: %d tokens exceed the sliding window %d", T, c.sliding_window);
    hipStream_t st = ctx->stream;
    const long rows = (long)B * T;
    m->ws_ks.ensure((size_t)2 * B * 4);

    // key_start[b] from the mask, on the device; the form 0..0 1..1 is checked there and reported here
    int32_t* key_start = m->ws_ks.as<int32_t>();
    launch_gemma_mask_scan(a.mask, B, T, key_start, key_start + B, st);
    std::vector<int32_t> status(B);
    HIP_CHECK(hipMemcpyAsync(status.data(), key_start + B, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    for (int b = 0; b < B; ++b)
        if (!status[b])
            LTX_THROW(LTXS_INVALID_CONFIGURATION, "gemma_encode: the attention mask of batch element %d is not left-padded (0..0 1..1 with at least one 1)", b);

    GemmaEmbedArgs em;  // slot 0: embedding * bf16(sqrt(hidden)) (Gemma3Model.swift:209-211)
    em.ids = a.ids; em.table = m->embed; em.out = a.hidden; em.rows = (int)rows; em.D = H; em.vocab = c.vocab;
    em.scale = host_bf16_to_f32(host_f32_to_bf16(sqrtf((float)H)));
    launch_gemma_embed(em, st);
    GemmaStackRun s;
    s.B = B; s.T = T; s.key_start = key_start;
    s.rope = m->rope.as<float>(); s.tab = (size_t)c.sliding_window * 128;
    s.hidden = a.hidden;
    gemma_run_layers(ctx, m, s);
}

void gemma_run_layers(ltx_ctx* ctx, GemmaModel* m, const GemmaStackRun& s) {
    const GemmaConfig& c = m->cfg;
    const int B = s.B, T = s.T, H = c.hidden, I = c.intermediate, L = c.layers;
    const int Dq = c.heads * 256, Dk = c.kv_heads * 256, Dqk = Dq + Dk;
    LTX_REQUIRE(!s.vtcache || B == 1, "gemma: a V^T cache holds one sequence");
    hipStream_t st = ctx->stream;
    const long rows = (long)B * T;
    const int Tpad = ((T + 63) / 64) * 64;
    m->ws_xn.ensure((size_t)rows * H * 2);
    m->ws_qk.ensure((size_t)rows * Dqk * 2);
    if (!s.vtcache) m->ws_vt.ensure((size_t)B * Dk * Tpad * 2, true);
    m->ws_ao.ensure((size_t)rows * Dq * 2);
    m->ws_r.ensure((size_t)rows * H * 2);
    m->ws_h.ensure((size_t)rows * H * 2);
    m->ws_gu.ensure((size_t)rows * 2 * I * 2);
    m->ws_ff.ensure((size_t)rows * I * 2);

    bf16_t* xn = m->ws_xn.as<bf16_t>();
    bf16_t* qk = m->ws_qk.as<bf16_t>();
    bf16_t* ao = m->ws_ao.as<bf16_t>();
    bf16_t* r = m->ws_r.as<bf16_t>();
    bf16_t* h = m->ws_h.as<bf16_t>();
    bf16_t* gu = m->ws_gu.as<bf16_t>();
    bf16_t* ff = m->ws_ff.as<bf16_t>();
    const size_t slot = (size_t)rows * H;
    auto slot_in = [&](int l) { return s.hidden + (size_t)(s.ping_pong ? (l & 1) : l) * slot; };
    auto slot_out = [&](int l) { return s.hidden + (size_t)(s.ping_pong ? ((l + 1) & 1) : l + 1) * slot; };

    GemmaNormArgs n0;  // layer 0's input norm
    n0.r = s.hidden; n0.ldr = H; n0.w = m->layers[0].in_norm; n0.h = xn; n0.ldh = H; n0.rows = (int)rows; n0.D = H; n0.eps = c.rms_eps;
    launch_gemma_norm(n0, st);

    for (int l = 0; l < L; ++l) {
        const GemmaLayer& ly = m->layers[l];
        const bf16_t* x = slot_in(l);
        // where this layer's K rows and V^T live: the row buffer and the workspace (encoder), or the session's cache (prefill)
        bf16_t* kdst = s.kcache ? s.kcache + (size_t)l * s.k_stride : qk + Dq;
        const long ldk = s.kcache ? Dk : Dqk;
        bf16_t* vt = s.vtcache ? s.vtcache + (size_t)l * s.vt_stride : m->ws_vt.as<bf16_t>();
        const long ldvt = s.vtcache ? s.ldvt : Tpad;
        // q|k row-major, V as V^T per batch element (the DiT's pair of launches; q and k differ in width, so not the fused one)
        GemmEpilogue eqk;
        eqk.out_bf16 = qk;
        eqk.ld_bf16 = Dqk;
        gemm_linear(xn, H, ly.qk, (int)rows, eqk, st);
        for (int b = 0; b < B; ++b) gemm_vt(xn + (size_t)b * T * H, H, T, ly.v, vt + (size_t)b * Dk * ldvt, ldvt, st);
        GemmaQkArgs qa;  // q in place; k in place, or straight into the cache rows
        qa.job[0].x = qk; qa.job[0].ldx = Dqk; qa.job[0].w = ly.qn; qa.job[0].out = qk; qa.job[0].ldo = Dqk; qa.job[0].heads = c.heads;
        qa.job[1].x = qk + Dq; qa.job[1].ldx = Dqk; qa.job[1].w = ly.kn; qa.job[1].out = kdst; qa.job[1].ldo = ldk; qa.job[1].heads = c.kv_heads;
        const float* tb = s.rope + (gemma_layer_is_global(c, l) ? 2 * s.tab : 0);
        qa.cos = tb; qa.sin = tb + s.tab; qa.T = T; qa.rows = (int)rows; qa.eps = c.rms_eps;
        launch_gemma_qknorm_rope(qa, st);
        AttnArgs at;
        at.head_dim = 256; at.causal = 1; at.key_start = s.key_start;
        at.Q = qk; at.ldq = Dqk; at.q_bstride = (long)T * Dqk;
        at.K = kdst; at.ldk = ldk; at.k_bstride = (long)T * ldk;
        at.Vt = vt; at.ldvt = ldvt; at.vt_bstride = (long)Dk * ldvt;
        at.O = ao; at.ldo = Dq; at.o_bstride = (long)T * Dq;
        at.B = B; at.H = c.heads; at.Hkv = c.kv_heads; at.Tq = T; at.Tk = T;
        at.scale = 1.0f / sqrtf(c.query_pre_attn_scalar);  // not a function of the head dim (Gemma3Model.swift:41-42)
        launch_attention(at, st);
        GemmEpilogue eo;
        eo.out_bf16 = r;
        eo.ld_bf16 = H;
        gemm_linear(ao, Dq, ly.o, (int)rows, eo, st);
        GemmaNormArgs n1;  // h = x + post_attention_layernorm(r); xn = pre_feedforward_layernorm(h)
        n1.r = r; n1.ldr = H; n1.w = ly.post_attn; n1.x = x; n1.ldx = H; n1.h = h; n1.ldh = H;
        n1.w2 = ly.pre_ff; n1.n = xn; n1.ldn = H; n1.rows = (int)rows; n1.D = H; n1.eps = c.rms_eps;
        launch_gemma_norm(n1, st);
        GemmEpilogue eg;
        eg.out_bf16 = gu;
        eg.ld_bf16 = 2 * I;
        gemm_linear(xn, H, ly.gu, (int)rows, eg, st);
        GegluArgs ga;
        ga.gu = gu; ga.ldgu = 2 * I; ga.out = ff; ga.ldo = I; ga.rows = (int)rows; ga.I = I;
        launch_geglu(ga, st);
        GemmEpilogue ed;
        ed.out_bf16 = r;
        ed.ld_bf16 = H;
        gemm_linear(ff, I, ly.down, (int)rows, ed, st);
        GemmaNormArgs n2;  // out = h + post_feedforward_layernorm(r), straight into its slot; the next input norm, or model.norm, beside it
        n2.r = r; n2.ldr = H; n2.w = ly.post_ff; n2.x = h; n2.ldx = H; n2.rows = (int)rows; n2.D = H; n2.eps = c.rms_eps;
        if (l + 1 < L) {
            n2.h = slot_out(l); n2.ldh = H;
            n2.w2 = m->layers[l + 1].in_norm; n2.n = xn; n2.ldn = H;
        } else {  // the raw output of the last layer is not exported: the last slot is model.norm of it (Gemma3Model.swift:286-300)
            n2.n_only = 1;
            n2.w2 = m->final_norm; n2.n = slot_out(l); n2.ldn = H;
            if (s.final_out) {  // generation: only the last row's model.norm is read (:433)
                n2.r = r + (size_t)(rows - 1) * H; n2.x = h + (size_t)(rows - 1) * H; n2.n = s.final_out; n2.rows = 1;
            }
        }
        launch_gemma_norm(n2, st);
    }
}
