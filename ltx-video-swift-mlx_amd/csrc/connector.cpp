// connector.cpp - see connector.h.
#include "connector.h"

#include <string.h>

#include "attention.h"
#include "elementwise.h"
#include "gemm.h"
#include "hostmath.h"
#include "linear_ops.h"

namespace {
// the registers and the blocks of one Embeddings1DConnector, under the module keys of the video one (the audio set keeps a table of
// its own with the same keys: connector_load_safetensors strips the "audio_" of its file keys)
void declare_stack(ParamTable& pt, ConnStack& s, const ConnectorConfig& cfg) {
    const int D = cfg.dim;
    s.blocks.resize(cfg.layers);
    pt.add("embeddings_connector.learnable_registers", (void**)&s.registers, SLOT_F32, cfg.registers, D);
    for (int i = 0; i < cfg.layers; ++i) {
        ConnBlock& b = s.blocks[i];
        const std::string p = "embeddings_connector.transformer_1d_blocks." + std::to_string(i) + ".";
        b.qk.out = 2 * D;
        b.qk.in = D;
        pt.add_hidden((void**)&b.qk.w, SLOT_BF16, 2 * D, D);
        pt.add_hidden((void**)&b.qk.b, SLOT_F32, 2 * D, 0);
        pt.add_linear(p + "attn1.to_v", b.v, D, D);
        pt.add_linear(p + "attn1.to_out", b.o, D, D);
        pt.add(p + "attn1.q_norm.weight", (void**)&b.qn, SLOT_F32, D, 0, 1);
        pt.add(p + "attn1.k_norm.weight", (void**)&b.kn, SLOT_F32, D, 0, 1);
        pt.add_linear(p + "ff.project_in.proj", b.ff1, 4 * D, D);
        pt.add_linear(p + "ff.project_out", b.ff2, D, 4 * D);
    }
}
void view_stack(ParamTable& pt, ConnStack& s, const ConnectorConfig& cfg) {
    const int D = cfg.dim;
    for (int i = 0; i < cfg.layers; ++i) {
        ConnBlock& b = s.blocks[i];
        const std::string p = "embeddings_connector.transformer_1d_blocks." + std::to_string(i) + ".";
        pt.view(p + "attn1.to_q.weight", b.qk.w, SLOT_BF16, D, D);
        pt.view(p + "attn1.to_k.weight", b.qk.w + (long)D * D, SLOT_BF16, D, D);
        pt.view(p + "attn1.to_q.bias", b.qk.b, SLOT_F32, D, 0);
        pt.view(p + "attn1.to_k.bias", b.qk.b + D, SLOT_F32, D, 0);
    }
}
const char kAudioPrefix[] = "audio_embeddings_connector";
}  // namespace

ConnectorModel* connector_create(const ConnectorConfig& cfg) {
    LTX_REQUIRE(cfg.dim == cfg.heads * 128, "connector: dim %d must be heads (%d) x 128", cfg.dim, cfg.heads);
    LTX_REQUIRE(cfg.dim % 64 == 0 && cfg.dim <= 8192, "connector: dim %d must be a multiple of 64 and <= 8192", cfg.dim);
    LTX_REQUIRE(cfg.layers >= 1 && cfg.registers >= 1 && cfg.states >= 1, "connector: empty model");
    ConnectorModel* m = new ConnectorModel();
    m->cfg = cfg;
    const int D = cfg.dim;
    ParamTable& pt = m->params;
    m->fe.out = D;
    m->fe.in = D * cfg.states;
    pt.add("feature_extractor.aggregate_embed.weight", (void**)&m->fe.w, SLOT_BF16, D, (long)D * cfg.states);
    declare_stack(pt, m->video, cfg);
    m->weight_bytes = pt.place(false);
    view_stack(pt, m->video, cfg);
    return m;
}

void connector_add_audio(ConnectorModel* m) {
    if (m->audio) return;
    ConnAudioSet* a = new ConnAudioSet();
    declare_stack(a->params, a->stack, m->cfg);
    a->weight_bytes = a->params.place(false);
    view_stack(a->params, a->stack, m->cfg);
    m->audio = a;
}

void connector_destroy(ConnectorModel* m) {
    if (m) delete m->audio;
    delete m;
}

void connector_load_safetensors(ltx_ctx* ctx, ConnectorModel* m, const std::string& path) {
    SafeTensors st;
    st.open(path);
    // an audio set is there when the file has its registers and its first q projection in this configuration's shapes; a stray
    // audio_embeddings_connector.* tensor of another model is skipped with the rest of a unified file, as before
    const long D = m->cfg.dim;
    bool has_registers = false, has_q = false;
    for (const auto& kv : st.tensors) {
        std::string mk;
        if (!map_text_encoder_file_key(kv.first, &mk)) continue;
        if (mk == std::string(kAudioPrefix) + ".learnable_registers") has_registers = kv.second.numel() == m->cfg.registers * D;
        if (mk == std::string(kAudioPrefix) + ".transformer_1d_blocks.0.attn1.to_q.weight") has_q = kv.second.numel() == D * D;
    }
    const bool has_audio = has_registers && has_q;
    // the second, independently weighted Embeddings1DConnector (LTXTextEncoder.swift:628-636; key rules ModelDownloader.swift:930-941):
    // loaded when the file has it, absent otherwise. Its load comes first so that the load report is the video set's, as before
    if (has_audio) {
        connector_add_audio(m);
        param_table_load(ctx, m->audio->params, st, [](const std::string& fk, std::string* mk) {
            if (!map_text_encoder_file_key(fk, mk) || mk->compare(0, sizeof(kAudioPrefix) - 1, kAudioPrefix) != 0) return false;
            mk->erase(0, 6);  // "audio_": the audio table names its slots as the video one does
            return true;
        });
    }
    param_table_load(ctx, m->params, st, [](const std::string& fk, std::string* mk) {
        // false: DiT / VAE / audio tensors of a unified file, and the audio connector's
        return map_text_encoder_file_key(fk, mk) && mk->compare(0, sizeof(kAudioPrefix) - 1, kAudioPrefix) != 0;
    });
}

void connector_init_synthetic(ltx_ctx* ctx, ConnectorModel* m, uint64_t seed) {
    const float fe_std = 1.0f / sqrtf((float)m->fe.in);
    const ParamFillRule rule = [&](const std::string& key, const ParamSlot& s) -> std::pair<float, float> {
        if (key.find("aggregate_embed") != std::string::npos) return {0.f, fe_std};
        if (key.find("learnable_registers") != std::string::npos) return {0.f, 0.5f};
        return param_fill_rule_default(key, s);
    };
    param_table_fill_synthetic(ctx, m->params, seed, 0, rule);
    connector_add_audio(m);  // the audio set from a seed of its own: different weights, the same rule
    param_table_fill_synthetic(ctx, m->audio->params, seed ^ 0xA0D10C0FFEEull, 0, rule);
}

void connector_encode(ltx_ctx* ctx, ConnectorModel* m, const ConnectorArgs& a) {
    const ConnectorConfig& c = m->cfg;
    const int D = c.dim, NS = c.states, B = a.B, T = a.T;
    LTX_REQUIRE(a.hidden && a.mask && a.out, "connector_encode: null argument");
    if (a.out_audio && !m->audio) LTX_THROW(LTXS_MODEL_NOT_LOADED, "Model not loaded: audio embeddings connector (the file had no audio_embeddings_connector.* tensors)");
    LTX_REQUIRE(B >= 1 && T >= 1, "connector_encode: empty batch");
    if (T % c.registers != 0)  // fatalError in the reference (LTXTextEncoder.swift:435-437)
        LTX_THROW(LTXS_INVALID_CONFIGURATION, "Sequence length %d must be divisible by numLearnableRegisters %d", T, c.registers);
    hipStream_t st = ctx->stream;
    const long rows = (long)B * T;
    const int Tpad = ((T + 63) / 64) * 64;
    bool grew = false;
    grew |= m->ws_nc.ensure((size_t)rows * D * NS * 2);
    grew |= m->ws_part.ensure((size_t)fe_stats_partials_floats(NS, B, T, D) * 4);
    grew |= m->ws_stats.ensure((size_t)NS * B * 2 * 4);
    grew |= m->ws_enc.ensure((size_t)rows * D * 2);
    grew |= m->ws_src.ensure((size_t)rows * 4);
    grew |= m->ws_x.ensure((size_t)rows * D * 4);
    grew |= m->ws_xn.ensure((size_t)rows * D * 2);
    grew |= m->ws_qk.ensure((size_t)rows * 2 * D * 4);
    grew |= m->ws_q.ensure((size_t)rows * D * 2);
    grew |= m->ws_k.ensure((size_t)rows * D * 2);
    grew |= m->ws_vt.ensure((size_t)B * D * Tpad * 2, true);
    grew |= m->ws_ao.ensure((size_t)rows * D * 2);
    grew |= m->ws_ffh.ensure((size_t)rows * 4 * D * 2);
    if (m->rope_T != T) {
        std::vector<float> hc, hs;
        rope_tables_1d(T, D, (double)c.theta, c.max_pos, &hc, &hs);
        for (auto& v : hc) v = host_bf16_to_f32(host_f32_to_bf16(v));  // cast to the activations' dtype (:498)
        for (auto& v : hs) v = host_bf16_to_f32(host_f32_to_bf16(v));
        HIP_CHECK(hipStreamSynchronize(st));
        m->rope_cos.ensure(hc.size() * 4);
        m->rope_sin.ensure(hs.size() * 4);
        HIP_CHECK(hipMemcpy(m->rope_cos.p, hc.data(), hc.size() * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(m->rope_sin.p, hs.data(), hs.size() * 4, hipMemcpyHostToDevice));
        m->rope_T = T;
    }
    (void)grew;
    bf16_t* nc = m->ws_nc.as<bf16_t>();
    bf16_t* enc = m->ws_enc.as<bf16_t>();
    float* x = m->ws_x.as<float>();
    bf16_t* xn = m->ws_xn.as<bf16_t>();
    float* qk = m->ws_qk.as<float>();
    bf16_t* q = m->ws_q.as<bf16_t>();
    bf16_t* k = m->ws_k.as<bf16_t>();
    bf16_t* vt = m->ws_vt.as<bf16_t>();
    bf16_t* ao = m->ws_ao.as<bf16_t>();
    bf16_t* ffh = m->ws_ffh.as<bf16_t>();

    // feature extractor: per-(state, batch) statistics over the valid tokens, 8*(x-mean)/(range+eps), concat, projection
    launch_fe_stats(a.hidden, a.mask, NS, B, T, D, a.padding_right, c.eps, m->ws_part.as<float>(), m->ws_stats.as<float>(), st);
    launch_fe_norm_concat(a.hidden, a.mask, m->ws_stats.as<float>(), NS, B, T, D, a.padding_right, c.eps, nc, st);
    {
        GemmEpilogue e;  // f32 accumulate over 188160 products, one rounding to bf16 (LTXTextEncoder.swift:180-186)
        e.out_bf16 = enc;
        e.ld_bf16 = D;
        gemm_linear(nc, (long)D * NS, m->fe, (int)rows, e, st);
    }
    if (a.dbg_nc) HIP_CHECK(hipMemcpyAsync(a.dbg_nc, nc, (size_t)rows * D * NS * 2, hipMemcpyDeviceToDevice, st));
    if (a.dbg_fe) HIP_CHECK(hipMemcpyAsync(a.dbg_fe, enc, (size_t)rows * D * 2, hipMemcpyDeviceToDevice, st));
    launch_register_plan(a.mask, B, T, m->ws_src.as<int32_t>(), st);

    // one Embeddings1DConnector on the feature extractor's output: (weight set, enc) -> out. Both sets run the same launches on the
    // same workspaces, one after the other on the stream
    auto run_stack = [&](const ConnStack& set, bf16_t* out, float* dbg_reg) {
        // learnable registers replace the padded positions (valid tokens first)
        launch_register_gather(enc, set.registers, m->ws_src.as<int32_t>(), B, T, D, c.registers, x, st);
        if (dbg_reg) HIP_CHECK(hipMemcpyAsync(dbg_reg, x, (size_t)rows * D * 4, hipMemcpyDeviceToDevice, st));

        NormModArgs nm;  // the plain RMS norms of the stream, x -> xn (the last one -> a.out)
        nm.x = x; nm.ldx = D; nm.rows_per_batch = T;
        nm.out = xn; nm.ldo = D;
        nm.rows = (int)rows; nm.D = D; nm.eps = c.eps;
        QkNormRopeArgs qkn;  // q and k of the fused projection, two jobs
        qkn.job[0].x = qk; qkn.job[0].out = q;
        qkn.job[1].x = qk + D; qkn.job[1].out = k;
        qkn.ldx = 2 * D; qkn.ldo = D;
        qkn.cos = m->rope_cos.as<float>(); qkn.sin = m->rope_sin.as<float>();
        qkn.T = T; qkn.rows = (int)rows; qkn.D = D; qkn.eps = c.eps;
        for (int l = 0; l < c.layers; ++l) {
            const ConnBlock& blk = set.blocks[l];
            launch_norm_mod(nm, st);
            GemmEpilogue eqk;
            eqk.out_f32 = qk;
            eqk.ld_f32 = 2 * D;
            gemm_linear(xn, D, blk.qk, (int)rows, eqk, st);
            qkn.job[0].w = blk.qn; qkn.job[1].w = blk.kn;
            launch_qknorm_rope(qkn, st);
            for (int b = 0; b < B; ++b) gemm_vt(xn + (size_t)b * T * D, D, T, blk.v, vt + (size_t)b * D * Tpad, Tpad, st);
            AttnArgs at;
            at.Q = q; at.ldq = D; at.q_bstride = (long)T * D;
            at.K = k; at.ldk = D; at.k_bstride = (long)T * D;
            at.Vt = vt; at.ldvt = Tpad; at.vt_bstride = (long)D * Tpad;
            at.O = ao; at.ldo = D; at.o_bstride = (long)T * D;
            at.B = B; at.H = c.heads; at.Tq = T; at.Tk = T;
            launch_attention(at, st);
            GemmEpilogue eo;  // x += to_out(attn)
            eo.out_f32 = x;
            eo.ld_f32 = D;
            eo.resid = 1;
            eo.gate_scalar = 1.0f;
            gemm_linear(ao, D, blk.o, (int)rows, eo, st);
            launch_norm_mod(nm, st);
            GemmEpilogue e1;
            e1.out_bf16 = ffh;
            e1.ld_bf16 = 4 * D;
            e1.act = LTX_ACT_GELU_TANH;
            gemm_linear(xn, D, blk.ff1, (int)rows, e1, st);
            GemmEpilogue e2;  // x += project_out(h)
            e2.out_f32 = x;
            e2.ld_f32 = D;
            e2.resid = 1;
            e2.gate_scalar = 1.0f;
            gemm_linear(ffh, 4 * D, blk.ff2, (int)rows, e2, st);
        }
        nm.out = out;
        launch_norm_mod(nm, st);
    };
    run_stack(m->video, a.out, a.dbg_reg);
    if (a.out_audio) run_stack(m->audio->stack, a.out_audio, nullptr);  // LTXTextEncoder.swift:628-636
    // after the register replacement every position is valid: the mask the loop receives is all ones (:466-468, :622-626)
    if (a.out_mask) launch_fill_const_i32(a.out_mask, rows, 1, st);
}
