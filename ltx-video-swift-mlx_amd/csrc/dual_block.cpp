// dual_block.cpp - see dual_block.h. One forward = L x LTX2TransformerBlock.callAsFunction (LTX2TransformerBlock.swift:174-297).
#include "dual_block.h"

#include <string.h>

#include <algorithm>

#include "attention.h"
#include "elementwise.h"
#include "gemm.h"
#include "linear_ops.h"

namespace {

void destroy_blocks(DualStack* m) {
    for (DualBlock& b : m->blocks)
        for (AttnModule** a : {&b.attn1, &b.attn2, &b.audio_attn1, &b.audio_attn2, &b.a2v, &b.v2a}) {
            if (*a) attn_module_destroy(*a);
            *a = nullptr;
        }
}

}  // namespace

DualStack::~DualStack() { destroy_blocks(this); }

DualStack* dual_create(const DualBlockConfig& cfg) {
    if (cfg.num_layers < 1 || cfg.num_layers > 256 || cfg.video_heads < 1 || cfg.audio_heads < 1 || cfg.video_heads > 64 || cfg.audio_heads > 128)
        LTX_THROW(LTXS_INVALID_CONFIGURATION, "dual blocks: %d layers, %d video heads, %d audio heads", cfg.num_layers, cfg.video_heads, cfg.audio_heads);
    if (cfg.video_dim != cfg.video_heads * 128 || cfg.audio_dim != cfg.audio_heads * 64)
        LTX_THROW(LTXS_INVALID_CONFIGURATION, "dual blocks: video_dim %d must be %d heads x 128 and audio_dim %d must be %d heads x 64", cfg.video_dim,
                  cfg.video_heads, cfg.audio_dim, cfg.audio_heads);
    if (cfg.video_context_dim < 64 || cfg.audio_context_dim < 64 || cfg.video_context_dim % 64 != 0 || cfg.audio_context_dim % 64 != 0 ||
        cfg.video_context_dim > 8192 || cfg.audio_context_dim > 8192)
        LTX_THROW(LTXS_INVALID_CONFIGURATION, "dual blocks: context dims %d / %d must be multiples of 64 up to 8192", cfg.video_context_dim,
                  cfg.audio_context_dim);
    if (!(cfg.norm_eps > 0.f) || !(cfg.rope_theta > 1.f) || cfg.audio_max_pos < 1 || cfg.max_pos[0] < 1 || cfg.max_pos[1] < 1 || cfg.max_pos[2] < 1 ||
        !(cfg.fps > 0.f))
        LTX_THROW(LTXS_INVALID_CONFIGURATION, "dual blocks: norm_eps, rope_theta, max_pos and fps must be positive");
    DualStack* m = new DualStack();
    try {
        m->cfg = cfg;
        m->L = cfg.num_layers;
        const int L = m->L, Dv = m->Dv = cfg.video_dim, Da = m->Da = cfg.audio_dim;
        m->blocks.resize(L);
        ParamTable& pt = m->params;
        pt.add_hidden((void**)&m->sst_v, SLOT_F32, (long)L * 6, Dv);
        pt.add_hidden((void**)&m->sst_a, SLOT_F32, (long)L * 6, Da);
        pt.add_hidden((void**)&m->sst_ca_v, SLOT_F32, (long)L * 5, Dv);
        pt.add_hidden((void**)&m->sst_ca_a, SLOT_F32, (long)L * 5, Da);
        for (int i = 0; i < L; ++i) {
            DualBlock& b = m->blocks[i];
            const std::string p = "transformer_blocks." + std::to_string(i) + ".";
            b.attn1 = attn_module_create_ex(Dv, Dv, cfg.video_heads, 128, true, true);
            b.attn2 = attn_module_create_ex(Dv, cfg.video_context_dim, cfg.video_heads, 128, false, true);
            b.audio_attn1 = attn_module_create_ex(Da, Da, cfg.audio_heads, 64, true, true);
            b.audio_attn2 = attn_module_create_ex(Da, cfg.audio_context_dim, cfg.audio_heads, 64, false, true);
            b.a2v = attn_module_create_ex(Dv, Da, cfg.audio_heads, 64, false, true);
            b.v2a = attn_module_create_ex(Da, Dv, cfg.audio_heads, 64, false, true);
            const std::pair<const char*, AttnModule*> mods[] = {{"attn1.", b.attn1},           {"attn2.", b.attn2},
                                                                 {"audio_attn1.", b.audio_attn1}, {"audio_attn2.", b.audio_attn2},
                                                                 {"audio_to_video_attn.", b.a2v}, {"video_to_audio_attn.", b.v2a}};
            for (auto& mm : mods) {
                mm.second->eps = cfg.norm_eps;
                for (auto& kv : mm.second->params.slots) pt.slots[p + mm.first + kv.first] = kv.second;
            }
            pt.add_linear(p + "ff.project_in.proj", b.ff1, 4 * Dv, Dv);
            pt.add_linear(p + "ff.project_out", b.ff2, Dv, 4 * Dv);
            pt.add_linear(p + "audio_ff.project_in.proj", b.aff1, 4 * Da, Da);
            pt.add_linear(p + "audio_ff.project_out", b.aff2, Da, 4 * Da);
        }
        pt.place(true);
        for (int i = 0; i < L; ++i) {  // per-block views into the four stacked tables
            const std::string p = "transformer_blocks." + std::to_string(i) + ".";
            pt.view(p + "scale_shift_table", m->sst_v + (long)i * 6 * Dv, SLOT_F32, 6, Dv);
            pt.view(p + "audio_scale_shift_table", m->sst_a + (long)i * 6 * Da, SLOT_F32, 6, Da);
            pt.view(p + "scale_shift_table_a2v_ca_video", m->sst_ca_v + (long)i * 5 * Dv, SLOT_F32, 5, Dv);
            pt.view(p + "scale_shift_table_a2v_ca_audio", m->sst_ca_a + (long)i * 5 * Da, SLOT_F32, 5, Da);
        }
    } catch (...) {
        delete m;
        throw;
    }
    return m;
}

void dual_destroy(DualStack* m) { delete m; }

void dual_init_synthetic(ltx_ctx* ctx, DualStack* m, uint64_t seed) {
    // Linear weights N(0, 0.02^2), biases N(0, 0.01^2), q / k norm weights 1 + N(0, 0.02^2), scale-shift tables N(0, 0.02^2); bf16 values
    param_table_fill_synthetic(ctx, m->params, seed, 0, param_fill_rule_default);
}

void dual_load(ltx_ctx* ctx, DualStack* m, const std::string& path, int first_block) {
    if (first_block < 0) LTX_THROW(LTXS_INVALID_CONFIGURATION, "dual blocks: first_block %d", first_block);
    SafeTensors st;
    st.open(path);
    const std::string tb = "transformer_blocks.";
    // "transformer_blocks.{first_block + i}.x" of the file is block i of this stack; other blocks and top-level keys are not its own
    const std::string first_missing = param_table_load(ctx, m->params, st, [&](const std::string& fk, std::string* mk) {
        if (fk.compare(0, tb.size(), tb) != 0) return false;
        const size_t dot = fk.find('.', tb.size());
        if (dot == std::string::npos || dot == tb.size() || dot - tb.size() > 6) return false;
        int idx = 0;
        bool digits = true;
        for (size_t i = tb.size(); i < dot; ++i) {
            digits = digits && fk[i] >= '0' && fk[i] <= '9';
            idx = idx * 10 + (fk[i] - '0');
        }
        if (!digits || idx < first_block || idx >= first_block + m->L) return false;
        *mk = tb + std::to_string(idx - first_block) + transformer_module_spelling(fk.substr(dot));
        return true;
    });
    if (!first_missing.empty())
        LTX_THROW(LTXS_WEIGHT_LOADING_FAILED, "Failed to load weights: %s (block %d of the file) and %d more are not in %s", first_missing.c_str(),
                  first_block, ctx->n_missing - 1, path.c_str());
}

// ---------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------
namespace {

void upload(ltx_ctx* ctx, DevBuf& buf, const std::vector<float>& v) {
    buf.ensure(v.size() * 4);
    HIP_CHECK(hipMemcpyAsync(buf.p, v.data(), v.size() * 4, hipMemcpyHostToDevice, ctx->stream));
}

void ensure_rope(ltx_ctx* ctx, DualStack* m, int F, int H, int W, int Ta) {
    const DualBlockConfig& c = m->cfg;
    const bool video = !(m->rope_F == F && m->rope_H == H && m->rope_W == W && m->rope_v_cos.p);
    const bool audio = !(m->rope_Ta == Ta && m->rope_a_cos.p);
    if (!video && !audio) return;
    std::vector<float> vc, vs, cvc, cvs, ac, as, cac, cas;
    const int Ia = m->Da;  // audio inner dim = audioCrossAttentionDim: the width of both cross-modal tables (LTX2Transformer.swift:210-233)
    if (video) {
        TransformerConfig tc;
        tc.num_heads = c.video_heads;
        tc.head_dim = 128;
        tc.rope_theta = c.rope_theta;
        for (int i = 0; i < 3; ++i) tc.max_pos[i] = c.max_pos[i];
        rope_tables(tc, F, H, W, c.fps, &vc, &vs);
        const std::vector<float> pos = video_temporal_positions(F, H, W, c.fps);
        rope_tables_positions(pos.data(), (int)pos.size(), Ia, (double)c.rope_theta, c.audio_max_pos, &cvc, &cvs);
        upload(ctx, m->rope_v_cos, vc);
        upload(ctx, m->rope_v_sin, vs);
        upload(ctx, m->rope_cv_cos, cvc);
        upload(ctx, m->rope_cv_sin, cvs);
    }
    if (audio) {
        const std::vector<float> pos = audio_positions(Ta);
        rope_tables_positions(pos.data(), Ta, Ia, (double)c.rope_theta, c.audio_max_pos, &ac, &as);
        rope_tables_positions(pos.data(), Ta, Ia, (double)c.rope_theta, c.audio_max_pos, &cac, &cas);
        upload(ctx, m->rope_a_cos, ac);
        upload(ctx, m->rope_a_sin, as);
        upload(ctx, m->rope_ca_cos, cac);
        upload(ctx, m->rope_ca_sin, cas);
    }
    HIP_CHECK(hipStreamSynchronize(ctx->stream));  // the host vectors go out of scope
    if (video) {
        m->rope_F = F;
        m->rope_H = H;
        m->rope_W = W;
    }
    if (audio) m->rope_Ta = Ta;
}

// adaLN / FFN phase of one stream (phases 7 and 8): x += gate * ff2(gelu(ff1(norm(x) * (1 + scale) + shift)))
void ffn_phase(float* x, int D, int T, long rows, const float* mod, long mod_bs, const int32_t* rmap, const LinearW& ff1, const LinearW& ff2,
               bf16_t* xn, bf16_t* ffh, float eps, const SplitWs& sk, hipStream_t st) {
    NormModArgs n;
    n.x = x; n.ldx = D;
    n.scale = mod + 4L * D; n.shift = mod + 3L * D; n.mod_bstride = mod_bs; n.rows_per_batch = T; n.row_map = rmap;
    n.out = xn; n.ldo = D;
    n.rows = (int)rows; n.D = D; n.eps = eps;
    launch_norm_mod(n, st);
    GemmEpilogue e1;
    e1.out_bf16 = ffh;
    e1.ld_bf16 = 4L * D;
    e1.act = LTX_ACT_GELU_TANH;
    gemm_linear(xn, D, ff1, (int)rows, e1, st, sk);
    GemmEpilogue e2;
    e2.out_f32 = x;
    e2.ld_f32 = D;
    e2.resid = 1;
    e2.gate = mod + 5L * D;
    e2.gate_bstride = mod_bs;
    e2.rows_per_batch = T;
    e2.gate_rowmap = rmap;
    gemm_linear(ffh, 4L * D, ff2, (int)rows, e2, st, sk);
}

// where block l's four cached tensors start (elements of bf16)
struct TextCacheSlices {
    bf16_t *k_v, *vt_v, *k_a, *vt_a;
};
TextCacheSlices text_cache_slices(const DualTextCache& c, int l, int Dv, int Da) {
    const long B = c.B, S = c.S, Sp = c.Spad;
    const long kv = B * S * Dv, vv = B * Dv * Sp, ka = B * S * Da, va = B * Da * Sp;
    bf16_t* base = c.buf.as<bf16_t>() + (long)l * (kv + vv + ka + va);
    return {base, base + kv, base + kv + vv, base + kv + vv + ka};
}

}  // namespace

void dual_prepare_text(ltx_ctx* ctx, DualStack* m, const bf16_t* ctx_video, const bf16_t* ctx_audio, int B, int S) {
    const int L = m->L, Dv = m->Dv, Da = m->Da;
    if (B < 1 || B > 8 || S < 1 || S > (1 << 20)) LTX_THROW(LTXS_INVALID_CONFIGURATION, "dual prepare text: bad shapes B=%d (1 .. 8) S=%d", B, S);
    if (!ctx_video || !ctx_audio) LTX_THROW(LTXS_INVALID_CONFIGURATION, "dual prepare text: null context pointer");
    hipStream_t st = ctx->stream;
    DualTextCache& c = m->text_cache;
    const int Spad = ((S + 63) / 64) * 64;
    const long bytes = (long)L * B * (S + Spad) * (Dv + Da) * 2;
    m->attn_ws.kraw.ensure((size_t)B * S * std::max(Dv, Da) * 4);
    m->ws_splitk.ensure((size_t)8 << 22);
    const bool fresh = c.buf.ensure((size_t)bytes);
    if (fresh || c.B != B || c.S != S) HIP_CHECK(hipMemsetAsync(c.buf.p, 0, (size_t)bytes, st));  // the pad columns of V^T must be finite
    c.B = B; c.S = S; c.Spad = Spad; c.bytes = bytes;
    const SplitWs sk{m->ws_splitk.as<float>(), (long)(m->ws_splitk.bytes / 4)};
    for (int l = 0; l < L; ++l) {
        DualBlock& b = m->blocks[l];
        const TextCacheSlices t = text_cache_slices(c, l, Dv, Da);
        AttnCoreArgs k;  // what phases 3 and 4 hand attn_module_core for the key side
        k.kv_bf16 = 1; k.B = B; k.Tk = S;
        k.split_ws = sk.p; k.split_ws_elems = sk.elems;
        k.ctx = ctx_video;
        attn_module_build_kv(ctx, b.attn2, k, &m->attn_ws, t.k_v, t.vt_v);
        k.ctx = ctx_audio;
        attn_module_build_kv(ctx, b.audio_attn2, k, &m->attn_ws, t.k_a, t.vt_a);
    }
    c.builds++;
}

void dual_forward(ltx_ctx* ctx, DualStack* m, const DualForwardArgs& a) {
    // every check comes before the first launch and before any allocation
    const int L = m->L, Dv = m->Dv, Da = m->Da, B = a.B, S = a.S, Ta = a.T_a;
    if (B < 1 || B > 8 || a.F < 1 || a.H < 1 || a.W < 1 || Ta < 1 || S < 1 || Ta > (1 << 20) || S > (1 << 20) || (long)a.F * a.H * a.W > (1 << 20))
        LTX_THROW(LTXS_INVALID_CONFIGURATION, "dual blocks forward: bad shapes B=%d (1 .. 8) F=%d H=%d W=%d T_a=%d S=%d", B, a.F, a.H, a.W, Ta, S);
    const DualTextCache* tc = a.text_cache;
    if (!a.x_video || !a.x_audio || (!tc && (!a.ctx_video || !a.ctx_audio)) || !a.temb_video || !a.temb_audio || !a.cross_video_ss || !a.cross_audio_ss)
        LTX_THROW(LTXS_INVALID_CONFIGURATION, "dual blocks forward: null stream, context or modulation pointer");
    if (tc && (tc->B != B || tc->S != S || !tc->buf.p))
        LTX_THROW(LTXS_INVALID_CONFIGURATION, "dual blocks forward: the text cache holds B=%d S=%d, the call has B=%d S=%d", tc->B, tc->S, B, S);
    if (a.phase_mask > 0xffu) LTX_THROW(LTXS_INVALID_CONFIGURATION, "dual blocks forward: phase_mask 0x%x has bits beyond the eight phases", a.phase_mask);
    const int G = a.n_groups;
    if (G < 1 || (long)B * G > 8 || (G > 1 && !a.video_row_map))
        LTX_THROW(LTXS_INVALID_CONFIGURATION, "dual blocks forward: n_groups=%d (B * n_groups = 1 .. 8; more than one group needs video_row_map)", G);
    const int32_t* rmap = a.video_row_map;  // null: one video modulation row per batch element
    const int BG = B * G;
    const unsigned phases = a.phase_mask ? a.phase_mask : 0xffu;
    auto on = [&](int p) { return (phases >> (p - 1)) & 1u; };
    const int Tv = a.F * a.H * a.W;
    const long vrows = (long)B * Tv, arows = (long)B * Ta;
    const float eps = m->cfg.norm_eps;
    hipStream_t st = ctx->stream;

    // scratch: grows to the largest shape seen
    {
        const DualBlock& b = m->blocks[0];  // every block has the same shapes: the V^T slots are shared by the blocks
        attn_core_reserve(b.attn1, &m->attn_ws, &m->vt[0], B, Tv, Tv);
        attn_core_reserve(b.audio_attn1, &m->attn_ws, &m->vt[1], B, Ta, Ta);
        attn_core_reserve(b.attn2, &m->attn_ws, &m->vt[2], B, Tv, S);
        attn_core_reserve(b.audio_attn2, &m->attn_ws, &m->vt[3], B, Ta, S);
        attn_core_reserve(b.a2v, &m->attn_ws, &m->vt[4], B, Tv, Ta);
        attn_core_reserve(b.v2a, &m->attn_ws, &m->vt[5], B, Ta, Tv);
        m->ws_vn.ensure((size_t)vrows * Dv * 2);
        m->ws_vn2.ensure((size_t)vrows * Dv * 2);
        m->ws_an.ensure((size_t)arows * Da * 2);
        m->ws_an2.ensure((size_t)arows * Da * 2);
        m->ws_ffh.ensure((size_t)std::max(vrows * 4 * Dv, arows * 4 * Da) * 2);
        m->ws_splitk.ensure((size_t)8 << 22);
        if (!a.bias_video || !a.bias_audio) m->zero_bias.ensure((size_t)B * S * 4, true);  // a growing buffer is zeroed again
        m->mod_v.ensure((size_t)BG * L * 6 * Dv * 4);
        m->mod_a.ensure((size_t)B * L * 6 * Da * 4);
        m->mod_ca_v.ensure((size_t)BG * L * 5 * Dv * 4);
        m->mod_ca_a.ensure((size_t)B * L * 5 * Da * 4);
    }
    ensure_rope(ctx, m, a.F, a.H, a.W, Ta);

    const SplitWs sk{m->ws_splitk.as<float>(), (long)(m->ws_splitk.bytes / 4)};
    bf16_t* vn = m->ws_vn.as<bf16_t>();
    bf16_t* vn2 = m->ws_vn2.as<bf16_t>();
    bf16_t* an = m->ws_an.as<bf16_t>();
    bf16_t* an2 = m->ws_an2.as<bf16_t>();
    bf16_t* ffh = m->ws_ffh.as<bf16_t>();
    float* xv = a.x_video;
    float* xa = a.x_audio;
    const float* bias_v = a.bias_video ? a.bias_video : m->zero_bias.as<float>();  // null = all zeros, bit for bit
    const float* bias_a = a.bias_audio ? a.bias_audio : m->zero_bias.as<float>();

    // mod[b][l][j][:] = table[l][j][:] + rows[b][j][:] for every block at once (the reference adds them per block: :182,195,229,230);
    // the video rows once per (batch element, timestep group), picked per token through the row map
    launch_make_mod(m->sst_v, a.temb_video, m->mod_v.as<float>(), BG, L, 6, Dv, st);
    launch_make_mod(m->sst_a, a.temb_audio, m->mod_a.as<float>(), B, L, 6, Da, st);
    launch_make_mod(m->sst_ca_v, a.cross_video_ss, m->mod_ca_v.as<float>(), BG, L, 5, Dv, st);
    launch_make_mod(m->sst_ca_a, a.cross_audio_ss, m->mod_ca_a.as<float>(), B, L, 5, Da, st);
    const long mv_bs = (long)L * 6 * Dv, ma_bs = (long)L * 6 * Da, cv_bs = (long)L * 5 * Dv, ca_bs = (long)L * 5 * Da;

    auto core = [&](AttnModule* mod, AttnVtSlot* vt, const bf16_t* xq, const bf16_t* cx, int kvb, int Tq, int Tk, const float* qc, const float* qs,
                    const float* kc, const float* ks, const float* bias, float* x, const float* gate, long gbs, const int32_t* gmap,
                    const bf16_t* ck = nullptr, const bf16_t* cvt = nullptr) {
        AttnCoreArgs c;
        c.cached_k = ck; c.cached_vt = cvt;
        c.xq = xq; c.ctx = cx; c.kv_bf16 = kvb;
        c.B = B; c.Tq = Tq; c.Tk = Tk;
        c.q_cos = qc; c.q_sin = qs; c.k_cos = kc; c.k_sin = ks;
        c.key_bias = bias;
        c.x = x; c.gate = gate; c.gate_bstride = gbs; c.gate_rowmap = gmap;
        c.split_ws = sk.p; c.split_ws_elems = sk.elems;
        attn_module_core(ctx, mod, c, &m->attn_ws, vt);
    };
    const float* rvc = m->rope_v_cos.as<float>();
    const float* rvs = m->rope_v_sin.as<float>();
    const float* rac = m->rope_a_cos.as<float>();
    const float* ras = m->rope_a_sin.as<float>();
    const float* cvc = m->rope_cv_cos.as<float>();
    const float* cvs = m->rope_cv_sin.as<float>();
    const float* cac = m->rope_ca_cos.as<float>();
    const float* cas = m->rope_ca_sin.as<float>();

    // the RMS norm (+ modulation) passes of the two streams: a launch sets its scale / shift rows, their batch stride and its output
    NormModArgs nv, na;
    nv.x = xv; nv.ldx = nv.ldo = Dv; nv.rows_per_batch = Tv; nv.rows = (int)vrows; nv.D = Dv; nv.eps = eps;
    nv.row_map = rmap;
    na.x = xa; na.ldx = na.ldo = Da; na.rows_per_batch = Ta; na.rows = (int)arows; na.D = Da; na.eps = eps;
    auto norm = [st](NormModArgs n, const float* scale, const float* shift, long mod_bs, bf16_t* out) {
        n.scale = scale; n.shift = shift; n.mod_bstride = mod_bs; n.out = out;
        launch_norm_mod(n, st);
    };

    for (int l = 0; l < L; ++l) {
        DualBlock& b = m->blocks[l];
        const TextCacheSlices tcs = tc ? text_cache_slices(*tc, l, Dv, Da) : TextCacheSlices{nullptr, nullptr, nullptr, nullptr};
        const float* mv = m->mod_v.as<float>() + (long)l * 6 * Dv;     // rows: 0 shift_msa 1 scale_msa 2 gate_msa 3 shift_mlp 4 scale_mlp 5 gate_mlp
        const float* ma = m->mod_a.as<float>() + (long)l * 6 * Da;
        const float* cv = m->mod_ca_v.as<float>() + (long)l * 5 * Dv;  // rows: 0 a2v scale 1 a2v shift 2 v2a scale 3 v2a shift 4 gate
        const float* ca = m->mod_ca_a.as<float>() + (long)l * 5 * Da;
        if (on(1)) {  // video self-attention
            norm(nv, mv + 1L * Dv, mv, mv_bs, vn);
            core(b.attn1, &m->vt[0], vn, nullptr, 0, Tv, Tv, rvc, rvs, nullptr, nullptr, nullptr, xv, mv + 2L * Dv, mv_bs, rmap);
        }
        if (on(2)) {  // audio self-attention
            norm(na, ma + 1L * Da, ma, ma_bs, an);
            core(b.audio_attn1, &m->vt[1], an, nullptr, 0, Ta, Ta, rac, ras, nullptr, nullptr, nullptr, xa, ma + 2L * Da, ma_bs, nullptr);
        }
        if (on(3)) {  // video text cross-attention on norm2(x_v)
            norm(nv, nullptr, nullptr, 0, vn);
            core(b.attn2, &m->vt[2], vn, a.ctx_video, 1, Tv, S, nullptr, nullptr, nullptr, nullptr, bias_v, xv, nullptr, 0, nullptr, tcs.k_v, tcs.vt_v);
        }
        if (on(4)) {  // audio text cross-attention on audio_norm2(x_a)
            norm(na, nullptr, nullptr, 0, an);
            core(b.audio_attn2, &m->vt[3], an, a.ctx_audio, 1, Ta, S, nullptr, nullptr, nullptr, nullptr, bias_a, xa, nullptr, 0, nullptr, tcs.k_a, tcs.vt_a);
        }
        if (on(5) || on(6)) {
            // normVCA / normACA once, before either update; vn / an: the a2v operands, vn2 / an2: the v2a operands
            if (m->use_norm_mod2) {
                NormMod2Job jv, ja;
                jv.x = xv; jv.ldx = Dv; jv.scale0 = cv; jv.shift0 = cv + 1L * Dv; jv.scale1 = cv + 2L * Dv; jv.shift1 = cv + 3L * Dv;
                jv.mod_bstride = cv_bs; jv.rows_per_batch = Tv; jv.out0 = vn; jv.out1 = vn2; jv.ldo = Dv; jv.rows = (int)vrows; jv.D = Dv; jv.row_map = rmap;
                ja.x = xa; ja.ldx = Da; ja.scale0 = ca; ja.shift0 = ca + 1L * Da; ja.scale1 = ca + 2L * Da; ja.shift1 = ca + 3L * Da;
                ja.mod_bstride = ca_bs; ja.rows_per_batch = Ta; ja.out0 = an; ja.out1 = an2; ja.ldo = Da; ja.rows = (int)arows; ja.D = Da;
                launch_norm_mod2(jv, ja, eps, st);
            } else {
                norm(nv, cv, cv + 1L * Dv, cv_bs, vn);
                norm(nv, cv + 2L * Dv, cv + 3L * Dv, cv_bs, vn2);
                norm(na, ca, ca + 1L * Da, ca_bs, an);
                norm(na, ca + 2L * Da, ca + 3L * Da, ca_bs, an2);
            }
            if (on(5)) core(b.a2v, &m->vt[4], vn, an, 0, Tv, Ta, cvc, cvs, cac, cas, nullptr, xv, cv + 4L * Dv, cv_bs, rmap);
            if (on(6)) core(b.v2a, &m->vt[5], an2, vn2, 0, Ta, Tv, cac, cas, cvc, cvs, nullptr, xa, ca + 4L * Da, ca_bs, nullptr);
        }
        if (on(7)) ffn_phase(xv, Dv, Tv, vrows, mv, mv_bs, rmap, b.ff1, b.ff2, vn, ffh, eps, sk, st);
        if (on(8)) ffn_phase(xa, Da, Ta, arows, ma, ma_bs, nullptr, b.aff1, b.aff2, an, ffh, eps, sk, st);
    }
}
