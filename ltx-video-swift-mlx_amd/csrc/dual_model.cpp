// dual_model.cpp - see dual_model.h. One forward = LTX2Transformer.callAsFunction (LTX2Transformer.swift:254-392).
#include "dual_model.h"

#include <string.h>

#include <algorithm>
#include <vector>

#include "elementwise.h"
#include "gemm.h"
#include "linear_ops.h"

namespace {

// offsets (in floats) of embedder j's [M][D] rows inside ws_h1 / ws_h2; a video embedder has Mv rows (one per batch element and
// timestep group), an audio embedder Ma (one per batch element)
long stage_offset(const DualModel* m, int j, int Mv, int Ma) {
    long off = 0;
    for (int i = 0; i < j; ++i) off += m->emb[i].audio ? (long)Ma * m->Da : (long)Mv * m->Dv;
    return off;
}

void ensure_embed_scratch(DualModel* m, int Mv, int Ma) {
    m->ws_emb256.ensure((size_t)(Mv + Ma) * 256 * 4);
    const size_t stage = (size_t)stage_offset(m, kDualEmbedders, Mv, Ma) * 4;
    m->ws_h1.ensure(stage);
    m->ws_h2.ensure(stage);
}

// The timestep path (LTX2Transformer.swift:272-312). No check and no allocation in here: the callers have done both.
// video_ts [Mv], audio_ts [Ma]. Mv == Ma: every stage is one grouped launch of six jobs. Mv != Ma (timestep groups): a grouped launch
// shares one M, so every stage is two - the three video embedders at Mv rows, the three audio embedders at Ma.
void embed_launches(ltx_ctx* ctx, DualModel* m, const float* video_ts, const float* audio_ts, int Mv, int Ma, int mode, const DualEmbedOut& o) {
    hipStream_t st = ctx->stream;
    const int Dv = m->Dv, Da = m->Da;
    const bool ungrouped = mode != 0;
    float* emb_v = m->ws_emb256.as<float>();
    float* emb_a = emb_v + (long)Mv * 256;
    launch_timestep_embedding(video_ts, m->cfg.timestep_scale_multiplier, emb_v, Mv, 256, st);
    launch_timestep_embedding(audio_ts, m->cfg.timestep_scale_multiplier, emb_a, Ma, 256, st);
    // stage 3 destinations: the four modulation tensors; the gate embedders write row 4 of the 5-row tensors
    float* dst3[kDualEmbedders] = {o.temb_v, o.temb_a, o.cross_v, o.cross_v + 4L * Dv, o.cross_a, o.cross_a + 4L * Da};
    const long ldo3[kDualEmbedders] = {6L * Dv, 6L * Da, 5L * Dv, 5L * Dv, 5L * Da, 5L * Da};
    // one table of the 18 Linears; the weights stay LinearW so that a bf16 and a quantised model fill the job type their kernel takes
    struct Job {
        const float* a; long lda; const LinearW* w; float* out; long ldo; int in_act;
    };
    Job s1[kDualEmbedders], s2[kDualEmbedders], s3[kDualEmbedders];
    for (int j = 0; j < kDualEmbedders; ++j) {
        const DualEmbedder& e = m->emb[j];
        const int D = e.audio ? Da : Dv;
        float* h1 = m->ws_h1.as<float>() + stage_offset(m, j, Mv, Ma);
        // the stage-2 outputs of adaln_single / audio_adaln_single are the embedded timesteps
        float* h2 = j == 0 ? o.embts_v : j == 1 ? o.embts_a : m->ws_h2.as<float>() + stage_offset(m, j, Mv, Ma);
        s1[j] = {e.audio ? emb_a : emb_v, 256, &e.l1, h1, D, LTX_ACT_NONE};
        s2[j] = {h1, D, &e.l2, h2, D, LTX_ACT_SILU};
        s3[j] = {h2, D, &e.lin, dst3[j], ldo3[j], LTX_ACT_SILU};
    }
    const bool quant = m->quant_bits != 16;
    // n jobs of one M in one launch: launch_gemv_group on bf16 weights, launch_gemv_group_q on codes
    auto group = [&](const Job* jobs, int n, int M) {
        if (quant) {
            GemvJobQ q[kDualEmbedders];
            for (int i = 0; i < n; ++i) {
                const Job& t = jobs[i];
                q[i].a = t.a; q[i].lda = t.lda; q[i].codes = t.w->q; q[i].scales = t.w->qs; q[i].biases = t.w->qb; q[i].bias = t.w->b;
                q[i].out = t.out; q[i].ldo = t.ldo; q[i].N = t.w->out; q[i].K = t.w->in; q[i].in_act = t.in_act;
            }
            launch_gemv_group_q(q, n, M, m->quant_bits, st);
            return;
        }
        GemvJob g[kDualEmbedders];
        for (int i = 0; i < n; ++i) {
            const Job& t = jobs[i];
            g[i].a = t.a; g[i].lda = t.lda; g[i].W = t.w->w; g[i].ldw = t.w->in; g[i].bias = t.w->b;
            g[i].out = t.out; g[i].ldo = t.ldo; g[i].N = t.w->out; g[i].K = t.w->in; g[i].in_act = t.in_act;
        }
        launch_gemv_group(g, n, M, st);
    };
    if (!ungrouped && Mv == Ma) {
        group(s1, kDualEmbedders, Mv);
        group(s2, kDualEmbedders, Mv);
        group(s3, kDualEmbedders, Mv);
        return;
    }
    if (!ungrouped) {
        for (const Job* s : {s1, s2, s3}) {
            Job v[kDualEmbedders], a[kDualEmbedders];
            int nv = 0, na = 0;
            for (int j = 0; j < kDualEmbedders; ++j) (m->emb[j].audio ? a[na++] : v[nv++]) = s[j];
            group(v, nv, Mv);
            group(a, na, Ma);
        }
        return;
    }
    for (const Job* s : {s1, s2, s3})
        for (int j = 0; j < kDualEmbedders; ++j) {
            const Job& t = s[j];
            const int M = m->emb[j].audio ? Ma : Mv;
            if (quant && mode != 2) {
                group(&t, 1, M);  // the same kernel, one job per launch
                continue;
            }
            // bf16 weights, or (mode 2) the composed alternative on codes: de-quantise into the scratch matrix in front of the gemv
            launch_gemv_f32(t.a, t.lda, dit_linear_weights(*t.w, st), t.w->in, t.w->b, t.out, t.ldo, M, t.w->out, t.w->in, t.in_act, st);
        }
}

// PixArtAlphaTextProjection of one context (LTX2Transformer.swift:275,282): Linear, GELU-tanh, Linear; the hidden activation goes
// through ws_cap_h (dual_model.h, rounding point 3)
void caption_launches(DualModel* m, const bf16_t* context, const LinearW& l1, const LinearW& l2, int D, long crows, bf16_t* out, hipStream_t st,
                      const SplitWs& sk) {
    GemmEpilogue e1;
    e1.out_bf16 = m->ws_cap_h.as<bf16_t>();
    e1.ld_bf16 = D;
    e1.act = LTX_ACT_GELU_TANH;
    gemm_linear(context, m->cfg.caption_channels, l1, (int)crows, e1, st, sk);
    GemmEpilogue e2;
    e2.out_bf16 = out;
    e2.ld_bf16 = D;
    gemm_linear(m->ws_cap_h.as<bf16_t>(), D, l2, (int)crows, e2, st, sk);
}

}  // namespace

DualModel::~DualModel() {
    if (stack) dual_destroy(stack);
}

DualModel* dual_model_create(const DualModelConfig& cfg) {
    const DualBlockConfig& bc = cfg.blocks;
    if (bc.video_context_dim != bc.video_dim || bc.audio_context_dim != bc.audio_dim)
        LTX_THROW(LTXS_INVALID_CONFIGURATION, "dual model: context dims %d / %d must equal the stream dims %d / %d (the caption projections' widths)",
                  bc.video_context_dim, bc.audio_context_dim, bc.video_dim, bc.audio_dim);
    for (int c : {cfg.in_channels, cfg.out_channels, cfg.audio_in_channels, cfg.audio_out_channels, cfg.caption_channels})
        if (c < 64 || c > 16384 || c % 64 != 0)
            LTX_THROW(LTXS_INVALID_CONFIGURATION, "dual model: channel count %d must be a multiple of 64 up to 16384", c);
    if (!(cfg.timestep_scale_multiplier > 0.f)) LTX_THROW(LTXS_INVALID_CONFIGURATION, "dual model: timestep_scale_multiplier must be positive");
    DualModel* m = new DualModel();
    try {
        m->stack = dual_create(bc);  // validates the block config
        m->cfg = cfg;
        const int Dv = m->Dv = bc.video_dim, Da = m->Da = bc.audio_dim;
        ParamTable& pt = m->params;
        pt.add_linear("patchify_proj", m->patchify, Dv, cfg.in_channels);
        pt.add_linear("audio_patchify_proj", m->audio_patchify, Da, cfg.audio_in_channels);
        const struct { const char* name; int n; bool audio; } embs[kDualEmbedders] = {
            {"adaln_single", 6, false},
            {"audio_adaln_single", 6, true},
            {"av_ca_video_scale_shift_adaln_single", 4, false},
            {"av_ca_a2v_gate_adaln_single", 1, false},
            {"av_ca_audio_scale_shift_adaln_single", 4, true},
            {"av_ca_v2a_gate_adaln_single", 1, true}};
        for (int j = 0; j < kDualEmbedders; ++j) {
            DualEmbedder& e = m->emb[j];
            e.name = embs[j].name;
            e.n = embs[j].n;
            e.audio = embs[j].audio;
            const int D = e.audio ? Da : Dv;
            pt.add_linear(std::string(e.name) + ".emb.linear_1", e.l1, D, 256);
            pt.add_linear(std::string(e.name) + ".emb.linear_2", e.l2, D, D);
            pt.add_linear(std::string(e.name) + ".linear", e.lin, e.n * D, D);
        }
        pt.add_linear("caption_projection.linear_1", m->cap1, Dv, cfg.caption_channels);
        pt.add_linear("caption_projection.linear_2", m->cap2, Dv, Dv);
        pt.add_linear("audio_caption_projection.linear_1", m->acap1, Da, cfg.caption_channels);
        pt.add_linear("audio_caption_projection.linear_2", m->acap2, Da, Da);
        pt.add("scale_shift_table", (void**)&m->sst_out_v, SLOT_F32, 2, Dv);
        pt.add("audio_scale_shift_table", (void**)&m->sst_out_a, SLOT_F32, 2, Da);
        pt.add_linear("proj_out", m->proj_out, cfg.out_channels, Dv);
        pt.add_linear("audio_proj_out", m->audio_proj_out, cfg.audio_out_channels, Da);
        pt.place(true);
    } catch (...) {
        delete m;
        throw;
    }
    return m;
}

void dual_model_destroy(DualModel* m) { delete m; }

void dual_model_init_synthetic(ltx_ctx* ctx, DualModel* m, uint64_t seed) {
    dual_init_synthetic(ctx, m->stack, seed);
    // the stack's distributions: Linear weights N(0, 0.02^2), biases N(0, 0.01^2), tables N(0, 0.02^2); bf16 values. A stream of seeds of
    // its own (the stack counts its slots from 1)
    param_table_fill_synthetic(ctx, m->params, seed, 1u << 20, param_fill_rule_default);
}

void dual_model_load(ltx_ctx* ctx, DualModel* m, const std::string& path) {
    dual_load(ctx, m->stack, path, 0);  // the blocks; starts the load report; throws on a missing block parameter
    SafeTensors st;
    st.open(path);
    // a file that holds two spellings of one parameter (proj_in.weight and patchify_proj.weight) is accepted, the later key in
    // map order wins and the parameter counts once: the reference's mapped dictionary behaves the same way
    const std::string first_missing = param_table_load(
        ctx, m->params, st,
        [](const std::string& fk, std::string* mk) {
            if (fk.compare(0, 19, "transformer_blocks.") == 0) return false;  // dual_load has seen it
            *mk = transformer_module_spelling(fk);
            return true;
        },
        true);
    if (!first_missing.empty())
        LTX_THROW(LTXS_WEIGHT_LOADING_FAILED, "Failed to load weights: %s and %d more are not in %s", first_missing.c_str(), ctx->n_missing - 1,
                  path.c_str());
}

void dual_model_quantize(ltx_ctx* ctx, DualModel* m, int bits, int group) {
    quantize_check_request(bits, group, m->quant_bits);
    std::vector<LinearW*> lins = {&m->patchify, &m->audio_patchify, &m->cap1, &m->cap2, &m->acap1, &m->acap2, &m->proj_out, &m->audio_proj_out};
    for (DualEmbedder& e : m->emb)
        for (LinearW* l : {&e.l1, &e.l2, &e.lin}) lins.push_back(l);
    DualStack* s = m->stack;
    std::vector<ParamTable*> tables = {&m->params, &s->params};  // the stack's table holds copies of its modules' slots: both are re-pointed
    std::vector<AttnModule*> fused;
    for (DualBlock& b : s->blocks) {
        for (AttnModule* a : {b.attn1, b.attn2, b.audio_attn1, b.audio_attn2, b.a2v, b.v2a}) {
            tables.push_back(&a->params);
            lins.push_back(&a->q);
            if (a->fused_qk)
                fused.push_back(a);  // to_k is rows [inner, 2 inner) of to_q's matrix
            else
                lins.push_back(&a->k);
            lins.push_back(&a->v);
            lins.push_back(&a->o);
        }
        for (LinearW* l : {&b.ff1, &b.ff2, &b.aff1, &b.aff2}) lins.push_back(l);
    }
    // the fused [2 inner][Dq] matrix is quantised as ONE Linear; its `out` says inner again afterwards, whatever happens in between
    for (AttnModule* a : fused) a->q.out = 2 * a->inner;
    try {
        quantize_linears(ctx, lins, tables, m->qarena, m->dq, bits);
    } catch (...) {
        for (AttnModule* a : fused) a->q.out = a->inner;
        throw;
    }
    for (AttnModule* a : fused) {
        a->q.out = a->inner;
        const long off = (long)a->inner * a->Dq;  // elements: whole rows, whole groups
        a->k.q = a->q.q + off * bits / 8;
        a->k.qs = a->q.qs + off / 64;
        a->k.qb = a->q.qb + off / 64;
        a->k.qbits = bits;
        a->k.dq = a->q.dq;
        a->k.w = nullptr;
    }
    m->quant_bits = bits;
    // K / V^T of the text cache came from the bf16 weights: the next cached forward needs dual_model_prepare_text again
    DualTextCache& tc = s->text_cache;
    tc.buf.release();
    tc.B = tc.S = tc.Spad = 0;
    tc.bytes = 0;
}

void dual_model_memory_info(const DualModel* m, long* bf16_weights, long* quantised, long* scratch, long* other) {
    size_t w = 0, o = 0;
    auto table = [&](const ParamTable& t) {
        w += t.warena.buf.p ? t.warena.buf.bytes : 0;
        o += t.arena.buf.p ? t.arena.buf.bytes : 0;
    };
    table(m->params);
    table(m->stack->params);
    for (const DualBlock& b : m->stack->blocks)
        for (const AttnModule* a : {b.attn1, b.attn2, b.audio_attn1, b.audio_attn2, b.a2v, b.v2a}) table(a->params);
    o += m->stack->text_cache.buf.p ? m->stack->text_cache.buf.bytes : 0;
    if (bf16_weights) *bf16_weights = (long)w;
    if (quantised) *quantised = m->qarena.buf.p ? (long)m->qarena.buf.bytes : 0;
    if (scratch) *scratch = m->dq.buf.p ? (long)m->dq.buf.bytes : 0;
    if (other) *other = (long)o;
}

const ParamSlot* dual_model_find(const DualModel* m, const std::string& name) {
    const ParamSlot* s = m->params.find(name);
    return s ? s : m->stack->params.find(name);
}

void dual_model_embed(ltx_ctx* ctx, DualModel* m, const float* video_ts, const float* audio_ts, int B, int ungrouped, const DualEmbedOut& o) {
    if (B < 1 || B > 8) LTX_THROW(LTXS_INVALID_CONFIGURATION, "dual model embed: B=%d (1 .. 8)", B);
    if (!video_ts || !audio_ts || !o.temb_v || !o.temb_a || !o.cross_v || !o.cross_a || !o.embts_v || !o.embts_a)
        LTX_THROW(LTXS_INVALID_CONFIGURATION, "dual model embed: null timestep or output pointer");
    ensure_embed_scratch(m, B, B);
    embed_launches(ctx, m, video_ts, audio_ts, B, B, ungrouped, o);
}

void dual_model_forward(ltx_ctx* ctx, DualModel* m, const DualModelForwardArgs& a) {
    // every check comes before the first launch and before any allocation; the shape rules are dual_forward's, so that it cannot refuse
    // the call after the launches in front of it
    const int Dv = m->Dv, Da = m->Da, B = a.B, S = a.S, Ta = a.T_a;
    if (B < 1 || B > 8 || a.F < 1 || a.H < 1 || a.W < 1 || Ta < 1 || S < 1 || Ta > (1 << 20) || S > (1 << 20) || (long)a.F * a.H * a.W > (1 << 20))
        LTX_THROW(LTXS_INVALID_CONFIGURATION, "dual model forward: bad shapes B=%d (1 .. 8) F=%d H=%d W=%d T_a=%d S=%d", B, a.F, a.H, a.W, Ta, S);
    const int G = a.n_groups;
    if (G < 1 || (long)B * G > 8 || (G > 1 && !a.video_row_map))
        LTX_THROW(LTXS_INVALID_CONFIGURATION, "dual model forward: n_groups=%d (B * n_groups = 1 .. 8; more than one group needs video_row_map)", G);
    const int BG = B * G;
    const bool cached = a.text_cache != 0;
    if (!a.video_latent || !a.audio_latent || (!cached && (!a.video_context || !a.audio_context)) || !a.video_timesteps || !a.audio_timesteps ||
        !a.video_velocity || !a.audio_velocity)
        LTX_THROW(LTXS_INVALID_CONFIGURATION, "dual model forward: null latent, context, timestep or velocity pointer");
    const DualTextCache& tc = m->stack->text_cache;
    if (cached && (tc.B != B || tc.S != S || !tc.buf.p))
        LTX_THROW(LTXS_INVALID_CONFIGURATION, "dual model forward: text_cache needs dual_model_prepare_text at B=%d S=%d (the cache holds B=%d S=%d)", B,
                  S, tc.B, tc.S);
    const int Tv = a.F * a.H * a.W;
    const long vrows = (long)B * Tv, arows = (long)B * Ta, crows = (long)B * S;
    const float eps = m->cfg.blocks.norm_eps;
    hipStream_t st = ctx->stream;

    // scratch: grows to the largest shape seen
    m->ws_xv.ensure((size_t)vrows * Dv * 4);
    m->ws_xa.ensure((size_t)arows * Da * 4);
    if (!cached) {
        m->ws_ctx_v.ensure((size_t)crows * Dv * 2);
        m->ws_ctx_a.ensure((size_t)crows * Da * 2);
        m->ws_cap_h.ensure((size_t)crows * std::max(Dv, Da) * 2);  // shared by both caption projections; audio_dim may exceed video_dim
        if (a.video_mask) m->ws_bias_v.ensure((size_t)crows * 4);
        if (a.audio_mask) m->ws_bias_a.ensure((size_t)crows * 4);
    }
    ensure_embed_scratch(m, BG, B);
    m->ws_temb_v.ensure((size_t)BG * 6 * Dv * 4);
    m->ws_temb_a.ensure((size_t)B * 6 * Da * 4);
    m->ws_cross_v.ensure((size_t)BG * 5 * Dv * 4);
    m->ws_cross_a.ensure((size_t)B * 5 * Da * 4);
    m->ws_modout_v.ensure((size_t)BG * 2 * Dv * 4);
    m->ws_modout_a.ensure((size_t)B * 2 * Da * 4);
    m->ws_xn.ensure((size_t)std::max(vrows * Dv, arows * Da) * 2);
    m->ws_splitk.ensure((size_t)8 << 22);
    const SplitWs sk{m->ws_splitk.as<float>(), (long)(m->ws_splitk.bytes / 4)};
    float* xv = m->ws_xv.as<float>();
    float* xa = m->ws_xa.as<float>();

    // 1. patchify (LTX2Transformer.swift:271,278): the streams start as the bf16 value of the projection (dual_model.h, rounding point 1)
    {
        GemmEpilogue e;
        e.out_f32 = xv;
        e.ld_f32 = Dv;
        e.round_bf16 = 1;
        gemm_linear(a.video_latent, m->cfg.in_channels, m->patchify, (int)vrows, e, st, sk);
        e.out_f32 = xa;
        e.ld_f32 = Da;
        gemm_linear(a.audio_latent, m->cfg.audio_in_channels, m->audio_patchify, (int)arows, e, st, sk);
    }
    // 2. timestep path (:272-312). The embedded timesteps live in the first two [B][D] blocks of ws_h2.
    DualEmbedOut eo;
    eo.temb_v = m->ws_temb_v.as<float>();
    eo.temb_a = m->ws_temb_a.as<float>();
    eo.cross_v = m->ws_cross_v.as<float>();
    eo.cross_a = m->ws_cross_a.as<float>();
    eo.embts_v = m->ws_h2.as<float>() + stage_offset(m, 0, BG, B);
    eo.embts_a = m->ws_h2.as<float>() + stage_offset(m, 1, BG, B);
    embed_launches(ctx, m, a.video_timesteps, a.audio_timesteps, BG, B, a.ungrouped, eo);
    // 3. text (:275,282,315-316); a cached forward reads what dual_model_prepare_text left
    if (!cached) {
        caption_launches(m, a.video_context, m->cap1, m->cap2, Dv, crows, m->ws_ctx_v.as<bf16_t>(), st, sk);
        caption_launches(m, a.audio_context, m->acap1, m->acap2, Da, crows, m->ws_ctx_a.as<bf16_t>(), st, sk);
        if (a.video_mask) launch_mask_to_bias(a.video_mask, m->ws_bias_v.as<float>(), crows, st);
        if (a.audio_mask) launch_mask_to_bias(a.audio_mask, m->ws_bias_a.as<float>(), crows, st);
    }
    // 4. the blocks (:361-372)
    DualForwardArgs f;
    f.x_video = xv;
    f.x_audio = xa;
    if (cached) {
        f.text_cache = &tc;
        f.bias_video = m->tc_has_bias_v ? m->tc_bias_v.as<float>() : nullptr;
        f.bias_audio = m->tc_has_bias_a ? m->tc_bias_a.as<float>() : nullptr;
    } else {
        f.ctx_video = m->ws_ctx_v.as<bf16_t>();
        f.ctx_audio = m->ws_ctx_a.as<bf16_t>();
        f.bias_video = a.video_mask ? m->ws_bias_v.as<float>() : nullptr;
        f.bias_audio = a.audio_mask ? m->ws_bias_a.as<float>() : nullptr;
    }
    f.temb_video = eo.temb_v;
    f.temb_audio = eo.temb_a;
    f.cross_video_ss = eo.cross_v;
    f.cross_audio_ss = eo.cross_a;
    f.B = B; f.F = a.F; f.H = a.H; f.W = a.W; f.T_a = Ta; f.S = S;
    f.n_groups = G; f.video_row_map = a.video_row_map;
    dual_forward(ctx, m->stack, f);
    // 5. heads (:375-389): mod[b][j][:] = table[j][:] + embedded_ts[b][:], j = 0 shift, 1 scale - launch_make_mod with the table's two
    // rows as its "layers" and one row per batch element (video: per batch element and timestep group, picked through the row map)
    auto head = [&](const float* x, int D, int T, long rows, const float* table, const float* embts, int M, const int32_t* rmap, float* mod,
                    const LinearW& proj, float* out) {
        launch_make_mod(table, embts, mod, M, 2, 1, D, st);
        NormModArgs n;
        n.x = x; n.ldx = D;
        n.scale = mod + D; n.shift = mod; n.mod_bstride = 2L * D; n.rows_per_batch = T; n.row_map = rmap;
        n.out = m->ws_xn.as<bf16_t>(); n.ldo = D;
        n.rows = (int)rows; n.D = D; n.norm_kind = LTX_NORM_LAYER; n.eps = eps;
        launch_norm_mod(n, st);
        GemmEpilogue e;
        e.out_f32 = out;
        e.ld_f32 = proj.out;
        gemm_linear(m->ws_xn.as<bf16_t>(), D, proj, (int)rows, e, st, sk);
    };
    head(xv, Dv, Tv, vrows, m->sst_out_v, eo.embts_v, BG, a.video_row_map, m->ws_modout_v.as<float>(), m->proj_out, a.video_velocity);
    head(xa, Da, Ta, arows, m->sst_out_a, eo.embts_a, B, nullptr, m->ws_modout_a.as<float>(), m->audio_proj_out, a.audio_velocity);
}

void dual_model_prepare_text(ltx_ctx* ctx, DualModel* m, const bf16_t* video_context, const bf16_t* audio_context, const int32_t* video_mask,
                             const int32_t* audio_mask, int B, int S) {
    // the checks of dual_prepare_text, before any launch or allocation
    if (B < 1 || B > 8 || S < 1 || S > (1 << 20)) LTX_THROW(LTXS_INVALID_CONFIGURATION, "dual model prepare text: bad shapes B=%d (1 .. 8) S=%d", B, S);
    if (!video_context || !audio_context) LTX_THROW(LTXS_INVALID_CONFIGURATION, "dual model prepare text: null context pointer");
    const int Dv = m->Dv, Da = m->Da;
    const long crows = (long)B * S;
    hipStream_t st = ctx->stream;
    m->tc_ctx_v.ensure((size_t)crows * Dv * 2);
    m->tc_ctx_a.ensure((size_t)crows * Da * 2);
    m->ws_cap_h.ensure((size_t)crows * std::max(Dv, Da) * 2);
    if (video_mask) m->tc_bias_v.ensure((size_t)crows * 4);
    if (audio_mask) m->tc_bias_a.ensure((size_t)crows * 4);
    m->ws_splitk.ensure((size_t)8 << 22);
    const SplitWs sk{m->ws_splitk.as<float>(), (long)(m->ws_splitk.bytes / 4)};
    caption_launches(m, video_context, m->cap1, m->cap2, Dv, crows, m->tc_ctx_v.as<bf16_t>(), st, sk);
    caption_launches(m, audio_context, m->acap1, m->acap2, Da, crows, m->tc_ctx_a.as<bf16_t>(), st, sk);
    if (video_mask) launch_mask_to_bias(video_mask, m->tc_bias_v.as<float>(), crows, st);
    if (audio_mask) launch_mask_to_bias(audio_mask, m->tc_bias_a.as<float>(), crows, st);
    m->tc_has_bias_v = video_mask != nullptr;
    m->tc_has_bias_a = audio_mask != nullptr;
    dual_prepare_text(ctx, m->stack, m->tc_ctx_v.as<bf16_t>(), m->tc_ctx_a.as<bf16_t>(), B, S);
}
