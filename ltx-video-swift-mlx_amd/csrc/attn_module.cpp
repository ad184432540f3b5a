// attn_module.cpp - see attn_module.h.
#include "attn_module.h"

#include <vector>

#include "attention.h"
#include "elementwise.h"
#include "gemm.h"
#include "linear_ops.h"

namespace {
// the file's spelling of a module key (ModelDownloader.swift:756-803 maps the other way)
std::string file_spelling(const std::string& key) {
    if (key.compare(0, 7, "to_out.") == 0) return "to_out.0." + key.substr(7);
    if (key.compare(0, 7, "q_norm.") == 0) return "norm_q." + key.substr(7);
    if (key.compare(0, 7, "k_norm.") == 0) return "norm_k." + key.substr(7);
    return key;
}
const StTensor* find_tensor(const SafeTensors& st, const std::string& prefix, const std::string& key) {
    auto it = st.tensors.find(prefix + key);
    if (it == st.tensors.end()) it = st.tensors.find(prefix + file_spelling(key));
    return it == st.tensors.end() ? nullptr : &it->second;
}
}  // namespace

AttnModule* attn_module_create(int query_dim, int context_dim, int heads) { return attn_module_create_ex(query_dim, context_dim, heads, 64, false, false); }

AttnModule* attn_module_create_ex(int query_dim, int context_dim, int heads, int head_dim, bool fused_qk, bool split_weights) {
    if (heads < 1 || heads > 128 || query_dim < 64 || context_dim < 64 || query_dim % 64 != 0 || context_dim % 64 != 0 || query_dim > 8192 ||
        context_dim > 8192)
        LTX_THROW(LTXS_INVALID_CONFIGURATION, "attention module: query_dim %d / context_dim %d must be multiples of 64 up to 8192, heads %d in 1 .. 128",
                  query_dim, context_dim, heads);
    if ((head_dim != 64 && head_dim != 128) || (long)heads * head_dim > 8192 || (fused_qk && context_dim != query_dim))
        LTX_THROW(LTXS_INVALID_CONFIGURATION, "attention module: head dim %d (64 or 128), inner dim up to 8192, fused q|k only for self-attention", head_dim);
    AttnModule* m = new AttnModule();
    m->heads = heads;
    m->head_dim = head_dim;
    m->fused_qk = fused_qk;
    m->inner = heads * head_dim;
    m->Dq = query_dim;
    m->Dc = context_dim;
    const long I = m->inner, Dq = query_dim, Dc = context_dim;
    m->q.out = m->k.out = m->v.out = (int)I;
    m->q.in = (int)Dq;
    m->k.in = m->v.in = (int)Dc;
    m->o.out = (int)Dq;
    m->o.in = (int)I;
    try {
        ParamTable& pt = m->params;
        if (fused_qk) {
            // to_k directly behind to_q, weights and biases (every size here is a multiple of the arena's 256-byte grain)
            pt.add("to_q.weight", (void**)&m->q.w, SLOT_BF16, I, Dq);
            pt.add("to_k.weight", (void**)&m->k.w, SLOT_BF16, I, Dc);
            pt.add("to_q.bias", (void**)&m->q.b, SLOT_F32, I, 0);
            pt.add("to_k.bias", (void**)&m->k.b, SLOT_F32, I, 0);
        } else {
            pt.add_linear("to_q", m->q, (int)I, (int)Dq);
            pt.add_linear("to_k", m->k, (int)I, (int)Dc);
        }
        pt.add_linear("to_v", m->v, (int)I, (int)Dc);
        pt.add_linear("to_out", m->o, (int)Dq, (int)I);
        pt.add("q_norm.weight", (void**)&m->qn, SLOT_F32, I, 0);
        pt.add("k_norm.weight", (void**)&m->kn, SLOT_F32, I, 0);
        pt.place(split_weights);  // true: the bf16 weights in params.warena, which a quantising owner releases
        if (fused_qk && (m->k.w != m->q.w + I * Dq || m->k.b != m->q.b + I))
            LTX_THROW(LTXS_GENERATION_FAILED, "attention module: the fused q|k rows are not contiguous");
    } catch (...) {
        delete m;
        throw;
    }
    return m;
}

void attn_module_destroy(AttnModule* m) { delete m; }

void attn_module_init_synthetic(ltx_ctx* ctx, AttnModule* m, uint64_t seed) {
    // Linear weights N(0, 0.02^2), biases N(0, 0.01^2), q / k norm weights 1 + N(0, 0.02^2)
    param_table_fill_synthetic(ctx, m->params, seed, 0, param_fill_rule_default);
}

void attn_module_file_shape(const std::string& path, const std::string& prefix, int* query_dim, int* context_dim, int* inner) {
    SafeTensors st;
    st.open(path);
    const StTensor* wq = find_tensor(st, prefix, "to_q.weight");
    const StTensor* wk = find_tensor(st, prefix, "to_k.weight");
    if (!wq || !wk || wq->shape.size() != 2 || wk->shape.size() != 2)
        LTX_THROW(LTXS_WEIGHT_LOADING_FAILED, "Failed to load weights: no attention module under '%s' in %s", prefix.c_str(), path.c_str());
    if (wq->shape[0] != wk->shape[0] || wq->shape[0] > 8192 || wq->shape[1] > 8192 || wk->shape[1] > 8192)
        LTX_THROW(LTXS_WEIGHT_LOADING_FAILED, "Failed to load weights: %sto_q [%ld, %ld] and to_k [%ld, %ld] do not form one module", prefix.c_str(),
                  wq->shape[0], wq->shape[1], wk->shape[0], wk->shape[1]);
    *inner = (int)wq->shape[0];
    *query_dim = (int)wq->shape[1];
    *context_dim = (int)wk->shape[1];
}

void attn_module_load(ltx_ctx* ctx, AttnModule* m, const std::string& path, const std::string& prefix) {
    SafeTensors st;
    st.open(path);
    ctx->n_loaded = ctx->n_missing = ctx->n_unmatched = 0;
    std::vector<uint8_t> staging;
    for (auto& kv : m->params.slots) {
        ParamSlot& s = kv.second;
        s.loaded = false;
        const StTensor* t = find_tensor(st, prefix, kv.first);
        if (!t) LTX_THROW(LTXS_WEIGHT_LOADING_FAILED, "Failed to load weights: %s%s is not in %s", prefix.c_str(), kv.first.c_str(), path.c_str());
        param_check_shape(prefix + kv.first, *t, s);
        param_upload(st, *t, s, &staging);
        s.loaded = true;
        ctx->n_loaded++;
    }
}

void attn_module_forward(ltx_ctx* ctx, AttnModule* m, const AttnModuleArgs& a) {
    // every check comes before the first launch
    if (!a.x || !a.out || a.B < 1 || a.Tq < 1 || a.Tk < 1 || a.B > 64 || a.Tq > (1 << 20) || a.Tk > (1 << 20))
        LTX_THROW(LTXS_INVALID_CONFIGURATION, "attention module: bad arguments (B=%d Tq=%d Tk=%d)", a.B, a.Tq, a.Tk);
    if (!a.context && (a.Tk != a.Tq || m->Dc != m->Dq || a.context_bf16))
        LTX_THROW(LTXS_INVALID_CONFIGURATION, "attention module: self-attention needs Tk == Tq (%d, %d), context_dim == query_dim (%d, %d) and f32 rows",
                  a.Tk, a.Tq, m->Dc, m->Dq);
    if ((a.q_cos == nullptr) != (a.q_sin == nullptr) || (a.k_cos == nullptr) != (a.k_sin == nullptr) || (a.k_cos && !a.q_cos))
        LTX_THROW(LTXS_INVALID_CONFIGURATION, "attention module: cos and sin tables come in pairs, and key tables only with query tables");
    if (a.q_cos && a.q_rows < a.Tq)
        LTX_THROW(LTXS_INVALID_CONFIGURATION, "attention module: the query RoPE tables have %d rows for Tq = %d", a.q_rows, a.Tq);
    if (a.q_cos && (a.k_cos ? a.k_rows : a.q_rows) < a.Tk)
        LTX_THROW(LTXS_INVALID_CONFIGURATION, "attention module: the key RoPE tables have %d rows for Tk = %d", a.k_cos ? a.k_rows : a.q_rows, a.Tk);

    hipStream_t st = ctx->stream;
    const int I = m->inner, Dq = m->Dq, Dc = m->Dc, B = a.B, Tq = a.Tq, Tk = a.Tk;
    const long qrows = (long)B * Tq, krows = (long)B * Tk;
    const int Tpad = ((Tk + 63) / 64) * 64;
    const bool kb = a.context_bf16 != 0;  // bf16 context: k leaves its projection in bf16
    bool grew = false;
    grew |= m->ws_xb.ensure((size_t)qrows * Dq * 2);
    if (a.context && !kb) grew |= m->ws_cb.ensure((size_t)krows * Dc * 2);
    grew |= m->ws_qraw.ensure((size_t)qrows * I * 4);
    grew |= m->ws_kraw.ensure((size_t)krows * I * 4);
    grew |= m->ws_q.ensure((size_t)qrows * I * 2);
    grew |= m->ws_k.ensure((size_t)krows * I * 2);
    grew |= m->ws_vt.ensure((size_t)B * I * Tpad * 2, true);  // zeroed: the pad columns of V^T must be finite
    grew |= m->ws_ao.ensure((size_t)qrows * I * 2);
    (void)grew;

    bf16_t* xb = m->ws_xb.as<bf16_t>();
    launch_cast_f32_bf16(a.x, xb, qrows * Dq, st);
    const bf16_t* cb = xb;
    if (a.context) {
        if (kb) {
            cb = (const bf16_t*)a.context;
        } else {
            launch_cast_f32_bf16((const float*)a.context, m->ws_cb.as<bf16_t>(), krows * Dc, st);
            cb = m->ws_cb.as<bf16_t>();
        }
    }
    float* qraw = m->ws_qraw.as<float>();
    float* kraw = m->ws_kraw.as<float>();
    bf16_t* q = m->ws_q.as<bf16_t>();
    bf16_t* k = m->ws_k.as<bf16_t>();
    bf16_t* vt = m->ws_vt.as<bf16_t>();
    bf16_t* ao = m->ws_ao.as<bf16_t>();

    GemmEpilogue eq;
    eq.out_f32 = qraw;
    eq.ld_f32 = I;
    gemm_linear(xb, Dq, m->q, (int)qrows, eq, st);
    GemmEpilogue ek;
    if (kb) {
        ek.out_bf16 = (bf16_t*)kraw;
        ek.ld_bf16 = I;
    } else {
        ek.out_f32 = kraw;
        ek.ld_f32 = I;
    }
    gemm_linear(cb, Dc, m->k, (int)krows, ek, st);
    for (int b = 0; b < B; ++b) gemm_vt(cb + (size_t)b * Tk * Dc, Dc, Tk, m->v, vt + (size_t)b * I * Tpad, Tpad, st);

    // q and k come from different inputs, token counts and tables: two one-job launches
    QkNormRopeArgs n;
    n.job[0].x = qraw; n.job[0].w = m->qn; n.job[0].out = q; n.job[0].out_scale = kAttnQueryPrescale64;
    n.ldx = n.ldo = I;
    n.cos = a.q_cos; n.sin = a.q_sin;
    n.T = Tq; n.rows = (int)qrows; n.D = I; n.eps = m->eps; n.head_dim = 64;
    launch_qknorm_rope(n, st);
    n.job[0].x = kraw; n.job[0].w = m->kn; n.job[0].out = k; n.job[0].out_scale = 1.0f;
    n.cos = a.q_cos ? (a.k_cos ? a.k_cos : a.q_cos) : nullptr; n.sin = a.q_cos ? (a.k_cos ? a.k_sin : a.q_sin) : nullptr;
    n.T = Tk; n.rows = (int)krows; n.x_bf16 = kb;
    launch_qknorm_rope(n, st);

    AttnArgs at;
    at.head_dim = 64;
    at.Q = q; at.ldq = I; at.q_bstride = (long)Tq * I;
    at.K = k; at.ldk = I; at.k_bstride = (long)Tk * I;
    at.Vt = vt; at.ldvt = Tpad; at.vt_bstride = (long)I * Tpad;
    at.O = ao; at.ldo = I; at.o_bstride = (long)Tq * I;
    at.bias = a.key_bias; at.bias_bstride = Tk;
    at.B = B; at.H = m->heads; at.Tq = Tq; at.Tk = Tk;
    at.scale = 0.125f;
    at.q_prescaled = 1;
    launch_attention(at, st);

    GemmEpilogue eo;
    eo.out_f32 = a.out;
    eo.ld_f32 = Dq;
    gemm_linear(ao, I, m->o, (int)qrows, eo, st);
}

void attn_core_reserve(const AttnModule* m, AttnCoreScratch* ws, AttnVtSlot* vt, int B, int Tq, int Tk) {
    const long I = m->inner, qrows = (long)B * Tq, krows = (long)B * Tk;
    const int Tpad = ((Tk + 63) / 64) * 64;
    ws->qraw.ensure((size_t)qrows * I * 4 * (m->fused_qk ? 2 : 1));
    ws->kraw.ensure((size_t)krows * I * 4);
    ws->q.ensure((size_t)qrows * I * 2);
    ws->k.ensure((size_t)krows * I * 2);
    ws->ao.ensure((size_t)qrows * I * 2);
    if (m->head_dim == 128) {
        const long need = attn_split_ws_bytes(B, m->heads, Tq, Tk);
        if (need > 0) ws->attn_split.ensure((size_t)need);
    }
    if (vt->buf.ensure((size_t)B * I * Tpad * 2)) vt->inner = vt->Tpad = vt->B = 0;  // new memory: zeroed by the first launch sequence
}

namespace {
// the key side of attn_module_core when q and k are separate projections: k GEMM, k norm + RoPE, V^T per batch element
void launch_k_gemm(AttnModule* m, const bf16_t* cb, bool kb, long krows, float* kraw, hipStream_t st, const SplitWs& sk) {
    GemmEpilogue ek;
    if (kb) {
        ek.out_bf16 = (bf16_t*)kraw;
        ek.ld_bf16 = m->inner;
    } else {
        ek.out_f32 = kraw;
        ek.ld_f32 = m->inner;
    }
    gemm_linear(cb, m->Dc, m->k, (int)krows, ek, st, sk);
}
void launch_k_norm(AttnModule* m, const float* kraw, const float* kc, const float* ks, int Tk, bf16_t* k, long krows, bool kb, hipStream_t st) {
    QkNormRopeArgs n;
    n.job[0].x = kraw; n.job[0].w = m->kn; n.job[0].out = k;
    n.ldx = n.ldo = m->inner;
    n.cos = kc; n.sin = ks;
    n.T = Tk; n.rows = (int)krows; n.D = m->inner; n.eps = m->eps; n.x_bf16 = kb; n.head_dim = m->head_dim;
    launch_qknorm_rope(n, st);
}
void launch_vt(AttnModule* m, const bf16_t* cb, int B, int Tk, int Tpad, bf16_t* vt, hipStream_t st, const SplitWs& sk) {
    for (int b = 0; b < B; ++b) gemm_vt(cb + (size_t)b * Tk * m->Dc, m->Dc, Tk, m->v, vt + (size_t)b * m->inner * Tpad, Tpad, st, sk);
}
}  // namespace

void attn_module_build_kv(ltx_ctx* ctx, AttnModule* m, const AttnCoreArgs& a, AttnCoreScratch* ws, bf16_t* k_out, bf16_t* vt_out) {
    hipStream_t st = ctx->stream;
    const long krows = (long)a.B * a.Tk;
    const int Tpad = ((a.Tk + 63) / 64) * 64;
    const SplitWs sk{a.split_ws, a.split_ws_elems};
    const bool kb = a.kv_bf16 != 0;
    const float* kc = a.q_cos ? (a.k_cos ? a.k_cos : a.q_cos) : nullptr;
    const float* ks = a.q_cos ? (a.k_cos ? a.k_sin : a.q_sin) : nullptr;
    float* kraw = ws->kraw.as<float>();
    launch_k_gemm(m, a.ctx, kb, krows, kraw, st, sk);
    launch_k_norm(m, kraw, kc, ks, a.Tk, k_out, krows, kb, st);
    launch_vt(m, a.ctx, a.B, a.Tk, Tpad, vt_out, st, sk);
}

void attn_module_core(ltx_ctx* ctx, AttnModule* m, const AttnCoreArgs& a, AttnCoreScratch* ws, AttnVtSlot* vs) {
    hipStream_t st = ctx->stream;
    const int I = m->inner, Dq = m->Dq, Dc = m->Dc, B = a.B, Tq = a.Tq, Tk = a.Tk, hd = m->head_dim;
    const long qrows = (long)B * Tq, krows = (long)B * Tk;
    const int Tpad = ((Tk + 63) / 64) * 64;
    const SplitWs sk{a.split_ws, a.split_ws_elems};
    const bool cached = a.cached_k && a.cached_vt;
    if (!cached && (vs->inner != I || vs->Tpad != Tpad || vs->B != B)) {  // the pad columns of V^T must be finite
        HIP_CHECK(hipMemsetAsync(vs->buf.p, 0, (size_t)B * I * Tpad * 2, st));
        vs->inner = I;
        vs->Tpad = Tpad;
        vs->B = B;
    }
    const bf16_t* cb = a.ctx ? a.ctx : a.xq;
    const bool kb = a.kv_bf16 != 0;
    float* qraw = ws->qraw.as<float>();
    float* kraw = ws->kraw.as<float>();
    bf16_t* q = ws->q.as<bf16_t>();
    const bf16_t* k = cached ? a.cached_k : ws->k.as<bf16_t>();
    const bf16_t* vt = cached ? a.cached_vt : vs->buf.as<bf16_t>();
    bf16_t* ao = ws->ao.as<bf16_t>();
    const float qscale = hd == 64 ? kAttnQueryPrescale64 : kAttnQueryPrescale;
    const float* kc = a.q_cos ? (a.k_cos ? a.k_cos : a.q_cos) : nullptr;
    const float* ks = a.q_cos ? (a.k_cos ? a.k_sin : a.q_sin) : nullptr;

    QkNormRopeArgs qn;  // the query's pass; q | k of the same rows: k rides as a second job
    qn.job[0].x = qraw; qn.job[0].w = m->qn; qn.job[0].out = q; qn.job[0].out_scale = qscale;
    qn.ldx = qn.ldo = I;
    qn.cos = a.q_cos; qn.sin = a.q_sin;
    qn.T = Tq; qn.rows = (int)qrows; qn.D = I; qn.eps = m->eps; qn.head_dim = hd;
    if (m->fused_qk && !a.ctx) {
        // q | k of the same rows: one GEMM over the [2 inner][Dq] matrix, one norm + RoPE launch with two jobs
        LinearW qk = m->q;
        qk.out = 2 * I;
        GemmEpilogue e;
        e.out_f32 = qraw;
        e.ld_f32 = 2 * I;
        gemm_linear(a.xq, Dq, qk, (int)qrows, e, st, sk);
        qn.job[1].x = qraw + I; qn.job[1].w = m->kn; qn.job[1].out = ws->k.as<bf16_t>();
        qn.ldx = 2 * I;
        launch_qknorm_rope(qn, st);
    } else {
        GemmEpilogue eq;
        eq.out_f32 = qraw;
        eq.ld_f32 = I;
        gemm_linear(a.xq, Dq, m->q, (int)qrows, eq, st, sk);
        if (!cached) launch_k_gemm(m, cb, kb, krows, kraw, st, sk);
        // q and k come from different inputs, token counts and tables: two one-job launches
        launch_qknorm_rope(qn, st);
        if (!cached) launch_k_norm(m, kraw, kc, ks, Tk, ws->k.as<bf16_t>(), krows, kb, st);
    }
    if (!cached) launch_vt(m, cb, B, Tk, Tpad, vs->buf.as<bf16_t>(), st, sk);

    AttnArgs at;
    at.head_dim = hd;
    at.Q = q; at.ldq = I; at.q_bstride = (long)Tq * I;
    at.K = k; at.ldk = I; at.k_bstride = (long)Tk * I;
    at.Vt = vt; at.ldvt = Tpad; at.vt_bstride = (long)I * Tpad;
    at.O = ao; at.ldo = I; at.o_bstride = (long)Tq * I;
    at.bias = a.key_bias; at.bias_bstride = Tk;
    at.B = B; at.H = m->heads; at.Tq = Tq; at.Tk = Tk;
    if (hd == 64) at.scale = 0.125f;
    at.q_prescaled = 1;
    if (hd == 128) {
        at.split_ws = ws->attn_split.p;
        at.split_ws_bytes = (long)ws->attn_split.bytes;
    }
    launch_attention(at, st);

    GemmEpilogue eo;
    eo.out_f32 = a.x;
    eo.ld_f32 = Dq;
    eo.resid = 1;
    eo.gate = a.gate;
    eo.gate_bstride = a.gate_bstride;
    eo.gate_rowmap = a.gate_rowmap;
    eo.rows_per_batch = Tq;
    gemm_linear(ao, I, m->o, (int)qrows, eo, st, sk);
}
