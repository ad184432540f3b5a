// gemma_generate.cpp - Gemma-3 token generation on a KV cache (gemma.h, second half): session, prefill, step, generate loop and
// the host sampler. Reference: Gemma3TextModel.generateTokens (Gemma3Model.swift:375-492), Gemma3Attention's cache: path (:73-110).
// The prefill is gemma_encode's layer loop (gemma_run_layers) writing K / V^T into the cache; the step is one query row through
// gemv_bf16_kernel (gemm.hip), the existing row passes with rows = 1 and attn256_decode_kernel (attention.hip): 10 launches per layer.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <numeric>

#include "attention.h"
#include "elementwise.h"
#include "gemm.h"
#include "gemma.h"
#include "hostmath.h"
#include "linear_ops.h"
#include "options.h"

namespace {
struct StepRows {  // GemmaLm::sb carved
    bf16_t *x[2], *xn, *qk, *ao, *r, *h, *ff, *fin;
};
size_t step_rows_elems(const GemmaConfig& c) { return (size_t)6 * c.hidden + (size_t)(2 * c.heads + c.kv_heads) * 256 + c.intermediate; }
StepRows step_rows(const GemmaModel* m) {
    const GemmaConfig& c = m->cfg;
    const int H = c.hidden, Dq = c.heads * 256, Dk = c.kv_heads * 256;
    StepRows s;
    bf16_t* p = m->lm->sb.as<bf16_t>();
    s.x[0] = p; p += H;
    s.x[1] = p; p += H;
    s.xn = p; p += H;
    s.qk = p; p += Dq + Dk;
    s.ao = p; p += Dq;
    s.r = p; p += H;
    s.h = p; p += H;
    s.ff = p; p += c.intermediate;
    s.fin = p;
    return s;
}
GemmaLm* need_session(GemmaModel* m, const char* who) {
    if (!m->lm) LTX_THROW(LTXS_INVALID_CONFIGURATION, "%s: no generation session (ltx_lm_begin)", who);
    return m->lm;
}

// one Linear of the step at M = 1. Option "lm_gemm" sends it through the few-row GEMM instead (the measurement baseline: one row padded
// to a 128-row tile); the GeGLU then runs as its own pass over a [2I] row.
void step_linear(const GemmaModel* m, const bf16_t* x, const LinearW& w, int epilogue, bf16_t* out, float* out_f32, bf16_t* gu_scratch, hipStream_t st) {
    const int N = epilogue == GEMV_EPI_GEGLU ? w.out / 2 : w.out;
    if (ltx_opt(OPT_LM_GEMM)) {
        GemmEpilogue e;
        if (epilogue == GEMV_EPI_F32) {
            e.out_f32 = out_f32; e.ld_f32 = w.out; e.round_bf16 = 1;
        } else {
            e.out_bf16 = epilogue == GEMV_EPI_GEGLU ? gu_scratch : out; e.ld_bf16 = w.out;
        }
        gemm_linear(x, w.in, w, 1, e, st);
        if (epilogue == GEMV_EPI_GEGLU) {
            GegluArgs ga;
            ga.gu = gu_scratch; ga.ldgu = w.out; ga.out = out; ga.ldo = N; ga.rows = 1; ga.I = N;
            launch_geglu(ga, st);
        }
        return;
    }
    GemvBf16Args g;
    g.x = x; g.W = w.w; g.ldw = w.in; g.N = N; g.K = w.in; g.epilogue = epilogue; g.out_bf16 = out; g.out_f32 = out_f32;
    launch_gemv_bf16(g, st);
}

void logits_of_fin(ltx_ctx* ctx, GemmaModel* m) {  // the tied embedding as lm_head (:378-379, :433, :487)
    LinearW head;
    head.w = m->embed; head.out = m->cfg.vocab; head.in = m->cfg.hidden;
    step_linear(m, step_rows(m).fin, head, GEMV_EPI_F32, nullptr, m->lm->logits.as<float>(), nullptr, ctx->stream);
}
}  // namespace

void gemma_lm_begin(ltx_ctx* ctx, GemmaModel* m, int cap) {
    const GemmaConfig& c = m->cfg;
    LTX_REQUIRE(cap >= 1 && cap <= (1 << 20), "lm_begin: capacity %d out of range (1 .. 2^20)", cap);
    LTX_REQUIRE(c.heads / c.kv_heads <= 4, "lm_begin: %d query heads per K/V head (the decode attention takes up to 4)", c.heads / c.kv_heads);
    LTX_REQUIRE(c.hidden <= 16384 && c.intermediate <= 16384 && c.heads * 256 <= 16384, "lm_begin: a Linear's input width above 16384");
    gemma_lm_end(ctx, m);
    GemmaLm* lm = new GemmaLm();
    try {
        const size_t Dk = (size_t)c.kv_heads * 256, L = c.layers;
        lm->cap = cap;
        lm->ldvt = ((long)cap + 63) / 64 * 64;
        lm->kc.ensure(L * cap * Dk * 2);
        lm->vt.ensure(L * Dk * lm->ldvt * 2, true);
        const size_t tab = (size_t)cap * 128;
        lm->rope.ensure(4 * tab * 4);
        float* r = lm->rope.as<float>();
        launch_gemma_rope_tables(r, r + tab, cap, c.rope_local_base, ctx->stream);
        launch_gemma_rope_tables(r + 2 * tab, r + 3 * tab, cap, c.rope_theta, ctx->stream);
        lm->hid.ensure((size_t)2 * std::min(cap, c.sliding_window) * c.hidden * 2);
        lm->sb.ensure(step_rows_elems(c) * 2 + (size_t)2 * c.intermediate * 2);  // + the [2I] row of the lm_gemm baseline
        lm->logits.ensure((size_t)c.vocab * 4);
        lm->hist.ensure(((size_t)cap + 2) * 4);
        lm->dec_ws.ensure((size_t)attn_decode_ws_bytes(c.heads, cap));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    } catch (...) {
        delete lm;
        throw;
    }
    m->lm = lm;
}

size_t gemma_lm_end(ltx_ctx* ctx, GemmaModel* m) {
    if (!m->lm) return 0;
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    const size_t n = m->lm->cache_bytes() + m->lm->workspace_bytes();
    delete m->lm;
    m->lm = nullptr;
    return n;
}

bf16_t* gemma_lm_state(GemmaModel* m) { return step_rows(m).fin; }

void gemma_lm_prefill(ltx_ctx* ctx, GemmaModel* m, const int32_t* ids, int T) {
    const GemmaConfig& c = m->cfg;
    GemmaLm* lm = need_session(m, "lm_prefill");
    LTX_REQUIRE(ids && T >= 1, "lm_prefill: null ids or an empty prompt");
    if (T > c.sliding_window)  // the prefill's window mask is not built, exactly as in gemma_encode
        LTX_THROW(LTXS_INVALID_CONFIGURATION, "lm_prefill: %d tokens exceed the sliding window %d", T, c.sliding_window);
    LTX_REQUIRE(T <= lm->cap, "lm_prefill: %d tokens exceed the session's capacity %d", T, lm->cap);
    hipStream_t st = ctx->stream;
    const size_t Dk = (size_t)c.kv_heads * 256;
    lm->len = 0;
    GemmaEmbedArgs em;
    em.ids = ids; em.table = m->embed; em.out = lm->hid.as<bf16_t>(); em.rows = T; em.D = c.hidden; em.vocab = c.vocab;
    em.scale = host_bf16_to_f32(host_f32_to_bf16(sqrtf((float)c.hidden)));
    launch_gemma_embed(em, st);
    GemmaStackRun s;
    s.B = 1; s.T = T;
    s.rope = lm->rope.as<float>(); s.tab = (size_t)lm->cap * 128;
    s.hidden = lm->hid.as<bf16_t>(); s.ping_pong = 1;
    s.kcache = lm->kc.as<bf16_t>(); s.k_stride = (size_t)lm->cap * Dk;
    s.vtcache = lm->vt.as<bf16_t>(); s.vt_stride = Dk * lm->ldvt; s.ldvt = lm->ldvt;
    s.final_out = step_rows(m).fin;
    gemma_run_layers(ctx, m, s);
    logits_of_fin(ctx, m);
    lm->len = T;
}

void gemma_lm_step(ltx_ctx* ctx, GemmaModel* m, const int32_t* token) {
    const GemmaConfig& c = m->cfg;
    GemmaLm* lm = need_session(m, "lm_step");
    LTX_REQUIRE(token, "lm_step: null token");
    LTX_REQUIRE(lm->len >= 1, "lm_step: the session holds no prompt (ltx_lm_prefill)");
    LTX_REQUIRE(lm->len < lm->cap, "lm_step: the cache is full (%d positions)", lm->cap);
    hipStream_t st = ctx->stream;
    const int H = c.hidden, L = c.layers, Dq = c.heads * 256, Dk = c.kv_heads * 256;
    const int pos = lm->len;
    const StepRows b = step_rows(m);
    const size_t tab = (size_t)lm->cap * 128;

    GemmaEmbedArgs em;
    em.ids = token; em.table = m->embed; em.out = b.x[0]; em.rows = 1; em.D = H; em.vocab = c.vocab;
    em.scale = host_bf16_to_f32(host_f32_to_bf16(sqrtf((float)H)));
    launch_gemma_embed(em, st);
    GemmaNormArgs n0;
    n0.r = b.x[0]; n0.ldr = H; n0.w = m->layers[0].in_norm; n0.h = b.xn; n0.ldh = H; n0.rows = 1; n0.D = H; n0.eps = c.rms_eps;
    launch_gemma_norm(n0, st);
    for (int l = 0; l < L; ++l) {
        const GemmaLayer& ly = m->layers[l];
        const bf16_t* x = b.x[l & 1];
        bf16_t* kc = lm->kc.as<bf16_t>() + (size_t)l * lm->cap * Dk;
        bf16_t* vt = lm->vt.as<bf16_t>() + (size_t)l * Dk * lm->ldvt;
        step_linear(m, b.xn, ly.qk, GEMV_EPI_BF16, b.qk, nullptr, nullptr, st);
        GemvBf16Args gv;  // V straight into cache column pos (the GEMM has no strided store: this one stays a gemv under "lm_gemm" too)
        gv.x = b.xn; gv.W = ly.v.w; gv.ldw = H; gv.N = Dk; gv.K = H; gv.out_bf16 = vt + pos; gv.out_stride = lm->ldvt;
        launch_gemv_bf16(gv, st);
        GemmaQkArgs qa;  // rows = 1, T = 1, tables advanced to position pos: q in place, k into cache row pos
        qa.job[0].x = b.qk; qa.job[0].ldx = Dq + Dk; qa.job[0].w = ly.qn; qa.job[0].out = b.qk; qa.job[0].ldo = Dq + Dk; qa.job[0].heads = c.heads;
        qa.job[1].x = b.qk + Dq; qa.job[1].ldx = Dq + Dk; qa.job[1].w = ly.kn; qa.job[1].out = kc + (size_t)pos * Dk; qa.job[1].ldo = Dk;
        qa.job[1].heads = c.kv_heads;
        const float* tb = lm->rope.as<float>() + (gemma_layer_is_global(c, l) ? 2 * tab : 0);
        qa.cos = tb + (size_t)pos * 128; qa.sin = tb + tab + (size_t)pos * 128; qa.T = 1; qa.rows = 1; qa.eps = c.rms_eps;
        launch_gemma_qknorm_rope(qa, st);
        AttnDecodeArgs at;  // all pos + 1 keys on every layer: mask .none on a KVCacheSimple (:481-484)
        at.q = b.qk; at.K = kc; at.ldk = Dk; at.Vt = vt; at.ldvt = lm->ldvt; at.O = b.ao;
        at.Hq = c.heads; at.Hkv = c.kv_heads; at.n_keys = pos + 1;
        at.scale = 1.0f / sqrtf(c.query_pre_attn_scalar);
        at.ws = lm->dec_ws.p; at.ws_bytes = (long)lm->dec_ws.bytes;
        launch_attention_decode(at, st);
        step_linear(m, b.ao, ly.o, GEMV_EPI_BF16, b.r, nullptr, nullptr, st);
        GemmaNormArgs n1;
        n1.r = b.r; n1.ldr = H; n1.w = ly.post_attn; n1.x = x; n1.ldx = H; n1.h = b.h; n1.ldh = H;
        n1.w2 = ly.pre_ff; n1.n = b.xn; n1.ldn = H; n1.rows = 1; n1.D = H; n1.eps = c.rms_eps;
        launch_gemma_norm(n1, st);
        step_linear(m, b.xn, ly.gu, GEMV_EPI_GEGLU, b.ff, nullptr, b.fin + H, st);
        step_linear(m, b.ff, ly.down, GEMV_EPI_BF16, b.r, nullptr, nullptr, st);
        GemmaNormArgs n2;
        n2.r = b.r; n2.ldr = H; n2.w = ly.post_ff; n2.x = b.h; n2.ldx = H; n2.rows = 1; n2.D = H; n2.eps = c.rms_eps;
        if (l + 1 < L) {
            n2.h = b.x[(l + 1) & 1]; n2.ldh = H;
            n2.w2 = m->layers[l + 1].in_norm; n2.n = b.xn; n2.ldn = H;
        } else {
            n2.n_only = 1;
            n2.w2 = m->final_norm; n2.n = b.fin; n2.ldn = H;
        }
        launch_gemma_norm(n2, st);
    }
    logits_of_fin(ctx, m);
    lm->len = pos + 1;
}

int gemma_lm_generate(ltx_ctx* ctx, GemmaModel* m, const int32_t* ids, int T, const GemmaLmParams& p, int32_t* out) {
    const GemmaConfig& c = m->cfg;
    GemmaLm* lm = need_session(m, "lm_generate");
    LTX_REQUIRE(ids && out && T >= 1, "lm_generate: null ids / out or an empty prompt");
    LTX_REQUIRE(p.max_new >= 0 && p.n_eos >= 0 && p.n_eos <= 8 && p.context >= 0, "lm_generate: max_new %d, %d stop ids (up to 8), context %d", p.max_new,
                p.n_eos, p.context);
    LTX_REQUIRE(p.penalty > 0.f && (p.temperature <= 0.f || (p.top_p > 0.f && p.top_p <= 1.f)), "lm_generate: penalty %g must be positive, top_p %g in (0, 1]",
                (double)p.penalty, (double)p.top_p);
    LTX_REQUIRE((long)T + p.max_new <= lm->cap, "lm_generate: %d prompt tokens + %d new exceed the session's capacity %d", T, p.max_new, lm->cap);
    if (T > c.sliding_window) LTX_THROW(LTXS_INVALID_CONFIGURATION, "lm_generate: %d tokens exceed the sliding window %d", T, c.sliding_window);
    for (int i = 0; i < T; ++i)
        LTX_REQUIRE(ids[i] >= 0 && ids[i] < c.vocab, "lm_generate: token id %d at position %d is outside the vocabulary of %d", ids[i], i, c.vocab);
    hipStream_t st = ctx->stream;
    const bool greedy = p.temperature <= 0.f;
    // everything the loop needs exists before it starts: the sampled path's host logits and the sampler's scratch too
    std::vector<float> host_logits(greedy ? 0 : c.vocab);
    LmSampleScratch scratch;
    if (!greedy) scratch.reserve(c.vocab);
    int32_t* hist = lm->hist.as<int32_t>();
    HIP_CHECK(hipMemcpyAsync(hist, ids, (size_t)T * 4, hipMemcpyHostToDevice, st));  // the prompt rides in the still unused history (T <= cap)
    gemma_lm_prefill(ctx, m, hist, T);
    int n = 0;
    while (n < p.max_new) {
        int32_t tok = 0;
        if (greedy) {
            LmPickArgs pk;
            pk.logits = lm->logits.as<float>(); pk.vocab = c.vocab; pk.hist = hist; pk.n_gen = n; pk.context = p.context; pk.penalty = p.penalty;
            pk.out = hist + lm->cap + 1;
            launch_lm_pick(pk, st);
            HIP_CHECK(hipMemcpyAsync(&tok, pk.out, 4, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
        } else {
            HIP_CHECK(hipMemcpyAsync(host_logits.data(), lm->logits.p, (size_t)c.vocab * 4, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            tok = lm_sample_host(host_logits.data(), c.vocab, out, n, p.context, p.penalty, p.temperature, p.top_p, p.seed, n, &scratch);
            HIP_CHECK(hipMemcpyAsync(hist + n, &tok, 4, hipMemcpyHostToDevice, st));
            HIP_CHECK(hipStreamSynchronize(st));  // tok is a stack variable
        }
        if (std::find(p.eos, p.eos + p.n_eos, tok) != p.eos + p.n_eos) break;
        out[n++] = tok;
        if (n == p.max_new) break;  // the reference runs one more step whose logits nobody reads (:476-488)
        gemma_lm_step(ctx, m, hist + n - 1);
    }
    return n;
}

int32_t lm_sample_host(float* logits, int vocab, const int32_t* generated, int n_generated, int context, float penalty, float temperature,
                       float top_p, uint64_t seed, int step, LmSampleScratch* scratch) {
    const int n_recent = std::min(context, n_generated);
    if (penalty != 1.0f && n_recent > 0) {
        const int32_t* recent = generated + (n_generated - n_recent);
        for (int t = 0; t < n_recent; ++t) {
            const int id = recent[t];
            if (id < 0 || id >= vocab || std::find(recent, recent + t, id) != recent + t) continue;  // each distinct id once
            logits[id] = logits[id] > 0.f ? logits[id] / penalty : logits[id] * penalty;
        }
    }
    int best = 0;
    for (int i = 1; i < vocab; ++i)
        if (logits[i] > logits[best]) best = i;
    if (temperature <= 0.f) return best;
    const double lmax = (double)logits[best] / (double)temperature;
    LmSampleScratch local;  // a stand-alone call brings none: allocated here, once per call
    if (!scratch) scratch = &local;
    scratch->reserve(vocab);
    std::vector<double>& w = scratch->w;
    std::vector<int32_t>& order = scratch->order;
    double Z = 0.0;
    for (int i = 0; i < vocab; ++i) {
        w[i] = exp((double)logits[i] / (double)temperature - lmax);
        Z += w[i];
    }
    std::iota(order.begin(), order.end(), 0);
    auto before = [&](int32_t a, int32_t b) { return w[a] > w[b] || (w[a] == w[b] && a < b); };
    // the nucleus is usually a handful of tokens: sort a prefix of 64, and grow it fourfold while its mass stays short of top_p
    const double want = (double)top_p * Z;
    int sorted = 0, n_nuc = 0;
    double mass = 0.0;
    while (n_nuc == 0) {
        const int upto = sorted == 0 ? std::min(vocab, 64) : std::min(vocab, sorted * 4);
        std::partial_sort(order.begin() + sorted, order.begin() + upto, order.end(), before);
        for (int j = sorted; j < upto && n_nuc == 0; ++j) {
            mass += w[order[j]];
            if (mass >= want) n_nuc = j + 1;
        }
        sorted = upto;
        if (sorted == vocab && n_nuc == 0) n_nuc = vocab;  // rounding kept the whole mass below top_p * Z
    }
    uint32_t key[2], out[2];
    const uint32_t ctr[2] = {0, 0};
    mlx_draw_key(seed, step, key);
    threefry2x32(key, ctr, out);
    const double u = (double)(out[0] >> 8) * (1.0 / 16777216.0);
    const double target = u * mass;  // mass: the nucleus's, summed in its order
    double cum = 0.0;
    for (int j = 0; j < n_nuc; ++j) {
        cum += w[order[j]];
        if (cum > target) return order[j];
    }
    return order[n_nuc - 1];
}
