// abi_hooks.cpp - extern "C" surface of libltxhip.so (include/ltxhip.h), part 3 of 3: what tests, tools and the bench use to reach
// below the models - the ltx_op_* kernel hooks, the ltx_prof_* timers, the device fills and the parameter export. No product code
// path goes through this file.
#include <vector>

#include "abi_internal.h"
#include "attention.h"
#include "audio.h"
#include "elementwise.h"
#include "gemm.h"
#include "hostmath.h"
#include "linear_ops.h"
#include "noise.h"

namespace {

// the context-owned workspace that the hooks lend a launcher, as the model graphs lend theirs
void op_workspace(ltx_ctx* ctx, size_t bytes) {
    if (ctx->op_ws.ensure(bytes)) HIP_CHECK(hipStreamSynchronize(ctx->stream));
}

// Zero-haloed, channels-last operand of the audio conv hooks, built in ctx->audio_op[0]: `lines` lines of `width` rows (Cin bf16
// each) of x land at row first + l * pitch of a buffer of `total` rows, every other row is zero. Returns row 0 of the buffer.
const bf16_t* audio_halo_operand(ltx_ctx* ctx, const uint16_t* x, int Cin, int lines, int width, int pitch, size_t first, size_t total) {
    const size_t row = (size_t)Cin * 2;
    ctx->audio_op[0].ensure(total * row);
    char* base = ctx->audio_op[0].as<char>();
    if (pitch == width) {  // one contiguous signal: only the two halos need zeroing
        HIP_CHECK(hipMemsetAsync(base, 0, first * row, ctx->stream));
        const size_t end = first + (size_t)lines * width;
        HIP_CHECK(hipMemsetAsync(base + end * row, 0, (total - end) * row, ctx->stream));
        HIP_CHECK(hipMemcpyAsync(base + first * row, x, (size_t)lines * width * row, hipMemcpyDeviceToDevice, ctx->stream));
    } else {
        HIP_CHECK(hipMemsetAsync(base, 0, total * row, ctx->stream));
        HIP_CHECK(hipMemcpy2DAsync(base + first * row, pitch * row, x, width * row, width * row, lines, hipMemcpyDeviceToDevice, ctx->stream));
    }
    return (const bf16_t*)base;
}

void audio_op_epilogue(AConvArgs& a, const float* resid, int f32_act, int transposed, float* out_f32, long rows_out, int bf16_act,
                       float slope, uint16_t* out_bf16) {
    a.resid = resid;
    a.out_f32 = out_f32;
    a.f32_act = f32_act;
    a.f32_transposed = transposed ? 1 : 0;
    a.ldo = transposed ? rows_out : a.Cout;
    a.out_bf16 = out_bf16;
    a.ldb = a.Cout;
    a.bf16_act = bf16_act;
    a.slope = slope;
}

}  // namespace

extern "C" {

long ltx_dit_export_param(ltx_ctx* ctx, const char* module_key, float* out, long cap) {
    return export_param_body(
        ctx, "ltx_dit_export_param", module_key, out, cap, [&] { return need(ctx->dit, kNoDit)->params.find(module_key); },
        [&](const ParamSlot& s, float* o) { dit_export_slot(ctx, ctx->dit, s, o); });
}

int ltx_prof_enable(ltx_ctx* ctx, int on) {
    return with_ctx(ctx, [&] {
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        ctx->prof.collect();
        ctx->prof.on = on != 0;
    });
}

int ltx_prof_collect(ltx_ctx* ctx, int kind, double* total_ms, long* launches, double* work, int reset) {
    if (!ctx || kind < 0 || kind >= PROF_NKINDS) return LTX_ERR_INVALID_CONFIGURATION;
    return guarded(ctx, [&] {
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        ctx->prof.collect();
        if (total_ms) *total_ms = ctx->prof.total_ms[kind];
        if (launches) *launches = ctx->prof.launches[kind];
        if (work) *work = ctx->prof.total_work[kind];
        if (reset) ctx->prof.reset();
    });
}

int ltx_op_fill_normal_bf16(ltx_ctx* ctx, uint16_t* p, long n, uint64_t seed, float mean, float stddev) {
    return with_ctx(ctx, [&] { launch_fill_normal_bf16(p, n, seed, mean, stddev, ctx->stream); });
}
int ltx_op_fill_normal_f32(ltx_ctx* ctx, float* p, long n, uint64_t seed, float mean, float stddev) {
    return with_ctx(ctx, [&] { launch_fill_normal_f32(p, n, seed, mean, stddev, 0, ctx->stream); });
}

// ---- MLX-compatible noise on the device (noise.h) ----
int ltx_op_mlx_normal_group(ltx_ctx* ctx, const ltx_noise_job* jobs, int n_jobs) {
    return with_ctx(ctx, [&] { launch_mlx_normal_group(jobs, n_jobs, ctx->stream); });
}
int ltx_mlx_random_normal_dev(ltx_ctx* ctx, uint64_t seed, int draw_index, float* out_dev, long n, float scale) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(draw_index >= 0, "ltx_mlx_random_normal_dev: draw_index=%d", draw_index);
        ltx_noise_job j;
        mlx_draw_key(seed, draw_index, j.key);
        j.dst = out_dev; j.n = n; j.scale = scale; j.raw_bits = 0;
        launch_mlx_normal_group(&j, 1, ctx->stream);
    });
}

// ---- GEMM ----
int ltx_op_gemm_bf16(ltx_ctx* ctx, const uint16_t* A, long lda, const uint16_t* B, long ldb, const float* bias, int M,
                     int N, int K, int act, int tile_cfg, float* out_f32, long ld_f32, uint16_t* out_bf16,
                     long ld_bf16) {
    return with_ctx(ctx, [&] {
        GemmArgs g;
        g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.M = M; g.N = N; g.K = K;
        g.ep.bias_n = bias;
        g.ep.act = act;
        g.ep.out_f32 = out_f32; g.ep.ld_f32 = ld_f32;
        g.ep.out_bf16 = out_bf16; g.ep.ld_bf16 = ld_bf16;
        if (tile_cfg >= 100) {  // S*100 + cfg: S-way split-K on a ring tile (workspace owned by the context)
            g.split_k = tile_cfg / 100;
            tile_cfg %= 100;
            op_workspace(ctx, (size_t)g.split_k * M * N * 4);
            g.split_ws = ctx->op_ws.as<float>();
            g.split_ws_elems = (long)(ctx->op_ws.bytes / 4);
        }
        if (tile_cfg < 0) launch_gemm_bf16(g, ctx->stream); else launch_gemm_bf16_cfg(g, tile_cfg, ctx->stream);
    });
}

int ltx_op_gemm_q8(ltx_ctx* ctx, const uint16_t* A, long lda, const uint8_t* codes, const uint16_t* scales, const uint16_t* biases,
                   const float* bias, int M, int N, int K, int split_k, int via_scratch, int tile_cfg, float* out_f32, long ld_f32) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(A && codes && scales && biases && out_f32 && split_k >= 1, "ltx_op_gemm_q8: null argument");
        LTX_REQUIRE(gemm_takes_codes(M, N, K), "ltx_op_gemm_q8: few-row launches only (M <= 256, K %% 64 == 0, K >= 256, N %% 4 == 0; M=%d N=%d K=%d)", M, N, K);
        GemmArgs g;
        g.A = A; g.lda = lda; g.ldb = K; g.M = M; g.N = N; g.K = K;
        g.ep.bias_n = bias;
        g.ep.out_f32 = out_f32; g.ep.ld_f32 = ld_f32;
        DevBuf scratch;
        if (via_scratch) {  // the path every other launch of a quantised Linear takes: codes -> bf16 scratch matrix -> the same kernel
            scratch.ensure((size_t)N * K * 2);
            launch_dequant(codes, scales, biases, N, K, 8, scratch.as<bf16_t>(), ctx->stream);
            g.B = scratch.as<bf16_t>();
        } else {
            g.Bq = codes; g.Bqs = scales; g.Bqb = biases;
        }
        if (split_k > 1) {
            g.split_k = split_k;
            op_workspace(ctx, (size_t)split_k * M * N * 4);
            g.split_ws = ctx->op_ws.as<float>();
        }
        LTX_REQUIRE(tile_cfg == 29 || (tile_cfg == 30 && gemm_fewrow_takes(M, N, K, split_k)), "ltx_op_gemm_q8: tile_cfg 29 (ring kernel) or 30 (few-row kernel: M <= 128, N %% 64 == 0, whole 256-wide macro-tiles of K per split)");
        launch_gemm_bf16_cfg(g, tile_cfg, ctx->stream);
        if (via_scratch) HIP_CHECK(hipStreamSynchronize(ctx->stream));
    });
}

int ltx_op_value_projection_t(ltx_ctx* ctx, const uint16_t* X, long ldx, int tokens, const uint16_t* W, const float* bias, int out_features,
                              int in_features, uint16_t* vt, long ldvt) {
    return with_ctx(ctx, [&] {
        LinearW w;
        w.w = (bf16_t*)W;
        w.b = (float*)bias;
        w.out = out_features;
        w.in = in_features;
        gemm_vt(X, ldx, tokens, w, vt, ldvt, ctx->stream);
    });
}

int ltx_op_qkv_projection(ltx_ctx* ctx, const uint16_t* X, long ldx, int rows, int rows_per_batch, const uint16_t* Wqk, const float* bqk,
                          const uint16_t* Wv, const float* bv, int D, int K, uint16_t* qk_out, long ld_qk, uint16_t* vt_out, long ldvt, int fused) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(X && Wqk && Wv && qk_out && vt_out && rows > 0 && rows_per_batch > 0 && rows % rows_per_batch == 0 && D > 0 && K > 0,
                    "ltx_op_qkv_projection: null argument or rows not a multiple of rows_per_batch");
        LinearW wqk, wv;
        wqk.w = (bf16_t*)Wqk;
        wqk.b = (float*)bqk;
        wqk.out = 2 * D;
        wv.w = (bf16_t*)Wv;
        wv.b = (float*)bv;
        wv.out = D;
        wqk.in = wv.in = K;
        gemm_qkv(X, ldx, rows, rows_per_batch, wqk, wv, qk_out, ld_qk, vt_out, ldvt, (long)D * ldvt, fused != 0, ctx->stream);
    });
}

int ltx_op_gemm_bf16_gated_residual(ltx_ctx* ctx, const uint16_t* A, long lda, const uint16_t* B, long ldb,
                                    const float* bias, const float* gate, float gate_scalar, int M, int N, int K,
                                    float* x, long ldx, uint16_t* mirror, long ld_mirror) {
    return with_ctx(ctx, [&] {
        GemmArgs g;
        g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.M = M; g.N = N; g.K = K;
        g.ep.bias_n = bias;
        g.ep.out_f32 = x; g.ep.ld_f32 = ldx;
        g.ep.resid = 1;
        g.ep.gate = gate; g.ep.gate_bstride = 0; g.ep.rows_per_batch = M; g.ep.gate_scalar = gate_scalar;
        g.ep.out_bf16 = mirror; g.ep.ld_bf16 = ld_mirror;
        launch_gemm_bf16(g, ctx->stream);
    });
}

int ltx_op_gemm_bf16_gated_residual_norm(ltx_ctx* ctx, const uint16_t* A, long lda, const uint16_t* B, long ldb,
                                         const float* bias, const float* gate, float gate_scalar, int M, int N, int K,
                                         float* x, long ldx, const float* scale, const float* shift, float eps,
                                         uint16_t* xn, long ldxn, int fused) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(A && B && x && scale && shift && xn, "ltx_op_gemm_bf16_gated_residual_norm: null argument");
        GemmArgs g;
        g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.M = M; g.N = N; g.K = K;
        g.ep.bias_n = bias;
        g.ep.out_f32 = x; g.ep.ld_f32 = ldx;
        g.ep.resid = 1;
        g.ep.gate = gate; g.ep.gate_bstride = 0; g.ep.rows_per_batch = M; g.ep.gate_scalar = gate_scalar;
        // the DiT graph's launches bring a workspace and leave the split to the launcher
        op_workspace(ctx, (size_t)2 * M * N * 4);
        g.split_k = 0;
        g.split_ws = ctx->op_ws.as<float>();
        g.split_ws_elems = (long)(ctx->op_ws.bytes / 4);
        NormAfter na;
        na.scale = scale; na.shift = shift; na.mod_bstride = 0; na.rows_per_batch = M;
        na.out = xn; na.ldo = ldxn; na.eps = eps; na.norm_kind = LTX_NORM_RMS;
        if (fused) {
            launch_gemm_bf16(g, ctx->stream, &na);
        } else {
            launch_gemm_bf16(g, ctx->stream);
            NormModArgs n;
            n.x = x; n.ldx = ldx; n.scale = scale; n.shift = shift; n.rows_per_batch = M;
            n.out = xn; n.ldo = ldxn; n.rows = M; n.D = N; n.eps = eps;
            launch_norm_mod(n, ctx->stream);
        }
    });
}

int ltx_op_gemm_tile(ltx_ctx* ctx, const ltx_gemm_tile_launch* l) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(l && l->struct_size == sizeof(ltx_gemm_tile_launch), "ltx_op_gemm_tile: null argument or a struct_size of another ABI");
        LTX_REQUIRE(l->tile_cfg == 75 || l->tile_cfg == 76, "ltx_op_gemm_tile: tile_cfg %d is neither 75 (192x256) nor 76 (384x256)", l->tile_cfg);
        LTX_REQUIRE(l->A && l->B && l->split_k >= 1, "ltx_op_gemm_tile: null operand or split_k < 1");
        GemmArgs g;
        g.A = l->A; g.lda = l->lda; g.B = l->B; g.ldb = l->ldb; g.M = l->M; g.N = l->N; g.K = l->K;
        GemmEpilogue& e = g.ep;
        e.bias_n = l->bias_n; e.bias_m = l->bias_m; e.act = l->act; e.round_bf16 = l->round_bf16;
        e.out_f32 = l->out_f32; e.ld_f32 = l->ld_f32; e.out_bf16 = l->out_bf16; e.ld_bf16 = l->ld_bf16;
        e.resid = l->resid; e.resid_src = l->resid_src; e.ld_resid = l->ld_resid;
        e.gate = l->gate; e.gate_bstride = l->gate_bstride; e.gate_rowmap = l->gate_rowmap; e.gate_scalar = l->gate_scalar;
        e.rows_per_batch = l->rows_per_batch > 0 ? l->rows_per_batch : l->M;
        if (l->split_k > 1) {
            g.split_k = l->split_k;
            g.split_bf16 = l->split_bf16;
            op_workspace(ctx, (size_t)g.split_k * l->M * l->N * 4);
            g.split_ws = ctx->op_ws.as<float>();
            g.split_ws_elems = (long)(ctx->op_ws.bytes / 4);
        }
        launch_gemm_bf16_cfg(g, l->tile_cfg, ctx->stream);
    });
}

int ltx_op_gemv_f32(ltx_ctx* ctx, const float* a, long lda, const uint16_t* W, long ldw, const float* bias, float* out,
                    long ldo, int M, int N, int K, int in_act) {
    return with_ctx(ctx, [&] { launch_gemv_f32(a, lda, W, ldw, bias, out, ldo, M, N, K, in_act, ctx->stream); });
}

int ltx_op_gemv_group(ltx_ctx* ctx, const ltx_gemv_job* jobs, int n_jobs, int M) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(jobs && n_jobs >= 1 && n_jobs <= 8, "ltx_op_gemv_group: %d jobs out of range (1..8)", n_jobs);
        GemvJob g[8];
        for (int j = 0; j < n_jobs; ++j) {
            const ltx_gemv_job& q = jobs[j];
            g[j].a = q.a; g[j].lda = q.lda; g[j].W = q.W; g[j].ldw = q.ldw; g[j].bias = q.bias;
            g[j].out = q.out; g[j].ldo = q.ldo; g[j].N = q.N; g[j].K = q.K; g[j].in_act = q.in_act;
        }
        launch_gemv_group(g, n_jobs, M, ctx->stream);
    });
}

int ltx_op_gemv_group_q(ltx_ctx* ctx, const ltx_gemv_job_q* jobs, int n_jobs, int M, int bits) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(jobs && n_jobs >= 1 && n_jobs <= 8, "ltx_op_gemv_group_q: %d jobs out of range (1..8)", n_jobs);
        GemvJobQ g[8];
        for (int j = 0; j < n_jobs; ++j) {
            const ltx_gemv_job_q& q = jobs[j];
            g[j].a = q.a; g[j].lda = q.lda; g[j].codes = q.codes; g[j].scales = q.scales; g[j].biases = q.biases; g[j].bias = q.bias;
            g[j].out = q.out; g[j].ldo = q.ldo; g[j].N = q.N; g[j].K = q.K; g[j].in_act = q.in_act;
        }
        launch_gemv_group_q(g, n_jobs, M, bits, ctx->stream);
    });
}

int ltx_op_conv3d(ltx_ctx* ctx, const uint16_t* x, int F, int H, int W, int Cin, const uint16_t* w, const float* bias,
                  int Cout, int causal, float* out) {
    return with_ctx(ctx, [&] {
        GemmArgs g;
        g.A = x; g.B = w; g.ldb = 27L * Cin;
        g.M = F * H * W; g.N = Cout; g.K = 27 * Cin;
        g.conv = 1;
        g.geom.F = F; g.geom.H = H; g.geom.W = W; g.geom.C = Cin; g.geom.causal = causal; g.geom.pad_mode = 0;
        g.ep.bias_n = bias;
        g.ep.out_f32 = out; g.ep.ld_f32 = Cout;
        // a workspace, as the VAE graph passes one: the launcher may run a last partial round of tiles as a split-K launch
        op_workspace(ctx, (size_t)64 << 20);
        g.split_ws = ctx->op_ws.as<float>();
        g.split_ws_elems = (long)(ctx->op_ws.bytes / 4);
        launch_gemm_bf16(g, ctx->stream);
    });
}

int ltx_conv_takes_d2s_pn(int F, int H, int W, int C) {
    GemmArgs g;  // an upsampler conv C -> 4C of the VAE decoder at (F, H, W), as vae.cpp forms it
    g.ldb = 27L * C; g.M = (int)((long)F * H * W); g.N = 4 * C; g.K = 27 * C;
    g.conv = 1;
    g.geom.F = F; g.geom.H = H; g.geom.W = W; g.geom.C = C;
    g.ep.d2s = 1;
    return (long)F * H * W <= 0x7fffffffL && gemm_conv_takes_d2s_pn(g) ? 1 : 0;
}

int ltx_gemm_dense_tile_cfg(int M, int N, int K, int act, int flags, int ncu) {
    if (M < 1 || N < 1 || K < 64 || K % 64 != 0 || ncu < 1) return -1;
    // the launch as ltx_op_gemm_bf16 forms it; the pointers only say which operands and outputs exist and are never followed
    static const uintptr_t present = 256;
    GemmArgs g;
    g.A = (const bf16_t*)present; g.lda = K; g.B = (const bf16_t*)present; g.ldb = K; g.M = M; g.N = N; g.K = K;
    g.ep.bias_n = (const float*)present;
    g.ep.act = act;
    if (flags & 1) { g.ep.out_f32 = (float*)present; g.ep.ld_f32 = N; }
    if (flags & 2) { g.ep.out_bf16 = (bf16_t*)present; g.ep.ld_bf16 = N; }
    if (flags & 4) { g.ep.resid = 1; g.ep.gate = (const float*)present; g.ep.rows_per_batch = M; }
    if (flags & 8) { g.ep.out_bf16_t = (bf16_t*)present; g.ep.ld_bf16_t = M; }
    if (flags & 16) g.ep.bias_m = (const float*)present;
    return gemm_dense_cfg(g, ncu);
}

// ---- attention and row kernels ----
int ltx_op_attention(ltx_ctx* ctx, const uint16_t* Q, const uint16_t* K, const uint16_t* Vt, long ldvt,
                     const float* bias, int B, int H, int Tq, int Tk, float scale, uint16_t* O) {
    return with_ctx(ctx, [&] {
        AttnArgs a;
        const long D = (long)H * 128;
        a.Q = Q; a.ldq = D; a.q_bstride = (long)Tq * D;
        a.K = K; a.ldk = D; a.k_bstride = (long)Tk * D;
        a.Vt = Vt; a.ldvt = ldvt; a.vt_bstride = D * ldvt;
        a.O = O; a.ldo = D; a.o_bstride = (long)Tq * D;
        a.bias = bias; a.bias_bstride = Tk;
        a.B = B; a.H = H; a.Tq = Tq; a.Tk = Tk; a.scale = scale;
        a.q_prescaled = scale <= 0.f ? 1 : 0;  // Q already carries scale * log2(e): scores are base-2 exponents
        // few queries against many keys: lend the launcher room to divide the keys over workgroups, as the DiT forward does
        if (const long need_bytes = attn_split_ws_bytes(B, H, Tq, Tk)) {
            op_workspace(ctx, (size_t)need_bytes);
            a.split_ws = ctx->op_ws.p;
            a.split_ws_bytes = (long)ctx->op_ws.bytes;
        }
        launch_attention(a, ctx->stream);
    });
}

int ltx_op_attention_hd(ltx_ctx* ctx, const uint16_t* Q, const uint16_t* K, const uint16_t* Vt, long ldvt, const float* bias, int B, int H,
                        int Tq, int Tk, int head_dim, float scale, uint16_t* O) {
    if (head_dim == 128) return ltx_op_attention(ctx, Q, K, Vt, ldvt, bias, B, H, Tq, Tk, scale, O);
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(head_dim == 64, "ltx_op_attention_hd: head dim %d (64 or 128)", head_dim);
        AttnArgs a;
        const long D = (long)H * 64;
        a.head_dim = 64;
        a.Q = Q; a.ldq = D; a.q_bstride = (long)Tq * D;
        a.K = K; a.ldk = D; a.k_bstride = (long)Tk * D;
        a.Vt = Vt; a.ldvt = ldvt; a.vt_bstride = D * ldvt;
        a.O = O; a.ldo = D; a.o_bstride = (long)Tq * D;
        a.bias = bias; a.bias_bstride = Tk;
        a.B = B; a.H = H; a.Tq = Tq; a.Tk = Tk; a.scale = scale;
        a.q_prescaled = scale <= 0.f ? 1 : 0;
        launch_attention(a, ctx->stream);
    });
}

int ltx_op_attention_causal_ld(ltx_ctx* ctx, const uint16_t* Q, long ldq, long q_bstride, const uint16_t* K, long ldk, long k_bstride,
                               const uint16_t* Vt, long ldvt, long vt_bstride, const int32_t* key_start, int B, int Hq, int Hkv, int T,
                               int head_dim, float scale, uint16_t* O, long ldo, long o_bstride) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(head_dim == 256, "ltx_op_attention_causal: head dim %d (256)", head_dim);
        LTX_REQUIRE(Q && K && Vt && O, "ltx_op_attention_causal: null argument");
        AttnArgs a;
        a.head_dim = 256; a.causal = 1; a.key_start = key_start;
        a.Q = Q; a.ldq = ldq; a.q_bstride = q_bstride;
        a.K = K; a.ldk = ldk; a.k_bstride = k_bstride;
        a.Vt = Vt; a.ldvt = ldvt; a.vt_bstride = vt_bstride;
        a.O = O; a.ldo = ldo; a.o_bstride = o_bstride;
        a.B = B; a.H = Hq; a.Hkv = Hkv; a.Tq = T; a.Tk = T; a.scale = scale;
        launch_attention(a, ctx->stream);
    });
}

int ltx_op_attention_causal(ltx_ctx* ctx, const uint16_t* Q, const uint16_t* K, const uint16_t* Vt, long ldvt, const int32_t* key_start,
                            int B, int Hq, int Hkv, int T, int head_dim, float scale, uint16_t* O) {
    const long Dq = (long)Hq * 256, Dk = (long)Hkv * 256;  // dense operands
    return ltx_op_attention_causal_ld(ctx, Q, Dq, (long)T * Dq, K, Dk, (long)T * Dk, Vt, ldvt, Dk * ldvt, key_start, B, Hq, Hkv, T, head_dim,
                                      scale, O, Dq, (long)T * Dq);
}

int ltx_op_gemma_norm(ltx_ctx* ctx, const uint16_t* r, const float* w, const uint16_t* x, const float* w2, int rows, int D, float eps,
                      uint16_t* h, uint16_t* n) {
    return with_ctx(ctx, [&] {
        GemmaNormArgs a;
        a.r = r; a.ldr = D; a.w = w; a.x = x; a.ldx = D; a.h = h; a.ldh = D; a.w2 = w2; a.n = n; a.ldn = D;
        a.n_only = h ? 0 : 1; a.rows = rows; a.D = D; a.eps = eps;
        launch_gemma_norm(a, ctx->stream);
    });
}

int ltx_op_gemma_qknorm_rope(ltx_ctx* ctx, uint16_t* qk, long ld, const float* wq, const float* wk, int q_heads, int k_heads,
                             const float* cos_t, const float* sin_t, int T, int rows, float eps) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(qk && q_heads > 0 && k_heads >= 0 && ld >= (long)(q_heads + k_heads) * 256, "ltx_op_gemma_qknorm_rope: shape");
        GemmaQkArgs a;
        a.job[0].x = qk; a.job[0].ldx = ld; a.job[0].w = wq; a.job[0].out = qk; a.job[0].ldo = ld; a.job[0].heads = q_heads;
        a.job[1].x = qk + q_heads * 256; a.job[1].ldx = ld; a.job[1].w = wk; a.job[1].out = qk + q_heads * 256; a.job[1].ldo = ld;
        a.job[1].heads = k_heads;
        a.cos = cos_t; a.sin = sin_t; a.T = T; a.rows = rows; a.eps = eps;
        launch_gemma_qknorm_rope(a, ctx->stream);
    });
}

int ltx_op_gemma_rope_tables(ltx_ctx* ctx, int T, float base, float* cos_t, float* sin_t) {
    return with_ctx(ctx, [&] { launch_gemma_rope_tables(cos_t, sin_t, T, base, ctx->stream); });
}

int ltx_op_geglu(ltx_ctx* ctx, const uint16_t* gu, int rows, int I, uint16_t* out) {
    return with_ctx(ctx, [&] {
        GegluArgs a;
        a.gu = gu; a.ldgu = 2L * I; a.out = out; a.ldo = I; a.rows = rows; a.I = I;
        launch_geglu(a, ctx->stream);
    });
}

int ltx_op_gemma_embed(ltx_ctx* ctx, const int32_t* ids, const uint16_t* table, int rows, int D, int vocab, uint16_t* out) {
    return with_ctx(ctx, [&] {
        GemmaEmbedArgs a;
        a.ids = ids; a.table = table; a.out = out; a.rows = rows; a.D = D; a.vocab = vocab;
        a.scale = host_bf16_to_f32(host_f32_to_bf16(sqrtf((float)D)));
        launch_gemma_embed(a, ctx->stream);
    });
}

int ltx_op_gemv_bf16(ltx_ctx* ctx, const uint16_t* x, const uint16_t* W, long ldw, int M, int N, int K, int epilogue, uint16_t* out_bf16,
                     long out_stride, float* out_f32) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(M == 1, "ltx_op_gemv_bf16: M=%d (the decode path has one row)", M);
        GemvBf16Args a;
        a.x = x; a.W = W; a.ldw = ldw; a.N = N; a.K = K; a.epilogue = epilogue; a.out_bf16 = out_bf16; a.out_stride = out_stride; a.out_f32 = out_f32;
        launch_gemv_bf16(a, ctx->stream);
    });
}

int ltx_gemv_bf16_rows_per_workgroup(int N, int epilogue) { return gemv_bf16_rows_per_workgroup(N, epilogue); }

int ltx_op_attention_decode(ltx_ctx* ctx, const uint16_t* q, const uint16_t* K, long ldk, const uint16_t* Vt, long ldvt, int Hq, int Hkv,
                            int n_keys, float scale, uint16_t* O) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(Hq >= 1 && n_keys >= 1 && n_keys <= (1 << 24), "ltx_op_attention_decode: Hq=%d n_keys=%d", Hq, n_keys);
        ctx->op_ws.ensure((size_t)attn_decode_ws_bytes(Hq, n_keys));
        AttnDecodeArgs a;
        a.q = q; a.K = K; a.ldk = ldk; a.Vt = Vt; a.ldvt = ldvt; a.O = O; a.Hq = Hq; a.Hkv = Hkv; a.n_keys = n_keys; a.scale = scale;
        a.ws = ctx->op_ws.p; a.ws_bytes = (long)ctx->op_ws.bytes;
        launch_attention_decode(a, ctx->stream);
    });
}

int ltx_op_lm_pick(ltx_ctx* ctx, float* logits, int vocab, int32_t* hist, int n_gen, int context, float penalty, int32_t* out) {
    return with_ctx(ctx, [&] {
        LmPickArgs a;
        a.logits = logits; a.vocab = vocab; a.hist = hist; a.n_gen = n_gen; a.context = context; a.penalty = penalty; a.out = out;
        launch_lm_pick(a, ctx->stream);
    });
}

int ltx_attention_hd_workgroup_queries(int B, int H, int Tq, int head_dim) {
    if (B < 1 || H < 1 || Tq < 1 || head_dim != 64) return 0;
    return attn64_queries_per_workgroup(B, H, Tq);
}

int ltx_attention_key_splits(int B, int H, int Tq, int Tk) {
    if (B < 1 || H < 1 || Tq < 1 || Tk < 1) return 1;
    return attn_key_splits(B, H, Tq, Tk);
}

int ltx_op_norm_mod(ltx_ctx* ctx, const float* x, const float* scale, const float* shift, int rows, int D,
                    int norm_kind, float eps, int round_norm_bf16, uint16_t* out) {
    return with_ctx(ctx, [&] {
        NormModArgs n;
        n.x = x; n.ldx = D; n.scale = scale; n.shift = shift; n.rows_per_batch = rows;
        n.out = out; n.ldo = D; n.rows = rows; n.D = D;
        n.norm_kind = norm_kind; n.eps = eps; n.round_norm_bf16 = round_norm_bf16;
        launch_norm_mod(n, ctx->stream);
    });
}

int ltx_op_qknorm_rope(ltx_ctx* ctx, const float* x, long ldx, const float* w, const float* cos_t, const float* sin_t,
                       int T, int rows, int D, float eps, uint16_t* out) {
    return ltx_op_qknorm_rope_hd(ctx, x, ldx, w, cos_t, sin_t, T, rows, D, 128, 1.0f, eps, out);
}

int ltx_op_qknorm_rope_hd(ltx_ctx* ctx, const float* x, long ldx, const float* w, const float* cos_t, const float* sin_t, int T, int rows,
                          int D, int head_dim, float out_scale, float eps, uint16_t* out) {
    return with_ctx(ctx, [&] {
        QkNormRopeArgs n;
        n.job[0].x = x; n.job[0].w = w; n.job[0].out = out; n.job[0].out_scale = out_scale;
        n.ldx = ldx; n.ldo = D; n.cos = cos_t; n.sin = sin_t;
        n.T = T; n.rows = rows; n.D = D; n.eps = eps; n.head_dim = head_dim;
        launch_qknorm_rope(n, ctx->stream);
    });
}

int ltx_op_norm_mod_ex(ltx_ctx* ctx, const float* x, long ldx, const float* scale, const float* shift, long mod_bstride,
                       int rows_per_batch, const int32_t* row_map, int rows, int D, int norm_kind, float eps,
                       int round_norm_bf16, uint16_t* out, long ldo) {
    return with_ctx(ctx, [&] {
        NormModArgs n;
        n.x = x; n.ldx = ldx; n.scale = scale; n.shift = shift; n.mod_bstride = mod_bstride; n.rows_per_batch = rows_per_batch;
        n.row_map = row_map; n.out = out; n.ldo = ldo; n.rows = rows; n.D = D;
        n.norm_kind = norm_kind; n.eps = eps; n.round_norm_bf16 = round_norm_bf16;
        launch_norm_mod(n, ctx->stream);
    });
}

int ltx_op_norm_mod2(ltx_ctx* ctx, const ltx_norm_mod2_job* video, const ltx_norm_mod2_job* audio, float eps) {
    return with_ctx(ctx, [&] {
        auto job = [](const ltx_norm_mod2_job* j) {
            NormMod2Job o;
            if (!j) return o;
            o.x = j->x; o.ldx = j->ldx;
            o.scale0 = j->scale0; o.shift0 = j->shift0; o.scale1 = j->scale1; o.shift1 = j->shift1;
            o.mod_bstride = j->mod_bstride; o.rows_per_batch = j->rows_per_batch;
            o.out0 = j->out0; o.out1 = j->out1; o.ldo = j->ldo;
            o.rows = j->rows; o.D = j->D; o.row_map = j->row_map;
            return o;
        };
        launch_norm_mod2(job(video), job(audio), eps, ctx->stream);
    });
}

int ltx_op_dual_step(ltx_ctx* ctx, const ltx_dual_step_job* video, const ltx_dual_step_job* audio, float sigma, float sigma_next) {
    return with_ctx(ctx, [&] {
        auto job = [](const ltx_dual_step_job* j) {
            DualStepJob o;
            if (!j) return o;
            o.latent = j->latent; o.v_cond = j->v_cond; o.v_uncond = j->v_uncond;
            o.cfg_scale = j->cfg_scale; o.form = j->form;
            o.tokens = j->tokens; o.copies = j->copies; o.v_out = j->v_out; o.n = j->n;
            o.n_keep = j->n_keep; o.keep_src = j->keep_src; o.keep_noise = j->keep_noise; o.keep_scale = j->keep_scale;
            return o;
        };
        launch_dual_step(job(video), job(audio), sigma, sigma_next, ctx->stream);
    });
}

int ltx_op_dual_restage(ltx_ctx* ctx, const ltx_dual_restage_job* video, const ltx_dual_restage_job* audio) {
    return with_ctx(ctx, [&] {
        auto job = [](const ltx_dual_restage_job* j) {
            DualRestageJob o;
            if (!j) return o;
            o.x = j->x; o.latent = j->latent; o.tokens = j->tokens; o.C = j->C; o.T = j->T;
            o.noise = j->noise; o.noise_scale = j->noise_scale; o.renoise = j->renoise;
            o.stats = j->stats; o.stats_ref = j->stats_ref;
            o.HW = j->HW; o.cond = j->cond; o.cond_noise = j->cond_noise; o.cond_scale = j->cond_scale; o.cond_sigma2 = j->cond_sigma2;
            return o;
        };
        DualRestageJob v = job(video), a = job(audio);
        const bool compute = v.T > 0 && !v.stats && !v.stats_ref;  // no statistics: two launch_mean_var, as ltx_adain_filter_latent makes them
        float* ws = nullptr;
        if (v.T > 0) {
            LTX_REQUIRE((v.stats != nullptr) == (v.stats_ref != nullptr), "dual_restage: give stats and stats_ref, or neither");
            LTX_REQUIRE(v.C >= 32 && v.C <= 4096 && v.C % 32 == 0, "dual_restage: C=%d must be a multiple of 32 (32 .. 4096)", v.C);
            if (compute) {
                LTX_REQUIRE(video->ref && video->T_ref >= 1 && video->T_ref <= (1L << 24), "dual_restage: no statistics and no reference latent to take them from");
                ws = video->stats_out;
                if (!ws) {
                    ctx->dn_stats.ensure((size_t)v.C * 4 * 4 + 64);
                    ws = ctx->dn_stats.as<float>();
                }
                v.stats = ws; v.stats_ref = ws + 2 * v.C;
            }
        }
        dual_restage_check(v, a);  // every check before the first launch
        if (compute) {
            launch_mean_var(v.x, v.T, v.C, ws, ctx->stream);
            launch_mean_var(video->ref, video->T_ref, v.C, ws + 2 * v.C, ctx->stream);
        } else if (v.T > 0 && video->stats_out) {
            HIP_CHECK(hipMemcpyAsync(video->stats_out, v.stats, (size_t)2 * v.C * 4, hipMemcpyDeviceToDevice, ctx->stream));
            HIP_CHECK(hipMemcpyAsync(video->stats_out + 2 * v.C, v.stats_ref, (size_t)2 * v.C * 4, hipMemcpyDeviceToDevice, ctx->stream));
        }
        launch_dual_restage(v, a, ctx->stream);
    });
}

int ltx_op_qknorm_rope_pair(ltx_ctx* ctx, const void* x0, const float* w0, uint16_t* out0, const void* x1, const float* w1,
                            uint16_t* out1, long ldx, long ldo, const float* cos_t, const float* sin_t, int T, int rows, int D,
                            float eps, float out_scale0, int x_bf16) {
    return with_ctx(ctx, [&] {
        QkNormRopeArgs n;
        n.job[0].x = x0; n.job[0].w = w0; n.job[0].out = out0; n.job[0].out_scale = out_scale0;
        n.job[1].x = x1; n.job[1].w = w1; n.job[1].out = out1;
        n.ldx = ldx; n.ldo = ldo; n.cos = cos_t; n.sin = sin_t;
        n.T = T; n.rows = rows; n.D = D; n.eps = eps; n.x_bf16 = x_bf16 != 0;
        launch_qknorm_rope(n, ctx->stream);
    });
}

// ---- helper passes (elementwise.h: the VAE, upscaler, guidance, scheduler and connector passes around the matrix cores) ----
// Each hook checks its pointers and sizes and makes the one launch on the context's stream; shapes are the launcher's (elementwise.h).
int ltx_op_mean_var(ltx_ctx* ctx, const float* x, long n_per_batch, int B, float* stats) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(x && stats && n_per_batch >= 1 && B >= 1, "ltx_op_mean_var: null argument or empty shape");
        launch_mean_var(x, n_per_batch, B, stats, ctx->stream);
    });
}

int ltx_op_guidance_rescale(ltx_ctx* ctx, float* cfg, const float* stats_cfg, const float* stats_cond, float phi, long n_per_batch, int B) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(cfg && stats_cfg && stats_cond && n_per_batch >= 1 && B >= 1, "ltx_op_guidance_rescale: null argument or empty shape");
        launch_guidance_rescale(cfg, stats_cfg, stats_cond, phi, n_per_batch, B, ctx->stream);
    });
}

int ltx_op_adain(ltx_ctx* ctx, float* x, const float* stats_x, const float* stats_ref, float factor, long n_per_chan, int BC) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(x && stats_x && stats_ref && n_per_chan >= 1 && BC >= 1, "ltx_op_adain: null argument or empty shape");
        launch_adain(x, stats_x, stats_ref, factor, n_per_chan, BC, ctx->stream);
    });
}

int ltx_op_groupnorm_stats(ltx_ctx* ctx, const float* x, long P, int C, int G, float eps, float* stats) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(x && stats && P >= 1 && C >= 1 && G >= 1, "ltx_op_groupnorm_stats: null argument or empty shape");
        launch_groupnorm_stats(x, P, C, G, eps, stats, ctx->stream);
    });
}

int ltx_op_groupnorm_apply(ltx_ctx* ctx, const float* x, const float* stats, const float* w, const float* b, const float* resid,
                           int act_silu, float* out_f32, uint16_t* out_bf16, long P, int C, int G) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(x && stats && w && b && (out_f32 || out_bf16), "ltx_op_groupnorm_apply: null argument");
        LTX_REQUIRE(P >= 1 && C >= 1 && G >= 1 && C % G == 0, "ltx_op_groupnorm_apply: P=%ld C=%d G=%d", P, C, G);
        launch_groupnorm_apply(x, stats, w, b, resid, act_silu, out_f32, out_bf16, P, C, G, ctx->stream);
    });
}

int ltx_op_pixelnorm_silu(ltx_ctx* ctx, const float* x, const float* scale, const float* shift, uint16_t* out, long P, int C) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(x && out && P >= 1 && C >= 1, "ltx_op_pixelnorm_silu: null argument or empty shape");
        launch_pixelnorm_silu(x, scale, shift, out, P, C, ctx->stream);
    });
}

int ltx_op_vae_prepare(ltx_ctx* ctx, const float* latent, long chan_stride, const float* noise, float noise_scale, const float* mean,
                       const float* std_, uint16_t* out, int C, long P) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(latent && mean && std_ && out, "ltx_op_vae_prepare: null argument");
        LTX_REQUIRE(C >= 1 && P >= 1 && chan_stride >= P, "ltx_op_vae_prepare: C=%d P=%ld chan_stride=%ld", C, P, chan_stride);
        launch_vae_prepare(latent, chan_stride, noise, noise_scale, mean, std_, out, C, P, ctx->stream);
    });
}

int ltx_op_upscaler_finish(ltx_ctx* ctx, const float* x, const float* mean, const float* std_, float* out, long P, int C) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(x && mean && std_ && out && P >= 1 && C >= 1, "ltx_op_upscaler_finish: null argument or empty shape");
        launch_upscaler_finish(x, mean, std_, out, P, C, ctx->stream);
    });
}

int ltx_op_blend_frames(ltx_ctx* ctx, float* r, const float* nx, int n_frames, long frame_elems) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(r && nx && n_frames >= 1 && frame_elems >= 1, "ltx_op_blend_frames: null argument or empty shape");
        launch_blend_frames(r, nx, n_frames, frame_elems, ctx->stream);
    });
}

int ltx_op_patchify_bf16(ltx_ctx* ctx, const float* latent, uint16_t* tokens, int B, int C, int T) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(latent && tokens && B >= 1 && C >= 1 && T >= 1, "ltx_op_patchify_bf16: null argument or empty shape");
        launch_patchify_bf16(latent, tokens, B, C, T, ctx->stream);
    });
}

int ltx_op_unpatchify_f32(ltx_ctx* ctx, const float* tokens, float* latent, int B, int C, int T) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(tokens && latent && B >= 1 && C >= 1 && T >= 1, "ltx_op_unpatchify_f32: null argument or empty shape");
        launch_unpatchify_f32(tokens, latent, B, C, T, ctx->stream);
    });
}

int ltx_op_euler_step(ltx_ctx* ctx, float* latent, const float* velocity, float sigma, float sigma_next, long n, int skip_hw, int frames) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(latent && velocity && n >= 1 && skip_hw >= 0, "ltx_op_euler_step: null argument or empty shape");
        launch_euler_step(latent, velocity, sigma, sigma_next, n, ctx->stream, skip_hw, frames);
    });
}

int ltx_op_set_frame0(ltx_ctx* ctx, float* latent, const float* cond, const float* noise, float scale, float sigma2, int C, int F, int HW) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(latent && cond && C >= 1 && F >= 1 && HW >= 1, "ltx_op_set_frame0: null argument or empty shape");
        launch_set_frame0(latent, cond, noise, scale, sigma2, C, F, HW, ctx->stream);
    });
}

int ltx_op_make_mod(ltx_ctx* ctx, const float* tables, const float* ada, float* mod, int B, int L, int J, int D) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(tables && ada && mod && B >= 1 && L >= 1 && J >= 1 && D >= 1, "ltx_op_make_mod: null argument or empty shape");
        launch_make_mod(tables, ada, mod, B, L, J, D, ctx->stream);
    });
}

long ltx_fe_stats_partials_floats(int states, int B, int T, int D) {
    if (states < 1 || B < 1 || T < 1 || D < 1) return 0;
    return fe_stats_partials_floats(states, B, T, D);
}

int ltx_op_fe_stats(ltx_ctx* ctx, const uint16_t* hidden, const int32_t* mask, int states, int B, int T, int D, int padding_right,
                    float eps, float* partials, float* stats) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(hidden && mask && partials && stats, "ltx_op_fe_stats: null argument");
        LTX_REQUIRE(states >= 1 && B >= 1 && T >= 1 && D >= 1, "ltx_op_fe_stats: states=%d B=%d T=%d D=%d", states, B, T, D);
        launch_fe_stats(hidden, mask, states, B, T, D, padding_right, eps, partials, stats, ctx->stream);
    });
}

int ltx_op_fe_norm_concat(ltx_ctx* ctx, const uint16_t* hidden, const int32_t* mask, const float* stats, int states, int B, int T, int D,
                          int padding_right, float eps, uint16_t* out) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(hidden && mask && stats && out, "ltx_op_fe_norm_concat: null argument");
        LTX_REQUIRE(states >= 1 && B >= 1 && T >= 1 && D >= 1, "ltx_op_fe_norm_concat: states=%d B=%d T=%d D=%d", states, B, T, D);
        launch_fe_norm_concat(hidden, mask, stats, states, B, T, D, padding_right, eps, out, ctx->stream);
    });
}

// ---- helper passes, the rest: guidance combines, casts, embedding, connector registers, VAE encoder (elementwise.h) ----
int ltx_op_cfg_combine(ltx_ctx* ctx, const float* uncond, const float* cond, float scale, float* out, long n) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(uncond && cond && out && n >= 1, "ltx_op_cfg_combine: null argument or empty shape");
        launch_cfg_combine(uncond, cond, scale, out, n, ctx->stream);
    });
}

int ltx_op_lincomb(ltx_ctx* ctx, const float* a, const float* b, float ca, float cb, float* out, long n) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(a && b && out && n >= 1, "ltx_op_lincomb: null argument or empty shape");
        launch_lincomb(a, b, ca, cb, out, n, ctx->stream);
    });
}

int ltx_op_axpby(ltx_ctx* ctx, const float* a, const float* b, float ca, float cb, float* out, long n) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(a && b && out && n >= 1, "ltx_op_axpby: null argument or empty shape");
        launch_axpby(a, b, ca, cb, out, n, ctx->stream);
    });
}

int ltx_op_ge(ltx_ctx* ctx, const float* a, const float* b, float g, float* out, long n) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(a && b && out && n >= 1, "ltx_op_ge: null argument or empty shape");
        launch_ge(a, b, g, out, n, ctx->stream);
    });
}

int ltx_op_scale_inplace(ltx_ctx* ctx, float* x, float s, long n) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(x && n >= 1, "ltx_op_scale_inplace: null argument or empty shape");
        launch_scale_inplace(x, s, n, ctx->stream);
    });
}

int ltx_op_clip01(ltx_ctx* ctx, float* x, long n) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(x && n >= 1, "ltx_op_clip01: null argument or empty shape");
        launch_clip01(x, n, ctx->stream);
    });
}

int ltx_op_mask_to_bias(ltx_ctx* ctx, const int32_t* mask, float* bias, long n) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(mask && bias && n >= 1, "ltx_op_mask_to_bias: null argument or empty shape");
        launch_mask_to_bias(mask, bias, n, ctx->stream);
    });
}

int ltx_op_cast_f32_bf16(ltx_ctx* ctx, const float* x, uint16_t* out, long n) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(x && out && n >= 1, "ltx_op_cast_f32_bf16: null argument or empty shape");
        launch_cast_f32_bf16(x, out, n, ctx->stream);
    });
}

int ltx_op_cast_bf16_f32(ltx_ctx* ctx, const uint16_t* x, float* out, long n) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(x && out && n >= 1, "ltx_op_cast_bf16_f32: null argument or empty shape");
        launch_cast_bf16_f32(x, out, n, ctx->stream);
    });
}

int ltx_op_timestep_embedding(ltx_ctx* ctx, const float* ts, float mult, float* out, int n, int dim) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(ts && out && n >= 1, "ltx_op_timestep_embedding: null argument or empty shape");
        LTX_REQUIRE(dim >= 2 && dim % 2 == 0, "ltx_op_timestep_embedding: dim=%d must be even", dim);
        launch_timestep_embedding(ts, mult, out, n, dim, ctx->stream);
    });
}

int ltx_vae_mods_max_jobs(void) { return VaeModsBatch::MAX_JOBS; }

int ltx_op_vae_make_mods_batch(ltx_ctx* ctx, const ltx_vae_mods_job* jobs, int n) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(jobs && n >= 1 && n <= VaeModsBatch::MAX_JOBS, "ltx_op_vae_make_mods_batch: %d jobs (1 .. %d)", n, (int)VaeModsBatch::MAX_JOBS);
        VaeModsBatch b;
        for (int i = 0; i < n; ++i) {
            LTX_REQUIRE(jobs[i].table && jobs[i].out && jobs[i].rows >= 1 && jobs[i].C >= 1, "ltx_op_vae_make_mods_batch: job %d: null argument or empty shape", i);
            b.job[i] = VaeModsJob{jobs[i].table, jobs[i].te, jobs[i].out, jobs[i].rows, jobs[i].C};
        }
        b.n = n;
        launch_vae_make_mods_batch(b, ctx->stream);
    });
}

int ltx_op_sp_vt_interleave(ltx_ctx* ctx, const uint16_t* gathered, uint16_t* vt, int N, int D, int Tn, long ld) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(gathered && vt && N >= 1 && D >= 1 && Tn >= 1, "ltx_op_sp_vt_interleave: null argument or empty shape");
        LTX_REQUIRE(Tn % 8 == 0 && ld % 8 == 0 && ld >= (long)N * Tn, "ltx_op_sp_vt_interleave: Tn=%d ld=%ld (multiples of 8, ld >= N * Tn)", Tn, ld);
        launch_sp_vt_interleave(gathered, vt, N, D, Tn, ld, ctx->stream);
    });
}

int ltx_op_register_plan(ltx_ctx* ctx, const int32_t* mask, int B, int T, int32_t* src) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(mask && src && B >= 1 && T >= 1, "ltx_op_register_plan: null argument or empty shape");
        launch_register_plan(mask, B, T, src, ctx->stream);
    });
}

int ltx_op_register_gather(ltx_ctx* ctx, const uint16_t* enc, const float* registers, const int32_t* src, int B, int T, int D, int R,
                           float* x) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(enc && registers && src && x && B >= 1 && T >= 1 && D >= 1, "ltx_op_register_gather: null argument or empty shape");
        LTX_REQUIRE(R >= 1, "ltx_op_register_gather: R=%d registers", R);
        launch_register_gather(enc, registers, src, B, T, D, R, x, ctx->stream);
    });
}

int ltx_op_enc_patchify(ltx_ctx* ctx, const float* pixels, uint16_t* out, int T, int H, int W) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(pixels && out && T >= 1 && H >= 1 && W >= 1, "ltx_op_enc_patchify: null argument or empty shape");
        LTX_REQUIRE(H % 4 == 0 && W % 4 == 0, "ltx_op_enc_patchify: H=%d W=%d must be multiples of 4", H, W);
        launch_enc_patchify(pixels, out, T, H, W, ctx->stream);
    });
}

int ltx_op_enc_s2d_residual(ltx_ctx* ctx, const float* conv, int Cc, const float* x, int Cx, float* out, int Cout, int T, int H, int W,
                            int ft, int fh, int fw) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(conv && x && out && Cc >= 1 && Cx >= 1 && Cout >= 1 && T >= 1 && H >= 1 && W >= 1,
                    "ltx_op_enc_s2d_residual: null argument or empty shape");
        LTX_REQUIRE(ft >= 1 && fh >= 1 && fw >= 1 && H % fh == 0 && W % fw == 0, "ltx_op_enc_s2d_residual: factors (%d,%d,%d) at H=%d W=%d",
                    ft, fh, fw, H, W);
        LTX_REQUIRE((long)Cc * ft * fh * fw == Cout && ((long)Cx * ft * fh * fw) % Cout == 0,
                    "ltx_op_enc_s2d_residual: Cc=%d Cx=%d Cout=%d (Cc * S == Cout, Cx * S a multiple of Cout)", Cc, Cx, Cout);
        launch_enc_s2d_residual(conv, Cc, x, Cx, out, Cout, T, H, W, ft, fh, fw, ctx->stream);
    });
}

int ltx_op_enc_finish(ltx_ctx* ctx, const float* z, long ldz, const float* mean, const float* std_, float* out, int C, long P) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(z && out && C >= 1 && P >= 1 && ldz >= C, "ltx_op_enc_finish: null argument, empty shape or ldz=%ld < C=%d", ldz, C);
        LTX_REQUIRE((mean == nullptr) == (std_ == nullptr), "ltx_op_enc_finish: give mean and std, or neither");
        launch_enc_finish(z, ldz, mean, std_, out, C, P, ctx->stream);
    });
}

int ltx_op_i2v_rowmap(ltx_ctx* ctx, int32_t* row_map, int B, int T, int first, int G) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(row_map && B >= 1 && T >= 1 && G >= 1 && first >= 0 && first <= T, "ltx_op_i2v_rowmap: B=%d T=%d first=%d G=%d", B, T, first, G);
        launch_i2v_rowmap(row_map, B, T, first, G, ctx->stream);
    });
}

int ltx_op_i2v_timesteps(ltx_ctx* ctx, float* ts, int B, int G, float sigma) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(ts && B >= 1 && G >= 1 && (long)B * G + B <= 64, "ltx_op_i2v_timesteps: B=%d G=%d (B * G + B <= 64)", B, G);
        launch_i2v_timesteps(ts, B, G, sigma, ctx->stream);
    });
}

int ltx_op_fill_const_i32(ltx_ctx* ctx, int32_t* p, long n, int32_t v) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(p && n >= 1, "ltx_op_fill_const_i32: null argument or empty shape");
        launch_fill_const_i32(p, n, v, ctx->stream);
    });
}

int ltx_op_gemma_mask_scan(ltx_ctx* ctx, const int32_t* mask, int B, int T, int32_t* key_start, int32_t* status) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(mask && key_start && status && B >= 1 && T >= 1, "ltx_op_gemma_mask_scan: null argument or empty shape");
        launch_gemma_mask_scan(mask, B, T, key_start, status, ctx->stream);
    });
}

// ---- audio row passes (audio.h): each writes only the interior of its haloed operand ----
int ltx_op_audio_pn_pad(ltx_ctx* ctx, const float* x, int H, int W, int C, int mode, uint16_t* out) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(x && out && H >= 1 && W >= 1 && C >= 1, "ltx_op_audio_pn_pad: null argument or empty shape");
        LTX_REQUIRE(mode == 0 || mode == 1, "ltx_op_audio_pn_pad: mode=%d (0 PixelNorm + SiLU, 1 copy)", mode);
        launch_audio_pn_pad(x, H, W, C, mode, out, ctx->stream);
    });
}

int ltx_op_audio_upsample_pad(ltx_ctx* ctx, const float* x, int H, int W, int C, uint16_t* out) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(x && out && H >= 1 && W >= 1 && C >= 1, "ltx_op_audio_upsample_pad: null argument or empty shape");
        LTX_REQUIRE(C % 4 == 0, "ltx_op_audio_upsample_pad: C=%d must be a multiple of 4", C);
        launch_audio_upsample_pad(x, H, W, C, out, ctx->stream);
    });
}

int ltx_op_audio_denorm_pad(ltx_ctx* ctx, const float* latent, const float* mean, const float* std_, int Cl, int T, int Wl, int Cpad,
                            uint16_t* out) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(latent && mean && std_ && out && Cl >= 1 && T >= 1 && Wl >= 1, "ltx_op_audio_denorm_pad: null argument or empty shape");
        LTX_REQUIRE(Cpad >= Cl, "ltx_op_audio_denorm_pad: Cpad=%d < Cl=%d", Cpad, Cl);
        launch_audio_denorm_pad(latent, mean, std_, Cl, T, Wl, Cpad, out, ctx->stream);
    });
}

int ltx_op_audio_mel_pack(ltx_ctx* ctx, const float* mel, int T, int M, uint16_t* out) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(mel && out && T >= 1 && M >= 1, "ltx_op_audio_mel_pack: null argument or empty shape");
        launch_audio_mel_pack(mel, T, M, out, ctx->stream);
    });
}

int ltx_op_audio_mean3_act(ltx_ctx* ctx, const float* a, const float* b, const float* c, long rows, int C, float slope, uint16_t* out,
                           long ldb) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(a && b && c && out && rows >= 1 && C >= 1, "ltx_op_audio_mean3_act: null argument or empty shape");
        LTX_REQUIRE(C % 4 == 0 && ldb % 4 == 0 && ldb >= C, "ltx_op_audio_mean3_act: C=%d ldb=%ld (multiples of 4, ldb >= C)", C, ldb);
        launch_audio_mean3_act(a, b, c, rows, C, slope, out, ldb, ctx->stream);
    });
}

// ---- audio convolutions ----
int ltx_op_conv1d(ltx_ctx* ctx, const uint16_t* x, int L, int Cin, const uint16_t* w, const float* bias, int Cout, int k, int dilation,
                  int tile, const float* resid, int f32_act, int transposed, float* out_f32, int bf16_act, float slope,
                  uint16_t* out_bf16) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(x && w && L >= 1 && L <= (1 << 24) && Cin >= 1 && Cin <= 4096 && Cout >= 1 && Cout <= 4096, "ltx_op_conv1d: bad shape");
        LTX_REQUIRE(k >= 1 && k <= ACONV_MAX_TAPS && k % 2 == 1 && dilation >= 1 && (k - 1) / 2 * dilation <= ACONV_HALO,
                    "ltx_op_conv1d: k=%d dilation=%d (odd k <= %d, reach <= %d rows)", k, dilation, (int)ACONV_MAX_TAPS, (int)ACONV_HALO);
        LTX_REQUIRE(Cin % 32 == 0, "ltx_op_conv1d: Cin=%d must be a multiple of 32", Cin);
        AConvArgs a;
        a.x = audio_halo_operand(ctx, x, Cin, 1, L, L, ACONV_HALO, (size_t)L + 2 * ACONV_HALO) + (size_t)ACONV_HALO * Cin;
        a.ldx = Cin;
        a.w = w;
        a.bias = bias;
        a.P = L;
        a.Cin = Cin;
        a.Cout = Cout;
        a.ntaps = k;
        for (int j = 0; j < k; ++j) a.off[j] = (j - (k - 1) / 2) * dilation;
        audio_op_epilogue(a, resid, f32_act, transposed, out_f32, L, bf16_act, slope, out_bf16);
        launch_audio_conv(a, tile, ctx->stream);
    });
}

int ltx_op_conv_transpose1d(ltx_ctx* ctx, const uint16_t* x, int L, int Cin, const uint16_t* w, const float* bias, int Cout, int k,
                            int stride, int padding, int tile, float* out_f32, int bf16_act, float slope, uint16_t* out_bf16) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(x && w && L >= 1 && L <= (1 << 22) && Cin >= 1 && Cin <= 4096 && Cout >= 1 && Cout <= 4096, "ltx_op_conv_transpose1d: bad shape");
        LTX_REQUIRE(Cin % 32 == 0, "ltx_op_conv_transpose1d: Cin=%d must be a multiple of 32", Cin);
        LTX_REQUIRE(stride >= 1 && stride <= 8 && k >= stride && k <= 64 && (k - stride) % 2 == 0 && padding == (k - stride) / 2,
                    "ltx_op_conv_transpose1d: k=%d stride=%d padding=%d (padding must be (k - stride) / 2: output length stride * L)", k,
                    stride, padding);
        const bf16_t* x0 = audio_halo_operand(ctx, x, Cin, 1, L, L, ACONV_HALO, (size_t)L + 2 * ACONV_HALO) + (size_t)ACONV_HALO * Cin;
        // the phase slabs come from the vocoder loader's own builder, convt_phase_slab (test hook: one round trip through the host)
        std::vector<bf16_t> wh((size_t)Cin * Cout * k);
        HIP_CHECK(hipMemcpyAsync(wh.data(), w, wh.size() * 2, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        std::vector<float> wf(wh.size());
        for (size_t i = 0; i < wh.size(); ++i) wf[i] = host_bf16_to_f32(wh[i]);
        std::vector<bf16_t> slabs;
        std::vector<std::vector<int>> offs((size_t)stride);
        std::vector<size_t> at((size_t)stride);
        for (int r = 0; r < stride; ++r) {
            const std::vector<int> js = convt_phase_taps(k, stride, padding, r, &offs[r]);
            LTX_REQUIRE(!js.empty() && (int)js.size() <= ACONV_MAX_TAPS, "ltx_op_conv_transpose1d: phase %d has %zu taps", r, js.size());
            for (int o : offs[r]) LTX_REQUIRE(o >= -ACONV_HALO && o <= ACONV_HALO, "ltx_op_conv_transpose1d: offset %d beyond the halo", o);
            at[r] = slabs.size();
            for (float v : convt_phase_slab(wf.data(), Cin, Cout, k, js, Cin)) slabs.push_back(host_f32_to_bf16(v));  // exact: v is a bf16 value
        }
        ctx->audio_op[1].ensure(slabs.size() * 2);
        HIP_CHECK(hipMemcpyAsync(ctx->audio_op[1].p, slabs.data(), slabs.size() * 2, hipMemcpyHostToDevice, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        for (int r = 0; r < stride; ++r) {
            AConvArgs a;
            a.x = x0;
            a.ldx = Cin;
            a.w = ctx->audio_op[1].as<bf16_t>() + at[r];
            a.bias = bias;
            a.P = L;
            a.Cin = Cin;
            a.Cout = Cout;
            a.ntaps = (int)offs[r].size();
            for (int t = 0; t < a.ntaps; ++t) a.off[t] = offs[r][t];
            a.omul = stride;
            a.oadd = r;
            audio_op_epilogue(a, nullptr, AACT_NONE, 0, out_f32, (long)L * stride, bf16_act, slope, out_bf16);
            launch_audio_conv(a, tile, ctx->stream);
        }
    });
}

int ltx_op_conv2d_causal(ltx_ctx* ctx, const uint16_t* x, int H, int W, int Cin, const uint16_t* w, const float* bias, int Cout, int ksize,
                         int tile, const float* resid, int transposed, float* out_f32, uint16_t* out_bf16) {
    return with_ctx(ctx, [&] {
        LTX_REQUIRE(x && w && H >= 1 && H <= 65536 && W >= 1 && W <= 4096 && Cin >= 1 && Cin <= 4096 && Cout >= 1 && Cout <= 4096,
                    "ltx_op_conv2d_causal: bad shape");
        LTX_REQUIRE(ksize == 1 || ksize == 3, "ltx_op_conv2d_causal: kernel %d (1 or 3)", ksize);
        LTX_REQUIRE(Cin % 32 == 0, "ltx_op_conv2d_causal: Cin=%d must be a multiple of 32", Cin);
        const int wp = W + 2;
        AConvArgs a;
        // the padded [(H+3)][W+2][Cin] operand of audio.h: image row h at padded row h+2, column w at w+1
        a.x = audio_halo_operand(ctx, x, Cin, H, W, wp, (size_t)2 * wp + 1, (size_t)(H + 3) * wp);
        a.ldx = Cin;
        a.w = w;
        a.bias = bias;
        a.P = H * wp;
        a.Cin = Cin;
        a.Cout = Cout;
        if (ksize == 3) {
            a.ntaps = 9;
            for (int kh = 0; kh < 3; ++kh)
                for (int kw = 0; kw < 3; ++kw) a.off[kh * 3 + kw] = kh * wp + kw;
        } else {
            a.ntaps = 1;
            a.off[0] = 2 * wp + 1;
        }
        a.wp = wp;
        a.wv = W;
        a.opitch = W;
        a.bpitch = W;
        audio_op_epilogue(a, resid, AACT_NONE, transposed, out_f32, (long)H * W, AACT_NONE, 0.f, out_bf16);
        launch_audio_conv(a, tile, ctx->stream);
    });
}

}  // extern "C"
