// elementwise.hip - HBM-bound kernels of the DiT / VAE path (see elementwise.h for the reference call sites).
// All are streaming kernels: 16-B (or 8-B bf16) accesses per lane, one pass over the data, reductions via
// wave shuffles + one LDS hop. Roofline for each is HBM bytes / 8 TB/s; none of them is reshaped into a GEMM.
#include "elementwise.h"

#include <stdlib.h>

#include <algorithm>

#include "options.h"
#include "runtime.h"

namespace {

constexpr int MAXV = 8;  // float4 chunks per thread kept in registers by the row kernels (D <= 8192)

LTX_DEVFN float block_reduce_sum(float v, float* red) {
    v = wave_reduce_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();  // protect `red` from a previous use
    if (lane == 0) red[w] = v;
    __syncthreads();
    float t = 0.f;
    const int nw = blockDim.x >> 6;
    for (int i = 0; i < nw; ++i) t += red[i];
    return t;
}

// The cross-wave half of the multi-row kernels' reductions: K sums (one per row a workgroup holds) share ONE barrier. post_wave_sums
// takes the K WAVE sums (wave_reduce_sum of each thread's share), lane 0 of every wave posts them, and behind its barrier
// four_wave_total(red, k) is sum k over the workgroup, the wave sums added in wave order as block_reduce_sum adds them.
template <int K>
LTX_DEVFN void post_wave_sums(const float (&wave_sum)[K], float (&red)[4][K]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[w][k] = wave_sum[k];
    }
    __syncthreads();
}
template <int K>
LTX_DEVFN float four_wave_total(const float (&red)[4][K], int k) {
    return red[0][k] + red[1][k] + red[2][k] + red[3][k];
}
// adaLN modulation of one normed value, and four results as bf16 at dst (8-byte store): the tail of every norm + modulation kernel
LTX_DEVFN float modulate(float y, float scale, float shift) { return y * (1.0f + scale) + shift; }
LTX_DEVFN void store_bf16x4(bf16_t* dst, f32x4 y) {
    uint2 pk;
    pk.x = pack_bf16x2(y[0], y[1]);
    pk.y = pack_bf16x2(y[2], y[3]);
    *(uint2*)dst = pk;
}

// one workgroup (256 threads) per row; NV = float4 chunks per thread (D <= NV*1024). The modulation vectors are
// fetched together with the row, BEFORE the reduction: every workgroup of the launch is resident at once, so the kernel
// costs one memory latency plus the transfer, and a second dependent load after the barrier doubled it (17 -> ~9 us).
template <int NV>
__global__ __launch_bounds__(256) void norm_mod_kernel(const float* __restrict__ x, long ldx,
                                                       const float* __restrict__ scale,
                                                       const float* __restrict__ shift, long mod_bstride,
                                                       int rows_per_batch, bf16_t* __restrict__ out, long ldo, int D,
                                                       int norm_kind, float eps, int round_norm_bf16,
                                                       const int32_t* __restrict__ row_map) {
    __shared__ float red[4];
    const int row = blockIdx.x;
    const float* xr = x + (long)row * ldx;
    const long b = row_map ? row_map[row] : row / rows_per_batch;  // modulation row (per-token timestep groups: I2V)
    const float* sc = scale ? scale + b * mod_bstride : nullptr;
    const float* sh = shift ? shift + b * mod_bstride : nullptr;
    f32x4 v[NV], s4[NV], h4[NV];
    float s1 = 0.f, s2 = 0.f;
    const int nchunk = D >> 2;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int c = threadIdx.x + j * 256;
        v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (c < nchunk) v[j] = *(const f32x4*)(xr + c * 4);
    }
    if (sc) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = threadIdx.x + j * 256;
            if (c < nchunk) {
                s4[j] = *(const f32x4*)(sc + c * 4);
                h4[j] = *(const f32x4*)(sh + c * 4);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            s1 += v[j][e];
            s2 += v[j][e] * v[j][e];
        }
    float mean = 0.f, rstd;
    if (norm_kind == LTX_NORM_LAYER) {
        mean = block_reduce_sum(s1, red) / (float)D;
        // two-pass variance on the register copy (population variance, as MLXNN.LayerNorm)
        float sv = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = threadIdx.x + j * 256;
            if (c < nchunk) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float d = v[j][e] - mean;
                    sv += d * d;
                }
            }
        }
        const float var = block_reduce_sum(sv, red) / (float)D;
        rstd = rsqrtf(var + eps);
    } else {
        const float ms = block_reduce_sum(s2, red) / (float)D;
        rstd = rsqrtf(ms + eps);
    }
    bf16_t* orow = out + (long)row * ldo;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int c = threadIdx.x + j * 256;
        if (c < nchunk) {
            f32x4 y;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                y[e] = (v[j][e] - mean) * rstd;
                if (round_norm_bf16) y[e] = bf16_to_f32(f32_to_bf16(y[e]));
            }
            if (sc) {
#pragma unroll
                for (int e = 0; e < 4; ++e) y[e] = modulate(y[e], s4[j][e], h4[j][e]);
            }
            store_bf16x4(orow + c * 4, y);
        }
    }
}

// R rows per workgroup (RMS norm, D = NV * 1024 exactly, rows of one batch element): the modulation vectors are the same for every
// row of a batch element, and one workgroup per row re-read their 2 x 4 D bytes from L2 for each row - twice the bytes of the row
// itself. Here they are fetched once per R rows, all R rows are loaded before the first reduction (one memory latency per
// workgroup, as before), and the R sums of squares share one barrier pair.
template <int NV, int R>
__global__ __launch_bounds__(256) void norm_mod_rows_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ scale,
                                                            const float* __restrict__ shift, long mod_bstride, int rows_per_batch,
                                                            bf16_t* __restrict__ out, long ldo, int rows, float eps, int round_norm_bf16) {
    __shared__ float red[4][R];
    const int row0 = blockIdx.x * R;
    const long b = row0 / rows_per_batch;   // the launcher guarantees that the R rows do not straddle a batch element
    const float* sc = scale + b * mod_bstride;
    const float* sh = shift + b * mod_bstride;
    constexpr int D = NV * 1024;
    f32x4 v[R][NV], s4[NV], h4[NV];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int row = (row0 + r) < rows ? (row0 + r) : rows - 1;
#pragma unroll
        for (int j = 0; j < NV; ++j) v[r][j] = *(const f32x4*)(x + (long)row * ldx + (threadIdx.x + j * 256) * 4);
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        s4[j] = *(const f32x4*)(sc + (threadIdx.x + j * 256) * 4);
        h4[j] = *(const f32x4*)(sh + (threadIdx.x + j * 256) * 4);
    }
    float ss[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < NV; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) a += v[r][j][e] * v[r][j][e];
        ss[r] = wave_reduce_sum(a);
    }
    post_wave_sums(ss, red);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (row0 + r >= rows) break;
        const float ms = four_wave_total(red, r) / (float)D;  // norm_mod_kernel's summation order
        const float rstd = rsqrtf(ms + eps);
        bf16_t* orow = out + (long)(row0 + r) * ldo;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            f32x4 y;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                y[e] = v[r][j][e] * rstd;
                if (round_norm_bf16) y[e] = bf16_to_f32(f32_to_bf16(y[e]));
                y[e] = modulate(y[e], s4[j][e], h4[j][e]);
            }
            store_bf16x4(orow + (threadIdx.x + j * 256) * 4, y);
        }
    }
}

// norm_mod_kernel for the cross-modal norms of the dual block (elementwise.h, NormMod2Job): one workgroup per row of either job
// (workgroups 0 .. j0.rows-1 take job 0, the rest job 1; the choice is uniform per workgroup). The row and both pairs of modulation
// vectors are fetched before the reduction, as norm_mod_kernel fetches its one pair; the row is normed once and stored twice. Same
// per-thread chunk assignment, same sum of squares per thread, same block_reduce_sum: out0 and out1 carry norm_mod_kernel's bits.
template <int NV>
__global__ __launch_bounds__(256) void norm_mod2_kernel(const NormMod2Job j0, const NormMod2Job j1, float eps) {
    __shared__ float red[4];
    constexpr bool EARLY = NV <= 4;  // NV = 8 (D > 4096) would hold 5 x 32 row registers across the barrier: it fetches the vectors after it
    const bool second = (int)blockIdx.x >= j0.rows;
    const int row = second ? (int)blockIdx.x - j0.rows : (int)blockIdx.x;
    const int D = second ? j1.D : j0.D;
    const long ldx = second ? j1.ldx : j0.ldx, ldo = second ? j1.ldo : j0.ldo, mbs = second ? j1.mod_bstride : j0.mod_bstride;
    const float* xr = (second ? j1.x : j0.x) + (long)row * ldx;
    const int32_t* rmap = second ? j1.row_map : j0.row_map;  // per-token timestep groups (image-to-video): one uniform load
    const long moff = (long)(rmap ? rmap[row] : row / (second ? j1.rows_per_batch : j0.rows_per_batch)) * mbs;
    const float* sc0 = second ? j1.scale0 : j0.scale0;
    const float* sh0 = second ? j1.shift0 : j0.shift0;
    const float* sc1 = second ? j1.scale1 : j0.scale1;
    const float* sh1 = second ? j1.shift1 : j0.shift1;
    f32x4 v[NV], s0[NV], h0[NV], s1[NV], h1[NV];
    const int nchunk = D >> 2;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = threadIdx.x + i * 256;
        v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (c < nchunk) v[i] = *(const f32x4*)(xr + c * 4);
    }
    auto fetch = [&](int i) {
        const int c = threadIdx.x + i * 256;
        if (c < nchunk) {
            if (sc0) {
                s0[i] = *(const f32x4*)(sc0 + moff + c * 4);
                h0[i] = *(const f32x4*)(sh0 + moff + c * 4);
            }
            if (sc1) {
                s1[i] = *(const f32x4*)(sc1 + moff + c * 4);
                h1[i] = *(const f32x4*)(sh1 + moff + c * 4);
            }
        }
    };
    if constexpr (EARLY) {
#pragma unroll
        for (int i = 0; i < NV; ++i) fetch(i);
    }
    float s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) s2 += v[i][e] * v[i][e];
    const float ms = block_reduce_sum(s2, red) / (float)D;
    const float rstd = rsqrtf(ms + eps);
    bf16_t* o0 = (second ? j1.out0 : j0.out0) + (long)row * ldo;
    bf16_t* o1 = (second ? j1.out1 : j0.out1) + (long)row * ldo;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = threadIdx.x + i * 256;
        if (c < nchunk) {
            if constexpr (!EARLY) fetch(i);
            f32x4 y, ya, yb;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                y[e] = v[i][e] * rstd;
                ya[e] = yb[e] = y[e];
            }
            if (sc0) {
#pragma unroll
                for (int e = 0; e < 4; ++e) ya[e] = modulate(y[e], s0[i][e], h0[i][e]);
            }
            if (sc1) {
#pragma unroll
                for (int e = 0; e < 4; ++e) yb[e] = modulate(y[e], s1[i][e], h1[i][e]);
            }
            store_bf16x4(o0 + c * 4, ya);
            store_bf16x4(o1 + c * 4, yb);
        }
    }
}

// ---- q/k RMSNorm + split RoPE: the pieces every kernel of the family is built from, then the three kernels ----
// One job of a launch: q or k of a projection. blockIdx.y (or the pair kernel's own loop) selects it.
struct QkJob {
    const float* x;
    const float* w;
    bf16_t* out;
    long ldx, ldo;
    float out_scale;  // multiplies the normed (and rotated) row before its ONE rounding to bf16 (1 = plain)
};
// row `row` of a job's input: the rows are f32, or (XB) bf16 with ldx counted in bf16 elements
template <bool XB>
LTX_DEVFN const float* qk_row(const float* x, long ldx, int row) {
    return XB ? (const float*)((const bf16_t*)x + (long)row * ldx) : x + (long)row * ldx;
}
// four consecutive elements of a q / k projection row as f32: the row is f32, or (XB) bf16 at the same element offsets
template <bool XB>
LTX_DEVFN f32x4 qk_load4(const float* x_row, int col) {
    if constexpr (XB) {
        const uint2 u = *(const uint2*)((const bf16_t*)x_row + col);
        return f32x4{__builtin_bit_cast(float, u.x << 16), __builtin_bit_cast(float, u.x & 0xffff0000u),
                     __builtin_bit_cast(float, u.y << 16), __builtin_bit_cast(float, u.y & 0xffff0000u)};
    } else {
        return *(const f32x4*)(x_row + col);
    }
}
// Pair chunk p (0 .. D/8-1) of a row whose heads are HD wide: head = p / (HD/8), i4 = p % (HD/8). A thread holds four elements `a` of
// the head's first half, at column head*HD + i4*4 of the row (LTX_QK_COL(HD, p, HD)), and the matching four `b` of its second half, HD/2
// columns further; both rotate with the cos/sin values at column head*(HD/2) + i4*4 of the table row (LTX_QK_COL(HD, p, HD / 2)): cos/sin
// rows are [T][D/2], head h uses columns h*HD/2 .. of them. HD = 128 is the DiT; HD = 64 is LTXAttention at 32 x 64, the audio /
// cross-modal attention of the dual block (halves [0:32] / [32:64] of a head). The norm is across the whole row for either head dim.
#define LTX_QK_COL(HD, p, head_width) (((p) >> ((HD) == 128 ? 4 : 3)) * (head_width) + ((p) & ((HD) / 8 - 1)) * 4)
// Split RoPE of one element pair in place, a of a head's first half against b of its second half, on the normed and weighted f32
// values: the reference rounds the normed q/k to its storage dtype before the f32 rotation only when that dtype is bf16 (cross-modal
// case); in the DiT q,k are f32 here (LTXRoPE.swift:90-92). Text and not a function, like LTX_QK_COL: a function is simplified on its
// own before it is inlined, and the kernels then come out with other instruction streams - for this line that can mean another choice
// of fused multiply-adds, i.e. other bits (tools/compare_isa.py, profiles/row_passes_isa.txt).
#define LTX_QK_ROTATE(a, b, c, s)               \
    do {                                        \
        const float a0 = (a), b0 = (b);         \
        (a) = a0 * (c) - b0 * (s);              \
        (b) = b0 * (c) + a0 * (s);              \
    } while (0)
// a chunk pair's last steps: the output scale, ONE rounding to bf16, 8-byte stores at `col` and half a head further
template <int HD>
LTX_DEVFN void qk_store(bf16_t* orow, int col, f32x4 a, f32x4 b, float osc) {
    uint2 pa, pb;
    pa.x = pack_bf16x2(a[0] * osc, a[1] * osc);
    pa.y = pack_bf16x2(a[2] * osc, a[3] * osc);
    pb.x = pack_bf16x2(b[0] * osc, b[1] * osc);
    pb.y = pack_bf16x2(b[2] * osc, b[3] * osc);
    *(uint2*)(orow + col) = pa;
    *(uint2*)(orow + col + HD / 2) = pb;
}
// one workgroup per row; thread handles float4 chunks of the first half `a` of a head and the matching `b` chunk (LTX_QK_COL).
// blockIdx.y selects the job (q or k of the fused projection): one launch normalises and rotates both. The weight and
// cos/sin chunks are fetched with the row, before the reduction (same reason as norm_mod_kernel).
template <int HD, int NP, bool XB>
__global__ __launch_bounds__(256) void qknorm_rope_kernel(QkJob j0, QkJob j1, const float* __restrict__ cosT,
                                                          const float* __restrict__ sinT, int T, int D, float eps) {
    __shared__ float red[4];
    const QkJob job = blockIdx.y ? j1 : j0;
    const int row = blockIdx.x;
    const float* xr = qk_row<XB>(job.x, job.ldx, row);
    const int npair = D >> 3;
    const int t = row % T;
    f32x4 va[NP], vb[NP], wa[NP], wb[NP], c4[NP], s4[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int p = threadIdx.x + j * 256;
        va[j] = vb[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (p < npair) {
            const int col = LTX_QK_COL(HD, p, HD);
            va[j] = qk_load4<XB>(xr, col);
            vb[j] = qk_load4<XB>(xr, col + HD / 2);
        }
    }
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int p = threadIdx.x + j * 256;
        if (p < npair) {
            const int col = LTX_QK_COL(HD, p, HD);
            wa[j] = *(const f32x4*)(job.w + col);
            wb[j] = *(const f32x4*)(job.w + col + HD / 2);
            if (cosT) {
                const int fc = LTX_QK_COL(HD, p, HD / 2);
                c4[j] = *(const f32x4*)(cosT + (long)t * (D >> 1) + fc);
                s4[j] = *(const f32x4*)(sinT + (long)t * (D >> 1) + fc);
            }
        }
    }
    float s2 = 0.f;
#pragma unroll
    for (int j = 0; j < NP; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) s2 += va[j][e] * va[j][e] + vb[j][e] * vb[j][e];
    const float rstd = rsqrtf(block_reduce_sum(s2, red) / (float)D + eps);
    const float osc = job.out_scale;
    bf16_t* orow = job.out + (long)row * job.ldo;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int p = threadIdx.x + j * 256;
        if (p < npair) {
            const int col = LTX_QK_COL(HD, p, HD);
            f32x4 a, b;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                a[e] = va[j][e] * rstd * wa[j][e];
                b[e] = vb[j][e] * rstd * wb[j][e];
            }
            if (cosT) {
#pragma unroll
                for (int e = 0; e < 4; ++e) LTX_QK_ROTATE(a[e], b[e], c4[j][e], s4[j][e]);
            }
            qk_store<HD>(orow, col, a, b, osc);
        }
    }
}

// R rows per workgroup of qknorm_rope_kernel<128> (D = 4096): the norm weights are fetched once per R rows instead of once per row
// (they are as many bytes as a row), every row is loaded before the first reduction, the R sums share one barrier pair.
template <int R, bool XB>
__global__ __launch_bounds__(256) void qknorm_rope_rows_kernel(QkJob j0, QkJob j1, const float* __restrict__ cosT, const float* __restrict__ sinT,
                                                               int T, int rows, float eps) {
    constexpr int HD = 128, NP = 2, D = 4096;
    __shared__ float red[4][R];
    const QkJob job = blockIdx.y ? j1 : j0;
    const int row0 = blockIdx.x * R;
    f32x4 va[R][NP], vb[R][NP], wa[NP], wb[NP];
    int col[NP], fc[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int p = threadIdx.x + j * 256;
        col[j] = LTX_QK_COL(HD, p, HD);
        fc[j] = LTX_QK_COL(HD, p, HD / 2);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int row = (row0 + r) < rows ? (row0 + r) : rows - 1;
        const float* xr = qk_row<XB>(job.x, job.ldx, row);
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            va[r][j] = qk_load4<XB>(xr, col[j]);
            vb[r][j] = qk_load4<XB>(xr, col[j] + HD / 2);
        }
    }
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        wa[j] = *(const f32x4*)(job.w + col[j]);
        wb[j] = *(const f32x4*)(job.w + col[j] + HD / 2);
    }
    // the table rows too, before the reduction: a dependent load behind the barrier costs a second memory latency per workgroup
    f32x4 c4[R][NP], s4[R][NP];
    if (cosT) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int row = (row0 + r) < rows ? (row0 + r) : rows - 1;
            const long tb = (long)(row % T) * (D >> 1);
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                c4[r][j] = *(const f32x4*)(cosT + tb + fc[j]);
                s4[r][j] = *(const f32x4*)(sinT + tb + fc[j]);
            }
        }
    }
    float ss[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < NP; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) a += va[r][j][e] * va[r][j][e] + vb[r][j][e] * vb[r][j][e];
        ss[r] = wave_reduce_sum(a);
    }
    post_wave_sums(ss, red);
    const float osc = job.out_scale;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int row = row0 + r;
        if (row >= rows) break;
        const float rstd = rsqrtf(four_wave_total(red, r) / (float)D + eps);
        bf16_t* orow = job.out + (long)row * job.ldo;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            f32x4 a, b;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                a[e] = va[r][j][e] * rstd * wa[j][e];
                b[e] = vb[r][j][e] * rstd * wb[j][e];
            }
            if (cosT) {
#pragma unroll
                for (int e = 0; e < 4; ++e) LTX_QK_ROTATE(a[e], b[e], c4[r][j][e], s4[r][j][e]);
            }
            qk_store<HD>(orow, col[j], a, b, osc);
        }
    }
}

// The self-attention pair (q and k of the same tokens) in one workgroup: R rows of BOTH jobs share one fetch of the rotary tables
// (a table row is as many bytes as the f32 row it rotates; with one workgroup per job the second fetch came from L2 / Infinity Cache,
// 768 workgroups later) and one barrier pair. The norm weights of a job are fetched behind the barrier, when its rows are finished.
template <int R, bool XB>
__global__ __launch_bounds__(256) void qknorm_rope_pair_kernel(QkJob j0, QkJob j1, const float* __restrict__ cosT, const float* __restrict__ sinT,
                                                               int T, int rows, float eps) {
    constexpr int HD = 128, NP = 2, D = 4096, NJ = 2;
    __shared__ float red[4][NJ * R];
    const int row0 = blockIdx.x * R;
    f32x4 va[NJ][R][NP], vb[NJ][R][NP], c4[R][NP], s4[R][NP];
    int col[NP], fc[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int p = threadIdx.x + j * 256;
        col[j] = LTX_QK_COL(HD, p, HD);
        fc[j] = LTX_QK_COL(HD, p, HD / 2);
    }
#pragma unroll
    for (int q = 0; q < NJ; ++q) {
        const QkJob& job = q ? j1 : j0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int row = (row0 + r) < rows ? (row0 + r) : rows - 1;
            const float* xr = qk_row<XB>(job.x, job.ldx, row);
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                va[q][r][j] = qk_load4<XB>(xr, col[j]);
                vb[q][r][j] = qk_load4<XB>(xr, col[j] + HD / 2);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int row = (row0 + r) < rows ? (row0 + r) : rows - 1;
        const long tb = (long)(row % T) * (D >> 1);
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            c4[r][j] = *(const f32x4*)(cosT + tb + fc[j]);
            s4[r][j] = *(const f32x4*)(sinT + tb + fc[j]);
        }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < NJ; ++q)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float a = 0.f;
#pragma unroll
            for (int j = 0; j < NP; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) a += va[q][r][j][e] * va[q][r][j][e] + vb[q][r][j][e] * vb[q][r][j][e];
            a = wave_reduce_sum(a);
            if (lane == 0) red[w][q * R + r] = a;  // posted behind each butterfly, not together (post_wave_sums): this kernel's order
        }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NJ; ++q) {
        const QkJob& job = q ? j1 : j0;
        const float osc = job.out_scale;
        f32x4 wa[NP], wb[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            wa[j] = *(const f32x4*)(job.w + col[j]);
            wb[j] = *(const f32x4*)(job.w + col[j] + HD / 2);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int row = row0 + r;
            if (row >= rows) break;
            const float rstd = rsqrtf(four_wave_total(red, q * R + r) / (float)D + eps);
            bf16_t* orow = job.out + (long)row * job.ldo;
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                f32x4 a, b;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    a[e] = va[q][r][j][e] * rstd * wa[j][e];
                    b[e] = vb[q][r][j][e] * rstd * wb[j][e];
                    LTX_QK_ROTATE(a[e], b[e], c4[r][j][e], s4[r][j][e]);
                }
                qk_store<HD>(orow, col[j], a, b, osc);
            }
        }
    }
}

__global__ void cast_f32_bf16_kernel(const float* __restrict__ x, bf16_t* __restrict__ out, long n) {
    long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const long stride = (long)gridDim.x * blockDim.x * 4;
    for (; i + 3 < n; i += stride) {
        const f32x4 v = *(const f32x4*)(x + i);
        uint2 pk;
        pk.x = pack_bf16x2(v[0], v[1]);
        pk.y = pack_bf16x2(v[2], v[3]);
        *(uint2*)(out + i) = pk;
    }
    if (i < n && i + 3 >= n)
        for (long k = i; k < n; ++k) out[k] = f32_to_bf16(x[k]);
}
__global__ void cast_bf16_f32_kernel(const bf16_t* __restrict__ x, float* __restrict__ out, long n) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    for (; i < n; i += stride) out[i] = bf16_to_f32(x[i]);
}

__global__ void timestep_embedding_kernel(const float* __restrict__ ts, float mult, float* __restrict__ out, int n,
                                          int dim) {
    const int half = dim >> 1;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * half) return;
    const int r = i / half, k = i - r * half;
    const float t = ts[r] * mult;
    const float freq = expf(-logf(10000.0f) * ((float)k / (float)half));
    const float arg = t * freq;
    out[(long)r * dim + k] = cosf(arg);
    out[(long)r * dim + half + k] = sinf(arg);
}

__global__ void make_mod_kernel(const float* __restrict__ tables, const float* __restrict__ ada,
                                float* __restrict__ mod, int B, int L, int J, int D) {
    const long n = (long)B * L * J * D;
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        const int d = i % D;
        long r = i / D;
        const int j = r % J;
        r /= J;
        const int l = r % L;
        const int b = r / L;
        mod[i] = tables[((long)l * J + j) * D + d] + ada[((long)b * J + j) * D + d];
    }
}

__global__ void mask_to_bias_kernel(const int32_t* __restrict__ mask, float* __restrict__ bias, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    // + 0.0f: an attended key (mask 1) gets +0, not the -0 that 0 * -10000 is
    if (i < n) bias[i] = (1.0f - (float)mask[i]) * -10000.0f + 0.0f;
}

// latent [B][C][T] f32 -> tokens [B][T][C] bf16 through a 32x32 LDS transpose tile
__global__ __launch_bounds__(256) void patchify_bf16_kernel(const float* __restrict__ latent,
                                                            bf16_t* __restrict__ tokens, int C, int T) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z;
    const int t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    for (int k = ty; k < 32; k += 8) {
        const int c = c0 + k, t = t0 + tx;
        tile[k][tx] = (c < C && t < T) ? latent[((long)b * C + c) * T + t] : 0.f;
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {
        const int t = t0 + k, c = c0 + tx;
        if (t < T && c < C) tokens[((long)b * T + t) * C + c] = f32_to_bf16(tile[tx][k]);
    }
}
__global__ __launch_bounds__(256) void unpatchify_f32_kernel(const float* __restrict__ tokens,
                                                             float* __restrict__ latent, int C, int T) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z;
    const int t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int k = ty; k < 32; k += 8) {
        const int t = t0 + k, c = c0 + tx;
        tile[k][tx] = (t < T && c < C) ? tokens[((long)b * T + t) * C + c] : 0.f;
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {
        const int c = c0 + k, t = t0 + tx;
        if (c < C && t < T) latent[((long)b * C + c) * T + t] = tile[tx][k];
    }
}

// skip_hw > 0: image-to-video slice step - frame 0 of every channel ([C][F][H*W] layout, skip_hw = H*W, frames = F) keeps its
// value (LTXPipeline.swift:2344-2357)
__global__ void euler_step_kernel(float* __restrict__ latent, const float* __restrict__ vel, float sigma,
                                  float sigma_next, long n, int skip_hw, int frames) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (skip_hw > 0 && (i / skip_hw) % frames == 0) return;
    const float x = latent[i];
    const float den = x - sigma * vel[i];
    latent[i] = (sigma_next > 0.f) ? den + sigma_next * (x - den) / sigma : den;
}
// CFG + Euler step + the next forward's bf16 tokens for both streams of the joint loop (elementwise.h, DualStepJob). Workgroups
// 0 .. wgs0-1 take job 0, the rest job 1 (uniform per workgroup); each job's workgroups stride over its own n. 16-byte loads and
// stores of f32, 8-byte stores of bf16; no LDS. Contraction is off for the whole body and the division is the correctly rounded one:
// every operation rounds on its own, as the reference's separate array ops do.
__global__ __launch_bounds__(256) void dual_step_kernel(const DualStepJob j0, const DualStepJob j1, int wgs0, float sigma, float sigma_next) {
#pragma clang fp contract(off)
    const bool second = (int)blockIdx.x >= wgs0;
    const int wg = second ? (int)blockIdx.x - wgs0 : (int)blockIdx.x;
    const int nwg = second ? (int)gridDim.x - wgs0 : wgs0;
    float* __restrict__ lat = second ? j1.latent : j0.latent;
    const float* vc = second ? j1.v_cond : j0.v_cond;  // may alias v_out: no __restrict__
    const float* __restrict__ vu = second ? j1.v_uncond : j0.v_uncond;
    float* vo = second ? j1.v_out : j0.v_out;
    bf16_t* __restrict__ tok = second ? j1.tokens : j0.tokens;
    const float sm1 = (second ? j1.cfg_scale : j0.cfg_scale) - 1.0f;
    const int form = second ? j1.form : j0.form;
    const int copies = second ? j1.copies : j0.copies;
    const long n = second ? j1.n : j0.n;
    // the frozen prefix (image-to-video: frame 0 in token layout): no Euler form, the conditioning latent re-noised for the NEXT forward
    const long n_keep = second ? j1.n_keep : j0.n_keep;
    const float* __restrict__ ksrc = second ? j1.keep_src : j0.keep_src;
    const float* __restrict__ knoise = second ? j1.keep_noise : j0.keep_noise;
    const float kscale = second ? j1.keep_scale : j0.keep_scale;
    const float sn2 = sigma_next * sigma_next;
    const float ds = sigma_next - sigma;
    const long stride = (long)nwg * 256 * 4;
    for (long i = ((long)wg * 256 + threadIdx.x) * 4; i < n; i += stride) {  // n % 4 == 0: whole vectors only
        const f32x4 x = *(const f32x4*)(lat + i);
        f32x4 v = *(const f32x4*)(vc + i);
        if (vu) {
            const f32x4 u = *(const f32x4*)(vu + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = v[e] - u[e];
                const float g = sm1 * d;
                v[e] = v[e] + g;
            }
        }
        if (vo) *(f32x4*)(vo + i) = v;
        f32x4 y;
        if (i < n_keep) {  // n_keep % 4 == 0: a vector is inside the prefix or outside it
            y = x;
            if (knoise) {
                const f32x4 c = *(const f32x4*)(ksrc + i);
                const f32x4 z = *(const f32x4*)(knoise + i);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float a = kscale * z[e];
                    const float b = a * sn2;
                    y[e] = c[e] + b;
                }
            }
        } else if (form == 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float sv = sigma * v[e];
                const float den = x[e] - sv;
                if (sigma_next > 0.f) {
                    const float back = x[e] - den;
                    const float num = sigma_next * back;
                    const float q = __fdiv_rn(num, sigma);
                    y[e] = den + q;
                } else {
                    y[e] = den;
                }
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float dv = ds * v[e];
                y[e] = x[e] + dv;
            }
        }
        *(f32x4*)(lat + i) = y;
        uint2 pk;
        pk.x = pack_bf16x2(y[0], y[1]);
        pk.y = pack_bf16x2(y[2], y[3]);
        *(uint2*)(tok + i) = pk;
        if (copies == 2) *(uint2*)(tok + n + i) = pk;
    }
}
// The bridge between the two stages of the two-stage video + audio path (elementwise.h, DualRestageJob). Workgroups 0 .. wgs_v-1 each
// take one 32 (t) x 32 (c) tile of the video job, the rest stride over the audio job (uniform per workgroup). Contraction is off for
// the whole body; division and square root are the correctly rounded ones.
__global__ __launch_bounds__(256) void dual_restage_kernel(const DualRestageJob jv, const DualRestageJob ja, int wgs_v) {
#pragma clang fp contract(off)
    __shared__ float tile[32][33];
    if ((int)blockIdx.x >= wgs_v) {  // audio: elementwise, in place
        const int wg = (int)blockIdx.x - wgs_v, nwg = (int)gridDim.x - wgs_v;
        const long n = ja.T * ja.C;  // C % 32 == 0: whole vectors only
        float* __restrict__ lat = ja.latent;
        const float* __restrict__ nz = ja.noise;
        bf16_t* __restrict__ tok = ja.tokens;
        const float s = ja.noise_scale, r = 1.0f - s;
        const long stride = (long)nwg * 256 * 4;
        for (long i = ((long)wg * 256 + threadIdx.x) * 4; i < n; i += stride) {
            f32x4 y = *(const f32x4*)(lat + i);
            if (nz) {
                const f32x4 z = *(const f32x4*)(nz + i);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float a = s * z[e];
                    const float b = r * y[e];
                    y[e] = a + b;
                }
                *(f32x4*)(lat + i) = y;
            }
            uint2 pk;
            pk.x = pack_bf16x2(y[0], y[1]);
            pk.y = pack_bf16x2(y[2], y[3]);
            *(uint2*)(tok + i) = pk;
        }
        return;
    }
    const long T = jv.T, HW = jv.cond ? jv.HW : 0;
    const int C = jv.C;
    const int nt = (int)((T + 31) >> 5);
    const long t0 = (long)((int)blockIdx.x % nt) * 32;
    const int c0 = ((int)blockIdx.x / nt) * 32;  // C % 32 == 0: every channel of the tile exists
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const float s = jv.noise_scale, r = 1.0f - s;
    const long t = t0 + tx;
    for (int k = ty; k < 32; k += 8) {
        const int c = c0 + k;
        float z = 0.f;
        if (t < HW) {  // frame 0 with an image latent
            z = jv.cond[(long)c * HW + t];
            if (jv.cond_noise) {
                const float a = jv.cond_scale * jv.cond_noise[(long)c * HW + t];
                const float b = a * jv.cond_sigma2;
                z = z + b;
            }
        } else if (t < T) {
            const float mu = jv.stats[2 * c], sd = sqrtf(jv.stats[2 * c + 1]);
            const float mur = jv.stats_ref[2 * c], sdr = sqrtf(jv.stats_ref[2 * c + 1]);
            const float d = jv.x[(long)c * T + t] - mu;
            const float den = sd + 1e-8f;
            const float q = __fdiv_rn(d, den);
            const float m = q * sdr;
            z = m + mur;
            if (jv.noise) {
                const float a = s * jv.noise[(long)c * T + t];
                const float b = r * z;
                z = a + b;
            }
        }
        tile[k][tx] = z;
    }
    __syncthreads();
    const int tr = threadIdx.x >> 3, cq = (threadIdx.x & 7) * 4;  // one token row, four channels
    const long to = t0 + tr;
    if (to < T) {
        f32x4 y;
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = tile[cq + e][tr];
        const long o = to * C + c0 + cq;
        *(f32x4*)(jv.latent + o) = y;
        uint2 pk;
        pk.x = pack_bf16x2(y[0], y[1]);
        pk.y = pack_bf16x2(y[2], y[3]);
        *(uint2*)(jv.tokens + o) = pk;
    }
}
__global__ void cfg_combine_kernel(const float* __restrict__ uncond, const float* __restrict__ cond, float sm1,
                                   float* __restrict__ out, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = cond[i] + sm1 * (cond[i] - uncond[i]);
}
// out = ca*(a-b) + cb_sel, where the two guidance forms are expressed as out = a*pa + b*pb
__global__ void lincomb_kernel(const float* __restrict__ a, const float* __restrict__ b, float ca, float cb,
                               float* __restrict__ out, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = ca * a[i] + cb * b[i];
}
__global__ void axpby_kernel(const float* __restrict__ a, const float* __restrict__ b, float ca, float cb,
                             float* __restrict__ out, long n) {
    // out = a*1 ... kept separate from lincomb to preserve the reference's operation order:
    // STG: v + s*(v - vp)  (ca = s, cb = 1 -> out = cb*a + ca*(a-b))
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = cb * a[i] + ca * (a[i] - b[i]);
}
__global__ void ge_kernel(const float* __restrict__ a, const float* __restrict__ b, float g, float* __restrict__ out, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = g * (a[i] - b[i]) + b[i];
}
__global__ void scale_inplace_kernel(float* __restrict__ x, float s, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] *= s;
}

// one workgroup per segment: population mean / variance (two-pass over a segment of n elements)
__global__ __launch_bounds__(1024) void mean_var_kernel(const float* __restrict__ x, long n, float* __restrict__ stats) {
    __shared__ float red[16];
    const float* xs = x + (long)blockIdx.x * n;
    float s = 0.f;
    for (long i = threadIdx.x; i < n; i += blockDim.x) s += xs[i];
    const float mean = block_reduce_sum(s, red) / (float)n;
    float v = 0.f;
    for (long i = threadIdx.x; i < n; i += blockDim.x) {
        const float d = xs[i] - mean;
        v += d * d;
    }
    const float var = block_reduce_sum(v, red) / (float)n;
    if (threadIdx.x == 0) {
        stats[blockIdx.x * 2 + 0] = mean;
        stats[blockIdx.x * 2 + 1] = var;
    }
}
__global__ void guidance_rescale_kernel(float* __restrict__ cfg, const float* __restrict__ st_cfg,
                                        const float* __restrict__ st_cond, float phi, long n_per_batch) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= n_per_batch) return;
    const float eps = 1e-8f;
    const float cfg_std = sqrtf(st_cfg[b * 2 + 1] + eps);
    const float cond_std = sqrtf(st_cond[b * 2 + 1] + eps);
    const float v = cfg[(long)b * n_per_batch + i];
    const float rescaled = v * (cond_std / cfg_std);
    cfg[(long)b * n_per_batch + i] = phi * rescaled + (1.0f - phi) * v;
}
__global__ void adain_kernel(float* __restrict__ x, const float* __restrict__ st_x, const float* __restrict__ st_ref,
                             float factor, long n_per_chan) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int bc = blockIdx.y;
    if (i >= n_per_chan) return;
    const float mu = st_x[bc * 2], sd = sqrtf(st_x[bc * 2 + 1]);
    const float mur = st_ref[bc * 2], sdr = sqrtf(st_ref[bc * 2 + 1]);
    const float v = x[(long)bc * n_per_chan + i];
    const float res = (v - mu) / (sd + 1e-8f) * sdr + mur;
    x[(long)bc * n_per_chan + i] = (factor >= 1.0f) ? res : factor * res + (1.0f - factor) * v;
}

// ---- VAE ----
// latent [C][P] f32 -> channels-last bf16 [P][C], with optional noise blend and per-channel denormalisation
__global__ __launch_bounds__(256) void vae_prepare_kernel(const float* __restrict__ latent, long chan_stride,
                                                          const float* __restrict__ noise, float noise_scale,
                                                          const float* __restrict__ mean,
                                                          const float* __restrict__ std_, bf16_t* __restrict__ out,
                                                          int C, long P) {
    __shared__ float tile[32][33];
    const long p0 = (long)blockIdx.x * 32;
    const int c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int k = ty; k < 32; k += 8) {
        const int c = c0 + k;
        const long p = p0 + tx;
        float v = 0.f;
        if (c < C && p < P) {
            v = latent[(long)c * chan_stride + p];
            if (noise) v = noise[(long)c * chan_stride + p] * noise_scale + (1.0f - noise_scale) * v;
            v = v * std_[c] + mean[c];
        }
        tile[k][tx] = v;
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {
        const long p = p0 + k;
        const int c = c0 + tx;
        if (p < P && c < C) out[p * C + c] = f32_to_bf16(tile[tx][k]);
    }
}

// one wave per position when C <= 256*... generic: a group of G = C/4 lanes (<= 256) per position
template <int LANES_PER_POS, int NJ = 4>
__global__ __launch_bounds__(256) void pixelnorm_silu_kernel(const float* __restrict__ x,
                                                             const float* __restrict__ scale,
                                                             const float* __restrict__ shift,
                                                             bf16_t* __restrict__ out, long P, int C) {
    // each lane owns C/(4*LANES_PER_POS) float4 chunks; LANES_PER_POS lanes cooperate via shuffles (<= 64)
    constexpr int POS_PER_BLOCK = 256 / LANES_PER_POS;
    const int sub = threadIdx.x % LANES_PER_POS;
    const long p = (long)blockIdx.x * POS_PER_BLOCK + threadIdx.x / LANES_PER_POS;
    const int nchunk = C >> 2;
    const bool active = p < P;
    const float* xr = x + (active ? p : 0) * (long)C;
    f32x4 v[NJ];
    float s2 = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = sub + j * LANES_PER_POS;
        if (c < nchunk) {
            v[j] = *(const f32x4*)(xr + c * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) s2 += v[j][e] * v[j][e];
        }
    }
#pragma unroll
    for (int off = LANES_PER_POS >> 1; off > 0; off >>= 1) s2 += __shfl_xor(s2, off, 64);
    const float inv = 1.0f / sqrtf(s2 / (float)C + 1e-8f);
    if (!active) return;
    bf16_t* orow = out + p * (long)C;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = sub + j * LANES_PER_POS;
        if (c < nchunk) {
            f32x4 s4 = f32x4{1.f, 1.f, 1.f, 1.f}, h4 = f32x4{0.f, 0.f, 0.f, 0.f};  // no modulation: the VAE encoder's blocks
            if (scale) {
                s4 = *(const f32x4*)(scale + c * 4);
                h4 = *(const f32x4*)(shift + c * 4);
            }
            f32x4 y;
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = silu_f(v[j][e] * inv * s4[e] + h4[e]);
            uint2 pk;
            pk.x = pack_bf16x2(y[0], y[1]);
            pk.y = pack_bf16x2(y[2], y[3]);
            *(uint2*)(orow + c * 4) = pk;
        }
    }
}

// every modulation table of a decode in one launch (21 of them at a few KB each were 21 launches of ~5 us)
__global__ void vae_make_mods_batch_kernel(const VaeModsBatch b) {
    const VaeModsJob& j = b.job[blockIdx.y];
    const long n = (long)j.rows * j.C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int r = i / j.C;
        j.out[i] = j.table[i] + (j.te ? j.te[i] : 0.f) + ((r & 1) ? 1.0f : 0.f);
    }
}
__global__ void blend_frames_kernel(float* __restrict__ r, const float* __restrict__ nx, int n_frames, long frame_elems) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int f = blockIdx.y;
    if (i >= frame_elems) return;
    const float w = (float)f / (float)n_frames;
    const long o = (long)f * frame_elems + i;
    r[o] = r[o] * (1.0f - w) + nx[o] * w;
}
__global__ void clip01_kernel(float* __restrict__ x, long n) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    for (; i < n; i += stride) x[i] = fminf(fmaxf((x[i] + 1.0f) * 0.5f, 0.f), 1.f);
}

// one workgroup per group: two passes (mean, then variance) over P positions x (C/G) channels
__global__ __launch_bounds__(1024) void groupnorm_stats_kernel(const float* __restrict__ x, long P, int C, int G, float eps,
                                                               float* __restrict__ stats) {
    __shared__ float red[16];
    const int g = blockIdx.x;
    const int cpg = C / G;
    const long n = P * cpg;
    const float* base = x + (long)g * cpg;
    float s = 0.f;
    for (long i = threadIdx.x; i < n; i += blockDim.x) s += base[(i / cpg) * C + (i % cpg)];
    const float mean = block_reduce_sum(s, red) / (float)n;
    float v = 0.f;
    for (long i = threadIdx.x; i < n; i += blockDim.x) {
        const float d = base[(i / cpg) * C + (i % cpg)] - mean;
        v += d * d;
    }
    const float var = block_reduce_sum(v, red) / (float)n;
    if (threadIdx.x == 0) {
        stats[g * 2 + 0] = mean;
        stats[g * 2 + 1] = 1.0f / sqrtf(var + eps);
    }
}
__global__ void groupnorm_apply_kernel(const float* __restrict__ x, const float* __restrict__ stats,
                                       const float* __restrict__ w, const float* __restrict__ b,
                                       const float* __restrict__ resid, int act_silu, float* __restrict__ out_f32,
                                       bf16_t* __restrict__ out_bf16, long n, int C, int G) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    const int cpg = C / G;
    for (; i < n; i += stride) {
        const int c = i % C;
        const int g = c / cpg;
        float y = (x[i] - stats[g * 2]) * stats[g * 2 + 1] * w[c] + b[c];
        if (resid) y += resid[i];
        if (act_silu) y = silu_f(y);
        if (out_f32) out_f32[i] = y;
        if (out_bf16) out_bf16[i] = f32_to_bf16(y);
    }
}
__global__ __launch_bounds__(256) void upscaler_finish_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                              const float* __restrict__ std_, float* __restrict__ out,
                                                              long P, int C) {
    __shared__ float tile[32][33];
    const long p0 = (long)blockIdx.x * 32;
    const int c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int k = ty; k < 32; k += 8) {
        const long p = p0 + k;
        const int c = c0 + tx;
        tile[k][tx] = (p < P && c < C) ? (x[p * C + c] - mean[c]) / std_[c] : 0.f;
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {
        const int c = c0 + k;
        const long p = p0 + tx;
        if (c < C && p < P) out[(long)c * P + p] = tile[tx][k];
    }
}

inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

}  // namespace

void launch_norm_mod(const NormModArgs& a, hipStream_t stream) {
    LTX_REQUIRE(a.D % 4 == 0 && a.D <= MAXV * 1024 && a.ldx % 4 == 0 && a.ldo % 4 == 0, "norm_mod: D=%d ldx=%ld ldo=%ld", a.D, a.ldx, a.ldo);
    LTX_REQUIRE((a.scale == nullptr) == (a.shift == nullptr), "norm_mod: scale/shift must both be set or both null");
    const int rpb = a.rows_per_batch < 1 ? 1 : a.rows_per_batch;
#ifdef LTX_EXPERIMENTS  // timing ablation (experiments library only): LTX_ABL_ROWS bit 0 drops this pass after the first 400 calls - the
    // buffers keep realistic stale values, so what the step then gains is the upper bound of any fusion of the pass (profiles/r04_row_ablation.txt)
    { const int abl = ltx_opt(OPT_ABL_ROWS); static long calls = 0; if ((abl & 1) && ++calls > 400) return; }
#endif
    ProfScope prof(PROF_ELEM, (double)a.rows * a.D * (4 + 2), stream);  // algorithmic bytes: f32 row in, bf16 row out
    // rows per workgroup: 4 share one fetch of the modulation vectors; at 1536 rows that is 384 workgroups = 1.5 per CU, and two rows per
    // workgroup (768 = 3 per CU) are 10 % faster (9.15 vs 10.2 us alone, 36.39 vs 36.53 ms per forward); no difference from 6144 rows up
    const int r_raw = ltx_opt(OPT_NORM_ROWS);  // A/B option "norm_rows": 2 or 4, anything else is ignored
    const int r_env = (r_raw == 2 || r_raw == 4) ? r_raw : 0;
    const int R_rows = r_env ? r_env : (a.rows <= 3072 ? 2 : 4);
    if (a.norm_kind == LTX_NORM_RMS && a.scale && !a.row_map && a.D == 4096 && a.rows >= 512 && rpb % R_rows == 0) {
#define LTX_ROWS_LAUNCH(R)                                                                                                                   \
    hipLaunchKernelGGL((norm_mod_rows_kernel<4, R>), dim3((a.rows + R - 1) / R), dim3(256), 0, stream, a.x, a.ldx, a.scale, a.shift, a.mod_bstride, \
                       rpb, a.out, a.ldo, a.rows, a.eps, a.round_norm_bf16)
        if (R_rows == 2) LTX_ROWS_LAUNCH(2);
        else LTX_ROWS_LAUNCH(4);
#undef LTX_ROWS_LAUNCH
        HIP_CHECK(hipGetLastError());
        return;
    }
#define LTX_NORM_LAUNCH(NV)                                                                                                            \
    hipLaunchKernelGGL(norm_mod_kernel<NV>, dim3(a.rows), dim3(256), 0, stream, a.x, a.ldx, a.scale, a.shift, a.mod_bstride, rpb, a.out, \
                       a.ldo, a.D, a.norm_kind, a.eps, a.round_norm_bf16, a.row_map)
    if (a.D <= 1024) LTX_NORM_LAUNCH(1);
    else if (a.D <= 2048) LTX_NORM_LAUNCH(2);
    else if (a.D <= 4096) LTX_NORM_LAUNCH(4);
    else LTX_NORM_LAUNCH(8);
#undef LTX_NORM_LAUNCH
    HIP_CHECK(hipGetLastError());
}

void launch_norm_mod2(const NormMod2Job& video, const NormMod2Job& audio, float eps, hipStream_t stream) {
    int maxD = 0;
    for (const NormMod2Job* j : {&video, &audio}) {
        LTX_REQUIRE(j->rows >= 0, "norm_mod2: rows=%d", j->rows);
        if (j->rows == 0) continue;
        LTX_REQUIRE(j->x && j->out0 && j->out1, "norm_mod2: null row or output pointer");
        LTX_REQUIRE(j->D >= 4 && j->D % 4 == 0 && j->D <= MAXV * 1024 && j->ldx % 4 == 0 && j->ldo % 4 == 0 && j->ldx >= j->D && j->ldo >= j->D,
                    "norm_mod2: D=%d ldx=%ld ldo=%ld", j->D, j->ldx, j->ldo);
        LTX_REQUIRE((j->scale0 == nullptr) == (j->shift0 == nullptr) && (j->scale1 == nullptr) == (j->shift1 == nullptr),
                    "norm_mod2: scale/shift must both be set or both null");
        LTX_REQUIRE(j->rows_per_batch >= 1 && j->mod_bstride >= 0, "norm_mod2: rows_per_batch=%d mod_bstride=%ld", j->rows_per_batch, j->mod_bstride);
        if (j->D > maxD) maxD = j->D;
    }
    const long total = (long)video.rows + audio.rows;
    LTX_REQUIRE(total <= 0x7fffffffL, "norm_mod2: %ld rows", total);
    if (total == 0) return;
    ProfScope prof(PROF_ELEM, ((double)video.rows * video.D + (double)audio.rows * audio.D) * (4 + 2 + 2), stream);  // f32 row in, two bf16 rows out
    NormMod2Job j0 = video, j1 = audio;
    if (j0.rows_per_batch < 1) j0.rows_per_batch = 1;  // an empty job is never indexed, but never divided by zero either
    if (j1.rows_per_batch < 1) j1.rows_per_batch = 1;
#define LTX_NORM2_LAUNCH(NV) hipLaunchKernelGGL(norm_mod2_kernel<NV>, dim3((unsigned)total), dim3(256), 0, stream, j0, j1, eps)
    if (maxD <= 1024) LTX_NORM2_LAUNCH(1);
    else if (maxD <= 2048) LTX_NORM2_LAUNCH(2);
    else if (maxD <= 4096) LTX_NORM2_LAUNCH(4);
    else LTX_NORM2_LAUNCH(8);
#undef LTX_NORM2_LAUNCH
    HIP_CHECK(hipGetLastError());
}

namespace {
// the generic kernel: NP pair chunks per thread from D
template <int HD, bool XB>
void launch_qk_generic(const QkJob& j0, const QkJob& j1, const QkNormRopeArgs& a, dim3 grid, int t, hipStream_t stream) {
#define LTX_QK_LAUNCH(NP) hipLaunchKernelGGL((qknorm_rope_kernel<HD, NP, XB>), grid, dim3(256), 0, stream, j0, j1, a.cos, a.sin, t, a.D, a.eps)
    if (a.D <= 2048) LTX_QK_LAUNCH(1);
    else if (a.D <= 4096) LTX_QK_LAUNCH(2);
    else LTX_QK_LAUNCH(4);
#undef LTX_QK_LAUNCH
}
// the kernel of a launch, for rows of one type
template <bool XB>
void launch_qk(const QkNormRopeArgs& a, hipStream_t stream) {
    const int jobs = a.job[1].x ? 2 : 1;
    const QkJob j0{(const float*)a.job[0].x, a.job[0].w, a.job[0].out, a.ldx, a.ldo, a.job[0].out_scale},
        j1{(const float*)a.job[1].x, a.job[1].w, a.job[1].out, a.ldx, a.ldo, a.job[1].out_scale};
    const dim3 grid(a.rows, jobs);
    const int t = a.T < 1 ? 1 : a.T;
    if (a.head_dim == 64) return launch_qk_generic<64, XB>(j0, j1, a, grid, t, stream);
    const bool no_pair = ltx_opt(OPT_QKNORM_NO_PAIR) != 0;  // A/B option "qknorm_no_pair"
    constexpr int R = 2;  // rows per workgroup at full width; 1 and 3: within the run-to-run noise of the forward (round 3)
    const dim3 grid_r((a.rows + R - 1) / R, jobs);
    if (a.D == 4096 && a.rows >= 512 && jobs == 2 && a.cos && !no_pair)  // q and k of the same tokens: one fetch of the tables (2.64 -> 2.54 ms of row passes per step)
        hipLaunchKernelGGL((qknorm_rope_pair_kernel<R, XB>), dim3(grid_r.x), dim3(256), 0, stream, j0, j1, a.cos, a.sin, t, a.rows, a.eps);
    else if (a.D == 4096 && a.rows >= 512)  // the DiT at full width: R rows per workgroup share one fetch of the norm weights
        hipLaunchKernelGGL((qknorm_rope_rows_kernel<R, XB>), grid_r, dim3(256), 0, stream, j0, j1, a.cos, a.sin, t, a.rows, a.eps);
    else
        launch_qk_generic<128, XB>(j0, j1, a, grid, t, stream);
}
}  // namespace

void launch_qknorm_rope(const QkNormRopeArgs& a, hipStream_t stream) {
    LTX_REQUIRE(a.head_dim == 64 || a.head_dim == 128, "qknorm_rope: head dim %d (64 or 128)", a.head_dim);
    LTX_REQUIRE(a.D % a.head_dim == 0 && a.D <= MAXV * 1024 && a.ldx % 4 == 0 && a.ldo % 4 == 0, "qknorm_rope: D=%d", a.D);
    const int jobs = a.job[1].x ? 2 : 1;
#ifdef LTX_EXPERIMENTS  // timing ablation (head dim 128): LTX_ABL_ROWS bit 1 drops the q|k pass, bit 2 the cross-attention q pass, after two forwards' worth of calls
    if (a.head_dim == 128) { const int abl = ltx_opt(OPT_ABL_ROWS); static long c2 = 0, c1 = 0;
      if (jobs == 2 && (abl & 2) && ++c2 > 200) return; if (jobs == 1 && (abl & 4) && ++c1 > 300) return; }
#endif
    // algorithmic bytes: the f32 (or bf16) rows in, the bf16 rows out, cos/sin rows once per job
    ProfScope prof(PROF_ELEM, (double)a.rows * a.D * jobs * ((a.x_bf16 ? 2 : 4) + 2 + (a.cos ? 4 : 0)), stream);
    if (a.x_bf16) launch_qk<true>(a, stream);
    else launch_qk<false>(a, stream);
    HIP_CHECK(hipGetLastError());
}

void launch_cast_f32_bf16(const float* x, bf16_t* out, long n, hipStream_t stream) {
    const int grid = cdiv(n, 4 * 256) < 2048 ? (cdiv(n, 4 * 256) < 1 ? 1 : cdiv(n, 4 * 256)) : 2048;
    hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3(grid), dim3(256), 0, stream, x, out, n);
    HIP_CHECK(hipGetLastError());
}
void launch_cast_bf16_f32(const bf16_t* x, float* out, long n, hipStream_t stream) {
    const int grid = cdiv(n, 256) < 4096 ? (cdiv(n, 256) < 1 ? 1 : cdiv(n, 256)) : 4096;
    hipLaunchKernelGGL(cast_bf16_f32_kernel, dim3(grid), dim3(256), 0, stream, x, out, n);
    HIP_CHECK(hipGetLastError());
}
void launch_timestep_embedding(const float* ts, float mult, float* out, int n, int dim, hipStream_t stream) {
    hipLaunchKernelGGL(timestep_embedding_kernel, dim3(cdiv((long)n * (dim / 2), 256)), dim3(256), 0, stream, ts, mult, out, n, dim);
    HIP_CHECK(hipGetLastError());
}
void launch_make_mod(const float* tables, const float* ada, float* mod, int B, int L, int J, int D, hipStream_t stream) {
    const long n = (long)B * L * J * D;
    const int grid = cdiv(n, 256) < 2048 ? cdiv(n, 256) : 2048;
    hipLaunchKernelGGL(make_mod_kernel, dim3(grid), dim3(256), 0, stream, tables, ada, mod, B, L, J, D);
    HIP_CHECK(hipGetLastError());
}
void launch_mask_to_bias(const int32_t* mask, float* bias, long n, hipStream_t stream) {
    hipLaunchKernelGGL(mask_to_bias_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, mask, bias, n);
    HIP_CHECK(hipGetLastError());
}
// [N][D][Tn] -> [D][ld]: one 16-byte piece (8 keys) per thread, rows stay contiguous on both sides
__global__ __launch_bounds__(256) void sp_vt_interleave_kernel(const bf16_t* __restrict__ g, bf16_t* __restrict__ vt, int N, int D,
                                                               int Tn, long ld) {
    const int per_row = Tn >> 3;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long total = (long)N * D * per_row;
    if (i >= total) return;
    const int c = (int)(i % per_row);
    const long rd = i / per_row;
    const int d = (int)(rd % D);
    const int r = (int)(rd / D);
    const uint4 v = *(const uint4*)(g + ((long)r * D + d) * Tn + c * 8);
    *(uint4*)(vt + (long)d * ld + (long)r * Tn + c * 8) = v;
}

void launch_sp_vt_interleave(const bf16_t* gathered, bf16_t* vt, int N, int D, int Tn, long ld, hipStream_t stream) {
    LTX_REQUIRE(Tn % 8 == 0 && ld % 8 == 0, "sp_vt_interleave: Tn=%d ld=%ld must be multiples of 8", Tn, ld);
    const long total = (long)N * D * (Tn >> 3);
    hipLaunchKernelGGL(sp_vt_interleave_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, gathered, vt, N, D, Tn, ld);
    HIP_CHECK(hipGetLastError());
}

void launch_patchify_bf16(const float* latent, bf16_t* tokens, int B, int C, int T, hipStream_t stream) {
    hipLaunchKernelGGL(patchify_bf16_kernel, dim3(cdiv(T, 32), cdiv(C, 32), B), dim3(256), 0, stream, latent, tokens, C, T);
    HIP_CHECK(hipGetLastError());
}
void launch_unpatchify_f32(const float* tokens, float* latent, int B, int C, int T, hipStream_t stream) {
    hipLaunchKernelGGL(unpatchify_f32_kernel, dim3(cdiv(T, 32), cdiv(C, 32), B), dim3(256), 0, stream, tokens, latent, C, T);
    HIP_CHECK(hipGetLastError());
}
void launch_euler_step(float* latent, const float* velocity, float sigma, float sigma_next, long n, hipStream_t stream, int skip_hw,
                       int frames) {
    hipLaunchKernelGGL(euler_step_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, latent, velocity, sigma, sigma_next, n, skip_hw,
                       frames < 1 ? 1 : frames);
    HIP_CHECK(hipGetLastError());
}

namespace {
// latent[c][0][hw] = cond[c][hw] (+ s * noise[c][hw])   (LTXPipeline.swift:2092-2094, :2225-2229)
// the reference evaluates cond + (scale * noise) * sigma^2 as three separate f32 ops: no fused multiply-add here
__global__ void set_frame0_kernel(float* __restrict__ latent, const float* __restrict__ cond, const float* __restrict__ noise,
                                  float scale, float sigma2, int C, int F, int HW) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)C * HW) return;
    const long c = i / HW, hw = i - c * HW;
    float v = cond[i];
    if (noise) {
        const float a = scale * noise[i];
        const float b = a * sigma2;
        v = v + b;
    }
    latent[(c * F) * HW + hw] = v;
}
// row_map[b*T + t] = b*G + (t < first ? 1 : 0): tokens of frame 0 use timestep group 1 (sigma 0), the rest group 0
__global__ void i2v_rowmap_kernel(int32_t* __restrict__ row_map, int B, int T, int first, int G) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * T) return;
    const int b = (int)(i / T), t = (int)(i - (long)b * T);
    row_map[i] = b * G + (t < first ? 1 : 0);
}
// ts[b*G + g] = g == 0 ? sigma : 0 for b < B (the video timesteps of launch_i2v_rowmap's groups), then B audio timesteps = sigma
__global__ void i2v_timesteps_kernel(float* __restrict__ ts, int B, int G, float sigma) {
    const int i = threadIdx.x;
    if (i >= B * G + B) return;
    ts[i] = (i < B * G && i % G != 0) ? 0.f : sigma;
}
}  // namespace
void launch_i2v_timesteps(float* ts, int B, int G, float sigma, hipStream_t stream) {
    LTX_REQUIRE(B >= 1 && G >= 1 && B * G + B <= 64, "i2v_timesteps: B=%d G=%d", B, G);
    hipLaunchKernelGGL(i2v_timesteps_kernel, dim3(1), dim3(64), 0, stream, ts, B, G, sigma);
    HIP_CHECK(hipGetLastError());
}
void launch_set_frame0(float* latent, const float* cond, const float* noise, float scale, float sigma2, int C, int F, int HW,
                       hipStream_t stream) {
    hipLaunchKernelGGL(set_frame0_kernel, dim3(cdiv((long)C * HW, 256)), dim3(256), 0, stream, latent, cond, noise, scale, sigma2, C, F, HW);
    HIP_CHECK(hipGetLastError());
}
void launch_i2v_rowmap(int32_t* row_map, int B, int T, int first, int G, hipStream_t stream) {
    hipLaunchKernelGGL(i2v_rowmap_kernel, dim3(cdiv((long)B * T, 256)), dim3(256), 0, stream, row_map, B, T, first, G);
    HIP_CHECK(hipGetLastError());
}
void launch_cfg_combine(const float* uncond, const float* cond, float scale, float* out, long n, hipStream_t stream) {
    hipLaunchKernelGGL(cfg_combine_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, uncond, cond, scale - 1.0f, out, n);
    HIP_CHECK(hipGetLastError());
}
void launch_dual_step(const DualStepJob& video, const DualStepJob& audio, float sigma, float sigma_next, hipStream_t stream) {
    LTX_REQUIRE(sigma > 0.f, "dual_step: sigma=%g must be positive", (double)sigma);
    long bytes = 0;
    for (const DualStepJob* j : {&video, &audio}) {
        LTX_REQUIRE(j->n >= 0 && j->n % 4 == 0, "dual_step: n=%ld must be a multiple of 4", j->n);
        if (j->n == 0) continue;
        LTX_REQUIRE(j->latent && j->v_cond && j->tokens, "dual_step: null latent, velocity or token pointer");
        LTX_REQUIRE(j->copies >= 1 && j->copies <= 2, "dual_step: copies=%d (1 .. 2)", j->copies);
        LTX_REQUIRE(j->form >= 0 && j->form <= 1, "dual_step: form=%d (0 .. 1)", j->form);
        LTX_REQUIRE(j->n_keep >= 0 && j->n_keep <= j->n && j->n_keep % 4 == 0, "dual_step: n_keep=%ld (a multiple of 4, 0 .. n=%ld)", j->n_keep, j->n);
        LTX_REQUIRE(!j->keep_noise || j->keep_src, "dual_step: keep_noise needs keep_src");
        bytes += j->n * (4 + 4 + (j->v_uncond ? 4 : 0) + 4 + (j->v_out ? 4 : 0) + 2 * j->copies);
    }
    // per job: one workgroup per 1024 elements, at most kMaxWgs (half the CUs each; the loop strides over the rest)
    constexpr long kMaxWgs = 128;
    auto wgs = [=](long n) { return (int)std::min<long>(cdiv(n, 4 * 256), kMaxWgs); };
    const int w0 = wgs(video.n), w1 = wgs(audio.n);
    if (w0 + w1 == 0) return;
    ProfScope prof(PROF_ELEM, (double)bytes, stream);
    hipLaunchKernelGGL(dual_step_kernel, dim3((unsigned)(w0 + w1)), dim3(256), 0, stream, video, audio, w0, sigma, sigma_next);
    HIP_CHECK(hipGetLastError());
}
void dual_restage_check(const DualRestageJob& video, const DualRestageJob& audio) {
    LTX_REQUIRE(video.T == 0 || video.x, "dual_restage: the video job needs its input latent x");
    LTX_REQUIRE(audio.T == 0 || (!audio.x && !audio.cond && !audio.cond_noise && !audio.stats && !audio.stats_ref),
                "dual_restage: the audio job works in place: x, cond, cond_noise, stats and stats_ref must be null");
    for (const DualRestageJob* j : {&video, &audio}) {
        LTX_REQUIRE(j->T >= 0 && j->T <= (1L << 24), "dual_restage: T=%ld (0 .. 2^24)", j->T);
        if (j->T == 0) continue;
        LTX_REQUIRE(j->C >= 32 && j->C <= 4096 && j->C % 32 == 0, "dual_restage: C=%d must be a multiple of 32 (32 .. 4096)", j->C);
        LTX_REQUIRE(j->latent && j->tokens, "dual_restage: null latent or token pointer");
        LTX_REQUIRE(((uintptr_t)j->latent & 15) == 0 && ((uintptr_t)j->tokens & 7) == 0, "dual_restage: latent must be 16-byte and tokens 8-byte aligned");
        LTX_REQUIRE((j->renoise != 0) == (j->noise != nullptr), "dual_restage: noise must be given exactly when a noise scale is (renoise=%d)", j->renoise);
    }
    if (video.T > 0) {
        LTX_REQUIRE(video.stats && video.stats_ref, "dual_restage: null statistics");
        LTX_REQUIRE(!video.cond_noise || video.cond, "dual_restage: cond_noise needs cond");
        LTX_REQUIRE(!video.cond || (video.HW >= 1 && video.HW <= video.T), "dual_restage: HW=%ld (1 .. T=%ld)", video.HW, video.T);
    }
}
void launch_dual_restage(const DualRestageJob& video, const DualRestageJob& audio, hipStream_t stream) {
    dual_restage_check(video, audio);
    const long nv = video.T * video.C, na = audio.T * audio.C;
    const int wv = video.T ? (int)cdiv(video.T, 32) * (video.C / 32) : 0;
    const int wa = (int)std::min<long>(cdiv(na, 4 * 256), 128);
    if (wv + wa == 0) return;
    // algorithmic bytes. video: x and the noise in, f32 + bf16 out; audio: the latent in (and, re-noised, the noise in and the latent out), bf16 out
    ProfScope prof(PROF_ELEM, (double)nv * (4 + (video.noise ? 4 : 0) + 4 + 2) + (double)na * (4 + (audio.noise ? 8 : 0) + 2), stream);
    hipLaunchKernelGGL(dual_restage_kernel, dim3((unsigned)(wv + wa)), dim3(256), 0, stream, video, audio, wv);
    HIP_CHECK(hipGetLastError());
}
void launch_axpby(const float* a, const float* b, float ca, float cb, float* out, long n, hipStream_t stream) {
    hipLaunchKernelGGL(axpby_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, a, b, ca, cb, out, n);
    HIP_CHECK(hipGetLastError());
}
void launch_ge(const float* a, const float* b, float g, float* out, long n, hipStream_t stream) {
    hipLaunchKernelGGL(ge_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, a, b, g, out, n);
    HIP_CHECK(hipGetLastError());
}
void launch_lincomb(const float* a, const float* b, float ca, float cb, float* out, long n, hipStream_t stream) {
    hipLaunchKernelGGL(lincomb_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, a, b, ca, cb, out, n);
    HIP_CHECK(hipGetLastError());
}
void launch_scale_inplace(float* x, float s, long n, hipStream_t stream) {
    hipLaunchKernelGGL(scale_inplace_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, x, s, n);
    HIP_CHECK(hipGetLastError());
}
void launch_mean_var(const float* x, long n_per_batch, int B, float* stats, hipStream_t stream) {
    hipLaunchKernelGGL(mean_var_kernel, dim3(B), dim3(1024), 0, stream, x, n_per_batch, stats);
    HIP_CHECK(hipGetLastError());
}
void launch_guidance_rescale(float* cfg, const float* stats_cfg, const float* stats_cond, float phi, long n_per_batch,
                             int B, hipStream_t stream) {
    hipLaunchKernelGGL(guidance_rescale_kernel, dim3(cdiv(n_per_batch, 256), B), dim3(256), 0, stream, cfg, stats_cfg, stats_cond, phi, n_per_batch);
    HIP_CHECK(hipGetLastError());
}
void launch_adain(float* x, const float* stats_x, const float* stats_ref, float factor, long n_per_chan, int BC,
                  hipStream_t stream) {
    hipLaunchKernelGGL(adain_kernel, dim3(cdiv(n_per_chan, 256), BC), dim3(256), 0, stream, x, stats_x, stats_ref, factor, n_per_chan);
    HIP_CHECK(hipGetLastError());
}
void launch_vae_prepare(const float* latent, long chan_stride, const float* noise, float noise_scale, const float* mean,
                        const float* std_, bf16_t* out, int C, long P, hipStream_t stream) {
    hipLaunchKernelGGL(vae_prepare_kernel, dim3(cdiv(P, 32), cdiv(C, 32)), dim3(256), 0, stream, latent, chan_stride, noise, noise_scale, mean, std_, out, C, P);
    HIP_CHECK(hipGetLastError());
}
void launch_vae_make_mods_batch(const VaeModsBatch& b, hipStream_t stream) {
    LTX_REQUIRE(b.n >= 1 && b.n <= VaeModsBatch::MAX_JOBS, "vae_make_mods_batch: %d jobs", b.n);
    hipLaunchKernelGGL(vae_make_mods_batch_kernel, dim3(4, b.n), dim3(256), 0, stream, b);
    HIP_CHECK(hipGetLastError());
}
void launch_blend_frames(float* r, const float* nx, int n_frames, long frame_elems, hipStream_t stream) {
    hipLaunchKernelGGL(blend_frames_kernel, dim3(cdiv(frame_elems, 256), n_frames), dim3(256), 0, stream, r, nx, n_frames, frame_elems);
    HIP_CHECK(hipGetLastError());
}
void launch_clip01(float* x, long n, hipStream_t stream) {
    const int grid = cdiv(n, 256) < 65535 * 16 ? cdiv(n, 256) : 65535 * 16;
    hipLaunchKernelGGL(clip01_kernel, dim3(grid), dim3(256), 0, stream, x, n);
    HIP_CHECK(hipGetLastError());
}
void launch_pixelnorm_silu(const float* x, const float* scale, const float* shift, bf16_t* out, long P, int C,
                           hipStream_t stream) {
    LTX_REQUIRE(C % 4 == 0 && C <= 2048, "pixelnorm: C=%d", C);
    LTX_REQUIRE((scale == nullptr) == (shift == nullptr), "pixelnorm: scale/shift must both be set or both null");
    if (C > 1024) {  // the encoder's 2048-channel mid block: 8 chunks per lane
        hipLaunchKernelGGL((pixelnorm_silu_kernel<64, 8>), dim3(cdiv(P, 4)), dim3(256), 0, stream, x, scale, shift, out, P, C);
        HIP_CHECK(hipGetLastError());
        return;
    }
    // lanes per position: enough that each lane holds <= 4 float4 chunks, power of two, <= 64
    const int nchunk = C / 4;
    int lpp = 1;
    while (lpp * 4 < nchunk) lpp <<= 1;
    if (lpp < 8) lpp = 8;
    LTX_REQUIRE(lpp <= 64, "pixelnorm: C=%d too wide", C);
#define PN_LAUNCH(L)                                                                                              \
    hipLaunchKernelGGL((pixelnorm_silu_kernel<L>), dim3(cdiv(P, 256 / L)), dim3(256), 0, stream, x, scale, shift, out, P, C)
    if (lpp == 8) PN_LAUNCH(8);
    else if (lpp == 16) PN_LAUNCH(16);
    else if (lpp == 32) PN_LAUNCH(32);
    else PN_LAUNCH(64);
#undef PN_LAUNCH
    HIP_CHECK(hipGetLastError());
}

void launch_groupnorm_stats(const float* x, long P, int C, int G, float eps, float* stats, hipStream_t stream) {
    LTX_REQUIRE(C % G == 0, "groupnorm: C=%d not divisible by G=%d", C, G);
    hipLaunchKernelGGL(groupnorm_stats_kernel, dim3(G), dim3(1024), 0, stream, x, P, C, G, eps, stats);
    HIP_CHECK(hipGetLastError());
}
void launch_groupnorm_apply(const float* x, const float* stats, const float* w, const float* b, const float* resid,
                            int act_silu, float* out_f32, bf16_t* out_bf16, long P, int C, int G, hipStream_t stream) {
    const long n = P * C;
    const int grid = cdiv(n, 256) < 4096 ? cdiv(n, 256) : 4096;
    hipLaunchKernelGGL(groupnorm_apply_kernel, dim3(grid), dim3(256), 0, stream, x, stats, w, b, resid, act_silu, out_f32, out_bf16, n, C, G);
    HIP_CHECK(hipGetLastError());
}
void launch_upscaler_finish(const float* x, const float* mean, const float* std_, float* out, long P, int C, hipStream_t stream) {
    hipLaunchKernelGGL(upscaler_finish_kernel, dim3(cdiv(P, 32), cdiv(C, 32)), dim3(256), 0, stream, x, mean, std_, out, P, C);
    HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------------------------
// text-embedding connector kernels
// ---------------------------------------------------------------------------------------------------------------
namespace {
constexpr int FE_CHUNK = 16384;  // elements of one (state, batch) plane per workgroup

LTX_DEVFN bool fe_token_valid(const int32_t* mrow, int t, int T, int n_valid, int padding_right) {
    // the reference rebuilds the mask from the sequence length and the padding side (LTXTextEncoder.swift:75-84)
    return padding_right ? (t < n_valid) : (t >= T - n_valid);
}

__global__ __launch_bounds__(256) void fe_stats_partial_kernel(const bf16_t* __restrict__ hidden, const int32_t* __restrict__ mask,
                                                               int B, int T, int D, int padding_right,
                                                               float* __restrict__ partials, int nchunk) {
    __shared__ float red[3][4];
    __shared__ int s_nvalid;
    const int plane = blockIdx.y;  // l*B + b
    const int b = plane % B;
    if (threadIdx.x == 0) s_nvalid = 0;
    __syncthreads();
    int cnt = 0;
    for (int t = threadIdx.x; t < T; t += 256) cnt += mask[(long)b * T + t] != 0;
    atomicAdd(&s_nvalid, cnt);
    __syncthreads();
    const int n_valid = s_nvalid;
    const bf16_t* x = hidden + (long)plane * T * D;
    const long total = (long)T * D;
    const long beg = (long)blockIdx.x * FE_CHUNK;
    const long end = beg + FE_CHUNK < total ? beg + FE_CHUNK : total;
    float s = 0.f, mn = INFINITY, mx = -INFINITY;
    for (long i = beg + threadIdx.x * 8; i < end; i += 256 * 8) {
        const int t = (int)(i / D);  // D % 8 == 0: the 8 elements share a token
        if (!fe_token_valid(nullptr, t, T, n_valid, padding_right)) continue;
        const uint4 raw = *(const uint4*)(x + i);
        const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float a = bf16_to_f32((bf16_t)(w[k] & 0xffff)), c = bf16_to_f32((bf16_t)(w[k] >> 16));
            s += a + c;
            mn = fminf(mn, fminf(a, c));
            mx = fmaxf(mx, fmaxf(a, c));
        }
    }
    s = wave_reduce_sum(s);
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o, 64));
        mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    }
    const int lane = threadIdx.x & 63, w_ = threadIdx.x >> 6;
    if (lane == 0) {
        red[0][w_] = s;
        red[1][w_] = mn;
        red[2][w_] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float* p = partials + ((long)plane * nchunk + blockIdx.x) * 3;
        p[0] = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        p[1] = fminf(fminf(red[1][0], red[1][1]), fminf(red[1][2], red[1][3]));
        p[2] = fmaxf(fmaxf(red[2][0], red[2][1]), fmaxf(red[2][2], red[2][3]));
    }
}

__global__ void fe_stats_final_kernel(const float* __restrict__ partials, const int32_t* __restrict__ mask, int B, int T, int D,
                                      float eps, int nchunk, float* __restrict__ stats, int planes) {
    const int plane = blockIdx.x * blockDim.x + threadIdx.x;
    if (plane >= planes) return;
    const int b = plane % B;
    int n_valid = 0;
    for (int t = 0; t < T; ++t) n_valid += mask[(long)b * T + t] != 0;
    double s = 0.0;  // fixed order over the chunks
    float mn = INFINITY, mx = -INFINITY;
    for (int c = 0; c < nchunk; ++c) {
        const float* p = partials + ((long)plane * nchunk + c) * 3;
        s += (double)p[0];
        mn = fminf(mn, p[1]);
        mx = fmaxf(mx, p[2]);
    }
    const float denom = (float)n_valid * (float)D + eps;
    stats[plane * 2 + 0] = (float)s / denom;
    stats[plane * 2 + 1] = (mx - mn) + eps;
}

__global__ __launch_bounds__(256) void fe_norm_concat_kernel(const bf16_t* __restrict__ hidden, const int32_t* __restrict__ mask,
                                                             const float* __restrict__ stats, int states, int B, int T, int D,
                                                             int padding_right, bf16_t* __restrict__ out) {
    __shared__ int s_nvalid;
    const int bt = blockIdx.x;  // b*T + t
    const int b = bt / T, t = bt - b * T;
    if (threadIdx.x == 0) s_nvalid = 0;
    __syncthreads();
    int cnt = 0;
    for (int i = threadIdx.x; i < T; i += 256) cnt += mask[(long)b * T + i] != 0;
    atomicAdd(&s_nvalid, cnt);
    __syncthreads();
    const bool valid = fe_token_valid(nullptr, t, T, s_nvalid, padding_right);
    bf16_t* orow = out + (long)bt * D * states;
    const long plane_stride = (long)B * T * D;
    for (int d = threadIdx.x; d < D; d += 256) {
        const bf16_t* x = hidden + ((long)b * T + t) * D + d;
        bf16_t* o = orow + (long)d * states;
        for (int l = 0; l < states; ++l) {
            float v = 0.f;
            if (valid) {
                const float xv = bf16_to_f32(x[(long)l * plane_stride]);
                v = 8.0f * (xv - stats[(l * B + b) * 2 + 0]) / stats[(l * B + b) * 2 + 1];
            }
            o[l] = f32_to_bf16(v);
        }
    }
}

__global__ void register_plan_kernel(const int32_t* __restrict__ mask, int T, int32_t* __restrict__ src) {
    // one thread per batch row: T <= a few thousand, runs once per prompt
    const int b = blockIdx.x;
    if (threadIdx.x != 0) return;
    const int32_t* m = mask + (long)b * T;
    int32_t* s = src + (long)b * T;
    int n = 0;
    for (int t = 0; t < T; ++t)
        if (m[t] != 0) s[n++] = t;  // valid tokens first, in order
    for (int t = 0; t < T; ++t)
        if (m[t] == 0) s[n++] = t;  // padded tokens after them (never kept unless the padding is on the right)
    for (int p = 0; p < T; ++p)
        if (m[T - 1 - p] == 0) s[p] = -1;  // reverse(valid)[p] == 0 -> learnable register
}

__global__ __launch_bounds__(256) void register_gather_kernel(const bf16_t* __restrict__ enc, const float* __restrict__ registers,
                                                              const int32_t* __restrict__ src, int T, int D, int R,
                                                              float* __restrict__ x) {
    const int bp = blockIdx.x;
    const int b = bp / T, p = bp - b * T;
    const int sidx = src[bp];
    float* o = x + (long)bp * D;
    if (sidx >= 0) {
        const bf16_t* e = enc + ((long)b * T + sidx) * D;
        for (int d = threadIdx.x; d < D; d += 256) o[d] = bf16_to_f32(e[d]);
    } else {
        const float* rg = registers + (long)(p % R) * D;
        for (int d = threadIdx.x; d < D; d += 256) o[d] = rg[d];
    }
}

__global__ void fill_const_i32_kernel(int32_t* p, long n, int32_t v) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}
}  // namespace

void launch_fe_stats(const bf16_t* hidden, const int32_t* mask, int states, int B, int T, int D, int padding_right, float eps,
                     float* partials, float* stats, hipStream_t stream) {
    LTX_REQUIRE(D % 8 == 0, "connector: hidden dim %d must be a multiple of 8", D);
    const int nchunk = (int)(((long)T * D + FE_CHUNK - 1) / FE_CHUNK);
    hipLaunchKernelGGL(fe_stats_partial_kernel, dim3(nchunk, states * B), dim3(256), 0, stream, hidden, mask, B, T, D, padding_right,
                       partials, nchunk);
    HIP_CHECK(hipGetLastError());
    const int planes = states * B;
    hipLaunchKernelGGL(fe_stats_final_kernel, dim3((planes + 63) / 64), dim3(64), 0, stream, partials, mask, B, T, D, eps, nchunk, stats,
                       planes);
    HIP_CHECK(hipGetLastError());
}
long fe_stats_partials_floats(int states, int B, int T, int D) {
    return (long)states * B * (((long)T * D + FE_CHUNK - 1) / FE_CHUNK) * 3;
}
void launch_fe_norm_concat(const bf16_t* hidden, const int32_t* mask, const float* stats, int states, int B, int T, int D,
                           int padding_right, float eps, bf16_t* out, hipStream_t stream) {
    (void)eps;
    hipLaunchKernelGGL(fe_norm_concat_kernel, dim3(B * T), dim3(256), 0, stream, hidden, mask, stats, states, B, T, D, padding_right, out);
    HIP_CHECK(hipGetLastError());
}
void launch_register_plan(const int32_t* mask, int B, int T, int32_t* src, hipStream_t stream) {
    hipLaunchKernelGGL(register_plan_kernel, dim3(B), dim3(64), 0, stream, mask, T, src);
    HIP_CHECK(hipGetLastError());
}
void launch_register_gather(const bf16_t* enc, const float* registers, const int32_t* src, int B, int T, int D, int R, float* x,
                            hipStream_t stream) {
    hipLaunchKernelGGL(register_gather_kernel, dim3(B * T), dim3(256), 0, stream, enc, registers, src, T, D, R, x);
    HIP_CHECK(hipGetLastError());
}
void launch_fill_const_i32(int32_t* p, long n, int32_t v, hipStream_t stream) {
    hipLaunchKernelGGL(fill_const_i32_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, p, n, v);
    HIP_CHECK(hipGetLastError());
}


// ---------------------------------------------------------------------------------------------------------------
// VAE encoder kernels (VideoEncoder.swift)
// ---------------------------------------------------------------------------------------------------------------
namespace {
// pixels f32 [3][T][H][W] -> bf16 channels-last [T][H/4][W/4][64]: channel = c*16 + pw*4 + ph for c < 3 (pW before pH,
// VideoEncoder.swift:25-31), channels 48..63 zero (K-tile padding of conv_in)
__global__ void enc_patchify_kernel(const float* __restrict__ px, bf16_t* __restrict__ out, int T, int H, int W) {
    const long n = (long)T * (H / 4) * (W / 4) * 64;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int ch = (int)(i & 63);
    long pos = i >> 6;
    const int w4 = (int)(pos % (W / 4));
    pos /= (W / 4);
    const int h4 = (int)(pos % (H / 4));
    const int t = (int)(pos / (H / 4));
    float v = 0.f;
    if (ch < 48) {
        const int c = ch >> 4, pw = (ch >> 2) & 3, ph = ch & 3;
        v = px[(((long)c * T + t) * H + (h4 * 4 + ph)) * W + (w4 * 4 + pw)];
    }
    out[i] = f32_to_bf16(v);
}

// out[t2][h2][w2][co] = s2d(conv)[co] + mean_g s2d(x)[co*G + g]  (VAESpaceToDepthDownsample3d, VideoEncoder.swift:146-167)
// s2d channel cs of a tensor with Cs source channels: source channel cs / S, sub = cs % S -> (it, ih, iw); an odd T is padded
// in FRONT with copies of frame 0, i.e. source frame max(0, t2*ft + it - padT)
__global__ void enc_s2d_residual_kernel(const float* __restrict__ conv, int Cc, const float* __restrict__ x, int Cx,
                                        float* __restrict__ out, int Cout, int T, int H, int W, int ft, int fh, int fw) {
    const int S = ft * fh * fw;
    const int padT = (ft - T % ft) % ft;
    const int T2 = (T + padT) / ft, H2 = H / fh, W2 = W / fw;
    const long n = (long)T2 * H2 * W2 * Cout;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int co = (int)(i % Cout);
    long pos = i / Cout;
    const int w2 = (int)(pos % W2);
    pos /= W2;
    const int h2 = (int)(pos % H2);
    const int t2 = (int)(pos / H2);
    auto fetch = [&](const float* src, int C, int cs) {
        const int c = cs / S, sub = cs - c * S;
        const int it = sub / (fh * fw), ih = (sub / fw) % fh, iw = sub % fw;
        int ts = t2 * ft + it - padT;
        ts = ts < 0 ? 0 : ts;
        return src[(((long)ts * H + (h2 * fh + ih)) * W + (w2 * fw + iw)) * C + c];
    };
    const int G = Cx * S / Cout;
    float acc = 0.f;
    for (int g = 0; g < G; ++g) acc += fetch(x, Cx, co * G + g);
    out[i] = fetch(conv, Cc, co) + acc / (float)G;
}

// z f32 [P][ldz] (first C channels) -> out [C][P] f32 with optional (z - mean[c]) / std[c]  (LTXPipeline.swift:1920-1927)
__global__ void enc_finish_kernel(const float* __restrict__ z, long ldz, const float* __restrict__ mean, const float* __restrict__ stdv,
                                  float* __restrict__ out, int C, long P) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)C * P) return;
    const int c = (int)(i / P);
    const long p = i - (long)c * P;
    float v = z[p * ldz + c];
    if (mean) v = (v - mean[c]) / stdv[c];
    out[i] = v;
}
}  // namespace

void launch_enc_patchify(const float* pixels, bf16_t* out, int T, int H, int W, hipStream_t stream) {
    LTX_REQUIRE(H % 4 == 0 && W % 4 == 0, "encoder patchify: H=%d W=%d must be multiples of 4", H, W);
    const long n = (long)T * (H / 4) * (W / 4) * 64;
    hipLaunchKernelGGL(enc_patchify_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, pixels, out, T, H, W);
    HIP_CHECK(hipGetLastError());
}
void launch_enc_s2d_residual(const float* conv, int Cc, const float* x, int Cx, float* out, int Cout, int T, int H, int W, int ft,
                             int fh, int fw, hipStream_t stream) {
    LTX_REQUIRE(H % fh == 0 && W % fw == 0 && (Cx * ft * fh * fw) % Cout == 0 && Cc * ft * fh * fw == Cout, "s2d: bad shapes");
    const int padT = (ft - T % ft) % ft;
    const long n = (long)((T + padT) / ft) * (H / fh) * (W / fw) * Cout;
    hipLaunchKernelGGL(enc_s2d_residual_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, conv, Cc, x, Cx, out, Cout, T, H, W, ft, fh, fw);
    HIP_CHECK(hipGetLastError());
}
void launch_enc_finish(const float* z, long ldz, const float* mean, const float* stdv, float* out, int C, long P, hipStream_t stream) {
    hipLaunchKernelGGL(enc_finish_kernel, dim3(cdiv((long)C * P, 256)), dim3(256), 0, stream, z, ldz, mean, stdv, out, C, P);
    HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------------------------
// Gemma-3 text encoder row passes (Gemma3Model.swift)
// ---------------------------------------------------------------------------------------------------------------
namespace {
LTX_DEVFN float bf16_round(float v) { return bf16_to_f32(f32_to_bf16(v)); }
LTX_DEVFN void load_bf16x8(const bf16_t* p, float (&v)[8]) {
    const uint4 u = *(const uint4*)p;
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[2 * i] = __builtin_bit_cast(float, w[i] << 16);
        v[2 * i + 1] = __builtin_bit_cast(float, w[i] & 0xffff0000u);
    }
}
LTX_DEVFN void store_bf16x8(bf16_t* p, const float (&v)[8]) {
    uint4 u;
    u.x = pack_bf16x2(v[0], v[1]);
    u.y = pack_bf16x2(v[2], v[3]);
    u.z = pack_bf16x2(v[4], v[5]);
    u.w = pack_bf16x2(v[6], v[7]);
    *(uint4*)p = u;
}
LTX_DEVFN void load_gain8(const float* w, float (&g)[8]) {  // g = bf16(1 + w)
    const f32x4 a = *(const f32x4*)w, b = *(const f32x4*)(w + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        g[e] = bf16_round(1.0f + a[e]);
        g[4 + e] = bf16_round(1.0f + b[e]);
    }
}

// The mean square of a row of bf16 values, defined so that a host replay can reproduce it bit for bit: the squares are exact in f32,
// their sum is taken in f64 (exact up to 2^-53, whatever the order) and rounded to f32 once; the division, the square root and the
// reciprocal are the correctly rounded f32 operations.
LTX_DEVFN float rstd_of(double sum_sq, int D, float eps) { return 1.0f / sqrtf((float)sum_sq / (float)D + eps); }
LTX_DEVFN double block_reduce_sum_f64(double v, double* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();  // protect `red` from a previous use
    if (lane == 0) red[w] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// one workgroup per row; NV chunks of 8 per thread (D <= NV * 2048)
template <int NV>
__global__ __launch_bounds__(256) void gemma_norm_kernel(const GemmaNormArgs a) {
    __shared__ double red[4];
    const int row = blockIdx.x;
    const int nchunk = a.D >> 3;
    float v[NV][8], g[NV][8];
    double ss = 0.0;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int c = threadIdx.x + j * 256;
        if (c < nchunk) {
            load_bf16x8(a.r + (long)row * a.ldr + c * 8, v[j]);
            load_gain8(a.w + c * 8, g[j]);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[j][e] = g[j][e] = 0.f;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) ss += (double)(v[j][e] * v[j][e]);
    }
    float rstd = rstd_of(block_reduce_sum_f64(ss, red), a.D, a.eps);
    ss = 0.0;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int c = threadIdx.x + j * 256;
        if (c < nchunk) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[j][e] = bf16_round(v[j][e] * rstd * g[j][e]);
            if (a.x) {
                float xr[8];
                load_bf16x8(a.x + (long)row * a.ldx + c * 8, xr);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[j][e] = bf16_round(xr[e] + v[j][e]);
            }
            if (!a.n_only) store_bf16x8(a.h + (long)row * a.ldh + c * 8, v[j]);
#pragma unroll
            for (int e = 0; e < 8; ++e) ss += (double)(v[j][e] * v[j][e]);
        }
    }
    if (!a.w2) return;
    rstd = rstd_of(block_reduce_sum_f64(ss, red), a.D, a.eps);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int c = threadIdx.x + j * 256;
        if (c < nchunk) {
            load_gain8(a.w2 + c * 8, g[j]);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[j][e] = v[j][e] * rstd * g[j][e];
            store_bf16x8(a.n + (long)row * a.ldn + c * 8, v[j]);
        }
    }
}

// half a wave per (row, head): lane l of the half holds elements 4l .. 4l+3 and 128 + 4l .. of the head, i.e. both members of four pairs
__global__ __launch_bounds__(256) void gemma_qknorm_rope_kernel(const GemmaQkArgs a, int heads_total) {
#pragma clang fp contract(off)  // the four products and two sums of a rotation are each rounded on their own: the replay's order
    const long unit = (long)blockIdx.x * 8 + (threadIdx.x >> 5);
    if (unit >= (long)a.rows * heads_total) return;  // whole half-waves leave together; the shuffles below stay inside a half
    const int row = (int)(unit / heads_total);
    int head = (int)(unit % heads_total);
    const bool second = head >= a.job[0].heads;
    if (second) head -= a.job[0].heads;
    const GemmaQkArgs::Job& j = a.job[second ? 1 : 0];
    const int l = threadIdx.x & 31;
    const bf16_t* xr = j.x + (long)row * j.ldx + head * 256 + 4 * l;
    const uint2 ulo = *(const uint2*)xr, uhi = *(const uint2*)(xr + 128);
    float lo[4] = {__builtin_bit_cast(float, ulo.x << 16), __builtin_bit_cast(float, ulo.x & 0xffff0000u), __builtin_bit_cast(float, ulo.y << 16),
                   __builtin_bit_cast(float, ulo.y & 0xffff0000u)};
    float hi[4] = {__builtin_bit_cast(float, uhi.x << 16), __builtin_bit_cast(float, uhi.x & 0xffff0000u), __builtin_bit_cast(float, uhi.y << 16),
                   __builtin_bit_cast(float, uhi.y & 0xffff0000u)};
    const f32x4 wlo = *(const f32x4*)(j.w + 4 * l), whi = *(const f32x4*)(j.w + 128 + 4 * l);
    const long p = row % a.T;
    const f32x4 cs = *(const f32x4*)(a.cos + p * 128 + 4 * l), sn = *(const f32x4*)(a.sin + p * 128 + 4 * l);
    double ss = 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) ss += (double)(lo[e] * lo[e]) + (double)(hi[e] * hi[e]);
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
    const float rstd = rstd_of(ss, 256, a.eps);
    float olo[4], ohi[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float y1 = bf16_round(lo[e] * rstd * bf16_round(1.0f + wlo[e]));
        const float y2 = bf16_round(hi[e] * rstd * bf16_round(1.0f + whi[e]));
        olo[e] = y1 * cs[e] - y2 * sn[e];
        ohi[e] = y1 * sn[e] + y2 * cs[e];
    }
    bf16_t* orow = j.out + (long)row * j.ldo + head * 256 + 4 * l;
    uint2 pk;
    pk.x = pack_bf16x2(olo[0], olo[1]);
    pk.y = pack_bf16x2(olo[2], olo[3]);
    *(uint2*)orow = pk;
    pk.x = pack_bf16x2(ohi[0], ohi[1]);
    pk.y = pack_bf16x2(ohi[2], ohi[3]);
    *(uint2*)(orow + 128) = pk;
}

// f64 evaluation, one rounding to f32 per entry: the tables are made once per model, and a host replay reproduces them to the last bit
// or two (an f32 evaluation of the angle is off by up to 1e-6 of it, i.e. 1e-3 rad at position 1023)
__global__ void gemma_rope_tables_kernel(float* __restrict__ cos_t, float* __restrict__ sin_t, int T, double log2_base) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T * 128) return;
    const double ang = (double)(i >> 7) * exp2(-((double)(i & 127) / 128.0) * log2_base);
    cos_t[i] = (float)cos(ang);
    sin_t[i] = (float)sin(ang);
}

__global__ __launch_bounds__(256) void geglu_kernel(const GegluArgs a) {
    const int per_row = a.I >> 3;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)a.rows * per_row) return;
    const long row = i / per_row;
    const int c = (int)(i % per_row) * 8;
    float g[8], u[8];
    load_bf16x8(a.gu + row * a.ldgu + c, g);
    load_bf16x8(a.gu + row * a.ldgu + a.I + c, u);
#pragma unroll
    for (int e = 0; e < 8; ++e) g[e] = bf16_round(gelu_tanh(g[e])) * u[e];
    store_bf16x8(a.out + row * a.ldo + c, g);
}

__global__ __launch_bounds__(256) void gemma_embed_kernel(const GemmaEmbedArgs a) {
    const int row = blockIdx.x;
    int id = a.ids[row];
    id = id < 0 ? 0 : (id >= a.vocab ? a.vocab - 1 : id);
    for (int c = threadIdx.x; c < (a.D >> 3); c += 256) {
        float v[8];
        load_bf16x8(a.table + (long)id * a.D + c * 8, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] *= a.scale;
        store_bf16x8(a.out + (long)row * a.D + c * 8, v);
    }
}

__global__ __launch_bounds__(256) void gemma_mask_scan_kernel(const int32_t* __restrict__ mask, int T, int32_t* __restrict__ key_start,
                                                              int32_t* __restrict__ status) {
    __shared__ int first, ones, bad;
    if (threadIdx.x == 0) {
        first = T;
        ones = 0;
        bad = 0;
    }
    __syncthreads();
    const int32_t* m = mask + (long)blockIdx.x * T;
    int f = T, n = 0, bd = 0;
    for (int t = threadIdx.x; t < T; t += 256) {
        const int v = m[t];
        if (v == 1) {
            f = f < t ? f : t;
            ++n;
        } else if (v != 0) {
            bd = 1;
        }
    }
    atomicMin(&first, f);
    atomicAdd(&ones, n);
    if (bd) atomicOr(&bad, 1);
    __syncthreads();
    if (threadIdx.x == 0) {
        key_start[blockIdx.x] = first;
        status[blockIdx.x] = (!bad && ones >= 1 && first == T - ones) ? 1 : 0;  // every position from the first 1 on is a 1
    }
}

// (value, index) order of the argmax: the greater value, and the LOWER index among equal values
LTX_DEVFN void pick_better(float& v, int& i, float v2, int i2) {
    if (v2 > v || (v2 == v && i2 < i)) {
        v = v2;
        i = i2;
    }
}
// one workgroup of 1024 threads. Phase 1: the penalty, in place - the thread that holds the FIRST occurrence of an id among the
// recent tokens rewrites that logit, so an id that occurs twice is penalised once. Phase 2 (behind the barrier): per-thread argmax
// over 16-byte vectors in ascending index order, then the wave and workgroup reductions in the order above.
__global__ __launch_bounds__(1024) void lm_pick_kernel(const LmPickArgs a) {
    __shared__ float best_v[16];
    __shared__ int best_i[16];
    const int tid = threadIdx.x;
    const int n_recent = a.n_gen < a.context ? a.n_gen : a.context;
    if (a.penalty != 1.0f && n_recent > 0) {
        const int32_t* recent = a.hist + (a.n_gen - n_recent);
        for (int t = tid; t < n_recent; t += 1024) {
            const int id = recent[t];
            bool first = id >= 0 && id < a.vocab;
            for (int u = 0; u < t && first; ++u) first = recent[u] != id;
            if (first) {
                const float l = a.logits[id];
                a.logits[id] = l > 0.f ? __fdiv_rn(l, a.penalty) : l * a.penalty;
            }
        }
    }
    __syncthreads();  // the rewritten logits are visible to the workgroup
    float v = -__builtin_inff();
    int idx = 0x7fffffff;
    const int nvec = a.vocab >> 2;
    for (int c = tid; c < nvec; c += 1024) {
        const f32x4 x = *(const f32x4*)(a.logits + 4 * c);
#pragma unroll
        for (int e = 0; e < 4; ++e) pick_better(v, idx, x[e], 4 * c + e);
    }
    for (int i = 4 * nvec + tid; i < a.vocab; i += 1024) pick_better(v, idx, a.logits[i], i);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) pick_better(v, idx, __shfl_xor(v, off, 64), __shfl_xor(idx, off, 64));
    if ((tid & 63) == 0) {
        best_v[tid >> 6] = v;
        best_i[tid >> 6] = idx;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; ++w) pick_better(v, idx, best_v[w], best_i[w]);
        if (idx == 0x7fffffff) idx = 0;  // nothing compared greater than -inf
        *a.out = idx;
        if (a.hist) a.hist[a.n_gen] = idx;
    }
}
}  // namespace

void launch_gemma_norm(const GemmaNormArgs& a, hipStream_t stream) {
    LTX_REQUIRE(a.r && a.w && (a.h || a.n_only) && a.rows > 0, "gemma_norm: null argument");
    LTX_REQUIRE(a.D % 8 == 0 && a.D >= 8 && a.D <= 8192, "gemma_norm: D %d must be a multiple of 8 up to 8192", a.D);
    LTX_REQUIRE(a.ldr % 8 == 0 && a.ldr >= a.D && (a.n_only || (a.ldh % 8 == 0 && a.ldh >= a.D)), "gemma_norm: leading dims");
    LTX_REQUIRE(!a.x || (a.ldx % 8 == 0 && a.ldx >= a.D), "gemma_norm: residual leading dim");
    LTX_REQUIRE(!a.w2 == !a.n && (!a.w2 || (a.ldn % 8 == 0 && a.ldn >= a.D)), "gemma_norm: the second norm needs w2 and n");
    LTX_REQUIRE(!a.n_only || a.w2, "gemma_norm: n_only without a second norm writes nothing");
    if (a.D <= 2048)
        hipLaunchKernelGGL(gemma_norm_kernel<1>, dim3(a.rows), dim3(256), 0, stream, a);
    else if (a.D <= 4096)
        hipLaunchKernelGGL(gemma_norm_kernel<2>, dim3(a.rows), dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL(gemma_norm_kernel<4>, dim3(a.rows), dim3(256), 0, stream, a);
    HIP_CHECK(hipGetLastError());
}

void launch_gemma_qknorm_rope(const GemmaQkArgs& a, hipStream_t stream) {
    const int heads = a.job[0].heads + a.job[1].heads;
    LTX_REQUIRE(a.rows > 0 && a.T > 0 && a.job[0].heads > 0 && a.job[1].heads >= 0 && a.cos && a.sin, "gemma_qknorm_rope: empty launch");
    for (int i = 0; i < 2; ++i) {
        const GemmaQkArgs::Job& j = a.job[i];
        if (j.heads == 0) continue;
        LTX_REQUIRE(j.x && j.w && j.out, "gemma_qknorm_rope: null argument");
        LTX_REQUIRE(j.ldx % 4 == 0 && j.ldo % 4 == 0 && j.ldx >= j.heads * 256 && j.ldo >= j.heads * 256, "gemma_qknorm_rope: leading dims");
        LTX_REQUIRE(((uintptr_t)j.x & 7) == 0 && ((uintptr_t)j.out & 7) == 0, "gemma_qknorm_rope: pointer alignment");
    }
    const long units = (long)a.rows * heads;
    hipLaunchKernelGGL(gemma_qknorm_rope_kernel, dim3((unsigned)((units + 7) / 8)), dim3(256), 0, stream, a, heads);
    HIP_CHECK(hipGetLastError());
}

void launch_gemma_rope_tables(float* cos_t, float* sin_t, int T, float base, hipStream_t stream) {
    LTX_REQUIRE(cos_t && sin_t && T > 0 && base > 1.0f, "gemma_rope_tables: arguments");
    hipLaunchKernelGGL(gemma_rope_tables_kernel, dim3((T * 128 + 255) / 256), dim3(256), 0, stream, cos_t, sin_t, T, log2((double)base));
    HIP_CHECK(hipGetLastError());
}

void launch_geglu(const GegluArgs& a, hipStream_t stream) {
    LTX_REQUIRE(a.gu && a.out && a.rows > 0, "geglu: null argument");
    LTX_REQUIRE(a.I % 8 == 0 && a.I >= 8 && a.ldgu % 8 == 0 && a.ldgu >= 2 * a.I && a.ldo % 8 == 0 && a.ldo >= a.I, "geglu: shape");
    const long n = (long)a.rows * (a.I >> 3);
    hipLaunchKernelGGL(geglu_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
    HIP_CHECK(hipGetLastError());
}

void launch_gemma_embed(const GemmaEmbedArgs& a, hipStream_t stream) {
    LTX_REQUIRE(a.ids && a.table && a.out && a.rows > 0 && a.vocab > 0, "gemma_embed: null argument");
    LTX_REQUIRE(a.D % 8 == 0 && a.D >= 8, "gemma_embed: D %d must be a multiple of 8", a.D);
    hipLaunchKernelGGL(gemma_embed_kernel, dim3(a.rows), dim3(256), 0, stream, a);
    HIP_CHECK(hipGetLastError());
}

void launch_lm_pick(const LmPickArgs& a, hipStream_t stream) {
    LTX_REQUIRE(a.logits && a.out && a.vocab >= 1, "lm_pick: null logits / out or an empty vocabulary");
    LTX_REQUIRE(((uintptr_t)a.logits & 15) == 0, "lm_pick: logits must be 16-byte aligned");
    LTX_REQUIRE(a.n_gen >= 0 && a.context >= 0 && (a.hist || a.n_gen == 0), "lm_pick: n_gen=%d context=%d need a history buffer", a.n_gen, a.context);
    LTX_REQUIRE(a.penalty > 0.f, "lm_pick: penalty %g must be positive", (double)a.penalty);
    hipLaunchKernelGGL(lm_pick_kernel, dim3(1), dim3(1024), 0, stream, a);
    HIP_CHECK(hipGetLastError());
}

void launch_gemma_mask_scan(const int32_t* mask, int B, int T, int32_t* key_start, int32_t* status, hipStream_t stream) {
    LTX_REQUIRE(mask && key_start && status && B > 0 && T > 0, "gemma_mask_scan: arguments");
    hipLaunchKernelGGL(gemma_mask_scan_kernel, dim3(B), dim3(256), 0, stream, mask, T, key_start, status);
    HIP_CHECK(hipGetLastError());
}
