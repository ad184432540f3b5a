// audio_conv.hip - the convolutions of the audio decode leg (audio.h) as one shifted-row multi-tap GEMM on gfx950.
//
//   out[p][co] = bias[co] + sum_tap sum_ci W[co][tap][ci] * x[p + off(tap)][ci]
//
// x is a zero-haloed, channels-last bf16 buffer, so a tap is a row offset and nothing is gathered:
//   Conv1d (k, dilation d)      off = (j - (k-1)/2) * d
//   causal Conv2d on [H+2][W+2] off = kh * (W+2) + kw      (two zero rows on top, none below: AudioVAE.swift:53-57)
//   ConvTransposed1d            one problem per output phase r = t mod stride with that phase's taps, stored to row t*stride + r
//
// Precision contract: bf16 operands (weights rounded at load), f32 accumulation in v_mfma_f32_16x16x32_bf16, f32 residual stream.
//
// Mapping: the MFMA's A operand is the weight slab (rows = co), B is the shifted input (columns = positions), so a lane ends with four
// consecutive output channels of one position: the channels-last epilogue is one 16-byte f32 access and one 8-byte bf16 store per
// fragment. Lane l holds A[co = l&15][k = 8(l>>4) .. +8] and B[k][p = l&15]: both are 16-byte loads of contiguous channels straight
// from HBM/L2 (rows of x are re-read by neighbouring taps and by the co-tiles of the same rows out of L1/L2; there is no LDS stage),
// prefetched one K-step ahead in registers.
// 256 threads = 4 waves arranged NWC x NWP, each wave owns (WC*16) channels x (WP*16) positions.
#include "audio.h"

namespace {

template <int WC, int WP, int NWC, int NWP>
__global__ __launch_bounds__(256) void audio_conv_kernel(const AConvArgs a) {
    static_assert(NWC * NWP == 4, "four waves");
    constexpr int BC = WC * 16 * NWC, BP = WP * 16 * NWP;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wc = wave % NWC, wq = wave / NWC;
    const int l15 = lane & 15, kq = (lane >> 4) * 8;
    const int co_base = blockIdx.y * BC + wc * WC * 16;
    const long p_base = (long)blockIdx.x * BP + wq * WP * 16;
    if (co_base >= a.Cout || p_base >= a.P) return;  // wave-uniform; no barriers in this kernel

    const long wrow_stride = (long)a.ntaps * a.Cin;
    const bf16_t* wrow[WC];
    bool wok[WC];
#pragma unroll
    for (int i = 0; i < WC; ++i) {
        const int co = co_base + i * 16 + l15;
        wok[i] = co < a.Cout;
        wrow[i] = a.w + (long)(wok[i] ? co : a.Cout - 1) * wrow_stride + kq;
    }
    const bf16_t* xrow[WP];
#pragma unroll
    for (int j = 0; j < WP; ++j) {
        long p = p_base + j * 16 + l15;
        p = p < a.P ? p : a.P - 1;  // rows past the end re-read the last row; their results are not stored
        xrow[j] = a.x + p * a.ldx + kq;
    }
    f32x4 acc[WC][WP];
#pragma unroll
    for (int i = 0; i < WC; ++i)
#pragma unroll
        for (int j = 0; j < WP; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // K loop over (tap, 32-channel step), flattened and software-pipelined one step deep: the 16-byte fragment loads of step s+1 are in
    // flight while the MFMAs of step s issue (few waves per SIMD on the short problems: nothing else hides the load latency)
    const bf16x8_t zero8 = {};
    int lt = 0, lc = 0;  // the next step to load
    auto load_step = [&](bf16x8_t(&af)[WC], bf16x8_t(&bf)[WP]) {
        const long xo = (long)a.off[lt] * a.ldx + lc;
        const long wo = (long)lt * a.Cin + lc;
#pragma unroll
        for (int i = 0; i < WC; ++i) af[i] = *(const bf16x8_t*)(wrow[i] + wo);
#pragma unroll
        for (int jj = 0; jj < WP; ++jj) bf[jj] = *(const bf16x8_t*)(xrow[jj] + xo);
        lc += 32;
        if (lc == a.Cin) {
            lc = 0;
            ++lt;
        }
    };
    auto mfma_step = [&](bf16x8_t(&af)[WC], bf16x8_t(&bf)[WP]) {
#pragma unroll
        for (int i = 0; i < WC; ++i) af[i] = wok[i] ? af[i] : zero8;
#pragma unroll
        for (int i = 0; i < WC; ++i)
#pragma unroll
            for (int jj = 0; jj < WP; ++jj) acc[i][jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bf[jj], acc[i][jj], 0, 0, 0);
    };
    const int nsteps = a.ntaps * (a.Cin >> 5);
    bf16x8_t a0[WC], b0[WP], a1[WC], b1[WP];
    load_step(a0, b0);
    for (int s = 0; s < nsteps; s += 2) {
        if (s + 1 < nsteps) load_step(a1, b1);
        mfma_step(a0, b0);
        if (s + 2 < nsteps) load_step(a0, b0);
        if (s + 1 < nsteps) mfma_step(a1, b1);
    }

    // epilogue: lane holds channels co0 .. co0+3 of position p
#pragma unroll
    for (int j = 0; j < WP; ++j) {
        const long p = p_base + j * 16 + l15;
        if (p >= a.P) continue;
        const long h = p / a.wp;
        const long w = p - h * a.wp;
        if (w >= a.wv) continue;
        const long rf = (h * a.opitch + w) * a.omul + a.oadd;
        const long rb = (h * a.bpitch + w) * a.omul + a.oadd;
#pragma unroll
        for (int i = 0; i < WC; ++i) {
            const int co0 = co_base + i * 16 + (lane >> 4) * 4;
            if (co0 >= a.Cout) continue;
            f32x4 v = acc[i][j];
            if (co0 + 3 < a.Cout && !a.f32_transposed) {
                if (a.bias) v += *(const f32x4*)(a.bias + co0);
                if (a.resid) v += *(const f32x4*)(a.resid + rf * a.ldo + co0);
                if (a.f32_act == AACT_TANH) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = tanhf(v[e]);
                }
                if (a.out_f32) *(f32x4*)(a.out_f32 + rf * a.ldo + co0) = v;
                if (a.out_bf16) {
                    if (a.bf16_act == AACT_LEAKY) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = v[e] >= 0.f ? v[e] : v[e] * a.slope;
                    }
                    uint2 pk;
                    pk.x = pack_bf16x2(v[0], v[1]);
                    pk.y = pack_bf16x2(v[2], v[3]);
                    *(uint2*)(a.out_bf16 + rb * a.ldb + co0) = pk;
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int co = co0 + e;
                    if (co >= a.Cout) break;
                    float s = v[e];
                    if (a.bias) s += a.bias[co];
                    const long fi = a.f32_transposed ? (long)co * a.ldo + rf : rf * a.ldo + co;
                    if (a.resid) s += a.resid[fi];
                    if (a.f32_act == AACT_TANH) s = tanhf(s);
                    if (a.out_f32) a.out_f32[fi] = s;
                    if (a.out_bf16) {
                        if (a.bf16_act == AACT_LEAKY) s = s >= 0.f ? s : s * a.slope;
                        a.out_bf16[rb * a.ldb + co] = f32_to_bf16(s);
                    }
                }
            }
        }
    }
}

template <int WC, int WP, int NWC, int NWP>
void launch_cfg(const AConvArgs& a, hipStream_t stream) {
    constexpr int BC = WC * 16 * NWC, BP = WP * 16 * NWP;
    dim3 grid((unsigned)((a.P + BP - 1) / BP), (unsigned)((a.Cout + BC - 1) / BC));
    hipLaunchKernelGGL((audio_conv_kernel<WC, WP, NWC, NWP>), grid, dim3(256), 0, stream, a);
}

// ---- row passes ----
// one wave per position; C <= 64 * 16
__global__ __launch_bounds__(256) void audio_pn_pad_kernel(const float* __restrict__ x, int H, int W, int C, int mode,
                                                           bf16_t* __restrict__ out) {
    const long pos = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (pos >= (long)H * W) return;
    const int h = (int)(pos / W), w = (int)(pos % W);
    const float* xr = x + pos * C;
    bf16_t* orow = out + ((long)(h + 2) * (W + 2) + (w + 1)) * C;
    float scale = 1.f;
    if (mode == 0) {
        float ss = 0.f;
        for (int c = lane; c < C; c += 64) ss += xr[c] * xr[c];
        ss = wave_reduce_sum(ss);
        scale = 1.0f / sqrtf(ss / (float)C + 1e-6f);
    }
    for (int c = lane; c < C; c += 64) {
        float v = xr[c];
        if (mode == 0) {
            v *= scale;
            v = silu_f(v);
        }
        orow[c] = f32_to_bf16(v);
    }
}

__global__ __launch_bounds__(256) void audio_upsample_pad_kernel(const float* __restrict__ x, int H, int W, int C, bf16_t* __restrict__ out) {
    // one thread per 4 channels of one upsampled position
    const int C4 = C >> 2;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long total = (long)2 * H * 2 * W * C4;
    if (i >= total) return;
    const int c = (int)(i % C4) * 4;
    const long uv = i / C4;
    const int v = (int)(uv % (2 * W)), u = (int)(uv / (2 * W));
    const f32x4 s = *(const f32x4*)(x + ((long)(u >> 1) * W + (v >> 1)) * C + c);
    uint2 pk;
    pk.x = pack_bf16x2(s[0], s[1]);
    pk.y = pack_bf16x2(s[2], s[3]);
    *(uint2*)(out + ((long)(u + 1) * (2 * W + 2) + (v + 1)) * C + c) = pk;
}

__global__ __launch_bounds__(256) void audio_denorm_pad_kernel(const float* __restrict__ latent, const float* __restrict__ mean,
                                                               const float* __restrict__ stdv, int Cl, int T, int Wl, int Cpad,
                                                               bf16_t* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)Cl * T * Wl) return;
    const int w = (int)(i % Wl);
    const int t = (int)((i / Wl) % T);
    const int c = (int)(i / ((long)Wl * T));
    const float v = latent[i] * stdv[c * Wl + w] + mean[c * Wl + w];
    out[((long)(t + 2) * (Wl + 2) + (w + 1)) * Cpad + c] = f32_to_bf16(v);
}

__global__ __launch_bounds__(256) void audio_mel_pack_kernel(const float* __restrict__ mel, int T, int M, bf16_t* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)2 * T * M) return;
    const int m = (int)(i % M);
    const int t = (int)((i / M) % T);
    const int c = (int)(i / ((long)M * T));
    out[(long)t * (2 * M) + c * M + m] = f32_to_bf16(mel[i]);
}

__global__ __launch_bounds__(256) void audio_mean3_act_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                              const float* __restrict__ c, long n4, int C4, float slope, bf16_t* __restrict__ out,
                                                              long ldb) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const f32x4 va = ((const f32x4*)a)[i], vb = ((const f32x4*)b)[i], vc = ((const f32x4*)c)[i];
    float r[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float s = (va[e] + vb[e] + vc[e]) / 3.0f;
        r[e] = s >= 0.f ? s : s * slope;
    }
    uint2 pk;
    pk.x = pack_bf16x2(r[0], r[1]);
    pk.y = pack_bf16x2(r[2], r[3]);
    *(uint2*)(out + (i / C4) * ldb + (i % C4) * 4) = pk;
}

unsigned blocks_for(long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

void launch_audio_conv(const AConvArgs& a, int tile, hipStream_t stream) {
    LTX_REQUIRE(a.x && a.w && (a.out_f32 || a.out_bf16), "audio conv: null operand or no output");
    LTX_REQUIRE(a.P >= 1 && a.Cout >= 1 && a.Cin >= 32 && a.Cin % 32 == 0, "audio conv: P=%d Cout=%d Cin=%d (Cin must be a multiple of 32)",
                a.P, a.Cout, a.Cin);
    LTX_REQUIRE(a.ntaps >= 1 && a.ntaps <= ACONV_MAX_TAPS, "audio conv: %d taps (1..%d)", a.ntaps, (int)ACONV_MAX_TAPS);
    LTX_REQUIRE(a.ldx >= a.Cin && a.ldx % 8 == 0, "audio conv: ldx=%ld (>= Cin, multiple of 8)", a.ldx);
    LTX_REQUIRE(a.wp >= 1 && a.wv >= 1 && a.omul >= 1 && a.oadd >= 0, "audio conv: bad row mapping");
    LTX_REQUIRE(!a.out_f32 || a.ldo >= (a.f32_transposed ? 1 : a.Cout), "audio conv: ldo=%ld", a.ldo);
    LTX_REQUIRE(!a.out_f32 || a.f32_transposed || a.Cout < 4 || a.ldo % 4 == 0, "audio conv: ldo=%ld must be a multiple of 4", a.ldo);
    LTX_REQUIRE(!a.out_bf16 || (a.ldb >= a.Cout && (a.Cout < 4 || a.ldb % 4 == 0)), "audio conv: ldb=%ld", a.ldb);
    LTX_REQUIRE(!a.resid || a.out_f32, "audio conv: a residual needs the f32 output");
    LTX_REQUIRE(a.f32_act == AACT_NONE || a.f32_act == AACT_TANH, "audio conv: f32_act=%d", a.f32_act);
    LTX_REQUIRE(a.bf16_act == AACT_NONE || a.bf16_act == AACT_LEAKY, "audio conv: bf16_act=%d", a.bf16_act);
    if (tile < 0) tile = a.Cout >= 128 ? 128 : a.Cout >= 64 ? 64 : 32;
    LTX_REQUIRE(tile == 128 || tile == 64 || tile == 32, "audio conv: no %d-column instance (128, 64, 32)", tile);
    ProfScope ps(PROF_CONV, 2.0 * a.P * (double)a.Cout * a.Cin * a.ntaps, stream);
    if (tile == 128) launch_cfg<4, 2, 2, 2>(a, stream);      // 128 channels x 64 positions
    else if (tile == 64) launch_cfg<2, 4, 2, 2>(a, stream);  // 64 x 128
    else launch_cfg<2, 2, 1, 4>(a, stream);                  // 32 x 128
    HIP_CHECK(hipGetLastError());
}

void launch_audio_pn_pad(const float* x, int H, int W, int C, int mode, bf16_t* out, hipStream_t stream) {
    ProfScope ps(PROF_ELEM, (double)H * W * C * 6, stream);
    hipLaunchKernelGGL(audio_pn_pad_kernel, dim3((unsigned)(((long)H * W + 3) / 4)), dim3(256), 0, stream, x, H, W, C, mode, out);
    HIP_CHECK(hipGetLastError());
}
void launch_audio_upsample_pad(const float* x, int H, int W, int C, bf16_t* out, hipStream_t stream) {
    LTX_REQUIRE(C % 4 == 0, "audio upsample: C=%d", C);
    ProfScope ps(PROF_ELEM, (double)H * W * C * 12, stream);
    hipLaunchKernelGGL(audio_upsample_pad_kernel, dim3(blocks_for((long)4 * H * W * (C / 4))), dim3(256), 0, stream, x, H, W, C, out);
    HIP_CHECK(hipGetLastError());
}
void launch_audio_denorm_pad(const float* latent, const float* mean, const float* stdv, int Cl, int T, int Wl, int Cpad, bf16_t* out,
                             hipStream_t stream) {
    hipLaunchKernelGGL(audio_denorm_pad_kernel, dim3(blocks_for((long)Cl * T * Wl)), dim3(256), 0, stream, latent, mean, stdv, Cl, T, Wl,
                       Cpad, out);
    HIP_CHECK(hipGetLastError());
}
void launch_audio_mel_pack(const float* mel, int T, int M, bf16_t* out, hipStream_t stream) {
    hipLaunchKernelGGL(audio_mel_pack_kernel, dim3(blocks_for((long)2 * T * M)), dim3(256), 0, stream, mel, T, M, out);
    HIP_CHECK(hipGetLastError());
}
void launch_audio_mean3_act(const float* a, const float* b, const float* c, long rows, int C, float slope, bf16_t* out, long ldb,
                            hipStream_t stream) {
    LTX_REQUIRE(C % 4 == 0 && ldb % 4 == 0 && ldb >= C, "audio mean3: C=%d ldb=%ld", C, ldb);
    const long n4 = rows * (C / 4);
    ProfScope ps(PROF_ELEM, (double)n4 * 56, stream);
    hipLaunchKernelGGL(audio_mean3_act_kernel, dim3(blocks_for(n4)), dim3(256), 0, stream, a, b, c, n4, C / 4, slope, out, ldb);
    HIP_CHECK(hipGetLastError());
}
