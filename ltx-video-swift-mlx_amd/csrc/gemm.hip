// gemm.hip - bf16 MFMA GEMM for gfx950 (CDNA4): C[M,N] = A[M,K] * B[N,K]^T, f32 accumulate, fused epilogues.
//
// This is the kernel that carries ~92 % of the DiT step's FLOPs (reference call sites: every `Linear` of
// LTXAttention.swift:171-175,217, LTXFeedForward.swift:26,49, LTXTransformer.swift:257,223) and, through the
// implicit-im2col A loader, every Conv3dFull of the VAE decoder (VideoConvolution.swift:238-347).
//
// Design (MI355X-first, not a translation of anything):
//   * 256-thread workgroup = 4 waves (2x2), each wave owns a (BM/2)x(BN/2) output sub-tile as
//     v_mfma_f32_16x16x32_bf16 accumulators.
//   * K is walked in 64-element (128-byte) tiles. Both operands are K-contiguous, so A and B tiles are the same
//     LDS image: [rows][128 B], filled by LDS-DMA (`global_load_lds_dwordx4`, 1 KiB per wave-instruction = 8 rows)
//     with the bank swizzle applied on the per-lane SOURCE address (16-B chunk c of row r lives at chunk
//     c ^ ((r>>1)&7)); fragments come back with conflict-free ds_read_b128.
//   * two LDS stages, one barrier per K-tile (prefetch tile t+1 while the MFMAs of tile t run).
//   * epilogue through a per-wave LDS transpose so global stores are 16 B/lane, row-contiguous.
//   * workgroup ids are remapped so that each XCD's L2 sees a contiguous chunk of the tile grid.
#include <type_traits>

#include "gemm.h"
#include "elementwise.h"

#include <stdlib.h>
#include "options.h"
#include "runtime.h"

namespace {

constexpr int BK = 64;            // bf16 elements per K-tile
constexpr int ROW_BYTES = BK * 2;  // 128 B per tile row

struct RowPos {  // conv3d: decoded output position of an A row
    int f, y, x;
};

LTX_DEVFN int reflect_idx(int i, int n) {
    // reflect padding by 1 (VideoConvolution.swift:258-266): -1 -> 1, n -> n-2
    i = (i < 0) ? -i : i;
    return (i >= n) ? (2 * n - 2 - i) : i;
}
LTX_DEVFN int clamp_idx(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }
// x / d == __umulhi(x, magic_u32(d)) for every x with x * d < 2^32 (d >= 2): the runtime divisors of the conv index arithmetic (W, H,
// slab rows) as multiply-high constants - an integer division by a runtime value is ~35 VALU instructions, and a tile needs dozens
// (d == 1 has no 32-bit constant - callers divide by 1 themselves; W, H >= 2 is checked by the launcher)
LTX_DEVFN unsigned magic_u32(int d) { return (unsigned)((0x100000000ull + (unsigned long long)(d - 1)) / (unsigned long long)d); }

// compile-time loop: the body gets an integral_constant, so accumulator arrays are only ever indexed with constants
// (a `#pragma unroll` that the optimiser declines leaves a runtime index and demotes the array to scratch memory)
template <int I, int N, class F>
LTX_DEVFN void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// Workgroup id -> output tile. Supertiles of group_m row-tiles x all column-tiles, row-tile fastest inside: the chunk
// of consecutive workgroups one XCD receives (xcd_remap) then spans group_m row-tiles x (chunk/group_m) column-tiles
// instead of every row-tile x few columns. Every XCD's L2 fetches each operand tile it touches once from the fabric, so
// this trades re-reads of A (rows) against re-reads of B (columns): measured on MI355X with group_m = 4 vs column-major:
// 6144x4096x4096 833 -> 1039 TFLOP/s, 4096^3 897 -> 1017, 1536x4096x16384 1099 -> 1146 (PMC: A was fetched 8x).
// conv launches with one column tile: position L of the launch order -> row tile, blocked 8 row-groups x 4 frames (Conv3dGeom::blk_rg)
LTX_DEVFN int conv_block_order(int L, int F, int RG) {
    constexpr int FB = 4;
    const int RB = RG < 8 ? RG : 8;
    const int fgi = L / (FB * RG);
    const int f0 = fgi * FB;
    const int nf = (F - f0) < FB ? (F - f0) : FB;
    const int w = L - fgi * FB * RG;
    const int per = nf * RB;
    const int rbi = w / per, v = w - rbi * per;
    const int fo = v / RB, ro = v - fo * RB;
    return (f0 + fo) * RG + rbi * RB + ro;
}

LTX_DEVFN void tile_coords(int group_m, int tiles_n, int bid, int tiles_m, int& tm, int& tn) {
    if (group_m > 0 && group_m < tiles_m) {
        const int per = group_m * tiles_n;
        const int grp = bid / per, rem = bid - grp * per;
        const int gm = (tiles_m - grp * group_m) < group_m ? (tiles_m - grp * group_m) : group_m;
        tn = rem / gm;
        tm = grp * group_m + (rem - tn * gm);
    } else {
        tm = bid % tiles_m;
        tn = bid / tiles_m;
    }
}
LTX_DEVFN void tile_coords(const GemmArgs& g, int bid, int tiles_m, int BN_, int& tm, int& tn) {
    tile_coords(g.group_m, (g.N + BN_ - 1) / BN_, bid, tiles_m, tm, tn);
}

// ---- epilogue: per-wave LDS transpose (16 rows at a time), then 16-B row-contiguous global accesses ----
// `get(mi_c, slab)` hands over the 16-row slab mi of this wave's accumulators (f32x4 slab[NI]) - an array copy for the kernels
// that accumulate in VGPRs, an AGPR read-out for the assembly kernel (whose 192 accumulator registers must never be live in
// VGPRs all at once next to this function's prefetch buffers).
// Residual-stream values of this wave's whole tile, loaded by the kernel under its last K-tiles (`gemm_residual_prefetch`) so that
// the epilogue of a gated-residual GEMM - one workgroup per CU, nothing else resident - does not start with an exposed HBM read.
// NSL: how many of the wave's 16-row slabs are held (all of them by default). A kernel whose registers are too few to hold the whole tile
// next to its accumulators keeps slab 0 only (the persistent conv kernel: 16 instead of 48 registers) and the epilogue fetches the
// others itself, one slab ahead.
template <int BM, int BN, int WGM, int WGN, int NSL = BM / WGM / 16>
struct ResidualTile {
    static constexpr int MI = NSL, NSLABS = NSL, NIT = (16 * (BN / WGN / 4)) / 64;
    f32x4 v[MI][NIT];
    f32x4 bias[NIT];          // the column bias: what the epilogue's first slab waits on in launches without a residual
    bool valid = false;       // v holds data
    bool bias_valid = false;  // bias holds data
};

// Column bias of this wave's tile (every launch with interior columns), fetched under the last K-tiles as well.
template <int BM, int BN, int WGM, int WGN, int NSL>
LTX_DEVFN void gemm_bias_prefetch(const GemmArgs& g, int n0, int wc, int lane, ResidualTile<BM, BN, WGM, WGN, NSL>& rt) {
    constexpr int WN = BN / WGN, LPR = WN / 4, NIT = (16 * LPR) / 64;
    const int gn_w = n0 + wc * WN;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int c4 = ((it * 64 + lane) % LPR) * 4;
        rt.bias[it] = g.ep.bias_n ? *(const f32x4*)(g.ep.bias_n + gn_w + c4) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    rt.bias_valid = true;
}

template <int BM, int BN, int WGM, int WGN, int NSL>
LTX_DEVFN void gemm_residual_prefetch(const GemmArgs& g, int m0, int n0, int wr, int wc, int lane, ResidualTile<BM, BN, WGM, WGN, NSL>& rt) {
    constexpr int WM = BM / WGM, WN = BN / WGN, MI = NSL, LPR = WN / 4, NIT = (16 * LPR) / 64;
    const GemmEpilogue& ep = g.ep;
    const float* rbase = ep.resid_src ? ep.resid_src : ep.out_f32;
    const long rld = ep.resid_src ? ep.ld_resid : ep.ld_f32;
    const int gn_w = n0 + wc * WN;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int chunk = it * 64 + lane;
            int gm = m0 + wr * WM + mi * 16 + chunk / LPR;
            gm = gm < g.M ? gm : g.M - 1;
            rt.v[mi][it] = *(const f32x4*)(rbase + (long)gm * rld + gn_w + (chunk % LPR) * 4);
        }
    rt.valid = true;
}

// PN: the fused PixelNorm + SiLU second output (GemmEpilogue::pn_out) is compiled in (conv instantiations only: it adds a
// workgroup barrier per 16-row slab and registers the dense kernels' epilogues do not have to spare).
// SCR: `get(mi_c, scr)` writes the 16 x WN slab row-major into this wave's LDS scratch itself (accumulators that are not in the
// 16x16 MFMA layout: the 32x32x16 kernel); the transposed store, which works from the 16x16 register layout, is then not available.
// SGATE: the launch never carries a gate VECTOR (conv launches: residual gate = gate_scalar) - the interior path then keeps no gate
// registers (32 per lane in the general form, which the persistent conv kernel does not have to spare).
// `hook()`: called once, at the point of the epilogue behind which it issues no further global LOAD (the interior path: right after the
// residual fetch of the last slab has been requested). A persistent kernel requests its next tile's first operands there: vmcnt retires
// loads in order, so anything requested earlier would be waited for by every later residual fetch of this epilogue.
struct NoHook { LTX_DEVFN void operator()() const {} };
template <int BM, int BN, int WGM = 2, int WGN = 2, bool PN = false, bool SCR = false, bool SGATE = false, class Get, class Pre = ResidualTile<BM, BN, WGM, WGN>,
          class Hook = NoHook>
LTX_DEVFN void gemm_epilogue_with(Get&& get, const GemmArgs& g, int m0, int n0, int wr, int wc, int lane, int wave, char* smem,
                                  const Pre* pre = nullptr, Hook&& hook = Hook{}) {
    constexpr int WM = BM / WGM, WN = BN / WGN, MI = WM / 16, NI = WN / 16;
    float* scr = (float*)(smem + wave * (16 * WN * 4));
    constexpr int LPR = WN / 4;    // lanes per output row
    const GemmEpilogue& ep = g.ep;
    if constexpr (!SCR)
    if (ep.out_bf16_t) {
        hook();
        // transposed bf16 store from the accumulator layout: acc[mi][ni][r] = C[16 mi + 4 (lane >> 4) + r][16 ni + (lane & 15)]
        static_for<0, MI>([&](auto mi_c) {
            constexpr int mi = decltype(mi_c)::value;
            f32x4 slab[NI];
            get(mi_c, slab);
            const int gm0 = m0 + wr * WM + mi * 16 + (lane >> 4) * 4;
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
                const int gn = n0 + wc * WN + ni * 16 + (lane & 15);
                if (gn >= g.N || gm0 >= g.M) continue;
                const float bn = ep.bias_n ? ep.bias_n[gn] : 0.f;
                bf16_t* o = ep.out_bf16_t + (long)gn * ep.ld_bf16_t + gm0;
                if (gm0 + 3 < g.M) {
                    uint2 pk;
                    pk.x = pack_bf16x2(slab[ni][0] + bn, slab[ni][1] + bn);
                    pk.y = pack_bf16x2(slab[ni][2] + bn, slab[ni][3] + bn);
                    *(uint2*)o = pk;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (gm0 + r < g.M) o[r] = f32_to_bf16(slab[ni][r] + bn);
                }
            }
        });
        return;
    }
    if (!ep.d2s && n0 + BN <= g.N) {
        // Interior columns (every DiT GEMM): branch-free 16-B accesses, and the residual-stream / gate reads of slab
        // mi+1 are issued BEFORE slab mi's LDS transpose so that their HBM/MALL latency overlaps it. One workgroup
        // per CU runs this tail with nothing else resident, so a dependent load -> fma -> store chain per 16-row slab
        // (the general path below) was costing 12-20 us per gated-residual GEMM (76.8 vs 57.1 us in the DiT block trace).
        constexpr int NIT = (16 * LPR) / 64;
        const bool has_res = ep.resid != 0;
        const bool pre_res = pre && pre->valid;  // workgroup-uniform
        const int gn_w = n0 + wc * WN;
        f32x4 bias[NIT], rs[2][NIT], gt[2][NIT];
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int c4 = ((it * 64 + lane) % LPR) * 4;
            if (pre && pre->bias_valid)
                bias[it] = pre->bias[it];
            else
                bias[it] = ep.bias_n ? *(const f32x4*)(ep.bias_n + gn_w + c4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const float* rbase = ep.resid_src ? ep.resid_src : ep.out_f32;
        const long rld = ep.resid_src ? ep.ld_resid : ep.ld_f32;
        // the usual case - all rows of this wave's tile in one batch element - needs one gate vector, not an integer division
        // per lane and slab: load it once, beside the bias
        const int row_lo = (m0 + wr * WM) < g.M ? (m0 + wr * WM) : g.M - 1;
        const int row_hi = (m0 + wr * WM + WM - 1) < g.M ? (m0 + wr * WM + WM - 1) : g.M - 1;
        const int gb_lo = row_lo / ep.rows_per_batch;
        const bool gate_uniform = !SGATE && has_res && ep.gate && !ep.gate_rowmap && gb_lo == row_hi / ep.rows_per_batch;
        f32x4 gtu[NIT];
        if (gate_uniform) {
#pragma unroll
            for (int it = 0; it < NIT; ++it) gtu[it] = *(const f32x4*)(ep.gate + (long)gb_lo * ep.gate_bstride + gn_w + ((it * 64 + lane) % LPR) * 4);
        }
        auto prefetch = [&](auto mi_c, auto buf_c) {
            constexpr int mi = decltype(mi_c)::value, buf = decltype(buf_c)::value;
            if (!has_res) return;
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int chunk = it * 64 + lane;
                const int c4 = (chunk % LPR) * 4;
                int gm = m0 + wr * WM + mi * 16 + chunk / LPR;
                gm = gm < g.M ? gm : g.M - 1;
                bool held = false;
                if constexpr (mi < Pre::NSLABS) {
                    if (pre_res) {
                        rs[buf][it] = pre->v[mi][it];
                        held = true;
                    }
                }
                if (!held) rs[buf][it] = *(const f32x4*)(rbase + (long)gm * rld + gn_w + c4);
                if constexpr (SGATE) {
                    // (nothing: the scalar gate is applied from ep.gate_scalar below)
                } else if (gate_uniform)
                    gt[buf][it] = gtu[it];
                else if (ep.gate)
                    gt[buf][it] = *(const f32x4*)(ep.gate + (long)(ep.gate_rowmap ? ep.gate_rowmap[gm] : gm / ep.rows_per_batch) * ep.gate_bstride + gn_w + c4);
                else
                    gt[buf][it] = f32x4{ep.gate_scalar, ep.gate_scalar, ep.gate_scalar, ep.gate_scalar};
            }
        };
        prefetch(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
        // fused PixelNorm: the two waves of a tile row-block (wc = 0 / 1) each hold 64 of a row's 128 channels; they trade their
        // partial sums of squares through LDS, double-buffered by slab parity so that one barrier per slab is enough
        const bool pn = PN && ep.pn_out != nullptr;  // workgroup-uniform
        float* pns = (float*)(smem + WGM * WGN * (16 * WN * 4));  // [2][waves][16 rows], behind the transpose scratch
        f32x4 pn_s4 = f32x4{1.f, 1.f, 1.f, 1.f}, pn_h4 = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (PN) {
            static_assert(WGN == 2 && LPR == 16, "fused PixelNorm: two waves per tile row, 16 lanes per 64-column half row");
            if (pn && ep.pn_scale) {
                pn_s4 = *(const f32x4*)(ep.pn_scale + gn_w + (lane % LPR) * 4);
                pn_h4 = *(const f32x4*)(ep.pn_shift + gn_w + (lane % LPR) * 4);
            }
        }
        static_for<0, MI>([&](auto mi_c) {
            constexpr int mi = decltype(mi_c)::value;
            constexpr int buf = mi & 1;
            if constexpr (mi + 1 < MI) prefetch(std::integral_constant<int, mi + 1>{}, std::integral_constant<int, (mi + 1) & 1>{});
            if constexpr (mi == (MI >= 2 ? MI - 2 : 0)) hook();  // the last residual fetch has just been requested
            if constexpr (SCR) {
                get(mi_c, scr);
            } else {
                f32x4 slab[NI];
                get(mi_c, slab);
                static_for<0, NI>([&](auto ni_c) {
                    constexpr int ni = decltype(ni_c)::value;
#pragma unroll
                    for (int r = 0; r < 4; ++r) scr[((lane >> 4) * 4 + r) * WN + ni * 16 + (lane & 15)] = slab[ni][r];
                });
            }
            f32x4 pn_v[PN ? NIT : 1];
            float pn_s2[PN ? NIT : 1];
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int chunk = it * 64 + lane;
                const int row = chunk / LPR;
                const int c4 = (chunk % LPR) * 4;
                f32x4 v = *(const f32x4*)(scr + row * WN + c4);
                const int gm = m0 + wr * WM + mi * 16 + row;
                const int gmc = gm < g.M ? gm : g.M - 1;
                v += bias[it];
                if (ep.bias_m) {
                    const float bm = ep.bias_m[gmc];
                    v += f32x4{bm, bm, bm, bm};
                }
                if (ep.act == LTX_ACT_GELU_TANH) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = gelu_tanh(v[e]);
                } else if (ep.act == LTX_ACT_SILU) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = silu_f(v[e]);
                }
                if (ep.round_bf16) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = bf16_to_f32(f32_to_bf16(v[e]));
                }
                if (has_res) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = rs[buf][it][e] + (SGATE ? ep.gate_scalar : gt[buf][it][e]) * v[e];
                }
#ifdef EPI_NO_STORE  // tools/ubench/gemm_stamps.hip timing experiment
                if (gm < 0) {
#else
                if (gm < g.M) {
#endif
                    uint2 pk;
                    pk.x = pack_bf16x2(v[0], v[1]);
                    pk.y = pack_bf16x2(v[2], v[3]);
                    if (ep.out_f32) *(f32x4*)(ep.out_f32 + (long)gm * ep.ld_f32 + gn_w + c4) = v;
                    if (ep.out_bf16) *(uint2*)(ep.out_bf16 + (long)gm * ep.ld_bf16 + gn_w + c4) = pk;
                }
                if constexpr (PN) {
                    if (pn) {
                        pn_v[it] = v;
                        pn_s2[it] = row16_allsum(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]);  // this wave's 64 channels of row it*4 + lane/16
                    }
                }
            }
            if constexpr (PN) {
                if (pn) {
                    float* mine = pns + (buf * WGM * WGN + wave) * 16;
                    const float* other = pns + (buf * WGM * WGN + (wave ^ 1)) * 16;
                    if ((lane & (LPR - 1)) == 0) {
#pragma unroll
                        for (int it = 0; it < NIT; ++it) mine[it * (64 / LPR) + (lane / LPR)] = pn_s2[it];
                    }
                    __syncthreads();
#pragma unroll
                    for (int it = 0; it < NIT; ++it) {
                        const int chunk = it * 64 + lane;
                        const int row = chunk / LPR;
                        const int c4 = (chunk % LPR) * 4;
                        const int gm = m0 + wr * WM + mi * 16 + row;
                        const float tot = pn_s2[it] + other[row];
                        const float inv = __builtin_amdgcn_rsqf(tot * (1.0f / (float)BN) + 1e-8f);
                        f32x4 y;
#pragma unroll
                        for (int e = 0; e < 4; ++e) y[e] = silu_f(pn_v[it][e] * inv * pn_s4[e] + pn_h4[e]);
                        if (gm < g.M) {
                            uint2 pk;
                            pk.x = pack_bf16x2(y[0], y[1]);
                            pk.y = pack_bf16x2(y[2], y[3]);
                            *(uint2*)(ep.pn_out + (long)gm * ep.ld_pn + gn_w + c4) = pk;
                        }
                    }
                }
            }
        });
        return;
    }
    // ---- depth-to-space store of the VAE upsampler (d2s == 1), interior columns, a wave's columns inside ONE sub-position: the
    // general path below spends ~25 us per tile here (three runtime divisions per 4-wide chunk, four dependent gather loads of the tiled
    // D2S residual, nothing prefetched - tools/ubench/conv_stamps.hip, CONV_D2S=1: epilogue 32.5 us against 7.2 us of a plain store).
    // Here the column part (sub-position, channel, residual column) is per-lane constant, a row splits into (frame, y, x) with two
    // multiply-high forms, and the residual gathers of slab mi + 1 are requested before slab mi is transposed.
    if (ep.d2s == 1 && n0 + BN <= g.N && ep.out_f32 && !ep.out_bf16 && !ep.bias_m && ep.act == LTX_ACT_NONE && !ep.round_bf16 &&
        ((g.N >> 3) % WN) == 0 && ((g.geom.C >> 3) & 3) == 0 && (long)g.M * g.geom.W < (1L << 32) &&
        (long)g.geom.F * g.geom.H * g.geom.H < (1L << 32) && g.geom.H >= 2 && g.geom.W >= 2) {  // (magic_u32(1) does not exist: round-4 advice)
        constexpr int NIT = (16 * LPR) / 64, RPI = 64 / LPR;
        const int cout = g.N >> 3, cd2s = g.geom.C >> 3;
        const int H = g.geom.H, W = g.geom.W;
        const unsigned mg_w = magic_u32(W), mg_h = magic_u32(H);
        const int gn = n0 + wc * WN + (lane % LPR) * 4;
        const int sub = gn / cout, c = gn - sub * cout;  // the wave's 64 columns share `sub` (cout is a multiple of WN)
        const int dt = sub >> 2, dh = (sub >> 1) & 1, dw = sub & 1;
        const int cm = (cd2s & (cd2s - 1)) == 0 ? (c & (cd2s - 1)) : (c % cd2s);
        // (if / else on VALUES: a ?: between `pre->bias[0]` and a global load becomes a select between two pointers, and the kernel's
        // ResidualTile then cannot be promoted to registers - the whole struct went to scratch, in every kernel that shares this function)
        f32x4 bias = f32x4{0.f, 0.f, 0.f, 0.f};
        if (ep.bias_n) bias = *(const f32x4*)(ep.bias_n + gn);
        const float* rcol = ep.resid_src ? ep.resid_src + cm * 8 + sub : nullptr;  // + gm * ld_resid + 8 e
        float* ocol = ep.out_f32 + c;
        f32x4 rs[2][NIT];
        long orow[2][NIT];  // -1: nothing to store (row past M, or the dropped first frame)
        auto fetch = [&](auto mi_c, auto buf_c) {
            constexpr int mi = decltype(mi_c)::value, buf = decltype(buf_c)::value;
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int gm = m0 + wr * WM + mi * 16 + it * RPI + lane / LPR;
                const int gmc = gm < g.M ? gm : g.M - 1;
                const int rowi = (int)__umulhi((unsigned)gmc, mg_w);  // image row over all frames
                const int x = gmc - rowi * W;
                const int f = (int)__umulhi((unsigned)rowi, mg_h);
                const int y = rowi - f * H;
                const int fo = 2 * f + dt - 1;  // first frame after D2S is dropped
                orow[buf][it] = (gm < g.M && fo >= 0) ? ((long)fo * (2 * H) + (2 * y + dh)) * (2 * W) + (2 * x + dw) : -1;
                if (rcol) {
                    const float* rp = rcol + (long)gmc * ep.ld_resid;
                    rs[buf][it] = f32x4{rp[0], rp[8], rp[16], rp[24]};
                } else {
                    rs[buf][it] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
        };
        fetch(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
        // fused PixelNorm of the upsampled voxel (round 5): with cout == BN a tile's 128 columns are ALL channels of one sub-position's
        // voxel, so the first res-block of the next stage gets its input (PixelNorm + modulation + SiLU of the value just stored) from
        // here instead of from a row pass over the whole f32 stream; same exchange between the two waves of a row block as above
        const bool pn = PN && ep.pn_out != nullptr && cout == BN;  // workgroup-uniform
        float* pns = (float*)(smem + WGM * WGN * (16 * WN * 4));
        f32x4 pn_s4 = f32x4{1.f, 1.f, 1.f, 1.f}, pn_h4 = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (PN) {
            if (pn && ep.pn_scale) {
                pn_s4 = *(const f32x4*)(ep.pn_scale + c);
                pn_h4 = *(const f32x4*)(ep.pn_shift + c);
            }
        }
        static_for<0, MI>([&](auto mi_c) {
            constexpr int mi = decltype(mi_c)::value;
            constexpr int buf = mi & 1;
            if constexpr (mi + 1 < MI) fetch(std::integral_constant<int, mi + 1>{}, std::integral_constant<int, (mi + 1) & 1>{});
            if constexpr (mi == (MI >= 2 ? MI - 2 : 0)) hook();  // the last residual gather has just been requested
            if constexpr (SCR) {
                get(mi_c, scr);
            } else {
                f32x4 slab[NI];
                get(mi_c, slab);
                static_for<0, NI>([&](auto ni_c) {
                    constexpr int ni = decltype(ni_c)::value;
#pragma unroll
                    for (int r = 0; r < 4; ++r) scr[((lane >> 4) * 4 + r) * WN + ni * 16 + (lane & 15)] = slab[ni][r];
                });
            }
            f32x4 pn_v[PN ? NIT : 1];
            float pn_s2[PN ? NIT : 1];
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int row = it * RPI + lane / LPR;
                f32x4 v = *(const f32x4*)(scr + row * WN + (lane % LPR) * 4);
                v += bias;
                v += rs[buf][it];
                if (orow[buf][it] >= 0) *(f32x4*)(ocol + orow[buf][it] * ep.ld_f32) = v;
                if constexpr (PN) {
                    if (pn) {
                        pn_v[it] = v;
                        pn_s2[it] = row16_allsum(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]);
                    }
                }
            }
            if constexpr (PN) {
                if (pn) {
                    static_assert(!PN || (WGN == 2 && LPR == 16), "fused PixelNorm: two waves per tile row, 16 lanes per 64-column half row");
                    float* mine = pns + (buf * WGM * WGN + wave) * 16;
                    const float* other = pns + (buf * WGM * WGN + (wave ^ 1)) * 16;
                    if ((lane & (LPR - 1)) == 0) {
#pragma unroll
                        for (int it = 0; it < NIT; ++it) mine[it * RPI + (lane / LPR)] = pn_s2[it];
                    }
                    __syncthreads();
#pragma unroll
                    for (int it = 0; it < NIT; ++it) {
                        const int row = it * RPI + lane / LPR;
                        const float inv = __builtin_amdgcn_rsqf((pn_s2[it] + other[row]) * (1.0f / (float)BN) + 1e-8f);
                        f32x4 y;
#pragma unroll
                        for (int e = 0; e < 4; ++e) y[e] = silu_f(pn_v[it][e] * inv * pn_s4[e] + pn_h4[e]);
                        if (orow[buf][it] >= 0) {
                            uint2 pk;
                            pk.x = pack_bf16x2(y[0], y[1]);
                            pk.y = pack_bf16x2(y[2], y[3]);
                            *(uint2*)(ep.pn_out + orow[buf][it] * ep.ld_pn + c) = pk;
                        }
                    }
                }
            }
        });
        return;
    }
    // ---- the decoder's final un-patchify store (d2s == 3; conv_out: 48 of the tile's 64 columns exist): the same treatment - the
    // column part (pixel row b, offset inside its 12 floats) is per-lane constant, rows split with two multiply-high forms
    if (ep.d2s == 3 && (g.N & 3) == 0 && ep.out_f32 && !ep.out_bf16 && !ep.bias_m && ep.act == LTX_ACT_NONE && !ep.round_bf16 && !ep.resid &&
        (long)g.M * g.geom.W < (1L << 32) && (long)g.geom.F * g.geom.H * g.geom.H < (1L << 32) && g.geom.H >= 2 && g.geom.W >= 2) {
        constexpr int NIT = (16 * LPR) / 64, RPI = 64 / LPR;
        hook();
        const int H = g.geom.H, W = g.geom.W;
        const unsigned mg_w = magic_u32(W), mg_h = magic_u32(H);
        const int gn = n0 + wc * WN + (lane % LPR) * 4;
        const bool col_ok = gn < g.N;  // N % 4 == 0: a 4-wide chunk exists entirely or not at all
        const int b = gn / 12, oc = gn - 12 * b;
        f32x4 bias = f32x4{0.f, 0.f, 0.f, 0.f};
        if (ep.bias_n && col_ok) bias = *(const f32x4*)(ep.bias_n + gn);
        static_for<0, MI>([&](auto mi_c) {
            constexpr int mi = decltype(mi_c)::value;
            if constexpr (SCR) {
                get(mi_c, scr);
            } else {
                f32x4 slab[NI];
                get(mi_c, slab);
                static_for<0, NI>([&](auto ni_c) {
                    constexpr int ni = decltype(ni_c)::value;
#pragma unroll
                    for (int r = 0; r < 4; ++r) scr[((lane >> 4) * 4 + r) * WN + ni * 16 + (lane & 15)] = slab[ni][r];
                });
            }
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int row = it * RPI + lane / LPR;
                const int gm = m0 + wr * WM + mi * 16 + row;
                f32x4 v = *(const f32x4*)(scr + row * WN + (lane % LPR) * 4);
                v += bias;
                if (ep.clip01) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fminf(fmaxf((v[e] + 1.0f) * 0.5f, 0.f), 1.f);
                }
                if (gm < g.M && col_ok) {
                    const int rowi = (int)__umulhi((unsigned)gm, mg_w);
                    const int x = gm - rowi * W;
                    const int f = (int)__umulhi((unsigned)rowi, mg_h);
                    const int y = rowi - f * H;
                    const long orow = (((long)f * (4 * H) + (4 * y + b)) * (4 * W) + 4 * x) * 3;  // ld_f32 is 1
                    *(f32x4*)(ep.out_f32 + orow * ep.ld_f32 + oc) = v;
                }
            }
        });
        return;
    }
    hook();
    static_for<0, MI>([&](auto mi_c) {
        constexpr int mi = decltype(mi_c)::value;
        if constexpr (SCR) {
            get(mi_c, scr);
        } else {
            f32x4 slab[NI];
            get(mi_c, slab);
            static_for<0, NI>([&](auto ni_c) {
                constexpr int ni = decltype(ni_c)::value;
#pragma unroll
                for (int r = 0; r < 4; ++r) scr[((lane >> 4) * 4 + r) * WN + ni * 16 + (lane & 15)] = slab[ni][r];
            });
        }
#pragma unroll
        for (int it = 0; it < (16 * LPR) / 64; ++it) {
            const int chunk = it * 64 + lane;  // 16 rows x LPR float4 chunks, row-major
            const int row = chunk / LPR;
            const int c4 = (chunk % LPR) * 4;
            f32x4 v = *(const f32x4*)(scr + row * WN + c4);
            const int gm = m0 + wr * WM + mi * 16 + row;
            const int gn = n0 + wc * WN + c4;
            if (gm >= g.M || gn >= g.N) continue;
            const int nv = (g.N - gn) < 4 ? (g.N - gn) : 4;
            if (ep.bias_n) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e < nv) v[e] += ep.bias_n[gn + e];
            }
            if (ep.bias_m) {
                const float bm = ep.bias_m[gm];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += bm;
            }
            if (ep.act == LTX_ACT_GELU_TANH) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = gelu_tanh(v[e]);
            } else if (ep.act == LTX_ACT_SILU) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = silu_f(v[e]);
            }
            if (ep.round_bf16) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = bf16_to_f32(f32_to_bf16(v[e]));
            }
            long orow = gm;  // output row (remapped for depth-to-space)
            int ocol = gn;
            if (ep.d2s == 2) {
                // latent upscaler: per-frame pixel shuffle (1,2,2); channels stored (i,j)-major: n' = sub*Cout + c
                const int cout = g.N >> 2;
                const int sub = gn / cout;
                const int c = gn - sub * cout;
                const int hw = g.geom.H * g.geom.W;
                const int f = gm / hw;
                const int rem = gm - f * hw;
                const int y = rem / g.geom.W;
                const int x = rem - y * g.geom.W;
                orow = ((long)f * (2 * g.geom.H) + (2 * y + (sub >> 1))) * (2 * g.geom.W) + (2 * x + (sub & 1));
                ocol = c;
            } else if (ep.d2s == 3) {
                // un-patchify store: this 4-wide chunk is one pixel row b, floats a*3 + c of its 12
                const int hw = g.geom.H * g.geom.W;
                const int f = gm / hw;
                const int rem = gm - f * hw;
                const int y = rem / g.geom.W;
                const int x = rem - y * g.geom.W;
                const int b = gn / 12;
                orow = (((long)f * (4 * g.geom.H) + (4 * y + b)) * (4 * g.geom.W) + 4 * x) * 3;  // ld_f32 is 1
                ocol = gn - b * 12;
                if (ep.clip01) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fminf(fmaxf((v[e] + 1.0f) * 0.5f, 0.f), 1.f);
                }
            } else if (ep.d2s) {
                // VAE upsampler (VideoDecoder.swift:201-251). Conv output channels were permuted at load time to
                // n' = sub*Cout + c (sub = dt*4+dh*2+dw), so this 4-wide chunk has one `sub` and consecutive c.
                const int cout = g.N >> 3;
                const int sub = gn / cout;
                const int c = gn - sub * cout;
                const int dt = sub >> 2, dh = (sub >> 1) & 1, dw = sub & 1;
                const int hw = g.geom.H * g.geom.W;
                const int f = gm / hw;
                const int rem = gm - f * hw;
                const int y = rem / g.geom.W;
                const int x = rem - y * g.geom.W;
                const int fo = 2 * f + dt - 1;  // first frame after D2S is dropped
                if (fo < 0) continue;
                orow = ((long)fo * (2 * g.geom.H) + (2 * y + dh)) * (2 * g.geom.W) + (2 * x + dw);
                ocol = c;
                if (ep.resid_src) {
                    // residual = D2S(x)[c mod C/8], tiled along channels (VideoDecoder.swift:219-234)
                    // c is a multiple of 4 and so is C/8: the chunk's four channels wrap together - one modulo, not four
                    const int cd2s = g.geom.C >> 3;
                    const int cm = (cd2s & (cd2s - 1)) == 0 ? (c & (cd2s - 1)) : (c % cd2s);
                    const float* rs = ep.resid_src + (long)gm * ep.ld_resid + cm * 8 + sub;
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (e < nv) v[e] += rs[e * 8];
                }
            } else if (ep.resid) {
                const float* rs = (ep.resid_src ? ep.resid_src + (long)gm * ep.ld_resid : ep.out_f32 + (long)gm * ep.ld_f32) + gn;
                f32x4 gt;
                if (ep.gate) {
                    const float* gp = ep.gate + (long)(ep.gate_rowmap ? ep.gate_rowmap[gm] : gm / ep.rows_per_batch) * ep.gate_bstride + gn;
#pragma unroll
                    for (int e = 0; e < 4; ++e) gt[e] = (e < nv) ? gp[e] : 0.f;
                } else {
                    gt = f32x4{ep.gate_scalar, ep.gate_scalar, ep.gate_scalar, ep.gate_scalar};
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e < nv) v[e] = rs[e] + gt[e] * v[e];
            }
            if (ep.out_f32) {
                float* o = ep.out_f32 + orow * ep.ld_f32 + ocol;
                if (nv == 4) {
                    *(f32x4*)o = v;
                } else {
                    for (int e = 0; e < nv; ++e) o[e] = v[e];
                }
            }
            if (ep.out_bf16) {
                bf16_t* o = ep.out_bf16 + orow * ep.ld_bf16 + ocol;
                if (nv == 4) {
                    uint2 pk;
                    pk.x = pack_bf16x2(v[0], v[1]);
                    pk.y = pack_bf16x2(v[2], v[3]);
                    *(uint2*)o = pk;
                } else {
                    for (int e = 0; e < nv; ++e) o[e] = f32_to_bf16(v[e]);
                }
            }
        }
    });
}

template <int BM, int BN, int WGM = 2, int WGN = 2, bool PN = false, bool SGATE = false, class Pre = ResidualTile<BM, BN, WGM, WGN>, class Hook = NoHook>
LTX_DEVFN void gemm_epilogue(f32x4 (&acc)[BM / WGM / 16][BN / WGN / 16], const GemmArgs& g, int m0, int n0, int wr, int wc,
                             int lane, int wave, char* smem, const Pre* pre = nullptr, Hook&& hook = Hook{}) {
    constexpr int NI = BN / WGN / 16;
    gemm_epilogue_with<BM, BN, WGM, WGN, PN, false, SGATE>(
        [&](auto mi_c, f32x4(&slab)[NI]) {
            constexpr int mi = decltype(mi_c)::value;
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) slab[ni] = acc[mi][ni];
        },
        g, m0, n0, wr, wc, lane, wave, smem, pre, hook);
}

template <int BM, int BN, bool CONV>
__global__ __launch_bounds__(256) void gemm_bf16_kernel(const GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int WM = BM / 2, WN = BN / 2, MI = WM / 16, NI = WN / 16;
    constexpr int A_BYTES = BM * ROW_BYTES, B_BYTES = BN * ROW_BYTES, STAGE = A_BYTES + B_BYTES;
    constexpr int A_PER_WAVE = BM / 32, B_PER_WAVE = BN / 32;  // wave-instructions (8 rows each) per wave

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;

    const int tiles_m = (g.M + BM - 1) / BM;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    int tm, tn;
    tile_coords(g, bid, tiles_m, BN, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;

    // ---- staging: per-lane source pointers (swizzle on the source side, LDS image stays lane-linear) ----
    const int srow = lane >> 3;  // row inside an 8-row wave-instruction
    const int pch = lane & 7;    // physical 16-B chunk the lane writes
    const bf16_t* a_src[A_PER_WAVE];
    const bf16_t* b_src[B_PER_WAVE];
    RowPos a_pos[A_PER_WAVE];
    int a_lch[A_PER_WAVE];
#pragma unroll
    for (int i = 0; i < A_PER_WAVE; ++i) {
        const int row = (wave + 4 * i) * 8 + srow;
        const int lch = pch ^ ((row >> 1) & 7);
        int gm = m0 + row;
        gm = gm < g.M ? gm : g.M - 1;
        a_lch[i] = lch;
        if constexpr (CONV) {
            const int hw = g.geom.H * g.geom.W;
            a_pos[i].f = gm / hw;
            const int rem = gm - a_pos[i].f * hw;
            a_pos[i].y = rem / g.geom.W;
            a_pos[i].x = rem - a_pos[i].y * g.geom.W;
            a_src[i] = g.A;
        } else {
            a_src[i] = g.A + (long)gm * g.lda + lch * 8;
        }
    }
#pragma unroll
    for (int i = 0; i < B_PER_WAVE; ++i) {
        const int row = (wave + 4 * i) * 8 + srow;
        const int lch = pch ^ ((row >> 1) & 7);
        int gn = n0 + row;
        gn = gn < g.N ? gn : g.N - 1;
        b_src[i] = g.B + (long)gn * g.ldb + lch * 8;
    }
    const int nk = g.K / BK;
    const int cpt = CONV ? (g.geom.C / BK) : 1;  // K-tiles per conv tap

    auto stage = [&](int s, int kt) {
        char* base = smem + s * STAGE;
        if constexpr (CONV) {
            const int tap = kt / cpt;
            const int cc = kt - tap * cpt;
            const int dt = (g.geom.kt == 3) ? tap / 9 : 1;
            const int t9 = (g.geom.kt == 3) ? tap - dt * 9 : tap;
            const int dy = t9 / 3, dx = t9 - dy * 3;
#pragma unroll
            for (int i = 0; i < A_PER_WAVE; ++i) {
                int fi = g.geom.causal ? (a_pos[i].f + dt - 2) : (a_pos[i].f + dt - 1);
                int yi = a_pos[i].y + dy - 1, xi = a_pos[i].x + dx - 1;
                long pos;
                if (g.geom.pad_mode == 1 || g.geom.pad_mode == 3) {
                    if (g.geom.pad_mode == 3) fi = clamp_idx(fi, g.geom.F);  // zeros in H/W, replicated frames in T
                    const bool ok = fi >= 0 && fi < g.geom.F && yi >= 0 && yi < g.geom.H && xi >= 0 && xi < g.geom.W;
                    pos = ok ? ((long)fi * g.geom.H + yi) * g.geom.W + xi : (long)g.geom.F * g.geom.H * g.geom.W;
                } else {
                    fi = clamp_idx(fi, g.geom.F);
                    if (g.geom.pad_mode == 0) {
                        yi = reflect_idx(yi, g.geom.H);
                        xi = reflect_idx(xi, g.geom.W);
                    } else {
                        yi = clamp_idx(yi, g.geom.H);
                        xi = clamp_idx(xi, g.geom.W);
                    }
                    pos = ((long)fi * g.geom.H + yi) * g.geom.W + xi;
                }
                const bf16_t* src = g.A + pos * g.geom.C + cc * BK + a_lch[i] * 8;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                 (__attribute__((address_space(3))) void*)(base + (wave + 4 * i) * 1024),
                                                 16, 0, 0);
            }
        } else {
#pragma unroll
            for (int i = 0; i < A_PER_WAVE; ++i) {
                __builtin_amdgcn_global_load_lds(
                    (const __attribute__((address_space(1))) void*)(a_src[i] + (long)kt * BK),
                    (__attribute__((address_space(3))) void*)(base + (wave + 4 * i) * 1024), 16, 0, 0);
            }
        }
#pragma unroll
        for (int i = 0; i < B_PER_WAVE; ++i) {
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void*)(b_src[i] + (long)kt * BK),
                (__attribute__((address_space(3))) void*)(base + A_BYTES + (wave + 4 * i) * 1024), 16, 0, 0);
        }
    };

    // ---- fragment read offsets (per lane constants; the row-dependent XOR term only depends on lane&15) ----
    const int frow = lane & 15;
    const int fsw = (lane >> 1) & 7;
    const int foff0 = frow * ROW_BYTES + ((((lane >> 4) + 0) ^ fsw) << 4);
    const int foff1 = frow * ROW_BYTES + ((((lane >> 4) + 4) ^ fsw) << 4);

    f32x4 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    stage(0, 0);
    __syncthreads();

    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) stage(cur ^ 1, kt + 1);
        const char* abase = smem + cur * STAGE + (wr * WM) * ROW_BYTES;
        const char* bbase = smem + cur * STAGE + A_BYTES + (wc * WN) * ROW_BYTES;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int fo = kk ? foff1 : foff0;
            s16x8 af[MI], bfr[NI];
#pragma unroll
            for (int i = 0; i < MI; ++i) af[i] = *(const s16x8*)(abase + i * 16 * ROW_BYTES + fo);
#pragma unroll
            for (int j = 0; j < NI; ++j) bfr[j] = *(const s16x8*)(bbase + j * 16 * ROW_BYTES + fo);
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, af[i]),
                                                                        __builtin_bit_cast(bf16x8_t, bfr[j]),
                                                                        acc[i][j], 0, 0, 0);
        }
        __syncthreads();  // LDS-DMA of the next stage has landed (vmcnt(0)) and every wave is done reading `cur`
    }

    gemm_epilogue<BM, BN>(acc, g, m0, n0, wr, wc, lane, wave, smem);
}


// ---------------------------------------------------------------------------------------------------------------
// v2 main loop: NSTAGE-deep LDS ring filled NSTAGE-1 tiles ahead by LDS-DMA, counted `s_waitcnt vmcnt(N)` + raw
// `s_barrier` (never vmcnt(0) in the steady state), and a skewed software pipeline on the register fragments:
//
//   iteration t:   ds_read frags(t, kk=1) -> set B      | MFMA(set A = frags(t, kk=0))      <- LDS latency hidden
//                  wait tile t+1 landed ; s_barrier
//                  LDS-DMA tile t+NSTAGE-1 -> ring slot of tile t-1 (every wave is past its reads of t-1)
//                  ds_read frags(t+1, kk=0) -> set A    | MFMA(set B)                       <- barrier + LDS latency hidden
//
// One barrier per K-tile, loads in flight across it (guide "Pipelining across barriers": counted vmcnt + raw barrier).
// ---------------------------------------------------------------------------------------------------------------
template <int N>
LTX_DEVFN void wait_lgkm_vmcnt_barrier() {
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
}
template <int N>
LTX_DEVFN void wait_lgkm_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory");
}
LTX_DEVFN void wait_lgkm_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
LTX_DEVFN void raw_barrier() { asm volatile("s_barrier" ::: "memory"); }
template <int N>
LTX_DEVFN void wait_vmcnt_barrier() {
    asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory");
}

// (Tried and removed: a ninth wave per workgroup that touched the B lines eight K-tiles ahead of the ring, one dword per
// 128-B line, to hide the HBM latency of the once-streamed DiT weights. Same-process A/B on MI355X: 779 vs 963 TFLOP/s
// cold and 932 vs 1040 warm at 1536x8192x4096 - every touched line crosses the CU's vector L1, +40 % bytes through the
// texture path that this loop already saturates. The ring depth stays the only latency cover.)
#if defined(GEMM_ASM_STAMPS) || defined(GEMM_V2_STAMPS) || defined(DTL_STAMPS) || defined(QKV_STAMPS) || defined(TALL_STAMPS)
__device__ unsigned long long g_gemm_stamps[5][8];  // diagnostic builds only (tools/ubench/gemm_stamps.hip)
#endif
// QB (few-row launches on a quantised Linear, round 3): B arrives as 8-bit codes + bf16 scale / bias per 64-wide group (one group =
// one K-tile) and is de-quantised IN the B stage: stage(t) brings A(t), the codes of tile t+1 (BN x 64 B, a quarter of the bf16
// bytes plus its 2 x BN scalars) into a code ring; the first half of K-tile t converts the codes of tile t+1 into the bf16 image of
// ring slot t+1 (w' = bf16(q * scale + bias), the arithmetic of quant_decode_kernel: the result is bit-identical to the scratch
// path), and the mid-tile barrier that already orders tile t+1's LDS-DMA makes the converted image visible before its first
// fragment read. The codes are read from HBM once and nothing is written back: a few-row GEMM streams half the bytes of the bf16 one.
template <int BM, int BN, int NSTAGE, bool CONV, int WGM = 2, int WGN = 2, bool QB = false>
__global__ __launch_bounds__(WGM * WGN * 64) void gemm_bf16_kernel_v2(const GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NW = WGM * WGN;  // waves per workgroup
    constexpr int WM = BM / WGM, WN = BN / WGN, MI = WM / 16, NI = WN / 16;
    constexpr int A_BYTES = BM * ROW_BYTES, B_BYTES = BN * ROW_BYTES, STAGE = A_BYTES + B_BYTES;
    constexpr int A_PER_WAVE = BM / 8 / NW, B_PER_WAVE = QB ? BN / 16 / NW + 1 : BN / 8 / NW;  // QB: code pieces of 16 rows + one scale / bias piece
    static_assert(A_PER_WAVE * 8 * NW == BM && (QB || B_PER_WAVE * 8 * NW == BN), "tile rows must split evenly over the waves");
    static_assert(!QB || (!CONV && BN % (16 * NW) == 0 && NW * 64 * 16 == BN * 64), "QB: one 16-byte conversion unit per thread");
    constexpr int NQ = NSTAGE + 1;                          // code / scalar ring slots (a tile's codes live from stage(t-1) to K-tile t-1)
    constexpr int Q_BYTES = BN * 64, SB_BYTES = NW * 256;   // codes [BN][64 B]; scalars: one dword per lane of one piece per wave
    constexpr int Q_OFF = NSTAGE * STAGE, SB_OFF = Q_OFF + NQ * Q_BYTES;
    constexpr int LPT = A_PER_WAVE + B_PER_WAVE;  // LDS-DMA instructions per wave per K-tile
    constexpr int PD = NSTAGE - 1;                // prefetch distance in tiles
    static_assert(NSTAGE >= 3, "ring needs >= 3 slots");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / WGN, wc = wave % WGN;

    const int tiles_m = (g.M + BM - 1) / BM;
    const int bid = xcd_remap(blockIdx.x, gridDim.x) + g.tile0;
    int tm, tn;
    tile_coords(g, bid, tiles_m, BN, tm, tn);
    if constexpr (CONV && BM == 192) {
        if (g.geom.blk_rg > 0 && g.tile_count == 0 && g.split_k <= 1 && g.N <= BN) tm = conv_block_order(tm, g.geom.F, g.geom.blk_rg);
    }
    const int m0 = tm * BM, n0 = tn * BN;
#ifdef GEMM_V2_STAMPS  // tools/ubench/gemm_stamps.hip: 100 MHz wall-clock stamps of one wave (prologue / main loop / epilogue)
    const unsigned long long st0 = wall_clock64();
#endif

    const int srow = lane >> 3;
    const int pch = lane & 7;
    const bf16_t* a_src[A_PER_WAVE];
    const bf16_t* b_src[B_PER_WAVE];
    int a_lch[A_PER_WAVE];
    // conv mode, separable tap tables: the voxel index of tap (dt, dy, dx) of a row is tf[dt] + ty[dy] + tx[dx] with the padding
    // rule (reflect / clamp / replicate) already applied per axis, and `bad` has one bit per (axis, tap index) that falls into ZERO
    // padding (those taps read the zero voxel behind the tensor). Built once per tile, branch-free; a tap change then costs a few
    // selects and adds per row instead of re-deriving the neighbour from (f, y, x) (the 128-channel convs change tap every second
    // K-tile).
    struct TapTab {
        int f0, f1, f2, y0, y1, y2, x0, x1, x2, bad;
    };
    TapTab a_tab[A_PER_WAVE];
    struct TapStep {
        int x01, x12, y01, y12, t01, t12;
    };
    TapStep a_step[CONV ? A_PER_WAVE : 1];
    const bool conv_steps = CONV && !(g.geom.pad_mode == 1 || g.geom.pad_mode == 3);  // no zero padding: taps are positions
    const bf16_t* a_row0[A_PER_WAVE];
#pragma unroll
    for (int i = 0; i < A_PER_WAVE; ++i) {
        const int row = (wave + NW * i) * 8 + srow;
        const int lch = pch ^ ((row >> 1) & 7);
        int gm = m0 + row;
        gm = gm < g.M ? gm : g.M - 1;
        a_lch[i] = lch;
        if constexpr (CONV) {
            const int F = g.geom.F, H = g.geom.H, W = g.geom.W, hw = H * W;
            const int pf = gm / hw;
            const int rem = gm - pf * hw;
            const int py = rem / W;
            const int px = rem - py * W;
            a_src[i] = g.A;
            a_row0[i] = g.A + lch * 8;
            const bool zero_t = g.geom.pad_mode == 1;
            const bool zero_hw = g.geom.pad_mode == 1 || g.geom.pad_mode == 3;
            const bool refl_hw = g.geom.pad_mode == 0;
            int bad = 0;
            auto axis_t = [&](int d) {
                const int fi = g.geom.causal ? (pf + d - 2) : (pf + d - 1);
                const bool out = fi < 0 || fi >= F;
                bad |= (zero_t && out) ? (1 << d) : 0;
                return clamp_idx(fi, F) * hw;
            };
            auto axis_s = [&](int p, int n, int d, int bit) {
                const int v = p + d - 1;
                const bool out = v < 0 || v >= n;
                bad |= (zero_hw && out) ? (bit << d) : 0;
                return refl_hw ? reflect_idx(v, n) : clamp_idx(v, n);
            };
            TapTab& t = a_tab[i];
            t.f0 = axis_t(0); t.f1 = axis_t(1); t.f2 = axis_t(2);
            t.y0 = axis_s(py, H, 0, 8) * W; t.y1 = axis_s(py, H, 1, 8) * W; t.y2 = axis_s(py, H, 2, 8) * W;
            t.x0 = axis_s(px, W, 0, 64); t.x1 = axis_s(px, W, 1, 64); t.x2 = axis_s(px, W, 2, 64);
            t.bad = bad;
            // without zero padding a tap is a position, and the next tap in (dt, dy, dx) order is that position plus one of six
            // per-row steps (elements): a tap change is then a 64-bit add per row
            TapStep& st = a_step[i];
            const int C = g.geom.C;
            st.x01 = (t.x1 - t.x0) * C;
            st.x12 = (t.x2 - t.x1) * C;
            st.y01 = (t.x0 - t.x2 + t.y1 - t.y0) * C;
            st.y12 = (t.x0 - t.x2 + t.y2 - t.y1) * C;
            st.t01 = (t.x0 - t.x2 + t.y0 - t.y2 + t.f1 - t.f0) * C;
            st.t12 = (t.x0 - t.x2 + t.y0 - t.y2 + t.f2 - t.f1) * C;
        } else {
            a_src[i] = g.A + (long)gm * g.lda + lch * 8;
        }
    }
    const uint8_t* q_src[QB ? BN / 16 / NW : 1];  // QB: this lane's 16 codes of a K-tile: row 16 (wave + NW i) + lane / 4, bytes 16 (lane % 4) ..
    const bf16_t* sb_src = nullptr;               // QB: this lane's scalar of a K-tile: lanes 0-15 scale, 16-31 bias of row 16 wave + (lane & 15)
    const int groups = g.K / BK;
    if constexpr (QB) {
#pragma unroll
        for (int i = 0; i < BN / 16 / NW; ++i) {
            int gn = n0 + (wave + NW * i) * 16 + (lane >> 2);
            gn = gn < g.N ? gn : g.N - 1;
            q_src[i] = g.Bq + (long)gn * g.K + (lane & 3) * 16;
        }
        int gn = n0 + wave * 16 + (lane & 15);
        gn = gn < g.N ? gn : g.N - 1;
        sb_src = ((lane & 16) ? g.Bqb : g.Bqs) + (long)gn * groups;
    } else {
#pragma unroll
        for (int i = 0; i < B_PER_WAVE; ++i) {
            const int row = (wave + NW * i) * 8 + srow;
            const int lch = pch ^ ((row >> 1) & 7);
            int gn = n0 + row;
            gn = gn < g.N ? gn : g.N - 1;
            b_src[i] = g.B + (long)gn * g.ldb + lch * 8;
        }
    }
    int nk = g.K / BK, kt0 = 0;  // this workgroup's K-tiles: [kt0, kt0 + nk)
    if (g.split_k > 1) {
        const int z = blockIdx.y;
        kt0 = (int)((long)nk * z / g.split_k);
        nk = (int)((long)nk * (z + 1) / g.split_k) - kt0;
    }
    const int cpt = CONV ? (g.geom.C / BK) : 1;
    // QB: codes + scalars of absolute K-tile `kt` (clamped: a tile past the end is staged into a free slot and never converted)
    auto stage_q = [&](int kt) {
        if constexpr (QB) {
            const int t = kt < groups ? kt : groups - 1;
            const int qslot = (kt - kt0 + NQ) % NQ;
#pragma unroll
            for (int i = 0; i < BN / 16 / NW; ++i)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(q_src[i] + (long)t * BK),
                                                 (__attribute__((address_space(3))) void*)(smem + Q_OFF + qslot * Q_BYTES + (wave + NW * i) * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(sb_src + t),
                                             (__attribute__((address_space(3))) void*)(smem + SB_OFF + qslot * SB_BYTES + wave * 256), 2, 0, 0);
        }
    };
    // QB: codes of tile index `j` (relative to kt0) -> bf16 image of ring slot `slot` (B part). Thread = (row tid / 4, 16 codes tid % 4).
    auto convert_q = [&](int slot, int j) {
        if constexpr (QB) {
            const int qslot = (j + NQ) % NQ;
            const int row = tid >> 2, c4 = tid & 3;
            const uint4 raw = *(const uint4*)(smem + Q_OFF + qslot * Q_BYTES + row * 64 + c4 * 16);
            const char* sbp = smem + SB_OFF + qslot * SB_BYTES + (row >> 4) * 256 + (row & 15) * 4;
            const float scale = bf16_to_f32((bf16_t)(*(const uint32_t*)sbp & 0xffffu));
            const float bias = bf16_to_f32((bf16_t)(*(const uint32_t*)(sbp + 64) & 0xffffu));
            const uint32_t wd[4] = {raw.x, raw.y, raw.z, raw.w};
            uint32_t out[8];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const float q0 = (float)((wd[i] >> (16 * jj)) & 0xffu), q1 = (float)((wd[i] >> (16 * jj + 8)) & 0xffu);
                    out[i * 2 + jj] = pack_bf16x2(q0 * scale + bias, q1 * scale + bias);
                }
            char* brow = smem + slot * STAGE + A_BYTES + row * ROW_BYTES;
            const int sw = (row >> 1) & 7;
            *(uint4*)(brow + (((2 * c4) ^ sw) << 4)) = uint4{out[0], out[1], out[2], out[3]};
            *(uint4*)(brow + (((2 * c4 + 1) ^ sw) << 4)) = uint4{out[4], out[5], out[6], out[7]};
        }
    };

    // conv mode: the gathered source pointers only change when the 3x3x3 tap changes (every C/64 K-tiles); inside a
    // tap they just advance by one K-tile. K-tiles are staged in increasing order, so the pointers are loop state.
    int a_fy[A_PER_WAVE];  // tf[dt] + ty[dy] of the current (dt, dy): changes every third tap
    int fy_of = -1;        // tap / 3 that a_fy belongs to
    auto conv_tap_ptrs = [&](int tap) {
        const int dt = (g.geom.kt == 3) ? tap / 9 : 1;
        const int t9 = (g.geom.kt == 3) ? tap - dt * 9 : tap;
        const int dy = t9 / 3, dx = t9 - dy * 3;
        // uniform all-ones / zero masks instead of `dt == 0 ? f0 : ...`: the compiler turns such a chain over struct fields into an
        // indexed scratch array (a scratch load + vmcnt(0) in the middle of the ring's counted waits)
        if (tap / 3 != fy_of) {
            fy_of = tap / 3;
            const int mt1 = -(dt == 1), mt2 = -(dt == 2), my1 = -(dy == 1), my2 = -(dy == 2);
#pragma unroll
            for (int i = 0; i < A_PER_WAVE; ++i) {
                const TapTab& t = a_tab[i];
                a_fy[i] = t.f0 + t.y0 + (((t.f1 - t.f0) & mt1) + ((t.f2 - t.f0) & mt2)) + (((t.y1 - t.y0) & my1) + ((t.y2 - t.y0) & my2));
            }
        }
        const int mx1 = -(dx == 1), mx2 = -(dx == 2);
        const int mask = (1 << dt) | (8 << dy) | (64 << dx);
        const int zero_vox = g.geom.F * g.geom.H * g.geom.W;  // the zero voxel the caller keeps behind the tensor
        const bool zero_pad = g.geom.pad_mode == 1 || g.geom.pad_mode == 3;
#pragma unroll
        for (int i = 0; i < A_PER_WAVE; ++i) {
            const TapTab& t = a_tab[i];
            int vox = a_fy[i] + t.x0 + (((t.x1 - t.x0) & mx1) + ((t.x2 - t.x0) & mx2));
            if (zero_pad) {
                const int hit = -(int)((t.bad & mask) != 0);
                vox = (zero_vox & hit) | (vox & ~hit);
            }
            a_src[i] = a_row0[i] + (long)vox * g.geom.C;
        }
    };
    // tap `from` -> from + 1 where taps are positions: one uniform branch picks the step, each arm is a 64-bit add per row
    auto conv_tap_step = [&](int from) {
        const int t9 = (g.geom.kt == 3) ? from % 9 : from;
        const int dt = (g.geom.kt == 3) ? from / 9 : 1;
        const int dy = t9 / 3, dx = t9 - dy * 3;
#define LTX_TAP_STEP(FIELD)                                                   \
    _Pragma("unroll") for (int i = 0; i < A_PER_WAVE; ++i) a_src[i] += (long)a_step[i].FIELD
        if (dx == 0) { LTX_TAP_STEP(x01); }
        else if (dx == 1) { LTX_TAP_STEP(x12); }
        else if (dy == 0) { LTX_TAP_STEP(y01); }
        else if (dy == 1) { LTX_TAP_STEP(y12); }
        else if (dt == 0) { LTX_TAP_STEP(t01); }
        else { LTX_TAP_STEP(t12); }
#undef LTX_TAP_STEP
    };
    int conv_tap = kt0 / cpt, conv_cc = kt0 - conv_tap * cpt;  // position of the NEXT K-tile to stage
    auto stage = [&](int slot, int kt) {
        char* base = smem + slot * STAGE;
        if constexpr (CONV) {
#pragma unroll
            for (int i = 0; i < A_PER_WAVE; ++i) {
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a_src[i] + conv_cc * BK),
                                                 (__attribute__((address_space(3))) void*)(base + (wave + NW * i) * 1024),
                                                 16, 0, 0);
            }
            if (++conv_cc == cpt) {  // the pointers of the next tap, behind the loads of this one
                conv_cc = 0;
                if (++conv_tap < 9 * g.geom.kt) {
                    if (conv_steps) conv_tap_step(conv_tap - 1); else conv_tap_ptrs(conv_tap);
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < A_PER_WAVE; ++i) {
                __builtin_amdgcn_global_load_lds(
                    (const __attribute__((address_space(1))) void*)(a_src[i] + (long)kt * BK),
                    (__attribute__((address_space(3))) void*)(base + (wave + NW * i) * 1024), 16, 0, 0);
            }
        }
        if constexpr (QB) {
            stage_q(kt + 1);  // the codes run one tile ahead of the activations: they are converted during K-tile kt
        } else {
            if (BM == 128 && BN == 64 && !CONV && g.b_nt) {  // uniform branch; the policy is an immediate of the instruction
#pragma unroll
                for (int i = 0; i < B_PER_WAVE; ++i) {
                    __builtin_amdgcn_global_load_lds(
                        (const __attribute__((address_space(1))) void*)(b_src[i] + (long)kt * BK),
                        (__attribute__((address_space(3))) void*)(base + A_BYTES + (wave + NW * i) * 1024), 16, 0, 2);
                }
            } else {
#pragma unroll
                for (int i = 0; i < B_PER_WAVE; ++i) {
                    __builtin_amdgcn_global_load_lds(
                        (const __attribute__((address_space(1))) void*)(b_src[i] + (long)kt * BK),
                        (__attribute__((address_space(3))) void*)(base + A_BYTES + (wave + NW * i) * 1024), 16, 0, 0);
                }
            }
        }
    };

    const int frow = lane & 15;
    const int fsw = (lane >> 1) & 7;
    const int foff0 = frow * ROW_BYTES + ((((lane >> 4) + 0) ^ fsw) << 4);
    const int foff1 = frow * ROW_BYTES + ((((lane >> 4) + 4) ^ fsw) << 4);
    const int a_wave_off = (wr * WM) * ROW_BYTES;
    const int b_wave_off = A_BYTES + (wc * WN) * ROW_BYTES;

    f32x4 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    s16x8 fa0[MI], fb0[NI], fa1[MI], fb1[NI];
    auto load_frags = [&](int slot, int fo, s16x8(&fa)[MI], s16x8(&fb)[NI]) {
        const char* base = smem + slot * STAGE;
#pragma unroll
        for (int i = 0; i < MI; ++i) fa[i] = *(const s16x8*)(base + a_wave_off + i * 16 * ROW_BYTES + fo);
#pragma unroll
        for (int j = 0; j < NI; ++j) fb[j] = *(const s16x8*)(base + b_wave_off + j * 16 * ROW_BYTES + fo);
    };
    // MFMAs idx in [FROM, TO) of the MIxNI grid (row-major) - split so that the compiler-inserted lgkmcnt wait sits
    // in front of the FIRST product only, while nothing younger is outstanding (see the loop below)
    auto mfma_first = [&](const s16x8(&fa)[MI], const s16x8(&fb)[NI]) {
        acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, fa[0]),
                                                            __builtin_bit_cast(bf16x8_t, fb[0]), acc[0][0], 0, 0, 0);
    };
    auto mfma_rest = [&](const s16x8(&fa)[MI], const s16x8(&fb)[NI]) {
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NI; ++j)
                if (i + j > 0)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, fa[i]),
                                                                        __builtin_bit_cast(bf16x8_t, fb[j]), acc[i][j], 0, 0, 0);
    };

    // prologue: fill PD ring slots, wait for tile 0, fetch its first fragments
    if constexpr (CONV) {
        conv_tap_ptrs(conv_tap);  // absolute pointers of the first tap (a K split may begin at any tap, in the middle of one)
    }
    if constexpr (QB) stage_q(kt0);  // codes of the first tile (stage(t) brings the codes of tile t + 1)
#pragma unroll
    for (int s = 0; s < PD; ++s)
        if (s < nk) stage(s, kt0 + s);
    if (nk >= PD) wait_vmcnt_barrier<(PD - 1) * LPT>(); else wait_vmcnt_barrier<0>();
    if constexpr (QB) {
        convert_q(0, 0);  // the first tile's weights, visible behind a barrier of their own
        wait_lgkm_barrier();
    }
#ifdef GEMM_V2_STAMPS
    const unsigned long long st1 = wall_clock64();
    const unsigned long long cy1 = __builtin_amdgcn_s_memtime();  // shader cycles next to wall time: the clock the part holds in the loop (round 5)
#endif
    load_frags(0, foff0, fa0, fb0);
    const bool late = NW == 8 && g.conv_stagger && wave >= NW / 2;  // wave-uniform (GemmArgs::conv_stagger: option "gemm_stagger" for dense launches)

    // One K-tile. STEADY iterations are branch-free so that each half is ONE scheduling region in which the LDS
    // fragment reads and the LDS-DMA issues are interleaved one-for-one with MFMAs (sched_group_barrier): their issue
    // cost then hides under the previous MFMA's execution instead of serialising in front of the MFMA cluster
    // (ablation on MI355X: MFMA 98 us, LDS reads+barriers 74 us, DMA issue 57 us were ADDING UP to 207 us).
    int slot = 0;  // ring slot of tile kt
    bool drained = false;
    auto ktile = [&](int kt, auto steady_tag) {
        constexpr bool STEADY = decltype(steady_tag)::value;
        int nslot = slot + 1;
        nslot = nslot == NSTAGE ? 0 : nslot;
        int pslot = slot - 1;  // slot of tile kt-1 == slot of tile kt+PD
        pslot = pslot < 0 ? NSTAGE - 1 : pslot;
        // ---- first half: the only LDS reads outstanding at the first MFMA are set A's (issued half a tile ago)
        mfma_first(fa0, fb0);
        __builtin_amdgcn_sched_barrier(0);
        load_frags(slot, foff1, fa1, fb1);
        if constexpr (QB) {
            if (kt + 1 < nk) convert_q(nslot, kt + 1);  // codes of tile kt+1 (visible since the previous mid-tile barrier) -> its bf16 image
        }
        mfma_rest(fa0, fb0);
        if constexpr (!QB) {
#pragma unroll
            for (int q = 0; q < MI + NI; ++q) {
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // one ds_read
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // one MFMA
            }
            __builtin_amdgcn_sched_group_barrier(0x008, MI * NI - 1 - (MI + NI), 0);
        }
        // ---- tile kt+1 must have landed for every wave; tiles kt+2 .. kt+PD-1 may stay in flight. The first tail tile drains the
        // ring (every remaining tile visible to every wave); the tail tiles after it stage nothing and need neither wait nor barrier.
        // QB: the barrier also publishes the image just converted (its ds_writes are retired first), so every tile has one.
        if constexpr (QB) {
            if constexpr (STEADY) wait_lgkm_vmcnt_barrier<(PD - 2) * LPT>(); else wait_lgkm_vmcnt_barrier<0>();
        } else {
            if constexpr (STEADY) wait_vmcnt_barrier<(PD - 2) * LPT>(); else if (!drained) wait_vmcnt_barrier<0>();
        }
        // ---- second half
        mfma_first(fa1, fb1);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (STEADY) {
            // staggered staging (round 5, as conv_halo.inc): of the two waves that share a SIMD (w, w + NW / 2) the second issues its
            // LDS-DMA pieces behind this half's MFMAs instead of in front of them, so that the two are not held by their pieces at the
            // same time. Same loads, same per-wave order, same barrier interval: the counted waits do not change.
            if (!late) stage(pslot, kt0 + kt + PD);
            load_frags(nslot, foff0, fa0, fb0);
            mfma_rest(fa1, fb1);
            if constexpr (!QB) {
#pragma unroll
                for (int q = 0; q < LPT; ++q) {
                    __builtin_amdgcn_sched_group_barrier(0x020, 1, 1);  // one LDS-DMA (VMEM read)
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 1);
                }
#pragma unroll
                for (int q = 0; q < MI + NI; ++q) {
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 1);
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 1);
                }
                __builtin_amdgcn_sched_group_barrier(0x008, MI * NI - 1 - (MI + NI) - LPT, 1);
            }
            if (late) stage(pslot, kt0 + kt + PD);
        } else {
            if (kt + 1 < nk) load_frags(nslot, foff0, fa0, fb0);
            mfma_rest(fa1, fb1);
        }
        slot = nslot;
    };
    int kt = 0;
    for (; kt < nk - PD; ++kt) ktile(kt, std::true_type{});
    ResidualTile<BM, BN, WGM, WGN> rt;
    if (kt < nk) {
        ktile(kt, std::false_type{});
        ++kt;
        drained = true;
        // gated-residual launches (the DiT's attention-out and FFN-out projections): fetch the residual-stream tile now, under the
        // MFMAs of the last PD-1 K-tiles, instead of at the top of the epilogue
        if (!g.ep.d2s && g.split_k <= 1 && n0 + BN <= g.N && kt < nk) {
            gemm_bias_prefetch(g, n0, wc, lane, rt);
            if (g.ep.resid) gemm_residual_prefetch(g, m0, n0, wr, wc, lane, rt);
        }
    }
    for (; kt < nk; ++kt) ktile(kt, std::false_type{});
    __syncthreads();
#ifdef GEMM_V2_STAMPS
    const unsigned long long st2 = wall_clock64();
    const unsigned long long cy2 = __builtin_amdgcn_s_memtime();
#endif
    if (g.split_k > 1) {
        GemmArgs gs = g;  // raw partial tile -> workspace slice of this split
        gs.ep = GemmEpilogue{};
        gs.ep.out_f32 = g.split_ws + ((long)blockIdx.y * (g.win_rows ? g.win_rows : g.M) - g.win_row0) * g.N;  // rows are absolute
        gs.ep.ld_f32 = g.N;
        gemm_epilogue<BM, BN, WGM, WGN>(acc, gs, m0, n0, wr, wc, lane, wave, smem);
        return;
    }
    gemm_epilogue<BM, BN, WGM, WGN, (CONV && BN == 128 && WGN == 2)>(acc, g, m0, n0, wr, wc, lane, wave, smem, &rt);
#ifdef GEMM_V2_STAMPS
    {
        const unsigned long long st3 = wall_clock64();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned long long st4 = wall_clock64();
        if (lane == 0 && (blockIdx.x == 7 || blockIdx.x == 200) && wave < 4) {
            unsigned long long* d = &g_gemm_stamps[blockIdx.x == 7 ? wave : 4][0];
            if (blockIdx.x == 7 || wave == 0) {
                d[0] = st0; d[1] = st1; d[2] = st2; d[3] = st3; d[4] = st4; d[5] = cy2 - cy1;
            }
        }
    }
#endif
}


#include "conv_halo.inc"
#include "conv_halo2.inc"


// ---------------------------------------------------------------------------------------------------------------
// small-M path: one wave per output column, f32 activations x bf16 weights
// ---------------------------------------------------------------------------------------------------------------
template <int MMAX>
__global__ __launch_bounds__(256) void gemv_f32_kernel(const float* __restrict__ a, long lda,
                                                       const bf16_t* __restrict__ W, long ldw,
                                                       const float* __restrict__ bias, float* __restrict__ out,
                                                       long ldo, int M, int N, int K, int in_act) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    float accv[MMAX];
#pragma unroll
    for (int m = 0; m < MMAX; ++m) accv[m] = 0.f;
    const bf16_t* wrow = W + (long)n * ldw;
    for (int k = lane * 8; k < K; k += 512) {
        const s16x8 wv = *(const s16x8*)(wrow + k);
        float wf[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) wf[e] = bf16_to_f32((bf16_t)wv[e]);
#pragma unroll
        for (int m = 0; m < MMAX; ++m) {
            if (m < M) {
                const f32x4 a0 = *(const f32x4*)(a + (long)m * lda + k);
                const f32x4 a1 = *(const f32x4*)(a + (long)m * lda + k + 4);
                float av[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float x = av[e];
                    if (in_act == LTX_ACT_SILU) x = silu_f(x);
                    // an explicit fma: left to contraction, the compiler fused this for some rows m and emitted (packed) mul + add for
                    // others, so identical rows of a batch differed by an ulp (round 4: found by the batch-consistency test)
                    accv[m] = __builtin_fmaf(x, wf[e], accv[m]);
                }
            }
        }
    }
#pragma unroll
    for (int m = 0; m < MMAX; ++m) {
        const float s = wave_reduce_sum(accv[m]);
        if (lane == 0 && m < M) out[(long)m * ldo + n] = s + (bias ? bias[n] : 0.f);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// grouped small-M path: up to 8 gemv_f32 jobs of one M in one launch (the six AdaLayerNormSingle embedders of the dual model, one
// launch per stage). Each job's arithmetic is gemv_f32_kernel's - the same lane -> k mapping (lane * 8 + 512 * trip), the same
// explicit fma chain in the same order, the same wave reduction and bias add - so every job is bit-equal to launch_gemv_f32 on its
// operands. What differs is when the weights are fetched: the 16-byte weight vectors of up to eight trips (4096 k, 32 VGPRs) are
// loaded straight to registers before the first fma of the chunk.
// ---------------------------------------------------------------------------------------------------------------
// one trip of gemv_f32_kernel's loop body: lane's 8 weights at k against rows 0 .. M-1
template <int MMAX>
LTX_DEVFN void gemv_trip(const float* __restrict__ a, long lda, const s16x8 wv, int k, int M, int in_act, float (&accv)[MMAX]) {
    float wf[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) wf[e] = bf16_to_f32((bf16_t)wv[e]);
#pragma unroll
    for (int m = 0; m < MMAX; ++m) {
        if (m < M) {
            const f32x4 a0 = *(const f32x4*)(a + (long)m * lda + k);
            const f32x4 a1 = *(const f32x4*)(a + (long)m * lda + k + 4);
            float av[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float x = av[e];
                if (in_act == LTX_ACT_SILU) x = silu_f(x);
                accv[m] = __builtin_fmaf(x, wf[e], accv[m]);  // explicit, as in gemv_f32_kernel
            }
        }
    }
}
// UN whole trips starting at the lane's k: every weight load is issued before the first fma; the fmas run in trip order
template <int MMAX, int UN>
LTX_DEVFN void gemv_chunk(const float* __restrict__ a, long lda, const bf16_t* __restrict__ wrow, int k, int M, int in_act, float (&accv)[MMAX]) {
    s16x8 wv[UN];
#pragma unroll
    for (int i = 0; i < UN; ++i) wv[i] = *(const s16x8*)(wrow + k + 512 * i);
#pragma unroll
    for (int i = 0; i < UN; ++i) gemv_trip<MMAX>(a, lda, wv[i], k + 512 * i, M, in_act, accv);
}

template <int MMAX>
__global__ __launch_bounds__(256) void gemv_group_kernel(const GemvGroup g) {
    // the job of this workgroup: uniform, from the prefix table (a job with N = 0 owns no workgroup and is stepped over)
    int j = 0;
    while (j < g.n_jobs - 1 && (int)blockIdx.x >= g.wg_end[j]) ++j;
    const GemvJob& job = g.job[j];
    const int wg0 = j ? g.wg_end[j - 1] : 0;
    const int lane = threadIdx.x & 63;
    const int n = ((int)blockIdx.x - wg0) * 4 + (threadIdx.x >> 6);
    const int M = g.M, N = job.N, K = job.K, in_act = job.in_act;
    if (n >= N) return;
    const float* __restrict__ a = job.a;
    const long lda = job.lda;
    float accv[MMAX];
#pragma unroll
    for (int m = 0; m < MMAX; ++m) accv[m] = 0.f;
    const bf16_t* wrow = job.W + (long)n * job.ldw;
    // whole chunks need no lane predicate: kb is uniform and every lane's k of the chunk is below K
    int kb = 0;
    for (; kb + 4096 <= K; kb += 4096) gemv_chunk<MMAX, 8>(a, lda, wrow, kb + lane * 8, M, in_act, accv);
    if (kb + 2048 <= K) {
        gemv_chunk<MMAX, 4>(a, lda, wrow, kb + lane * 8, M, in_act, accv);
        kb += 2048;
    }
    if (kb + 1024 <= K) {
        gemv_chunk<MMAX, 2>(a, lda, wrow, kb + lane * 8, M, in_act, accv);
        kb += 1024;
    }
    if (kb + 512 <= K) {
        gemv_chunk<MMAX, 1>(a, lda, wrow, kb + lane * 8, M, in_act, accv);
        kb += 512;
    }
    if (kb + lane * 8 < K) gemv_chunk<MMAX, 1>(a, lda, wrow, kb + lane * 8, M, in_act, accv);  // the partly filled last trip
    const float* bias = job.bias;
    float* out = job.out;
    const long ldo = job.ldo;
#pragma unroll
    for (int m = 0; m < MMAX; ++m) {
        const float s = wave_reduce_sum(accv[m]);
        if (lane == 0 && m < M) out[(long)m * ldo + n] = s + (bias ? bias[n] : 0.f);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// decode path, M = 1, bf16 x bf16 -> bf16 (gemm.h, GemvBf16Args): token generation reads every weight once per token, so this is a
// copy kernel with a dot product attached. The activation row goes to LDS once per workgroup (K <= 16384: 32 KB); a wave owns NR
// weight rows and walks K in trips of 512 (lane * 8 + 512 * trip, 16 bytes per lane). All NR * UN weight vectors of a chunk are
// issued before the first fma - straight to VGPRs, non-temporal, no LDS round trip - and the x vector of a trip is one ds_read_b128
// shared by the NR rows. NR * UN = 16 vectors (64 VGPRs) in flight per lane. Rows at or past N are clamped to row N - 1 for the
// loads (the address stays inside W) and their stores are skipped.
// ---------------------------------------------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;  // the non-temporal builtin takes clang vectors, not HIP's uint4
LTX_DEVFN void gemv_bf16_fma8(const u32x4 w, const u32x4 x, float& acc) {
    const uint32_t wv[4] = {w[0], w[1], w[2], w[3]}, xv[4] = {x[0], x[1], x[2], x[3]};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        acc = __builtin_fmaf(__builtin_bit_cast(float, xv[i] << 16), __builtin_bit_cast(float, wv[i] << 16), acc);
        acc = __builtin_fmaf(__builtin_bit_cast(float, xv[i] & 0xffff0000u), __builtin_bit_cast(float, wv[i] & 0xffff0000u), acc);
    }
}
template <int NR, int UN>
LTX_DEVFN void gemv_bf16_chunk(const bf16_t* const (&wrow)[NR], const u32x4* xs, int k, float (&acc)[NR]) {
    u32x4 wv[UN][NR];
#pragma unroll
    for (int i = 0; i < UN; ++i)
#pragma unroll
        for (int r = 0; r < NR; ++r) wv[i][r] = __builtin_nontemporal_load((const u32x4*)(wrow[r] + k + 512 * i));
#pragma unroll
    for (int i = 0; i < UN; ++i) {
        const u32x4 x = xs[(k >> 3) + 64 * i];
#pragma unroll
        for (int r = 0; r < NR; ++r) gemv_bf16_fma8(wv[i][r], x, acc[r]);
    }
}
LTX_DEVFN float gemv_bf16_round(float v) { return bf16_to_f32(f32_to_bf16(v)); }

// NR weight rows per wave; GEGLU: rows 0 .. NR/2-1 are gate rows n, rows NR/2 .. are up rows N + n of the same outputs
template <int NR, bool GEGLU>
__global__ __launch_bounds__(256) void gemv_bf16_kernel(const GemvBf16Args a) {
    __shared__ u32x4 xs[2048];
    constexpr int NO = GEGLU ? NR / 2 : NR;  // outputs per wave
    constexpr int UN = 16 / NR;
    const int K = a.K, N = a.N;
    for (int c = threadIdx.x; c < (K >> 3); c += 256) xs[c] = ((const u32x4*)a.x)[c];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const long n0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * NO;
    if (n0 >= N) return;
    const bf16_t* wrow[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        long n = n0 + (r % NO);
        n = n < N ? n : N - 1;
        if (GEGLU && r >= NO) n += N;
        wrow[r] = a.W + n * a.ldw;
    }
    float acc[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = 0.f;
    // whole chunks need no lane predicate: kb is uniform and every lane's k of the chunk is below K
    int kb = 0;
    for (; kb + 512 * UN <= K; kb += 512 * UN) gemv_bf16_chunk<NR, UN>(wrow, xs, kb + lane * 8, acc);
    if constexpr (UN > 4) {
        if (kb + 2048 <= K) {
            gemv_bf16_chunk<NR, 4>(wrow, xs, kb + lane * 8, acc);
            kb += 2048;
        }
    }
    if constexpr (UN > 2) {
        if (kb + 1024 <= K) {
            gemv_bf16_chunk<NR, 2>(wrow, xs, kb + lane * 8, acc);
            kb += 1024;
        }
    }
    if (kb + 512 <= K) {
        gemv_bf16_chunk<NR, 1>(wrow, xs, kb + lane * 8, acc);
        kb += 512;
    }
    if (kb + lane * 8 < K) gemv_bf16_chunk<NR, 1>(wrow, xs, kb + lane * 8, acc);  // the partly filled last trip
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = wave_reduce_sum(acc[r]);
    if (lane != 0) return;
#pragma unroll
    for (int o = 0; o < NO; ++o) {
        const long n = n0 + o;
        if (n >= N) break;
        if constexpr (GEGLU) {
            const float g = gemv_bf16_round(acc[o]), u = gemv_bf16_round(acc[NO + o]);
            a.out_bf16[n * a.out_stride] = f32_to_bf16(gemv_bf16_round(gelu_tanh(g)) * u);
        } else if (a.epilogue == GEMV_EPI_F32) {
            a.out_f32[n] = gemv_bf16_round(acc[o]);
        } else {
            a.out_bf16[n * a.out_stride] = f32_to_bf16(acc[o]);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// grouped small-M path on affine-quantised weights (gemm.h, GemvJobQ): gemv_group_kernel with the weights read as codes. A lane's 8
// weights of a trip (k = lane * 8 + 512 * trip) lie in ONE 64-wide group, so a trip costs the lane one 8-byte (8 bits) or 4-byte
// (4 bits) code load and one scale / bias pair. Each weight is rebuilt as bf16(q * scale + bias) - the value launch_dequant writes;
// q <= 255 times a bf16 scale is exact in f32, so contraction cannot move it - and goes through gemv_trip: the same fma chain in the
// same order, the same reduction and bias add, so every job is bit-equal to launch_gemv_f32 on the de-quantised matrix.
// Scale / bias of the 8 lanes that share a group, XL true (the default, option "gemvq_sb" = 1): lanes 0 .. 8 UN - 1 load the chunk's
// 8 UN consecutive groups once and every trip takes its pair with a cross-lane move; XL false: every lane loads its own pair per
// trip (8 lanes read one address). Measured on the dual model's timestep path: XL true is 7 - 11 % faster.
// ---------------------------------------------------------------------------------------------------------------
template <int BITS> struct GemvQRaw;
template <> struct GemvQRaw<8> { typedef uint2 type; };
template <> struct GemvQRaw<4> { typedef uint32_t type; };
LTX_DEVFN uint32_t gemvq_code(const uint2 raw, int e) { return ((e < 4 ? raw.x : raw.y) >> (8 * (e & 3))) & 0xffu; }
LTX_DEVFN uint32_t gemvq_code(const uint32_t raw, int e) { return (raw >> (4 * e)) & 0xfu; }  // even element in the low nibble

// UN whole trips starting at the lane's k: every code load is issued before the first fma; the fmas run in trip order
template <int MMAX, int BITS, int UN, bool XL>
LTX_DEVFN void gemvq_chunk(const float* __restrict__ a, long lda, const uint8_t* __restrict__ crow, const bf16_t* __restrict__ srow,
                           const bf16_t* __restrict__ brow, int k, int lane, int M, int in_act, float (&accv)[MMAX]) {
    typedef typename GemvQRaw<BITS>::type Raw;
    Raw raw[UN];
#pragma unroll
    for (int i = 0; i < UN; ++i) raw[i] = *(const Raw*)(crow + (long)(k + 512 * i) * BITS / 8);
    float sc[UN], bi[UN];
    if constexpr (XL) {
        // whole chunks only: the chunk's groups g0 .. g0 + 8 UN - 1 are all below K / 64 and every lane is active
        const int g0 = (k >> 6) - (lane >> 3);
        float sv = 0.f, bv = 0.f;
        if (lane < 8 * UN) {
            sv = bf16_to_f32(srow[g0 + lane]);
            bv = bf16_to_f32(brow[g0 + lane]);
        }
#pragma unroll
        for (int i = 0; i < UN; ++i) {
            sc[i] = __shfl(sv, (lane >> 3) + 8 * i, 64);
            bi[i] = __shfl(bv, (lane >> 3) + 8 * i, 64);
        }
    } else {
#pragma unroll
        for (int i = 0; i < UN; ++i) {
            sc[i] = bf16_to_f32(srow[(k + 512 * i) >> 6]);
            bi[i] = bf16_to_f32(brow[(k + 512 * i) >> 6]);
        }
    }
#pragma unroll
    for (int i = 0; i < UN; ++i) {
        s16x8 wv;
#pragma unroll
        for (int e = 0; e < 8; ++e) wv[e] = (short)f32_to_bf16((float)gemvq_code(raw[i], e) * sc[i] + bi[i]);
        gemv_trip<MMAX>(a, lda, wv, k + 512 * i, M, in_act, accv);
    }
}

template <int MMAX, int BITS, bool XL>
__global__ __launch_bounds__(256) void gemv_group_q_kernel(const GemvGroupQ g) {
    int j = 0;
    while (j < g.n_jobs - 1 && (int)blockIdx.x >= g.wg_end[j]) ++j;
    const GemvJobQ& job = g.job[j];
    const int wg0 = j ? g.wg_end[j - 1] : 0;
    const int lane = threadIdx.x & 63;
    const int n = ((int)blockIdx.x - wg0) * 4 + (threadIdx.x >> 6);
    const int M = g.M, N = job.N, K = job.K, in_act = job.in_act;
    if (n >= N) return;
    const float* __restrict__ a = job.a;
    const long lda = job.lda;
    float accv[MMAX];
#pragma unroll
    for (int m = 0; m < MMAX; ++m) accv[m] = 0.f;
    const uint8_t* crow = job.codes + (long)n * K * BITS / 8;
    const bf16_t* srow = job.scales + (long)n * (K >> 6);
    const bf16_t* brow = job.biases + (long)n * (K >> 6);
    int kb = 0;
    for (; kb + 4096 <= K; kb += 4096) gemvq_chunk<MMAX, BITS, 8, XL>(a, lda, crow, srow, brow, kb + lane * 8, lane, M, in_act, accv);
    if (kb + 2048 <= K) {
        gemvq_chunk<MMAX, BITS, 4, XL>(a, lda, crow, srow, brow, kb + lane * 8, lane, M, in_act, accv);
        kb += 2048;
    }
    if (kb + 1024 <= K) {
        gemvq_chunk<MMAX, BITS, 2, XL>(a, lda, crow, srow, brow, kb + lane * 8, lane, M, in_act, accv);
        kb += 1024;
    }
    if (kb + 512 <= K) {
        gemvq_chunk<MMAX, BITS, 1, XL>(a, lda, crow, srow, brow, kb + lane * 8, lane, M, in_act, accv);
        kb += 512;
    }
    // the partly filled last trip: K % 64 == 0, so an active lane's 8 codes and its group are inside the row; own loads (lanes diverge)
    if (kb + lane * 8 < K) gemvq_chunk<MMAX, BITS, 1, false>(a, lda, crow, srow, brow, kb + lane * 8, lane, M, in_act, accv);
    const float* bias = job.bias;
    float* out = job.out;
    const long ldo = job.ldo;
#pragma unroll
    for (int m = 0; m < MMAX; ++m) {
        const float s = wave_reduce_sum(accv[m]);
        if (lane == 0 && m < M) out[(long)m * ldo + n] = s + (bias ? bias[n] : 0.f);
    }
}

#ifdef LTX_EXPERIMENTS  // the kernels that were measured and not selected
#define LTX_GEMM_EXPERIMENTS_PART 1
#include "gemm_experiments.inc"
#endif

// split-K finish: out = epilogue(sum_z ws[z]) - every epilogue option except the depth-to-space stores; partials are summed in
// ascending z, so the result does not depend on scheduling.
// one 16-byte (f32) or 8-byte (bf16) group of a partial slice
LTX_DEVFN f32x4 ws_load4(const float* ws, long idx, int ws_bf16) {
    if (ws_bf16) {
        const uint2 u = *(const uint2*)((const bf16_t*)ws + idx);
        return f32x4{__builtin_bit_cast(float, u.x << 16), __builtin_bit_cast(float, u.x & 0xffff0000u),
                     __builtin_bit_cast(float, u.y << 16), __builtin_bit_cast(float, u.y & 0xffff0000u)};
    }
    return *(const f32x4*)(ws + idx);
}
__global__ __launch_bounds__(256) void splitk_finish_kernel(const float* __restrict__ ws, int S, int M, int N, GemmEpilogue ep, int ws_bf16 = 0) {
    const long n4 = N >> 2;
    const long total = (long)M * n4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long m = i / n4;
        const int c = (int)(i - m * n4) * 4;
        f32x4 v = ws_load4(ws, m * N + c, ws_bf16);
        for (int z = 1; z < S; ++z) v += ws_load4(ws, ((long)z * M + m) * N + c, ws_bf16);
        if (ep.bias_n) v += *(const f32x4*)(ep.bias_n + c);
        if (ep.bias_m) {
            const float bm = ep.bias_m[m];
            v += f32x4{bm, bm, bm, bm};
        }
        if (ep.act == LTX_ACT_SILU) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = silu_f(v[e]);
        } else if (ep.act == LTX_ACT_GELU_TANH) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = gelu_tanh(v[e]);
        }
        if (ep.round_bf16) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = bf16_to_f32(f32_to_bf16(v[e]));
        }
        if (ep.resid) {
            const float* rs = (ep.resid_src ? ep.resid_src + m * ep.ld_resid : ep.out_f32 + m * ep.ld_f32) + c;
            const f32x4 r4 = *(const f32x4*)rs;
            f32x4 gt = f32x4{ep.gate_scalar, ep.gate_scalar, ep.gate_scalar, ep.gate_scalar};
            if (ep.gate) gt = *(const f32x4*)(ep.gate + (long)(ep.gate_rowmap ? ep.gate_rowmap[m] : m / ep.rows_per_batch) * ep.gate_bstride + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = r4[e] + gt[e] * v[e];
        }
        if (ep.out_f32) *(f32x4*)(ep.out_f32 + m * ep.ld_f32 + c) = v;
        if (ep.out_bf16) {
            uint2 pk;
            pk.x = pack_bf16x2(v[0], v[1]);
            pk.y = pack_bf16x2(v[2], v[3]);
            *(uint2*)(ep.out_bf16 + m * ep.ld_bf16 + c) = pk;
        }
        if (ep.out_bf16_t) {  // transposed output (V^T of a few-row launch): 2-byte stores, a few hundred KB in all
#pragma unroll
            for (int e = 0; e < 4; ++e) ep.out_bf16_t[(long)(c + e) * ep.ld_bf16_t + m] = f32_to_bf16(v[e]);
        }
    }
}

// split-K finish of R whole rows of N = 4096 per workgroup + the RMS norm / adaLN modulation of the finished rows (NormAfter): the rows
// are in registers when their f32 values are stored, so the pass that would read them back next is applied here. The finish arithmetic is
// splitk_finish_kernel's and the norm arithmetic norm_mod_rows_kernel's (elementwise.hip), in the same order: the bf16 rows are
// bit-identical to the two launches (tests/test_kernels_gpu.py).
template <int R>
__global__ __launch_bounds__(256) void splitk_finish_norm_kernel(const float* __restrict__ ws, int S, int M, GemmEpilogue ep, NormAfter na, int ws_bf16) {
    constexpr int N = 4096, NV = 4;
    __shared__ float red[4][R];
    const int row0 = blockIdx.x * R;
    const long nb = row0 / na.rows_per_batch;  // the launcher guarantees that the R rows lie in one batch element
    const float* sc = na.scale + nb * na.mod_bstride;
    const float* sh = na.shift + nb * na.mod_bstride;
    f32x4 v[R][NV], s4[NV], h4[NV];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const long m = (row0 + r) < M ? (row0 + r) : M - 1;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = (threadIdx.x + j * 256) * 4;
            f32x4 t = ws_load4(ws, m * N + c, ws_bf16);
            for (int z = 1; z < S; ++z) t += ws_load4(ws, ((long)z * M + m) * N + c, ws_bf16);
            if (ep.bias_n) t += *(const f32x4*)(ep.bias_n + c);
            if (ep.resid) {
                const float* rs = (ep.resid_src ? ep.resid_src + m * ep.ld_resid : ep.out_f32 + m * ep.ld_f32) + c;
                const f32x4 r4 = *(const f32x4*)rs;
                f32x4 gt = f32x4{ep.gate_scalar, ep.gate_scalar, ep.gate_scalar, ep.gate_scalar};
                if (ep.gate) gt = *(const f32x4*)(ep.gate + (m / ep.rows_per_batch) * ep.gate_bstride + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) t[e] = r4[e] + gt[e] * t[e];
            }
            v[r][j] = t;
        }
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
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) red[w][r] = ss[r];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (row0 + r >= M) break;
        const long m = row0 + r;
        const float ms = (red[0][r] + red[1][r] + red[2][r] + red[3][r]) / (float)N;
        const float rstd = rsqrtf(ms + na.eps);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int c = (threadIdx.x + j * 256) * 4;
            if (ep.out_f32) *(f32x4*)(ep.out_f32 + m * ep.ld_f32 + c) = v[r][j];
            if (ep.out_bf16) {
                uint2 pk;
                pk.x = pack_bf16x2(v[r][j][0], v[r][j][1]);
                pk.y = pack_bf16x2(v[r][j][2], v[r][j][3]);
                *(uint2*)(ep.out_bf16 + m * ep.ld_bf16 + c) = pk;
            }
            f32x4 y;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                y[e] = v[r][j][e] * rstd;
                if (na.round_norm_bf16) y[e] = bf16_to_f32(f32_to_bf16(y[e]));
                y[e] = y[e] * (1.0f + s4[j][e]) + h4[j][e];
            }
            uint2 pk;
            pk.x = pack_bf16x2(y[0], y[1]);
            pk.y = pack_bf16x2(y[2], y[3]);
            *(uint2*)(na.out + m * na.ldo + c) = pk;
        }
    }
}
// what splitk_finish_norm_kernel covers of the two passes' options
static bool finish_takes_norm(const GemmArgs& a, const NormAfter& na) {
    const GemmEpilogue& e = a.ep;
    return a.N == 4096 && e.out_f32 && !e.out_bf16_t && !e.bias_m && e.act == LTX_ACT_NONE && !e.round_bf16 && !e.gate_rowmap && !e.d2s &&
           !e.pn_out && na.norm_kind == 0 && na.scale && na.shift && !na.row_map && na.out && na.ldo % 4 == 0 && e.ld_f32 % 4 == 0 &&
           na.rows_per_batch % 2 == 0 && (!e.gate || e.rows_per_batch % 2 == 0) && a.M % 2 == 0;
}
// the finish pass of a split-K launch over `rows` rows of the workspace (a row window passes its own rows and an epilogue that starts there)
void launch_splitk_finish(const GemmArgs& a, int rows, const GemmEpilogue& e, int ws_bf16, hipStream_t stream) {
    const long total = (long)rows * (a.N / 4);
    const int grid = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    hipLaunchKernelGGL(splitk_finish_kernel, dim3(grid), dim3(256), 0, stream, a.split_ws, a.split_k, rows, a.N, e, ws_bf16);
    HIP_CHECK(hipGetLastError());
}

// The options (options.h) the launchers below read, by value: every public entry takes ONE snapshot and hands it down, so the rules that
// route a launch and the launcher it is routed to see the same values whatever ltx_ctx_set_option does on another thread meanwhile.
struct GemmOpts {
    int conv_halo, conv_tall, conv_persist, conv_stagger, gemm_stagger, conv_cfg, conv_no_tail, smallm_cfg, b_nt, dtl_splitk, dtl_splitk_mink,
        split_f32, finish_norm, finish_rows, gemm_rowsplit, gemm_tall;
};
GemmOpts gemm_opts() {
    return {ltx_opt(OPT_CONV_HALO),  ltx_opt(OPT_CONV_TALL),    ltx_opt(OPT_CONV_PERSIST),  ltx_opt(OPT_CONV_STAGGER),
            ltx_opt(OPT_GEMM_STAGGER), ltx_opt(OPT_CONV_CFG),   ltx_opt(OPT_CONV_NO_TAIL),  ltx_opt(OPT_SMALLM_CFG),
            ltx_opt(OPT_B_NT),       ltx_opt(OPT_DTL_SPLITK),   ltx_opt(OPT_DTL_SPLITK_MINK), ltx_opt(OPT_SPLIT_F32),
            ltx_opt(OPT_FINISH_NORM), ltx_opt(OPT_FINISH_ROWS), ltx_opt(OPT_GEMM_ROWSPLIT), ltx_opt(OPT_GEMM_TALL)};
}

// Split count that fills the chip: 256 / tiles ranges of K, at most `cap` and at most one per eight K-tiles, shrunk until the partial
// slices (`slice` elements each) fit `ws_elems`. Each caller counts tiles of its own kernel and passes its own cap.
int fill_split_k(long tiles, int nk, int cap, long slice, long ws_elems) {
    long s = 256 / tiles;
    if (s > cap) s = cap;
    if (s > nk / 8) s = nk / 8;
    if (s < 1) s = 1;
    while (s > 1 && s * slice > ws_elems) --s;
    return (int)s;
}

template <int BM, int BN, bool CONV>
void launch_one(const GemmArgs& a, hipStream_t stream) {
    constexpr int smem = 2 * (BM + BN) * ROW_BYTES;
    static PerDeviceOnce attr_set;
    attr_set.run([&] {
        HIP_CHECK(hipFuncSetAttribute((const void*)gemm_bf16_kernel<BM, BN, CONV>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, smem));
    });
    const int tiles = ((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN);
    hipLaunchKernelGGL((gemm_bf16_kernel<BM, BN, CONV>), dim3(tiles), dim3(256), smem, stream, a);
    HIP_CHECK(hipGetLastError());
}

template <int BM, int BN, int NSTAGE, bool CONV, int WGM = 2, int WGN = 2, bool QB = false>
void launch_v2(const GemmArgs& a, const GemmOpts& o, hipStream_t stream) {
    constexpr int smem = NSTAGE * (BM + BN) * ROW_BYTES + (QB ? (NSTAGE + 1) * (BN * 64 + WGM * WGN * 256) : 0);
    static PerDeviceOnce attr_set;
    attr_set.run([&] {
        HIP_CHECK(hipFuncSetAttribute((const void*)gemm_bf16_kernel_v2<BM, BN, NSTAGE, CONV, WGM, WGN, QB>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, smem));
    });
    LTX_REQUIRE(QB == (a.Bq != nullptr), "gemm: quantised codes need the de-quantising instance of the ring kernel");
    const int all_tiles = ((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN);
    const int tiles = a.tile_count ? a.tile_count : all_tiles;
    LTX_REQUIRE(a.tile0 >= 0 && a.tile0 + tiles <= all_tiles, "gemm: tile window [%d, %d) outside %d tiles", a.tile0, a.tile0 + tiles, all_tiles);
    if (a.split_k > 1) {
        const GemmEpilogue& e = a.ep;
        LTX_REQUIRE(a.split_ws && a.N % 4 == 0 && !e.d2s, "gemm split-K: needs a workspace, N %% 4 == 0 and no depth-to-space epilogue");
        LTX_REQUIRE(a.split_k <= a.K / BK, "gemm split-K: %d splits for %d K-tiles", a.split_k, a.K / BK);
        LTX_REQUIRE(!a.win_rows || (!e.gate && !e.bias_m && !e.out_bf16_t && a.win_row0 + a.win_rows <= a.M),
                    "gemm split-K: a row window takes neither per-row gates / biases nor the transposed output");
    }
    GemmArgs ab = a;
    ab.conv_stagger = (CONV ? o.conv_stagger : o.gemm_stagger) != 0;
    hipLaunchKernelGGL((gemm_bf16_kernel_v2<BM, BN, NSTAGE, CONV, WGM, WGN, QB>), dim3(tiles, a.split_k > 1 ? a.split_k : 1),
                       dim3(WGM * WGN * 64), smem, stream, ab);
    HIP_CHECK(hipGetLastError());
    if (a.split_k > 1) {
        const int rows = a.win_rows ? a.win_rows : a.M;
        GemmEpilogue e = a.ep;  // the finish pass indexes rows from the window's first row
        if (a.win_rows) {
            if (e.out_f32) e.out_f32 += (long)a.win_row0 * e.ld_f32;
            if (e.out_bf16) e.out_bf16 += (long)a.win_row0 * e.ld_bf16;
            if (e.resid_src) e.resid_src += (long)a.win_row0 * e.ld_resid;
        }
        launch_splitk_finish(a, rows, e, 0, stream);
    }
}

void validate(const GemmArgs& a) {
    LTX_REQUIRE(a.M > 0 && a.N > 0 && a.K > 0, "gemm: empty problem M=%d N=%d K=%d", a.M, a.N, a.K);
    LTX_REQUIRE(a.K % BK == 0, "gemm: K=%d must be a multiple of %d", a.K, BK);
    LTX_REQUIRE(a.A && (a.B || (a.Bq && a.Bqs && a.Bqb)), "gemm: null operand");
    LTX_REQUIRE(((uintptr_t)a.A & 15) == 0 && ((uintptr_t)a.B & 15) == 0 && ((uintptr_t)a.Bq & 15) == 0, "gemm: operands must be 16-B aligned");
    LTX_REQUIRE(a.ldb % 8 == 0, "gemm: ldb=%ld must be a multiple of 8", a.ldb);
    if (a.conv) {
        LTX_REQUIRE(a.geom.kt == 1 || a.geom.kt == 3, "gemm/conv3d: kt=%d", a.geom.kt);
        LTX_REQUIRE(a.geom.C % BK == 0 && a.K == 9 * a.geom.kt * a.geom.C, "gemm/conv3d: C=%d K=%d kt=%d", a.geom.C, a.K, a.geom.kt);
        LTX_REQUIRE(a.M == a.geom.F * a.geom.H * a.geom.W, "gemm/conv3d: M=%d != F*H*W", a.M);
        LTX_REQUIRE(a.geom.pad_mode != 0 || (a.geom.H >= 2 && a.geom.W >= 2), "gemm/conv3d: reflect padding needs H,W >= 2");
    } else {
        LTX_REQUIRE(a.lda % 8 == 0, "gemm: lda=%ld must be a multiple of 8", a.lda);
    }
    const GemmEpilogue& e = a.ep;
    LTX_REQUIRE(e.out_f32 || e.out_bf16 || e.out_bf16_t || e.pn_out, "gemm: no output");
    if (e.pn_out) LTX_REQUIRE(e.ld_pn % 4 == 0 && ((uintptr_t)e.pn_out & 7) == 0, "gemm: PixelNorm output alignment");
    if (e.out_f32) LTX_REQUIRE((e.ld_f32 % 4 == 0 || e.d2s == 3) && ((uintptr_t)e.out_f32 & 15) == 0, "gemm: f32 output alignment");
    if (e.out_bf16) LTX_REQUIRE(e.ld_bf16 % 4 == 0 && ((uintptr_t)e.out_bf16 & 7) == 0, "gemm: bf16 output alignment");
    if (e.d2s == 3) LTX_REQUIRE(a.conv && a.N == 48 && e.out_f32 && e.ld_f32 == 1 && !e.out_bf16 && !e.resid && a.split_k <= 1, "gemm: the un-patchify store is for the 48-channel conv_out with one f32 output");
    if (e.resid && !e.d2s) LTX_REQUIRE(e.out_f32 || e.resid_src, "gemm: residual mode needs an f32 stream");
    if (!e.d2s) {  // the interior-column epilogue reads these with 16-B accesses
        LTX_REQUIRE(((uintptr_t)e.bias_n & 15) == 0, "gemm: bias must be 16-B aligned");
        LTX_REQUIRE(((uintptr_t)e.gate & 15) == 0 && e.gate_bstride % 4 == 0, "gemm: gate must be 16-B aligned (stride %ld)", (long)e.gate_bstride);
        LTX_REQUIRE(((uintptr_t)e.resid_src & 15) == 0 && (!e.resid_src || e.ld_resid % 4 == 0), "gemm: residual source alignment");
    }
    if (e.d2s && e.d2s != 3) LTX_REQUIRE(a.conv && a.N % 32 == 0, "gemm: d2s epilogue needs conv mode and N%%32==0");
    if (e.d2s == 1 && e.resid_src) LTX_REQUIRE(a.geom.C % 32 == 0, "gemm: the depth-to-space residual needs C %% 32 == 0 (C=%d)", a.geom.C);
}

}  // namespace


// the 192 x 256, 192 x 384 (q|k|v) and 384 x 256 kernels with a generated main loop, their predicates and launchers
#include "gemm_asm_tiles.inc"

// conv_halo.inc: which conv launches the halo-staged kernel takes (everything else stays on the ring kernel)
static bool conv_halo_takes(const GemmArgs& a, const GemmOpts& o) {
    const bool off = o.conv_halo == 0;  // A/B option "conv_halo"
    const Conv3dGeom& q = a.geom;
    // (win_rows on a launch without split-K is work accounting only: the head launch of a window pair)
    if (off || !a.conv || q.kt != 3 || !(q.pad_mode == 0 || q.pad_mode == 2) || q.C % 64 != 0 || a.split_k > 1 || a.tile0 != 0) return false;
    if (a.K != 27 * q.C || a.M != q.F * q.H * q.W || a.M < 192 || a.ldb % 8 != 0) return false;
    if ((long)a.M * q.C >= (1L << 31) || (long)a.N * a.ldb >= (1L << 31)) return false;  // the kernel addresses both operands with 32-bit element offsets
    if ((long)a.M * q.W >= (1L << 32) || (long)q.F * q.H * q.H >= (1L << 32) || q.H < 2 || q.W < 2) return false;  // ... and divides by W and H with multiply-high forms
    const bool w_ok = (q.W <= 192 && q.W >= 48 && 192 % q.W == 0) || (q.W % 192 == 0);
    return w_ok && !a.ep.out_bf16_t && !a.ep.gate;  // (its epilogue is the scalar-gate form)
}
template <int BN>
static void launch_conv_halo(const GemmArgs& a, const GemmOpts& o, hipStream_t stream);
// conv_halo2.inc: the 384 x 128 tile of NRT image rows -> 0 = not this launch, else NRT (1: W == 384, 2: W == 192, 4: W == 96)
static int conv_halo2_takes(const GemmArgs& a, const GemmOpts& o) {
    if (o.conv_tall == 0 || !conv_halo_takes(a, o)) return 0;
    const Conv3dGeom& q = a.geom;
    const int nrt = (q.W == 384 && o.conv_tall != 2) ? 1 : (q.W == 192 ? 2 : (q.W == 96 ? 4 : 0));  // (2: A/B without the W == 384 instance)
    if (!nrt || q.H % nrt != 0 || a.N % 128 != 0 || a.M % 384 != 0 || a.tile_count != 0 || a.tile0 != 0 || a.ldb % 8 != 0) return 0;
    if (nrt == 4 && q.C % 128 != 0) return 0;                       // (the row-slot rotation must come back to slot 0 or 4 at a tile boundary)
    if (a.ep.d2s != 0 && a.ep.d2s != 1) return 0;                   // plain / fused-PixelNorm / depth-to-space epilogues (conv_out's d2s == 3 has N = 48)
    if (a.ep.pn_out && !(a.N == 128 || (a.ep.d2s == 1 && a.N == 8 * 128))) return 0;
    if ((long)q.F * q.H * q.W * q.C >= (1L << 31) || (long)a.N * a.ldb >= (1L << 31)) return 0;  // 32-bit element offsets
    // A tall tile is two 192-row tiles on ONE CU: a launch whose tall tiles cover at most half the chip finishes sooner as 192-row tiles
    // on twice the CUs (small clips; the stages of a 256 x 256 decode). Option value 3 takes the tall kernel regardless (tests of small shapes).
    if (o.conv_tall != 3 && 2L * (a.M / 384) * (a.N / 128) <= device_cu_count()) return 0;
    return nrt;
}
template <int NRT>
static void launch_conv_halo2_nrt(const GemmArgs& a, const GemmOpts& o, hipStream_t stream) {
    constexpr int RSP = (384 / NRT + 2 + 7) / 8, NS = NRT == 1 ? 2 : (NRT == 2 ? 4 : 8);
    constexpr int smem = NS * RSP * 1024 + 1024 + 3 * 128 * ROW_BYTES;
    static PerDeviceOnce attr_set;
    attr_set.run([&] { HIP_CHECK(hipFuncSetAttribute((const void*)conv3d_halo2_kernel<NRT>, hipFuncAttributeMaxDynamicSharedMemorySize, smem)); });
    const int tiles_n = a.N / 128, rows_t = a.M / 384, tall = rows_t * tiles_n;
    const int ncu = device_cu_count() & ~7;
    // Whole rounds of tall tiles, one workgroup per CU walking its XCD's chunk; what is left over (768 x 512, 128 channels: 1600 = 6 x 256
    // + 64 tall tiles) would keep a quarter of the chip busy for a seventh round, so it runs as 192-row tiles of conv_halo.inc behind the
    // main launch (128 tiles = half a round of tiles half the size). The window starts at a whole number of that kernel's supertiles
    // (group_m row tiles x all column tiles) and of this kernel's row tiles.
    int main_tiles = tall;
    if (ncu >= 8 && tall > ncu && tall % ncu != 0 && tall % ncu <= ncu / 2) {
        const int m = tall / ncu * ncu;
        const int gm = a.group_m > 0 ? a.group_m : 1;
        if (m % tiles_n == 0 && (2 * (m / tiles_n)) % gm == 0) main_tiles = m;
    }
    GemmArgs b = a;
    b.tile_count = main_tiles == tall ? 0 : main_tiles;
    const int grid = (main_tiles > ncu && ncu >= 8) ? ncu : main_tiles;
    hipLaunchKernelGGL(conv3d_halo2_kernel<NRT>, dim3(grid), dim3(512), smem, stream, b);
    HIP_CHECK(hipGetLastError());
    if (main_tiles < tall) {
        GemmArgs t = a;
        t.tile0 = 2 * (main_tiles / tiles_n) * tiles_n;  // 192-row tiles in front of the window (conv_halo.inc's order: supertiles of group_m row tiles)
        t.tile_count = 2 * rows_t * tiles_n - t.tile0;
        launch_conv_halo<128>(t, o, stream);
    }
}
// nrt = what conv_halo2_takes said of this launch
static void launch_conv_halo2(const GemmArgs& a, int nrt, const GemmOpts& o, hipStream_t stream) {
    if (nrt == 1) launch_conv_halo2_nrt<1>(a, o, stream);
    else if (nrt == 2) launch_conv_halo2_nrt<2>(a, o, stream);
    else {
        LTX_REQUIRE(nrt == 4, "conv halo2: the launch is not one the tall kernel takes (W=%d H=%d N=%d M=%d)", a.geom.W, a.geom.H, a.N, a.M);
        launch_conv_halo2_nrt<4>(a, o, stream);
    }
}
// Both halo-staged kernels carry the depth-to-space + PixelNorm epilogue, and conv_halo2_takes is a subset of conv_halo_takes (it starts
// with it), so the wider rule decides; it reads no device property and can be asked without one.
static bool conv_takes_d2s_pn(const GemmArgs& a, const GemmOpts& o) { return a.ep.d2s == 1 && a.N == 8 * 128 && a.split_k <= 1 && conv_halo_takes(a, o); }
bool gemm_conv_takes_d2s_pn(const GemmArgs& a) { return conv_takes_d2s_pn(a, gemm_opts()); }
template <int BN>
static void launch_conv_halo(const GemmArgs& a, const GemmOpts& o, hipStream_t stream) {
    constexpr int smem = 2 * 32 * 1024 + 6 * BN * ROW_BYTES;
    static PerDeviceOnce attr_set;
    attr_set.run([&] { HIP_CHECK(hipFuncSetAttribute((const void*)conv3d_halo_kernel<BN>, hipFuncAttributeMaxDynamicSharedMemorySize, smem)); });
    const int all_tiles = ((a.M + 191) / 192) * ((a.N + BN - 1) / BN);
    const int tiles = a.tile_count ? a.tile_count : all_tiles;
    // (a window with tile0 > 0 - the tail behind the tall kernel's whole rounds - starts at a whole number of supertiles: launch_conv_halo2_nrt)
    LTX_REQUIRE(a.tile0 >= 0 && a.tile0 + tiles <= all_tiles, "conv halo: tile window [%d, %d) outside %d", a.tile0, a.tile0 + tiles, all_tiles);
    // persistent above one round: one workgroup per CU walks the tiles of its XCD's chunk and requests the next tile's first operands
    // before the epilogue of the current one (conv_halo.inc); option "conv_persist" = 0 restores one workgroup per tile (A/B)
    const bool persist = o.conv_persist != 0;
    const int ncu = device_cu_count() & ~7;
    const int grid = (persist && tiles > ncu && ncu >= 8) ? ncu : tiles;
    GemmArgs b = a;
    b.conv_stagger = o.conv_stagger != 0;
    hipLaunchKernelGGL(conv3d_halo_kernel<BN>, dim3(grid), dim3(512), smem, stream, b);
    HIP_CHECK(hipGetLastError());
}

// One launch on tile cfg `cfg`. nrt = conv_halo2_takes of a conv launch (read by cfg 21 only; 0 for a dense one).
static void launch_cfg(const GemmArgs& a, int cfg, const GemmOpts& o, int nrt, hipStream_t stream);

// The launchers of the experiments build and its hooks into the flow below: gemm_experiments_cfg runs a tile cfg that only that build knows,
// gemm_experiments_forced a dense launch whose cfg its environment forces (true = launched); gemm_experiments_group_m overrides group_m.
#ifdef LTX_EXPERIMENTS
#define LTX_GEMM_EXPERIMENTS_PART 2
#include "gemm_experiments.inc"
#else
static bool gemm_experiments_cfg(const GemmArgs&, int, const GemmOpts&, hipStream_t) { return false; }
static bool gemm_experiments_forced(const GemmArgs&, const GemmOpts&, hipStream_t) { return false; }
static void gemm_experiments_group_m(GemmArgs&) {}
#endif

static void launch_cfg(const GemmArgs& a, int cfg, const GemmOpts& o, int nrt, hipStream_t stream) {
    if (a.ep.out_bf16_t) {
        const GemmEpilogue& e = a.ep;
        LTX_REQUIRE(!e.out_f32 && !e.out_bf16 && !e.resid && !e.d2s && !e.bias_m && e.act == LTX_ACT_NONE && !e.round_bf16 &&
                        (cfg == 90 || cfg == 29 || cfg == 30 || (a.split_k <= 1 && !a.split_ws)) && e.ld_bf16_t % 4 == 0 && e.ld_bf16_t >= a.M && (cfg < 41 || cfg == 90),
                    "gemm: the transposed bf16 output takes bias_n only, no split-K, ld %% 4 == 0 (ld=%ld M=%d cfg=%d)", e.ld_bf16_t, a.M, cfg);
    }
    validate(a);
    LTX_REQUIRE(a.split_k <= 1 || (cfg >= 20 && cfg < 32) || cfg == 90 || cfg == 75, "gemm: split-K needs a ring kernel, the 192x256 kernel or the weight-streaming kernel (tile cfg %d)", cfg);
    LTX_REQUIRE(!a.Bq || cfg == 90 || cfg == 29 || cfg == 30, "gemm: quantised codes are read by the few-row ring kernel only (tile cfg %d)", cfg);
    ProfScope prof(a.conv ? PROF_CONV : PROF_GEMM, 2.0 * (a.win_rows ? a.win_rows : a.M) * a.N * a.K, stream);  // a tile window's rows
    // cfg 0..2: v1 (2-stage, one barrier + full drain per K-tile); cfg 10..: v2 (ring + counted vmcnt)
    if (a.conv) {
        switch (cfg) {
            case 21:  // 8 waves (4x2), per-wave 48x64: the halo-staged kernel where it applies (its tall form where THAT applies), else the 4-slot ring
                if (nrt) launch_conv_halo2(a, nrt, o, stream);
                else if (conv_halo_takes(a, o)) launch_conv_halo<128>(a, o, stream);
                else launch_v2<192, 128, 4, true, 4, 2>(a, o, stream);
                break;
            case 27:  // narrow outputs (the VAE's 128 -> 48 conv_out): the halo-staged kernel's 192x64 instance, else the 256x64 ring (per-wave 64x32)
                if (a.N <= 64 && conv_halo_takes(a, o)) launch_conv_halo<64>(a, o, stream); else launch_v2<256, 64, 4, true, 4, 2>(a, o, stream);
                break;
            default:
                if (!gemm_experiments_cfg(a, cfg, o, stream)) LTX_THROW(LTXS_INVALID_CONFIGURATION, "gemm: unknown tile cfg %d", cfg);
        }
    } else {
        switch (cfg) {
            case 0: launch_one<128, 128, false>(a, stream); break;
            case 1: launch_one<192, 128, false>(a, stream); break;
            case 3: launch_one<96, 128, false>(a, stream); break;
            case 4: launch_one<128, 96, false>(a, stream); break;
            case 21: launch_v2<192, 128, 4, false, 4, 2>(a, o, stream); break;  // 8 waves (4x2), per-wave 48x64, 4-slot ring
            case 22: { GemmArgs b = a; b.group_m = 0; launch_v2<192, 128, 4, false, 4, 2>(b, o, stream); break; }  // A/B: column-major order
            case 23: launch_v2<256, 128, 3, false, 4, 2>(a, o, stream); break;  // 8 waves, per-wave 64x64
            case 25: launch_v2<128, 192, 4, false, 2, 4>(a, o, stream); break;
            case 29:  // few rows: narrow column tiles, 4 waves, one workgroup per CU; 8-bit codes de-quantised in the B stage.
                      // bf16 weights: SIX ring slots (144 KB) - five K-tiles of weights in flight per CU instead of three: the
                      // weight stream of a 128-token launch goes from 3.45 to 3.65 TB/s (same-box A/B, tools/fewrow_stride.py)
                if (a.Bq) {
                    launch_v2<128, 64, 4, false, 2, 2, true>(a, o, stream);
                } else {
                    const int nt_env = o.b_nt;  // A/B option "b_nt": 0 / 1 overrides the launcher
                    if (nt_env >= 0 && a.b_nt != nt_env) {
                        GemmArgs b = a;
                        b.b_nt = nt_env;
                        launch_v2<128, 64, 6, false, 2, 2>(b, o, stream);
                    } else {
                        launch_v2<128, 64, 6, false, 2, 2>(a, o, stream);
                    }
                }
                break;
            case 75: launch_dtl(a, o, stream); break;  // 192x256, one wave per SIMD, fragments of a whole K-tile in registers, 2 + 3 LDS slots
            case 76: launch_tall(a, stream); break;  // 384x256, one wave per SIMD, B fragments of a K-tile in registers, A through a ring, 2 + 2 LDS slots
            default:
                if (!gemm_experiments_cfg(a, cfg, o, stream)) LTX_THROW(LTXS_INVALID_CONFIGURATION, "gemm: unknown tile cfg %d", cfg);
        }
    }
}
void launch_gemm_bf16_cfg(const GemmArgs& a, int cfg, hipStream_t stream) {
    const GemmOpts o = gemm_opts();
    launch_cfg(a, cfg, o, (a.conv && cfg == 21) ? conv_halo2_takes(a, o) : 0, stream);
}

bool gemm_takes_codes(int M, int N, int K) { return M >= 1 && M <= 256 && K % BK == 0 && K >= 4 * BK && N % 4 == 0; }
// the few-row kernel (tile_cfg 30): one 128-row tile, whole 64-column tiles, K of every split a whole number of 256-wide macro-tiles
bool gemm_fewrow_takes(int M, int N, int K, int splits) {
    if (splits < 1) splits = 1;
    return M >= 1 && M <= 128 && N % 64 == 0 && K % 256 == 0 && (K / 256) % splits == 0;
}

int gemm_suggest_split_k(int M, int N, int K) {
    const long tiles = (long)((M + 191) / 192) * ((N + 127) / 128);  // the 192x128 ring kernel's tiles
    const int nk = K / BK;
    if (tiles >= 160 || nk < 32) return 1;
    return fill_split_k(tiles, nk, 8, 0, 0);
}

// At most one round of 192x128 ring tiles with a long reduction (the FFN's second GEMM at 1536 tokens: 256 tiles, K = 16384) runs as K
// ranges of the 192x256 kernel, whose main loop reads half the fragments per MFMA, plus the finish pass: 36.46 -> 35.75 ms per headline
// step on one box. -> number of ranges, 0 = not this launch. Option "dtl_splitk" = 0 turns it off; "dtl_splitk_mink" = least K per range
// (8192; with 2048 the three K = 4096 launches of a block split too and the step LOSES 1.3 ms).
// Partial tiles of such a launch cross the workspace as bf16 ONLY when the caller asked for it (GemmArgs::split_bf16 - the DiT sets it for
// its FFN-down Linear, nothing else does: a generic or ABI launch keeps f32 partials, round-4 advice) and option "split_f32" is 0.
static int dtl_split_bf16(const GemmArgs& a, const GemmOpts& o) { return a.split_bf16 && o.split_f32 == 0; }
static int dtl_split_for(const GemmArgs& a, const GemmOpts& o) {
    const bool dtl_split = o.dtl_splitk != 0;
    const int dtl_mink = o.dtl_splitk_mink;
    if (!dtl_split || dtl_mink < 64 || a.conv || a.Bq || !a.split_ws || a.split_k != 0 || a.M % 192 != 0 || a.N % 256 != 0 || a.ep.d2s) return 0;
    if (gemm_suggest_split_k(a.M, a.N, a.K) > 1) return 0;  // fewer than 160 ring tiles: the ring kernel's own split-K
    const long t1 = (long)(a.M / 192) * (a.N / 256);
    const int ncu = device_cu_count();
    long s = ncu / t1;
    if (s > a.K / dtl_mink) s = a.K / dtl_mink;
    while (s > 1 && s * a.M * a.N > a.split_ws_elems) --s;
    if (s < 2 || s * t1 <= ncu / 2) return 0;
    GemmArgs b = a;
    b.split_k = (int)s;
    return gemm_dtl_takes(b) ? (int)s : 0;
}

// The tile choice of a dense launch without split-K as a pure function of the launch and the CU count: no device is touched
// (ltx_gemm_dense_tile_cfg pins the table in a CPU test). launch_dense may still split a ragged 192x256 launch by rows.
static int dense_cfg(const GemmArgs& a, int ncu, const GemmOpts& o) {
    struct Cand { int cfg, bm, bn, slots; double f; };
    //   cfg 75: 192x256 tile, one wave per SIMD, assembly main loop (tools/gen_gemm_asm_dtl.py): half the rounds of a 192x128 tile.
    //   Same measurement, round 2 (profiles/r02_gemm_microbench.txt): N=8192: cfg75 1165 | library GEMM 1116 | cfg1 936 | cfg21 959;
    //   N=16384: 1274 | 1294 | 1054 | 1009; 6144x4096x4096: 1290 | 1325 | 1093 | 1033; 1536x4096x4096 (128 tiles): 740 -> not chosen.
    static const Cand cands[] = {{75, 192, 256, 256, 1.22}, {1, 192, 128, 512, 1.00}, {21, 192, 128, 256, 0.95}, {25, 128, 192, 256, 0.90},
                                 {0, 128, 128, 512, 0.80},  {3, 96, 128, 512, 0.72},  {4, 128, 96, 512, 0.72}};
    int best = 0;
    double be = -1;
    for (const Cand& c : cands) {
        if (c.cfg == 75 && !gemm_dtl_takes(a)) continue;
        const long tiles = (long)((a.M + c.bm - 1) / c.bm) * ((a.N + c.bn - 1) / c.bn);
        const long rounds = (tiles + c.slots - 1) / c.slots;
        const double fill = ((double)a.M * a.N) / ((double)tiles * c.bm * c.bn);  // ragged edges waste MFMA work
        const double e = (double)tiles / (double)(rounds * c.slots) * c.f * fill;
        if (e > be + 1e-9) { be = e; best = c.cfg; }
    }
    // cfg 76: where the 192x256 kernel would run an even number of rounds, tiles twice as tall run half as many, each staging 29 % fewer
    // bytes per MFMA (the FFN-up projection, N = 16384). Option "gemm_tall" = 0 = off (A/B); bit-neutral.
    if (best == 75 && o.gemm_tall != 0 && gemm_tall_takes(a, ncu)) best = 76;
    return best;
}
int gemm_dense_cfg(const GemmArgs& a, int ncu) { return dense_cfg(a, ncu, gemm_opts()); }

// ---- launch_gemm_bf16: a conv, a dense launch whose split count is left to the launcher, or a plain dense launch ----
// Tile choice = workgroup-count quantisation x structure efficiency. Two structures:
//   v1 (cfg 0,1,3,4): 4 waves, 2 LDS stages, TWO workgroups resident per CU (512 slots) - two waves per SIMD from
//       co-residency; best when a launch has >= 512 tiles. Its single-tile prefetch exposes HBM latency on
//       weights that are streamed once (the DiT case), hence the lower factor for the small tiles.
//   v2 (cfg 21,23,25): 8 waves (two per SIMD inside ONE workgroup per CU, 256 slots), 3/4-slot LDS ring filled
//       2-3 K-tiles ahead with counted vmcnt - HBM-cold weights cost nothing; best at exactly k*256 tiles.
// Measured on MI355X, HBM-cold B operand, random data (tools/bench_gemm.py --cold), TFLOP/s:
//   M=1536 N=4096 K=4096 : cfg21 944 | cfg0 754 | cfg1 608      N=8192: cfg1 1026 | cfg21 949
//   N=16384: cfg1 1049 | cfg21 991         K=16384: cfg21 1094 | cfg0 864       M=4096 N=1536: cfg25 876 | cfg0 629
// (the candidates and their factors: dense_cfg)

// implicit-GEMM convs: the per-tap gather arithmetic must hide under MFMAs (8-wave ring kernels interleave it;
// the two-stage 4-wave kernel serialises it and ran the 256-channel VAE stage at 150 TFLOP/s). M is huge, so
// tile-count quantisation does not matter; N <= 128 wants the 192x128 tile, wide N the same (B re-use).
static void launch_conv(const GemmArgs& a, const GemmOpts& o, hipStream_t stream) {
    const int cc_opt = o.conv_cfg;  // A/B option "conv_cfg" for tile experiments (21 = 192x128 ring; 23 = 256x128 ring in the experiments build)
    const bool cc = cc_opt != 0;
    // N <= 64 (the decoder's conv_out, 128 -> 48 channels): a 192x128 tile spends 62 % of its MFMAs on padding columns
    const int conv_default = (a.N <= 64 && a.split_k <= 1) ? 27 : 21;
    const int nrt = conv_halo2_takes(a, o);  // the tall kernel's say on THIS launch, asked once (the head / tail launches below are not its)
    if (a.ep.pn_out) {
        // the fused PixelNorm output needs every channel of a row in ONE 128-column tile and the epilogue in the GEMM launch
        // (round 5: or, with the depth-to-space store of an upsampler, N == 8 x 128: a tile is one sub-position's 128 channels; only the
        // halo-staged kernels carry that epilogue)
        LTX_REQUIRE(((a.N == 128 && !a.ep.d2s) || conv_takes_d2s_pn(a, o)) && a.split_k <= 1 &&
                        (a.ep.pn_scale == nullptr) == (a.ep.pn_shift == nullptr),
                    "gemm: fused PixelNorm output needs N == 128 (got %d; 1024 with a depth-to-space store on a halo-staged launch) and no split-K", a.N);
        // (A last partial round - the 128-channel stage at 768x512 is 3200 tiles = 12.5 rounds - is NOT worth a launch of its own here:
        // running the 128 remaining tiles as 256 half-height tiles behind the whole rounds measured +0.28 ms per decode, round 3.
        // Tiles are dispatched as CUs free up, so the ragged end costs half a tile, less than a launch boundary.)
        launch_cfg(a, 21, o, nrt, stream);
        return;
    }
    if (!cc && conv_default == 21 && nrt) {  // the tall kernel balances its own last round (launch_conv_halo2_nrt)
        launch_cfg(a, 21, o, nrt, stream);
        return;
    }
    // Last partial round: T tiles = q full rounds of 256 + r. With r <= 128 the r tiles of the last round would run K-long on
    // r CUs while the others idle (the VAE's 256-channel stage: 832 tiles = 3.25 rounds, 19 % of every conv). Run the full
    // rounds as one launch and the remainder as a split-K launch over all CUs (window fields of GemmArgs).
    const bool no_tail = o.conv_no_tail != 0;  // A/B option "conv_no_tail"
    if (!no_tail && !cc && conv_default == 21 && a.split_k <= 1 && a.split_ws && !a.ep.d2s && a.N % 4 == 0 && !a.ep.gate && !a.ep.bias_m &&
        !a.ep.out_bf16_t && a.group_m > 0) {
        const int tiles_m = (a.M + 191) / 192, tiles_n = (a.N + 127) / 128, tiles = tiles_m * tiles_n;
        const int full = tiles / 256 * 256, tail = tiles - full, per = a.group_m * tiles_n, nk = a.K / BK;
        if (full >= 512 && tail > 0 && tail <= 128 && full % per == 0) {
            const int row0 = full / per * a.group_m * 192;  // whole supertiles before the window: it covers complete rows
            const int sk = fill_split_k(tail, nk, 8, (long)(a.M - row0) * a.N, a.split_ws_elems);
            if (sk > 1) {
                GemmArgs head = a, rest = a;
                head.tile_count = full;
                head.win_rows = row0;  // rows [0, row0): only the work accounting reads it on a launch without split-K
                head.split_ws = nullptr;
                rest.tile0 = full;
                rest.tile_count = tail;
                rest.split_k = sk;
                rest.win_row0 = row0;
                rest.win_rows = a.M - row0;
                launch_cfg(head, 21, o, 0, stream);
                launch_cfg(rest, 21, o, 0, stream);
                return;
            }
        }
    }
    launch_cfg(a, (cc && a.split_k <= 1) ? cc_opt : conv_default, o, nrt, stream);
}

static void launch_dense(const GemmArgs& a, const GemmOpts& o, hipStream_t stream);

// caller-provided workspace, split count left to the launcher: few output tiles and a long reduction (the DiT at
// small token counts, e.g. 256x256x9 -> 128 tokens: 32 tiles of weights to stream with 256 CUs) -> split K over the idle CUs
static void launch_dense_ws(const GemmArgs& a, const GemmOpts& o, hipStream_t stream) {
    GemmArgs b = a;
    b.split_k = gemm_suggest_split_k(a.M, a.N, a.K);
    // few rows (<= 128, e.g. 256x256x9): narrow 128x64 ring tiles - 64 column tiles at N = 4096, so 4 splits fill the chip and
    // the partial slices are a quarter of the weights (128x192 tiles needed 16 splits: as many partial bytes as weight bytes),
    // and the FFN's first GEMM (256 column tiles) needs no split at all. Config 1: 12.04 ms per forward against 12.25 (cfg 25).
    const int smallm_cfg = o.smallm_cfg;  // 30 (experiments build): the few-row kernel, 9 % slower
    // codes in the B stage exist only in the 128x64 ring (29) and the experiments build's few-row kernel (30): the hook cannot move a
    // quantised launch anywhere else
    const int smallm_q = (smallm_cfg == 29 || smallm_cfg == 30) ? smallm_cfg : 29;
    int cfg = a.Bq ? (a.M <= 128 ? smallm_q : 29) : ((a.M <= 128 && b.split_k > 1) ? smallm_cfg : 21);
    if (cfg == 29 || cfg == 30 || cfg == 25) {  // one row tile: column tiles of 64 (29, 30) or 192 (25) x up to 16 splits fill the chip
        const int bn = cfg == 25 ? 192 : 64;
        b.split_k = fill_split_k((a.N + bn - 1) / bn, a.K / BK, 16, (long)a.M * a.N, a.split_ws_elems);
    }
    if (cfg == 29 || cfg == 30) {
        if (cfg == 30 && !gemm_fewrow_takes(a.M, a.N, a.K, b.split_k)) cfg = 29;
        // once-read weights, non-temporal - from 64 MB up: the q|k, FFN-up and FFN-down launches gain 3-6 %, the 33.5 MB ones
        // (N = K = 4096, four splits) LOSE 12 % with it (profiles/r03_fewrow_bounds.txt)
        b.b_nt = (long)a.N * a.K >= (32L << 20) ? 1 : 0;
    }
    while (b.split_k > 1 && (long)b.split_k * a.M * a.N > a.split_ws_elems) --b.split_k;  // (the ring kernel's own count)
    LTX_REQUIRE(!a.Bq || (a.N % 4 == 0 && !a.ep.d2s), "gemm: quantised few-row launch with N %% 4 != 0");
    if ((b.split_k > 1 || cfg == 29 || cfg == 30) && a.N % 4 == 0 && !a.ep.d2s) {
        if (b.split_k <= 1) {
            b.split_k = 1;  // enough column tiles to fill the chip without a split (the FFN's first GEMM)
            b.split_ws = nullptr;
        }
        launch_cfg(b, cfg, o, 0, stream);
        return;
    }
    if (const int s2 = dtl_split_for(a, o)) {
        b.split_k = s2;
        b.split_bf16 = dtl_split_bf16(a, o);
        launch_cfg(b, 75, o, 0, stream);
        return;
    }
    b.split_k = 1;
    b.split_ws = nullptr;
    launch_dense(b, o, stream);
}

static void launch_dense(const GemmArgs& a, const GemmOpts& o, hipStream_t stream) {
    if (gemm_experiments_forced(a, o, stream)) return;
    const int ncu = device_cu_count();
    const int best = dense_cfg(a, ncu, o);
    // Ragged last round of the 192x256 kernel (round 4). With T = 9984 tokens the N = 4096 launches are 52 x 16 = 832 tiles = 3.25 rounds:
    // the fourth round runs 64 workgroups, K-long, on a quarter of the chip (19 % of the launch). Rows are independent, so such a launch is
    // split by rows into a head whose tiles are a whole number of rounds (48 row tiles = 768 tiles) and a tail (4 row tiles = 768 rows)
    // that goes through this function again - as 128 tiles of 192x128 on the ring kernel it takes half the time of the K-long quarter
    // round. Same kernels per output element as an unsplit launch of each part: bit-identical to those; option "gemm_rowsplit" = 0 = off (A/B).
    const bool rowsplit_on = o.gemm_rowsplit != 0;
    if (best == 75 && rowsplit_on && !a.ep.out_bf16_t && !a.ep.bias_m && a.split_k <= 1) {
        const int tm = a.M / 192, tn = a.N / 256;
        const long tiles = (long)tm * tn;
        const long rem = tiles % ncu;
        // the gate vector of a residual launch is indexed by m / rows_per_batch (or a row map): a row offset keeps that meaning only inside
        // one batch element
        const bool gate_ok = !a.ep.gate || a.ep.gate_rowmap || a.ep.rows_per_batch >= a.M;
        if (tiles > ncu && rem > 0 && rem <= ncu / 2 && gate_ok) {
            int g = tn, h = ncu;
            while (h) { const int t = g % h; g = h; h = t; }  // gcd(tn, ncu)
            const int step = ncu / g;                          // row tiles per whole number of rounds
            const int tm_head = (tm / step) * step;
            if (tm_head > 0 && tm_head < tm) {
                auto rows = [&](int row0, int nrows) {
                    GemmArgs s = a;
                    GemmEpilogue& e = s.ep;
                    s.A = a.A + (long)row0 * a.lda;
                    s.M = nrows;
                    if (e.out_f32) e.out_f32 += (long)row0 * e.ld_f32;
                    if (e.out_bf16) e.out_bf16 += (long)row0 * e.ld_bf16;
                    if (e.resid_src) e.resid_src += (long)row0 * e.ld_resid;
                    if (e.gate_rowmap) e.gate_rowmap += row0;
                    return s;
                };
                launch_cfg(rows(0, tm_head * 192), 75, o, 0, stream);
                launch_dense(rows(tm_head * 192, a.M - tm_head * 192), o, stream);
                return;
            }
        }
    }
    launch_cfg(a, best, o, 0, stream);
}

static void launch_gemm(const GemmArgs& a_in, const GemmOpts& o, hipStream_t stream) {
    if (a_in.conv) return launch_conv(a_in, o, stream);
    GemmArgs a = a_in;
    gemm_experiments_group_m(a);
    LTX_REQUIRE(!a.ep.pn_out, "gemm: the fused PixelNorm output exists for conv launches only");
    LTX_REQUIRE(!a.Bq || (gemm_takes_codes(a.M, a.N, a.K) && a.split_ws && a.split_k == 0),
                "gemm: 8-bit codes are de-quantised in the B stage of few-row launches only (M=%d N=%d K=%d)", a.M, a.N, a.K);
    if (a.split_ws && a.split_k == 0) launch_dense_ws(a, o, stream);
    else launch_dense(a, o, stream);
}
void launch_gemm_bf16(const GemmArgs& a, hipStream_t stream) { launch_gemm(a, gemm_opts(), stream); }

void launch_gemm_bf16(const GemmArgs& a, hipStream_t stream, const NormAfter* na) {
    LTX_REQUIRE(na && a.ep.out_f32 && !a.conv, "gemm: norm_after needs a dense launch with an f32 output");
    const GemmOpts o = gemm_opts();
    const bool fuse_on = o.finish_norm != 0;  // A/B option "finish_norm"
    const int s2 = (fuse_on && finish_takes_norm(a, *na)) ? dtl_split_for(a, o) : 0;
    if (s2) {
        GemmArgs b = a;
        b.split_k = s2;
        b.split_bf16 = dtl_split_bf16(a, o);
        validate(b);
        ProfScope prof(PROF_GEMM, 2.0 * a.M * a.N * a.K, stream);
        launch_dtl(b, o, stream, na);
        return;
    }
    launch_gemm(a, o, stream);
    NormModArgs n;  // the pass as a launch of its own, over the rows this launch wrote
    n.x = a.ep.out_f32; n.ldx = a.ep.ld_f32; n.rows = a.M; n.D = a.N;
    n.scale = na->scale; n.shift = na->shift; n.mod_bstride = na->mod_bstride; n.rows_per_batch = na->rows_per_batch; n.row_map = na->row_map;
    n.out = na->out; n.ldo = na->ldo;
    n.norm_kind = na->norm_kind; n.eps = na->eps; n.round_norm_bf16 = na->round_norm_bf16;
    launch_norm_mod(n, stream);
}

void launch_gemv_f32(const float* a, long lda, const bf16_t* W, long ldw, const float* bias, float* out, long ldo,
                     int M, int N, int K, int in_act, hipStream_t stream) {
    LTX_REQUIRE(M >= 1 && M <= 8, "gemv: M=%d out of range (1..8)", M);
    LTX_REQUIRE(K % 8 == 0 && lda % 4 == 0 && ldw % 8 == 0, "gemv: K=%d lda=%ld ldw=%ld alignment", K, lda, ldw);
    const int grid = (N + 3) / 4;
    if (M <= 2)
        hipLaunchKernelGGL((gemv_f32_kernel<2>), dim3(grid), dim3(256), 0, stream, a, lda, W, ldw, bias, out, ldo, M, N, K, in_act);
    else
        hipLaunchKernelGGL((gemv_f32_kernel<8>), dim3(grid), dim3(256), 0, stream, a, lda, W, ldw, bias, out, ldo, M, N, K, in_act);
    HIP_CHECK(hipGetLastError());
}

void launch_gemv_group(const GemvJob* jobs, int n_jobs, int M, hipStream_t stream) {
    // every check comes before the launch: a refused call writes nothing
    LTX_REQUIRE(jobs && n_jobs >= 1 && n_jobs <= 8, "gemv group: %d jobs out of range (1..8)", n_jobs);
    LTX_REQUIRE(M >= 1 && M <= 8, "gemv group: M=%d out of range (1..8)", M);
    GemvGroup g;
    g.n_jobs = n_jobs;
    g.M = M;
    long wgs = 0;
    for (int j = 0; j < 8; ++j) {
        g.job[j] = j < n_jobs ? jobs[j] : GemvJob{};
        const GemvJob& q = g.job[j];
        LTX_REQUIRE(q.N >= 0 && q.K >= 0 && q.K % 8 == 0 && q.lda % 4 == 0 && q.ldw % 8 == 0, "gemv group: job %d N=%d K=%d lda=%ld ldw=%ld alignment",
                    j, q.N, q.K, q.lda, q.ldw);
        LTX_REQUIRE(q.N == 0 || (q.a && q.W && q.out), "gemv group: job %d has a null a / W / out", j);
        wgs += (q.N + 3) / 4;
        LTX_REQUIRE(wgs < (1L << 30), "gemv group: too many output columns");
        g.wg_end[j] = (int)wgs;
    }
    if (wgs == 0) return;
    if (M <= 2)
        hipLaunchKernelGGL((gemv_group_kernel<2>), dim3((unsigned)wgs), dim3(256), 0, stream, g);
    else
        hipLaunchKernelGGL((gemv_group_kernel<8>), dim3((unsigned)wgs), dim3(256), 0, stream, g);
    HIP_CHECK(hipGetLastError());
}

// 4 rows per wave once that still gives 1024 workgroups (the logits: 16 388 of them); 2 below, so that a 3840-row Linear is 480
int gemv_bf16_rows_per_workgroup(int N, int epilogue) { return epilogue != GEMV_EPI_GEGLU && N >= 16384 ? 16 : 8; }

void launch_gemv_bf16(const GemvBf16Args& a, hipStream_t stream) {
    // every check comes before the launch: a refused call writes nothing
    LTX_REQUIRE(a.x && a.W, "gemv bf16: null x / W");
    LTX_REQUIRE(a.epilogue == GEMV_EPI_BF16 || a.epilogue == GEMV_EPI_F32 || a.epilogue == GEMV_EPI_GEGLU, "gemv bf16: epilogue %d (0 bf16, 1 f32, 2 geglu)", a.epilogue);
    LTX_REQUIRE(a.N >= 1 && a.N < (1 << 30), "gemv bf16: N=%d out of range", a.N);
    LTX_REQUIRE(a.K >= 8 && a.K % 8 == 0 && a.K <= 16384, "gemv bf16: K=%d must be a multiple of 8 up to 16384", a.K);
    LTX_REQUIRE(a.ldw % 8 == 0 && a.ldw >= a.K, "gemv bf16: ldw=%ld must be a multiple of 8, at least K=%d", a.ldw, a.K);
    LTX_REQUIRE(((uintptr_t)a.x & 15) == 0 && ((uintptr_t)a.W & 15) == 0, "gemv bf16: x / W must be 16-byte aligned");
    LTX_REQUIRE(a.epilogue == GEMV_EPI_F32 ? a.out_f32 != nullptr : (a.out_bf16 != nullptr && a.out_stride >= 1), "gemv bf16: null output or out_stride < 1");
    const int per_wg = gemv_bf16_rows_per_workgroup(a.N, a.epilogue);
    const dim3 grid((unsigned)((a.N + per_wg - 1) / per_wg)), block(256);
    if (a.epilogue == GEMV_EPI_GEGLU)
        hipLaunchKernelGGL((gemv_bf16_kernel<4, true>), grid, block, 0, stream, a);
    else if (per_wg == 16)
        hipLaunchKernelGGL((gemv_bf16_kernel<4, false>), grid, block, 0, stream, a);
    else
        hipLaunchKernelGGL((gemv_bf16_kernel<2, false>), grid, block, 0, stream, a);
    HIP_CHECK(hipGetLastError());
}

void launch_gemv_group_q(const GemvJobQ* jobs, int n_jobs, int M, int bits, hipStream_t stream) {
    // every check comes before the launch: a refused call writes nothing
    LTX_REQUIRE(jobs && n_jobs >= 1 && n_jobs <= 8, "gemv group q: %d jobs out of range (1..8)", n_jobs);
    LTX_REQUIRE(M >= 1 && M <= 8, "gemv group q: M=%d out of range (1..8)", M);
    LTX_REQUIRE(bits == 8 || bits == 4, "gemv group q: %d bits not supported (8, 4)", bits);
    GemvGroupQ g;
    g.n_jobs = n_jobs;
    g.M = M;
    long wgs = 0;
    for (int j = 0; j < 8; ++j) {
        g.job[j] = j < n_jobs ? jobs[j] : GemvJobQ{};
        const GemvJobQ& q = g.job[j];
        LTX_REQUIRE(q.N >= 0 && q.K >= 0 && q.K % 64 == 0 && q.lda % 4 == 0, "gemv group q: job %d N=%d K=%d (a multiple of the group, 64) lda=%ld alignment", j,
                    q.N, q.K, q.lda);
        LTX_REQUIRE(q.N == 0 || (q.a && q.codes && q.scales && q.biases && q.out), "gemv group q: job %d has a null a / codes / scales / biases / out", j);
        LTX_REQUIRE(((uintptr_t)q.codes & 7) == 0 && ((uintptr_t)q.scales & 1) == 0 && ((uintptr_t)q.biases & 1) == 0,
                    "gemv group q: job %d codes / scales / biases alignment (8 / 2 / 2 bytes)", j);
        wgs += (q.N + 3) / 4;
        LTX_REQUIRE(wgs < (1L << 30), "gemv group q: too many output columns");
        g.wg_end[j] = (int)wgs;
    }
    if (wgs == 0) return;
    const bool xl = ltx_opt(OPT_GEMVQ_SB) != 0;  // A/B option "gemvq_sb": how scale / bias reach the 8 lanes of a group (bit-neutral)
    const dim3 grid((unsigned)wgs), block(256);
#define LTX_GEMVQ_LAUNCH(MMAX, BITS)                                                                                \
    do {                                                                                                            \
        if (xl)                                                                                                     \
            hipLaunchKernelGGL((gemv_group_q_kernel<MMAX, BITS, true>), grid, block, 0, stream, g);                 \
        else                                                                                                        \
            hipLaunchKernelGGL((gemv_group_q_kernel<MMAX, BITS, false>), grid, block, 0, stream, g);                \
    } while (0)
    if (M <= 2) {
        if (bits == 8) LTX_GEMVQ_LAUNCH(2, 8); else LTX_GEMVQ_LAUNCH(2, 4);
    } else {
        if (bits == 8) LTX_GEMVQ_LAUNCH(8, 8); else LTX_GEMVQ_LAUNCH(8, 4);
    }
#undef LTX_GEMVQ_LAUNCH
    HIP_CHECK(hipGetLastError());
}
