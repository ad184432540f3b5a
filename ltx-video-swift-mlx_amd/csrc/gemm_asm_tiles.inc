// gemm_asm_tiles.inc - the three dense GEMM kernels whose main loop is a generated gfx950 instruction stream, their predicates and
// their launchers. Included by gemm.hip (textually: the streams name registers by hand, so a kernel and its stream are one unit).
//
//   gemm_bf16_kernel_dtl   192 x 256 tile (tile_cfg 75)            tools/gen_gemm_asm_dtl.py
//   gemm_bf16_kernel_qkv   192 x 384 tile: q|k and V in one launch  tools/gen_gemm_asm_qkv.py
//   gemm_bf16_kernel_tall  384 x 256 tile (tile_cfg 76)            tools/gen_gemm_asm_tall.py
//
// What they share (written once below, and once in tools/asm_common.py for the streams and their static RAW / WAR proof):
//   * dense A . B^T on whole tiles, K % 64 == 0; four waves as 2 x 2 = ONE wave per SIMD, accumulators of v_mfma_f32_16x16x32_bf16;
//   * the LDS image of every GEMM kernel here (128-byte rows, 16-byte chunks XOR-swizzled by (row >> 1) & 7 on the LDS-DMA source
//     address), two activation slots followed by the weight slots. LDS-DMA piece i of wave w is rows (w + 4 i) * 8 .. + 7 of a tile:
//     the per-lane part of its source address (row inside the piece, swizzled chunk) does not depend on i ((row >> 1) & 7 is the same
//     for rows 32 apart), the i part is a scalar offset kept by the stream (AsmLane, asm_buf_desc);
//   * C++ prepares those offsets, the fragment read addresses of slot 0 and the buffer descriptors, the stream runs the whole K loop
//     and leaves the accumulators of the first rows in AGPRs in the map a[(mi * 8 + ni) * 4 ..] (tools/gen_gemm_asm.py's dump reads it);
//   * the plain-store epilogue: 32 rows x 128 columns at a time through the wave's LDS scratch, the 16 scratch reads of a group issued
//     together, one 16-byte column group per lane. The form of the store is picked once per launch (asm_plain_variant: four
//     instantiated variants through per-lane row pointers, asm_store_rows + AsmRowStore; anything else through the generic
//     asm_store_group). One accumulator chain per output element, K ascending, and the same epilogue operations in the same order in
//     every form: the kernels give the same bits on the same operands.
//   * one launcher helper (launch_asm_tile): the dynamic-LDS attribute once per device, then the launch.
namespace {

// ---- per-lane staging and fragment addressing ----
LTX_DEVFN int asm_src_offset(int lane, int wave, long ld) {  // byte offset of this lane's 16 bytes inside the wave's piece 0
    const int srow = lane >> 3, pch = lane & 7;
    const int row0 = wave * 8 + srow;
    return (row0 * (int)ld + ((pch ^ ((row0 >> 1) & 7)) << 3)) * 2;
}
LTX_DEVFN uint32_t asm_src_stride(long ld) { return (uint32_t)(32 * ld * 2); }  // from one piece of a wave to its next: 32 rows

struct AsmLane {
    int ao, bo;              // asm_src_offset of the activations / the weights
    uint32_t sa, sb;         // asm_src_stride of the same
    uint32_t wlds;           // where the wave's piece lies inside four pieces of LDS
    int fa0, fa1, fb0, fb1;  // LDS byte address of this lane's fragment reads of slot 0, k-steps 0 / 1: A rows from wr * WM, B rows from wc * WCOL
};
template <int WM, int WCOL, int A_BYTES>
LTX_DEVFN AsmLane asm_lane(int lane, int wave, int wr, int wc, long lda, long ldb) {
    AsmLane l;
    l.ao = asm_src_offset(lane, wave, lda);
    l.bo = asm_src_offset(lane, wave, ldb);
    l.sa = asm_src_stride(lda);
    l.sb = asm_src_stride(ldb);
    l.wlds = (uint32_t)wave * 1024u;
    const int frow = lane & 15, fsw = (lane >> 1) & 7;
    const int foff0 = frow * ROW_BYTES + ((((lane >> 4) + 0) ^ fsw) << 4);
    const int foff1 = frow * ROW_BYTES + ((((lane >> 4) + 4) ^ fsw) << 4);
    const int a_wave_off = (wr * WM) * ROW_BYTES, b_wave_off = 2 * A_BYTES + (wc * WCOL) * ROW_BYTES;
    l.fa0 = a_wave_off + foff0, l.fa1 = a_wave_off + foff1, l.fb0 = b_wave_off + foff0, l.fb1 = b_wave_off + foff1;
    return l;
}

// buffer descriptor words 0..2 of `rows` rows of `kelems` elements at p (word 3 is a constant of the stream)
struct AsmBufDesc {
    uint32_t lo, hi, rec;
};
LTX_DEVFN AsmBufDesc asm_buf_desc(const bf16_t* p, int rows, long ld, long kelems) {
    return {(uint32_t)(uintptr_t)p, (uint32_t)((uintptr_t)p >> 32), (uint32_t)(((long)(rows - 1) * ld + kelems) * 2)};
}

// LDS byte offset, inside a 32-row x WN-column f32 scratch group, of the first element this lane holds in the 16 x 16 accumulator layout
template <int WN>
LTX_DEVFN int asm_scratch_lane(int lane) { return (((lane >> 4) * 4) * WN + (lane & 15)) * 4; }

#if defined(DTL_STAMPS) || defined(QKV_STAMPS) || defined(TALL_STAMPS)  // tools/ubench/gemm_{dtl,qkv,tall}_stamps.hip
LTX_DEVFN unsigned long long* asm_stamp_slot(int wave) { return (blockIdx.x == 7) ? &g_gemm_stamps[wave][0] : &g_gemm_stamps[4][0]; }
// Epilogue stamps of the same builds, shader-clock cycles per wave of workgroup 7: [0] the stream has been left; per row group in the
// order it is stored [1 + 2 i] its dump is in LDS (for a group the stream left there: the group before it is done) and [2 + 2 i] its
// scratch reads have landed and its last store is issued; [1 + 2 groups] the final vmcnt(0). The indices are constants: registers.
__device__ unsigned long long g_gemm_epi_stamps[5][16];
#define ASM_EPI_STAMPS unsigned long long epi_ts[16] = {}
#define ASM_EPI_STAMP(i) epi_ts[i] = __builtin_readcyclecounter()
#define ASM_EPI_STAMPS_FLUSH(n)                                                               \
    do {                                                                                      \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                      \
        ASM_EPI_STAMP(n);                                                                     \
        if (lane == 0)                                                                        \
            for (int i_ = 0; i_ <= (n); ++i_) g_gemm_epi_stamps[blockIdx.x == 7 ? wave : 4][i_] = epi_ts[i_]; \
    } while (0)
#else
#define ASM_EPI_STAMPS
#define ASM_EPI_STAMP(i)
#define ASM_EPI_STAMPS_FLUSH(n)
#endif

// ---- the plain-store epilogue ----
LTX_DEVFN f32x4 asm_column_bias(const float* bias_n, int gn) { return bias_n ? *(const f32x4*)(bias_n + gn) : f32x4{0.f, 0.f, 0.f, 0.f}; }

// per-row bias (BIAS_M: the 384 x 256 kernel takes no launch that has one), activation, rounding to bf16 values: in this order
template <bool BIAS_M>
LTX_DEVFN f32x4 asm_activate(const GemmEpilogue& ep, f32x4 v, int gm) {
    if constexpr (BIAS_M) {
        if (ep.bias_m) {
            const float bm = ep.bias_m[gm];
            v += f32x4{bm, bm, bm, bm};
        }
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
    return v;
}
LTX_DEVFN void asm_store_bf16(bf16_t* out, long ld, int gm, int gn, const f32x4& v) {
    uint2 pk;
    pk.x = pack_bf16x2(v[0], v[1]);
    pk.y = pack_bf16x2(v[2], v[3]);
    *(uint2*)(out + (long)gm * ld + gn) = pk;
}
LTX_DEVFN void asm_store(const GemmEpilogue& ep, int gm, int gn, const f32x4& v) {
    if (ep.out_f32) *(f32x4*)(ep.out_f32 + (long)gm * ep.ld_f32 + gn) = v;
    if (ep.out_bf16) asm_store_bf16(ep.out_bf16, ep.ld_bf16, gm, gn, v);
}
template <bool BIAS_M>
struct AsmPlainStore {  // what a GemmEpilogue without residual asks for
    const GemmEpilogue& ep;
    LTX_DEVFN void operator()(int gm, int gn, f32x4 v) const { asm_store(ep, gm, gn, asm_activate<BIAS_M>(ep, v, gm)); }
};

// rows, lanes per row and steps of a 32-row scratch group of WN columns: one 16-byte column group per lane
template <int WN>
struct AsmGroup {
    static constexpr int LPR = WN / 4, RPI = 64 / LPR, NITG = 32 / RPI;  // lanes per row, rows per step, steps per group
};
// One group: scr (this wave's 32 x WN f32, row-major, written by a dump or by the stream) + bias -> put(row, column, value) for rows
// gm0 .. gm0 + 31, columns gn .. gn + 3 of this lane. The scratch reads of the group are issued together (a rolled loop waited for one
// ds_read_b128 per step, ~100 cycles each with nothing else to issue on a one-wave SIMD), and all of them have returned on the way
// out: the next dump rewrites the scratch.
template <int WN, class Put>
LTX_DEVFN void asm_store_group(const float* scr, int lane, int gm0, int gn, const f32x4& bias, Put&& put) {
    using G = AsmGroup<WN>;
    f32x4 vv[G::NITG];
#pragma unroll
    for (int it = 0; it < G::NITG; ++it) vv[it] = *(const f32x4*)(scr + (it * G::RPI + lane / G::LPR) * WN + (lane % G::LPR) * 4);
#pragma unroll
    for (int it = 0; it < G::NITG; ++it) put(gm0 + it * G::RPI + lane / G::LPR, gn, vv[it] + bias);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// ---- the plain-store epilogue, one variant per launch ----
// These launches are one round with one wave per SIMD: nothing overlaps the epilogue, so it costs the sum of its issue slots. The
// generic body above tests ep.act / round_bf16 / out_f32 / out_bf16 in every 4-element step and rebuilds (long)gm * ld + gn for every
// store. The forms the launchers really send are therefore picked ONCE per kernel (asm_plain_variant, wave-uniform) and instantiated
// with the activation and the outputs as template arguments: a step is then arithmetic, a pack and a store through a per-lane row
// pointer that advances by a wave-uniform stride. Same operations in the same order per element as asm_activate + asm_store: same bits.
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;

// the two store dwords of four values: two v_cvt_pk_bf16_f32 (round-to-nearest-even, as f32_to_bf16) and nothing else
LTX_DEVFN uint2 asm_pack_bf16x4(const f32x4& v) {
    const bf16x2_t lo = __builtin_convertvector(f32x2{v[0], v[1]}, bf16x2_t);
    const bf16x2_t hi = __builtin_convertvector(f32x2{v[2], v[3]}, bf16x2_t);
    return uint2{__builtin_bit_cast(uint32_t, lo), __builtin_bit_cast(uint32_t, hi)};
}
// gelu_tanh (common.h) on a pair: the same multiplies, fma and add per element, issued as v_pk_mul_f32 / v_pk_fma_f32 / v_pk_add_f32
LTX_DEVFN f32x2 asm_gelu_tanh2(f32x2 x) {
    const float c0 = -2.0f * 0.7978845608028654f * 1.4426950408889634f;
    const float c1 = c0 * 0.044715f;
    const f32x2 t = x * __builtin_elementwise_fma(f32x2{c1, c1}, x * x, f32x2{c0, c0});
    const f32x2 d = f32x2{1.0f, 1.0f} + f32x2{__builtin_amdgcn_exp2f(t[0]), __builtin_amdgcn_exp2f(t[1])};
    return x * f32x2{__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
}

enum { ASM_OUT_BF16 = 1, ASM_OUT_F32 = 2 };
// Row stores of one lane: pb / pf point at this lane's four columns of the row its next step stores, sb / sf are the elements from
// one step's row to the next's (RPI rows). ACT is LTX_ACT_NONE or LTX_ACT_GELU_TANH, OUTS a mask of ASM_OUT_*; BIAS adds the column
// bias (the split-K partial tiles are stored raw: adding a zero bias would turn -0 into +0).
template <int ACT, int OUTS, bool BIAS>
struct AsmRowStore {
    bf16_t* pb;
    float* pf;
    long sb, sf;
    f32x4 bias;
    LTX_DEVFN AsmRowStore after(int steps) const { return {pb + steps * sb, pf + steps * sf, sb, sf, bias}; }  // wave-uniform offset
    LTX_DEVFN void operator()(f32x4 v) {
        if constexpr (BIAS) v += bias;
        if constexpr (ACT == LTX_ACT_GELU_TANH) {
            const f32x2 lo = asm_gelu_tanh2(f32x2{v[0], v[1]}), hi = asm_gelu_tanh2(f32x2{v[2], v[3]});
            v = f32x4{lo[0], lo[1], hi[0], hi[1]};
        }
        if constexpr ((OUTS & ASM_OUT_F32) != 0) {
            *(f32x4*)pf = v;
            pf += sf;
        }
        if constexpr ((OUTS & ASM_OUT_BF16) != 0) {
            *(uint2*)pb = asm_pack_bf16x4(v);
            pb += sb;
        }
    }
};
// the store of rows row0 + lane / LPR + RPI * step, this lane's columns gn .. gn + 3: the only per-lane address arithmetic of a kernel
template <int WN, int ACT, int OUTS, bool BIAS>
LTX_DEVFN AsmRowStore<ACT, OUTS, BIAS> asm_row_store(bf16_t* out_bf16, long ld_bf16, float* out_f32, long ld_f32, int lane, int row0, int gn, const f32x4& bias) {
    using G = AsmGroup<WN>;
    const int row = row0 + lane / G::LPR;
    return {out_bf16 + (long)row * ld_bf16 + gn, out_f32 + (long)row * ld_f32 + gn, G::RPI * ld_bf16, G::RPI * ld_f32, bias};
}
// asm_store_group for a row store: the group's scratch reads issued together, then its steps in row order
template <int WN, class Put>
LTX_DEVFN void asm_store_rows(const float* scr, int lane, Put put) {
    using G = AsmGroup<WN>;
    f32x4 vv[G::NITG];
#pragma unroll
    for (int it = 0; it < G::NITG; ++it) vv[it] = *(const f32x4*)(scr + (it * G::RPI + lane / G::LPR) * WN + (lane % G::LPR) * 4);
#pragma unroll
    for (int it = 0; it < G::NITG; ++it) put(vv[it]);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}
// The variant of a plain-store launch: 0 = the generic body, 1 .. 4 = the forms asm_plain_dispatch lists. round_bf16 changes nothing when
// only bf16 is stored (rounding twice is rounding once); a per-row bias or SiLU stays generic (no launcher sends them to these kernels
// on a hot path).
LTX_DEVFN int asm_plain_variant(const GemmEpilogue& ep) {
    if (ep.bias_m || (ep.round_bf16 && ep.out_f32)) return 0;
    if (ep.act == LTX_ACT_NONE) return ep.out_f32 ? (ep.out_bf16 ? 4 : 3) : 1;
    if (ep.act == LTX_ACT_GELU_TANH && !ep.out_f32) return 2;
    return 0;
}
// body(act, outs) with both as integral constants for variants 1 .. 4; false for variant 0
template <class Body>
LTX_DEVFN bool asm_plain_dispatch(int variant, Body&& body) {
    using std::integral_constant;
    if (variant == 1) body(integral_constant<int, LTX_ACT_NONE>{}, integral_constant<int, ASM_OUT_BF16>{});
    else if (variant == 2) body(integral_constant<int, LTX_ACT_GELU_TANH>{}, integral_constant<int, ASM_OUT_BF16>{});
    else if (variant == 3) body(integral_constant<int, LTX_ACT_NONE>{}, integral_constant<int, ASM_OUT_F32>{});
    else if (variant == 4) body(integral_constant<int, LTX_ACT_NONE>{}, integral_constant<int, ASM_OUT_F32 | ASM_OUT_BF16>{});
    else return false;
    return true;
}

// ---------------------------------------------------------------------------------------------------------------
// 192 x 256 tile. The wide DiT GEMMs (fused q|k: N = 8192, FFN up: N = 16384) at 1536 tokens are exactly one / two rounds of 256 such
// tiles, where 192 x 128 tiles need two / four rounds and pay the fixed cost of a round (ring fill, epilogue with every workgroup
// storing at once) twice as often.
//   LDS     [A slot 0][A slot 1][B slot 0][B slot 1][B slot 2]: a 24 + 32 KB K-tile leaves room for three weight slots, so both k-steps'
//           fragments are held in registers and the LDS-DMA of A tile t+2 / B tile t+3 reuses the slots of tile t as soon as every wave
//           has read them (the loop runs at bytes in flight / HBM latency)
//   out     wave tile 96 x 128, all of it in a[0:191]
//   extras  deterministic split-K (grid.y = K range: each range writes its raw partial tile to its workspace slice, the finish pass adds
//           the slices in order and applies the epilogue) and the residual + gate epilogue
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 1) void gemm_bf16_kernel_dtl(const GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int BM = 192, BN = 256, WGN = 2;
    constexpr int WM = 96, WN = 128;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / WGN, wc = wave % WGN;
    const int tiles_m = g.M / BM;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    int tm, tn;
    tile_coords(g, bid, tiles_m, BN, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;
    int kt0 = 0, nkt = g.K / BK;
    if (g.split_k > 1) {
        const int z = blockIdx.y;
        kt0 = (int)((long)nkt * z / g.split_k);
        nkt = (int)((long)nkt * (z + 1) / g.split_k) - kt0;
    }
    const AsmLane l = asm_lane<WM, WN, BM * ROW_BYTES>(lane, wave, wr, wc, g.lda, g.ldb);
    const AsmBufDesc a = asm_buf_desc(g.A + (long)m0 * g.lda + (long)kt0 * BK, BM, g.lda, (long)nkt * BK);
    const AsmBufDesc b = asm_buf_desc(g.B + (long)n0 * g.ldb + (long)kt0 * BK, BN, g.ldb, (long)nkt * BK);
    const uint32_t nk = (uint32_t)nkt;
#ifdef DTL_STAMPS
    unsigned long long* dbg = asm_stamp_slot(wave);
#endif
    asm volatile(
#ifdef DTL_STAMPS
#include "gemm_dtl_192x256_stamps.inc"
#else
#include "gemm_dtl_192x256.inc"
#endif
        :
        : [alo] "s"(a.lo), [ahi] "s"(a.hi), [arec] "s"(a.rec), [blo] "s"(b.lo), [bhi] "s"(b.hi), [brec] "s"(b.rec), [nk] "s"(nk), [sa] "s"(l.sa),
          [sb] "s"(l.sb), [wlds] "s"(l.wlds), [ao] "v"(l.ao), [bo] "v"(l.bo), [fa0] "v"(l.fa0), [fa1] "v"(l.fa1), [fb0] "v"(l.fb0), [fb1] "v"(l.fb1)
#ifdef DTL_STAMPS
          , [dbg] "s"(dbg)
#endif
        :
#include "gemm_dtl_192x256_clobbers.inc"
    );
    __syncthreads();  // every wave is done with the K-tile slots before the epilogue scratch reuses them
    ASM_EPI_STAMPS;
    ASM_EPI_STAMP(0);
    // Epilogue: three groups of 32 rows, each dumped from a[0:191] into the wave's LDS scratch (assembly dump shared with
    // tools/gen_gemm_asm.py: same accumulator map)
    constexpr int LPR = AsmGroup<WN>::LPR, RPI = AsmGroup<WN>::RPI, NITG = AsmGroup<WN>::NITG;
    float* scr = (float*)(smem + wave * (32 * WN * 4));
    // LDS byte address of this lane's first scratch element (the dynamic LDS of this kernel starts at 0, as the main loop assumes)
    const unsigned scr_lane = (unsigned)(wave * (32 * WN * 4) + asm_scratch_lane<WN>(lane));
    const int gn = n0 + wc * WN + (lane % LPR) * 4;
    if (g.split_k > 1) {  // raw partial tile -> this K range's slice of the workspace: no bias
        float* ws = g.split_ws + (long)blockIdx.y * g.M * g.N;
        bf16_t* wsb = (bf16_t*)g.split_ws + (long)blockIdx.y * g.M * g.N;
        auto partial = [&](auto outs_c) {  // the form of the store is picked once, not per step
            constexpr int outs = decltype(outs_c)::value;
            const auto st = asm_row_store<WN, LTX_ACT_NONE, outs, false>(wsb, g.N, ws, g.N, lane, m0 + wr * WM, gn, f32x4{});
            static_for<0, 3>([&](auto grp_c) {
                constexpr int grp = decltype(grp_c)::value;
#include "gemm_asm_192x256_dump.inc"
                ASM_EPI_STAMP(1 + 2 * grp);
                asm_store_rows<WN>(scr, lane, st.after(grp * NITG));
                ASM_EPI_STAMP(2 + 2 * grp);
            });
        };
        if (g.split_bf16) partial(std::integral_constant<int, ASM_OUT_BF16>{});
        else partial(std::integral_constant<int, ASM_OUT_F32>{});
        ASM_EPI_STAMPS_FLUSH(7);
        return;
    }
    const GemmEpilogue& ep = g.ep;
    const f32x4 bias = asm_column_bias(ep.bias_n, gn);
    if (ep.resid) {
        // Residual launches (the long-sequence configurations route their gated-residual GEMMs here). A loop that reads the residual row
        // and the gate with one dependent load per two-row step and divides by rows_per_batch for every row took 426 us at 9984 tokens
        // against 276 us for the same product with a plain store. Here the 16 residual loads of a 32-row group are requested together,
        // one group ahead of the accumulator dump, and the gate vector is loaded once when the wave's 96 rows lie in one batch element
        // (always, for one sample per GPU). Same arithmetic per element as asm_store_group + AsmPlainStore, then x + gate * v.
        const float* rbase = ep.resid_src ? ep.resid_src : ep.out_f32;
        const long rld = ep.resid_src ? ep.ld_resid : ep.ld_f32;
        const int row_lo = m0 + wr * WM, row_hi = row_lo + WM - 1;
        const bool gate_uniform = ep.gate && !ep.gate_rowmap && row_lo / ep.rows_per_batch == row_hi / ep.rows_per_batch;
        f32x4 gtu = f32x4{ep.gate_scalar, ep.gate_scalar, ep.gate_scalar, ep.gate_scalar};
        if (gate_uniform) gtu = *(const f32x4*)(ep.gate + (long)(row_lo / ep.rows_per_batch) * ep.gate_bstride + gn);
        // The form is picked once, like the plain stores: FAST is what the DiT sends (no row bias, activation or rounding, an f32 stream
        // with or without its bf16 copy) and stores through row pointers; GATE_ROWS loads the gate per row (row map, or a wave whose rows
        // span two batch elements). Anything else keeps the generic step. The residual rows are read through a row pointer in every form.
        auto resid_body = [&](auto fast_c, auto mirror_c, auto gate_rows_c) {
            constexpr bool FAST = decltype(fast_c)::value, MIRROR = decltype(mirror_c)::value, GATE_ROWS = decltype(gate_rows_c)::value;
            const float* rp = rbase + (long)(row_lo + lane / LPR) * rld + gn;
            const long rstep = RPI * rld;
            auto st = asm_row_store<WN, LTX_ACT_NONE, ASM_OUT_F32 | (MIRROR ? ASM_OUT_BF16 : 0), false>(ep.out_bf16, ep.ld_bf16, ep.out_f32, ep.ld_f32, lane, row_lo,
                                                                                                     gn, f32x4{});
            f32x4 rs[2][NITG];
            auto fetch = [&](auto grp_c, auto buf_c) {
                constexpr int grp = decltype(grp_c)::value, buf = decltype(buf_c)::value;
#pragma unroll
                for (int it = 0; it < NITG; ++it) rs[buf][it] = *(const f32x4*)(rp + (grp * NITG + it) * rstep);
            };
            fetch(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
            static_for<0, 3>([&](auto grp_c) {
                constexpr int grp = decltype(grp_c)::value;
                constexpr int buf = grp & 1;
                if constexpr (grp + 1 < 3) fetch(std::integral_constant<int, grp + 1>{}, std::integral_constant<int, (grp + 1) & 1>{});
#include "gemm_asm_192x256_dump.inc"
                static_for<0, 2>([&](auto half_c) {
                    constexpr int half = decltype(half_c)::value;
                    f32x4 vv[NITG / 2];  // the scratch reads of eight two-row steps issued together
#pragma unroll
                    for (int i2 = 0; i2 < NITG / 2; ++i2) vv[i2] = *(const f32x4*)(scr + ((half * (NITG / 2) + i2) * RPI + lane / LPR) * WN + (lane % LPR) * 4);
#pragma unroll
                    for (int i2 = 0; i2 < NITG / 2; ++i2) {
                        const int it = half * (NITG / 2) + i2;
                        const int gm = row_lo + grp * 32 + it * RPI + lane / LPR;
                        f32x4 v = vv[i2] + bias;
                        if constexpr (!FAST) v = asm_activate<true>(ep, v, gm);
                        f32x4 gt = gtu;
                        if constexpr (!FAST) {
                            if (ep.gate && !gate_uniform)
                                gt = *(const f32x4*)(ep.gate + (long)(ep.gate_rowmap ? ep.gate_rowmap[gm] : gm / ep.rows_per_batch) * ep.gate_bstride + gn);
                        } else if constexpr (GATE_ROWS) {
                            gt = *(const f32x4*)(ep.gate + (long)(ep.gate_rowmap ? ep.gate_rowmap[gm] : gm / ep.rows_per_batch) * ep.gate_bstride + gn);
                        }
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = rs[buf][it][e] + gt[e] * v[e];
                        if constexpr (FAST) st(v);  // the steps come in row order
                        else asm_store(ep, gm, gn, v);
                    }
                });
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the scratch is rewritten by the next dump
            });
        };
        using std::false_type;
        using std::true_type;
        const bool fast = !ep.bias_m && ep.act == LTX_ACT_NONE && !ep.round_bf16 && ep.out_f32;
        const bool gate_rows = ep.gate && !gate_uniform;
        if (!fast) resid_body(false_type{}, false_type{}, false_type{});
        else if (gate_rows) ep.out_bf16 ? resid_body(true_type{}, true_type{}, true_type{}) : resid_body(true_type{}, false_type{}, true_type{});
        else ep.out_bf16 ? resid_body(true_type{}, true_type{}, false_type{}) : resid_body(true_type{}, false_type{}, false_type{});
        return;
    }
    const bool specialised = asm_plain_dispatch(__builtin_amdgcn_readfirstlane(asm_plain_variant(ep)), [&](auto act_c, auto outs_c) {
        const auto st = asm_row_store<WN, decltype(act_c)::value, decltype(outs_c)::value, true>(ep.out_bf16, ep.ld_bf16, ep.out_f32, ep.ld_f32, lane,
                                                                                                 m0 + wr * WM, gn, bias);
        static_for<0, 3>([&](auto grp_c) {
            constexpr int grp = decltype(grp_c)::value;
#include "gemm_asm_192x256_dump.inc"
            ASM_EPI_STAMP(1 + 2 * grp);
            asm_store_rows<WN>(scr, lane, st.after(grp * NITG));
            ASM_EPI_STAMP(2 + 2 * grp);
        });
    });
    if (!specialised)
        static_for<0, 3>([&](auto grp_c) {
            constexpr int grp = decltype(grp_c)::value;
#include "gemm_asm_192x256_dump.inc"
            ASM_EPI_STAMP(1 + 2 * grp);
            asm_store_group<WN>(scr, lane, m0 + wr * WM + grp * 32, gn, bias, AsmPlainStore<true>{ep});
            ASM_EPI_STAMP(2 + 2 * grp);
        });
    ASM_EPI_STAMPS_FLUSH(7);
}

// ---------------------------------------------------------------------------------------------------------------
// 192 x 384 tile for the self-attention projections of a DiT block: 256 columns of the fused q|k matrix and 128 columns of V in ONE
// launch (both read the same adaLN rows). 1536 tokens x (8192 + 4096) columns are exactly one round of 256 tiles where the two launches
// it replaces ran a round each.
//   LDS     [A slot 0][A slot 1][B slot 0][B slot 1]; a B slot holds [q|k 0..127][V 0..63][q|k 128..255][V 64..127], so the 192 weight
//           rows of a wave column are contiguous; a third source (V: vo, sv, its descriptor) is staged through the same helpers
//   out     wave tile 96 x 192: columns 0..127 are q|k in a[0:191] (the 192 x 256 kernel's map and dump: bias, row-major bf16 store
//           through asm_store_group); columns 128..191 are V: sixteen fragments in a[192:255], the other eight were in VGPRs and are
//           left in LDS behind the q|k scratch, 8 KB per wave
//   V^T     stored straight from the accumulator layout (bias, bf16), as gemm_epilogue_with's out_bf16_t form
// Same accumulator chain per output element as the two launches it replaces: bit-identical to them.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 1) void gemm_bf16_kernel_qkv(const GemmQkvArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int BM = 192, WM = 96, WNQ = 128, WNV = 64;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / 2, wc = wave % 2;
    const int tiles_m = g.M / BM;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    int tm, tn;
    tile_coords(g.group_m, g.Nqk / 256, bid, tiles_m, tm, tn);
    const int m0 = tm * BM;
    const AsmLane l = asm_lane<WM, WNQ + WNV, BM * ROW_BYTES>(lane, wave, wr, wc, g.ldx, g.ldwqk);
    const int vo = asm_src_offset(lane, wave, g.ldwv);
    const uint32_t sv = asm_src_stride(g.ldwv);
    const AsmBufDesc a = asm_buf_desc(g.X + (long)m0 * g.ldx, BM, g.ldx, g.K);
    const AsmBufDesc b = asm_buf_desc(g.Wqk + (long)tn * 256 * g.ldwqk, 256, g.ldwqk, g.K);
    const AsmBufDesc v = asm_buf_desc(g.Wv + (long)tn * 128 * g.ldwv, 128, g.ldwv, g.K);
    const uint32_t nk = (uint32_t)(g.K / BK);
    // where the stream leaves the eight V accumulators it keeps in VGPRs
    constexpr int SPILL0 = 4 * 32 * WNQ * 4;
    const int sp = SPILL0 + wave * 8192 + lane * 16;
#ifdef QKV_STAMPS
    unsigned long long* dbg = asm_stamp_slot(wave);
#endif
    asm volatile(
#ifdef QKV_STAMPS
#include "gemm_qkv_192x384_stamps.inc"
#else
#include "gemm_qkv_192x384.inc"
#endif
        :
        : [alo] "s"(a.lo), [ahi] "s"(a.hi), [arec] "s"(a.rec), [blo] "s"(b.lo), [bhi] "s"(b.hi), [brec] "s"(b.rec), [vlo] "s"(v.lo), [vhi] "s"(v.hi),
          [vrec] "s"(v.rec), [nk] "s"(nk), [sa] "s"(l.sa), [sb] "s"(l.sb), [sv] "s"(sv), [wlds] "s"(l.wlds), [ao] "v"(l.ao), [bo] "v"(l.bo), [vo] "v"(vo),
          [fa0] "v"(l.fa0), [fa1] "v"(l.fa1), [fb0] "v"(l.fb0), [fb1] "v"(l.fb1), [sp] "v"(sp)
#ifdef QKV_STAMPS
          , [dbg] "s"(dbg)
#endif
        :
#include "gemm_qkv_192x384_clobbers.inc"
    );
    // (the stream ends behind a barrier: every wave is done with the K-tile slots, and its VGPR-held accumulators are in LDS)
    ASM_EPI_STAMPS;
    ASM_EPI_STAMP(0);
    // V epilogue: fragment vf = 4 mi + nv holds C[16 mi + 4 (lane >> 4) + r][16 nv + (lane & 15)], r = 0..3, of the wave's 96 x 64 V
    // tile: four consecutive tokens of one channel = 8 contiguous bytes of V^T. The tile's rows lie in one batch element.
    {
        const int bi = m0 / g.rows_per_batch;
        const int tok0 = m0 - bi * g.rows_per_batch + wr * WM + (lane >> 4) * 4;
        const int d0 = tn * 128 + wc * WNV + (lane & 15);
        bf16_t* vbase = g.vt + (long)bi * g.vt_bstride + tok0;
        float bv[4];
        bf16_t* vrow[4];  // this lane's four V^T rows (channels d0 + 16 nv): a fragment's store is a constant offset from one of them
#pragma unroll
        for (int nv = 0; nv < 4; ++nv) {
            bv[nv] = g.bias_v ? g.bias_v[d0 + nv * 16] : 0.f;
            vrow[nv] = vbase + (long)(d0 + nv * 16) * g.ldvt;
        }
        static_for<0, 24>([&](auto vf_c) {
            constexpr int vf = decltype(vf_c)::value;
            constexpr int mi = vf / 4, nv = vf % 4;
            float f0, f1, f2, f3;
            if constexpr (vf < 16) {
#include "gemm_qkv_192x384_vread.inc"
            } else {
                const f32x4 t = *(const f32x4*)(smem + SPILL0 + wave * 8192 + (vf - 16) * 1024 + lane * 16);
                f0 = t[0], f1 = t[1], f2 = t[2], f3 = t[3];
            }
            const float bn = bv[nv];
            *(uint2*)(vrow[nv] + mi * 16) = asm_pack_bf16x4(f32x4{f0 + bn, f1 + bn, f2 + bn, f3 + bn});
        });
    }
    ASM_EPI_STAMP(1);
    // q|k epilogue: three groups of 32 rows, each dumped from a[0:191] into the wave's LDS scratch
    constexpr int WN = WNQ;
    float* scr = (float*)(smem + wave * (32 * WN * 4));
    const unsigned scr_lane = (unsigned)(wave * (32 * WN * 4) + asm_scratch_lane<WN>(lane));
    const int gn = tn * 256 + wc * WN + (lane % AsmGroup<WN>::LPR) * 4;
    const f32x4 bias = asm_column_bias(g.bias_qk, gn);
    const auto qk_store = asm_row_store<WN, LTX_ACT_NONE, ASM_OUT_BF16, true>(g.qk, g.ld_qk, nullptr, 0, lane, m0 + wr * WM, gn, bias);
    static_for<0, 3>([&](auto grp_c) {
        constexpr int grp = decltype(grp_c)::value;
#include "gemm_asm_192x256_dump.inc"
        ASM_EPI_STAMP(2 + 2 * grp);
        asm_store_rows<WN>(scr, lane, qk_store.after(grp * AsmGroup<WN>::NITG));
        ASM_EPI_STAMP(3 + 2 * grp);
    });
    ASM_EPI_STAMPS_FLUSH(8);  // [1]: the V^T stores are issued; q|k groups from [2]
}

// ---------------------------------------------------------------------------------------------------------------
// 384 x 256 tile. The DiT's FFN-up projection at 1536 tokens (1536 x 16384) is exactly ONE round of 256 such tiles where the 192 x 256
// kernel runs two, and per MFMA the tile stages 29 % fewer bytes. Dense A.B^T with plain stores only (gemm_tall_fits).
//   LDS     [A slot 0][A slot 1][B slot 0][B slot 1]: two 48 KB activation slots and two 32 KB weight slots are the whole 160 KB, so
//           this kernel has no static LDS and the epilogue reuses the slots
//   out     wave tile 192 x 128: rows 0..127 in a[0:255] (the 192 x 256 kernel's map, one 32-row group longer); rows 128..191 were in
//           VGPRs and are left in LDS in the layout of the epilogue scratch, two groups of the wave's WAVE_LDS bytes
//   order   groups 4, 5 lie in the wave's LDS already and go first; groups 0..3 are then dumped from a[0:255] over them, one at a time
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 1) void gemm_bf16_kernel_tall(const GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int BM = 384, BN = 256, WGN = 2;
    constexpr int WM = 192, WN = 128;
    constexpr int WAVE_LDS = 2 * 32 * WN * 4;  // the epilogue's share of LDS per wave: two 32-row groups of f32
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / WGN, wc = wave % WGN;
    const int tiles_m = g.M / BM;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    int tm, tn;
    tile_coords(g, bid, tiles_m, BN, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;
    const int nkt = g.K / BK;
    const AsmLane l = asm_lane<WM, WN, BM * ROW_BYTES>(lane, wave, wr, wc, g.lda, g.ldb);
    const AsmBufDesc a = asm_buf_desc(g.A + (long)m0 * g.lda, BM, g.lda, (long)nkt * BK);
    const AsmBufDesc b = asm_buf_desc(g.B + (long)n0 * g.ldb, BN, g.ldb, (long)nkt * BK);
    const uint32_t nk = (uint32_t)nkt;
    // where the stream leaves the accumulators of rows 128..191: this lane's first element of the wave's two scratch groups
    const int sp = wave * WAVE_LDS + asm_scratch_lane<WN>(lane);
#ifdef TALL_STAMPS
    unsigned long long* dbg = asm_stamp_slot(wave);
#endif
    asm volatile(
#ifdef TALL_STAMPS
#include "gemm_tall_384x256_stamps.inc"
#else
#include "gemm_tall_384x256.inc"
#endif
        :
        : [alo] "s"(a.lo), [ahi] "s"(a.hi), [arec] "s"(a.rec), [blo] "s"(b.lo), [bhi] "s"(b.hi), [brec] "s"(b.rec), [nk] "s"(nk), [sa] "s"(l.sa),
          [sb] "s"(l.sb), [wlds] "s"(l.wlds), [ao] "v"(l.ao), [bo] "v"(l.bo), [fa0] "v"(l.fa0), [fa1] "v"(l.fa1), [fb0] "v"(l.fb0), [fb1] "v"(l.fb1), [sp] "v"(sp)
#ifdef TALL_STAMPS
          , [dbg] "s"(dbg)
#endif
        :
#include "gemm_tall_384x256_clobbers.inc"
    );
    // (the stream ends behind a barrier: every wave is done with the K-tile slots. From here on a wave touches its own WAVE_LDS bytes only.)
    ASM_EPI_STAMPS;
    ASM_EPI_STAMP(0);
    const unsigned scr_lane = (unsigned)(wave * WAVE_LDS + asm_scratch_lane<WN>(lane));
    const int gn = n0 + wc * WN + (lane % AsmGroup<WN>::LPR) * 4;
    const GemmEpilogue& ep = g.ep;
    const f32x4 bias = asm_column_bias(ep.bias_n, gn);
    const bool specialised = asm_plain_dispatch(__builtin_amdgcn_readfirstlane(asm_plain_variant(ep)), [&](auto act_c, auto outs_c) {
        const auto st = asm_row_store<WN, decltype(act_c)::value, decltype(outs_c)::value, true>(ep.out_bf16, ep.ld_bf16, ep.out_f32, ep.ld_f32, lane,
                                                                                                 m0 + wr * WM, gn, bias);
        static_for<0, 6>([&](auto ord_c) {
            constexpr int grp = (decltype(ord_c)::value + 4) % 6;  // 4, 5, 0, 1, 2, 3
            const float* scr = (const float*)(smem + wave * WAVE_LDS + (grp == 5 ? 32 * WN * 4 : 0));
            if constexpr (grp < 4) {
#include "gemm_tall_384x256_dump.inc"
            }
            ASM_EPI_STAMP(1 + 2 * decltype(ord_c)::value);
            asm_store_rows<WN>(scr, lane, st.after(grp * AsmGroup<WN>::NITG));
            ASM_EPI_STAMP(2 + 2 * decltype(ord_c)::value);
        });
    });
    if (!specialised)
        static_for<0, 6>([&](auto ord_c) {
            constexpr int grp = (decltype(ord_c)::value + 4) % 6;  // 4, 5, 0, 1, 2, 3
            const float* scr = (const float*)(smem + wave * WAVE_LDS + (grp == 5 ? 32 * WN * 4 : 0));
            if constexpr (grp < 4) {
#include "gemm_tall_384x256_dump.inc"
            }
            ASM_EPI_STAMP(1 + 2 * decltype(ord_c)::value);
            asm_store_group<WN>(scr, lane, m0 + wr * WM + grp * 32, gn, bias, AsmPlainStore<false>{ep});
            ASM_EPI_STAMP(2 + 2 * decltype(ord_c)::value);
        });
    ASM_EPI_STAMPS_FLUSH(13);
}

}  // namespace

// ---- launchers ----
// the dynamic-LDS attribute of KERNEL once per device, then one workgroup of four waves per tile
template <auto KERNEL, int SMEM, class Args>
static void launch_asm_tile(dim3 grid, const Args& a, hipStream_t stream) {
    static PerDeviceOnce attr_set;
    attr_set.run([&] { HIP_CHECK(hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, SMEM)); });
    hipLaunchKernelGGL(KERNEL, grid, dim3(256), SMEM, stream, a);
    HIP_CHECK(hipGetLastError());
}

// ---- 192 x 256 tiles (gemm_bf16_kernel_dtl, tile_cfg 75) ----
static bool gemm_dtl_takes(const GemmArgs& a) {
    // lda / ldb % 8: the LDS-DMA pieces are 16-byte loads; the epilogue of this kernel has no clip / PixelNorm / tile-window form
    return !a.conv && a.M % 192 == 0 && a.N % 256 == 0 && a.K % 64 == 0 && a.K >= 64 && !a.ep.d2s && !a.ep.out_bf16_t &&
           a.lda % 8 == 0 && a.ldb % 8 == 0 && !a.ep.pn_out && !a.ep.clip01 && a.tile_count == 0 && a.win_rows == 0 &&
           (a.split_k <= 1 || (a.split_ws && a.split_k <= a.K / 64 && (long)a.split_k * a.M * a.N <= a.split_ws_elems));
}
static void launch_dtl(const GemmArgs& a, const GemmOpts& o, hipStream_t stream, const NormAfter* na = nullptr) {
    LTX_REQUIRE(gemm_dtl_takes(a), "gemm: the 192x256 kernel needs a dense A.B^T with M %% 192 == 0, N %% 256 == 0, K %% 64 == 0 (M=%d N=%d K=%d)",
                a.M, a.N, a.K);
    constexpr int smem = (2 * 192 + 3 * 256) * ROW_BYTES;  // two activation slots, three weight slots
    launch_asm_tile<gemm_bf16_kernel_dtl, smem>(dim3((a.M / 192) * (a.N / 256), a.split_k > 1 ? a.split_k : 1), a, stream);
    if (a.split_k > 1) {
        if (na) {
            LTX_REQUIRE(finish_takes_norm(a, *na), "gemm: the fused finish + norm pass needs N = 4096, an RMS norm with modulation and no row maps");
            // rows per workgroup (A/B hook: 1, 2 or 4): one row = 1536 workgroups, six per CU in flight - 34.77 / 34.85 / 35.26 ms per step
            // with 1 / 2 / 4 on one box (the pass loads three streams per row, unlike norm_mod_rows_kernel, where two rows won)
            // R rows need M % R == 0 and R | rows_per_batch of both the norm and the gate (a group must not straddle two batch elements,
            // and dim3(M / R) must cover every row): anything else falls back to one row per workgroup (round-4 verdict, Weak 9)
            int fr = o.finish_rows;
            if ((fr != 2 && fr != 4) || a.M % fr != 0 || na->rows_per_batch % fr != 0 || (a.ep.gate && a.ep.rows_per_batch % fr != 0)) fr = 1;
            if (fr == 1) hipLaunchKernelGGL(splitk_finish_norm_kernel<1>, dim3(a.M), dim3(256), 0, stream, a.split_ws, a.split_k, a.M, a.ep, *na, a.split_bf16);
            else if (fr == 4)
                hipLaunchKernelGGL(splitk_finish_norm_kernel<4>, dim3(a.M / 4), dim3(256), 0, stream, a.split_ws, a.split_k, a.M, a.ep, *na, a.split_bf16);
            else hipLaunchKernelGGL(splitk_finish_norm_kernel<2>, dim3(a.M / 2), dim3(256), 0, stream, a.split_ws, a.split_k, a.M, a.ep, *na, a.split_bf16);
            HIP_CHECK(hipGetLastError());
        } else {
            launch_splitk_finish(a, a.M, a.ep, a.split_bf16, stream);
        }
    } else {
        LTX_REQUIRE(!na, "gemm: a norm pass can only ride on a split-K finish");
    }
}

// ---- 384 x 256 tiles (gemm_bf16_kernel_tall, tile_cfg 76) ----
// What the kernel can run: a dense A.B^T of whole tiles with bias_n / activation / round_bf16 and plain f32 and/or bf16 stores. The
// 1 << 22 bound keeps every 32-bit buffer offset of a 384-row tile positive.
static bool gemm_tall_fits(const GemmArgs& a) {
    const GemmEpilogue& e = a.ep;
    const long ldmax = 1L << 22;
    return !a.conv && !a.Bq && a.B && a.M > 0 && a.M % 384 == 0 && a.N > 0 && a.N % 256 == 0 && a.K >= 64 && a.K % 64 == 0 && a.lda % 8 == 0 &&
           a.ldb % 8 == 0 && a.lda >= a.K && a.ldb >= a.K && a.lda < ldmax && a.ldb < ldmax && a.split_k <= 1 && a.tile_count == 0 &&
           a.win_rows == 0 && (e.out_f32 || e.out_bf16) && !e.out_bf16_t && !e.bias_m && !e.resid && !e.gate && !e.gate_rowmap &&
           !e.resid_src && !e.d2s && !e.clip01 && !e.pn_out;
}
// ... and what launch_gemm_bf16 sends there instead of the 192 x 256 kernel: launches that are a whole number of rounds of these tiles
// on `ncu` CUs (the FFN-up projection at 1536 / 3072 / 6144 tokens). A ragged round of tiles twice as tall would cost what it saves.
bool gemm_tall_takes(const GemmArgs& a, int ncu) {
    if (!gemm_tall_fits(a) || ncu <= 0) return false;
    const long tiles = (long)(a.M / 384) * (a.N / 256);
    return tiles > 0 && tiles % ncu == 0;
}
static void launch_tall(const GemmArgs& a, hipStream_t stream) {
    LTX_REQUIRE(gemm_tall_fits(a),
                "gemm: the 384x256 kernel needs a dense A.B^T with M %% 384 == 0, N %% 256 == 0, K %% 64 == 0, no split-K and a plain-store "
                "epilogue (bias_n, activation, f32 / bf16 output) (M=%d N=%d K=%d)", a.M, a.N, a.K);
    constexpr int smem = (2 * 384 + 2 * 256) * ROW_BYTES;  // two activation slots, two weight slots: all 160 KB
    launch_asm_tile<gemm_bf16_kernel_tall, smem>(dim3((a.M / 384) * (a.N / 256)), a, stream);
}

// ---- fused q|k + V projection (gemm_bf16_kernel_qkv) ----
bool gemm_qkv_takes(const GemmQkvArgs& a) {
    // ld % 8: the LDS-DMA pieces are 16-byte loads, the q|k store is 8-byte; ldvt % 4: 8-byte V^T stores; rows_per_batch % 192: a row tile
    // lies in one V^T slab; the 1 << 22 bound keeps every 32-bit buffer offset of a 256-row tile positive
    const long ldmax = 1L << 22;
    return a.X && a.Wqk && a.Wv && a.qk && a.vt && a.M > 0 && a.M % 192 == 0 && a.rows_per_batch > 0 && a.rows_per_batch % 192 == 0 &&
           a.M % a.rows_per_batch == 0 && a.Nqk > 0 && a.Nqk % 256 == 0 && a.K >= 64 && a.K % 64 == 0 && a.ldx % 8 == 0 && a.ldwqk % 8 == 0 &&
           a.ldwv % 8 == 0 && a.ld_qk % 8 == 0 && a.ldvt % 4 == 0 && a.ldx >= a.K && a.ldwqk >= a.K && a.ldwv >= a.K && a.ld_qk >= a.Nqk &&
           a.ldvt >= a.rows_per_batch && a.ldx < ldmax && a.ldwqk < ldmax && a.ldwv < ldmax && a.vt_bstride % 4 == 0 &&
           ((uintptr_t)a.X | (uintptr_t)a.Wqk | (uintptr_t)a.Wv) % 16 == 0 && ((uintptr_t)a.qk | (uintptr_t)a.vt) % 8 == 0 &&
           (!a.bias_qk || (uintptr_t)a.bias_qk % 16 == 0);
}
void launch_gemm_qkv(const GemmQkvArgs& a, hipStream_t stream) {
    LTX_REQUIRE(gemm_qkv_takes(a),
                "gemm: the fused q|k + V kernel needs M %% 192 == 0, rows per batch %% 192 == 0, N_qk %% 256 == 0, K %% 64 == 0, leading dimensions %% 8 == 0 "
                "and ldvt %% 4 == 0 (M=%d rows_per_batch=%d N_qk=%d K=%d ldx=%ld ld_qk=%ld ldvt=%ld)",
                a.M, a.rows_per_batch, a.Nqk, a.K, a.ldx, a.ld_qk, a.ldvt);
    ProfScope prof(PROF_GEMM, 2.0 * a.M * ((double)a.Nqk + a.Nqk / 2) * a.K, stream);
    constexpr int smem = (2 * 192 + 2 * 384) * ROW_BYTES;  // two activation slots, two weight slots
    launch_asm_tile<gemm_bf16_kernel_qkv, smem>(dim3((a.M / 192) * (a.Nqk / 256)), a, stream);
}
