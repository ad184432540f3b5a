// gemm_experiments.inc - GEMM structures that were built, measured and NOT selected (DESIGN.md section 4), their launchers and the hooks
// that reach them. Compiled only with -DLTX_EXPERIMENTS (make EXPERIMENTS=1 -> build_exp/libltxhip_exp.so, used by tools/ and the
// `experiments`-marked tests); the product library does not contain them. gemm.hip includes this file twice,
// LTX_GEMM_EXPERIMENTS_PART selects what it gets:
//   1  inside the anonymous namespace, behind the product kernels: the phased 8-wave kernel (tile_cfg 41/42), the one-wave-per-SIMD
//      kernels with generated assembly main loops (71-74), the weight-streaming kernel (90), the few-row kernel (30) and the ring kernel on
//      32x32x16 MFMAs (31)
//   2  in front of launch_cfg: their launchers, the tile cfgs only this build knows (gemm_experiments_cfg) and the environment hooks of a
//      dense launch (gemm_experiments_group_m, gemm_experiments_forced)
#if LTX_GEMM_EXPERIMENTS_PART == 1
// v4: phased "ping-pong" kernel for the wide DiT GEMMs (fused q/k, FFN up): BMx256 output tile (BM = 192 or 256),
// BK = 64, 8 waves as 2(M) x 4(N). The two waves that share a SIMD (wave w and w+4: wave rows 0 and 1) run half a
// phase apart: while one is inside its MFMA cluster (priority 1) the other stages LDS-DMA pieces and waits; two
// workgroup barriers per phase hand the roles over. Per K-tile a wave walks its WMx64 output in four quadrants, each
// re-using one operand half held in registers; the fragments of the NEXT quadrant are read from LDS inside the
// current MFMA cluster (one ds_read per MFMA), so no LDS latency sits between the barriers.
//   even tile: (a0,b0) (a0,b1) (a1,b1) (a1,b0)      odd tile: (a0,b1) (a0,b0) (a1,b0) (a1,b1)   [serpentine: the first
//   quadrant of a tile needs only register sets the last quadrant of the previous tile does not use]
// LDS: 2 slots (K-tile parity) x [A image BM rows | B image 256 rows] x 128 B, rows ordered [half][wave row/col][..]
// so that an operand half is a contiguous row range; 16-B chunk c of LDS row r sits at chunk c ^ ((r >> 1) & 7).
// Staging: one wave-instruction = 8 rows; unit u of an operand = LDS rows [64u, 64u+64) over the 8 waves.
// Hazards (wave group 1 runs one barrier behind group 0; L(p)/M(p) = the load / MFMA section of phase p):
//   RAW: data read in M(p) must have been waited for (vmcnt) in L(p-1) or earlier by every wave.
//   WAR: a buffer last read in M(q) may be re-staged from L(q+2) on.
// Schedule for tile T (Bf/Bs = the B half its first / second quadrant pair needs):
//   staged:  Bf(T) in L(P2(T-2))   Bs(T) in L(P3(T-2))   A half 0 in L(P4(T-2))   A half 1 in L(P1(T-1))
//   read:    A half 0 + Bf(T) in M(P4(T-1))   Bs(T) in M(P1(T))   A half 1 in M(P2(T))
//   waited:  start of L(P3(T-1)): everything but {A half 1 (T), Bf(T+1)} ; start of L(P1(T)): everything but the three
//            groups of tile T+1 staged so far.  The weights (B, HBM-cold in the DiT) get 4-5 phases of flight.
// ---------------------------------------------------------------------------------------------------------------
template <int BM, int BN>
__global__ __launch_bounds__(512) void gemm_bf16_kernel_v4(const GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    static_assert(BN == 256 && (BM == 192 || BM == 256), "v4 tile shapes");
    constexpr int WGM = 2, WGN = 4;
    constexpr int WM = BM / WGM, WN = BN / WGN, MI = WM / 16, NI = WN / 16, MIH = MI / 2, NIH = NI / 2;
    constexpr int A_BYTES = BM * ROW_BYTES, B_BYTES = BN * ROW_BYTES, SLOT = A_BYTES + B_BYTES;
    constexpr int AU = BM / 64, BU = BN / 64;  // staging units (= LDS-DMA instructions per wave) per K-tile
    constexpr int HM = BM / 2, HN = BN / 2, QM = WM / 2, QN = WN / 2;
    // LDS-DMA instructions per wave of the four staging groups
    constexpr int G_BF = 2, G_BS = 2, G_A0 = 2, G_A1 = (BM == 256) ? 2 : 1;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / WGN, wc = wave % WGN;

    const int tiles_m = (g.M + BM - 1) / BM;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    int tm, tn;
    tile_coords(g, bid, tiles_m, BN, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;

    // ---- staging sources: LDS row -> tile row through the [half][wave row][quarter rows] ordering
    const int srow = lane >> 3, pch = lane & 7;
    const bf16_t* a_src[AU];
    const bf16_t* b_src[BU];
#pragma unroll
    for (int u = 0; u < AU; ++u) {
        const int lr = 64 * u + 8 * wave + srow;
        const int h = lr / HM, rem = lr - h * HM, w_ = rem / QM, i = rem - w_ * QM;
        int gm = m0 + w_ * WM + h * QM + i;
        gm = gm < g.M ? gm : g.M - 1;
        a_src[u] = g.A + (long)gm * g.lda + ((pch ^ ((lr >> 1) & 7)) << 3);
    }
#pragma unroll
    for (int u = 0; u < BU; ++u) {
        const int lr = 64 * u + 8 * wave + srow;
        const int h = lr / HN, rem = lr - h * HN, w_ = rem / QN, j = rem - w_ * QN;
        int gn = n0 + w_ * WN + h * QN + j;
        gn = gn < g.N ? gn : g.N - 1;
        b_src[u] = g.B + (long)gn * g.ldb + ((pch ^ ((lr >> 1) & 7)) << 3);
    }
    auto stage_a = [&](int slot, int u, int kt) {
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a_src[u] + (long)kt * BK),
                                         (__attribute__((address_space(3))) void*)(smem + slot * SLOT + (8 * u + wave) * 1024),
                                         16, 0, 0);
    };
    auto stage_b = [&](int slot, int u, int kt) {
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(b_src[u] + (long)kt * BK),
                                         (__attribute__((address_space(3))) void*)(smem + slot * SLOT + A_BYTES + (8 * u + wave) * 1024),
                                         16, 0, 0);
    };
    // B half h = units 2h, 2h+1. A half 0 = units 0,1 (BM=256) / 0 and the first half of 1 (BM=192: unit 1 straddles);
    // A half 1 = units 2,3 / 2. The straddling unit is staged with half 0: its half-1 rows are free by then (last read M(P2)).
    auto stage_bh = [&](int slot, int h, int kt) { stage_b(slot, 2 * h, kt); stage_b(slot, 2 * h + 1, kt); };
    auto stage_a0 = [&](int slot, int kt) { stage_a(slot, 0, kt); stage_a(slot, 1, kt); };
    auto stage_a1 = [&](int slot, int kt) {
        stage_a(slot, 2, kt);
        if constexpr (BM == 256) stage_a(slot, 3, kt);
    };

    // ---- fragment reads
    const int frow = lane & 15, fsw = (lane >> 1) & 7;
    const int fch0 = (((lane >> 4) + 0) ^ fsw) << 4, fch1 = (((lane >> 4) + 4) ^ fsw) << 4;
    const int a_off = (wr * QM + frow) * ROW_BYTES;            // + h*HM*128 + i*16*128 + chunk
    const int b_off = A_BYTES + (wc * QN + frow) * ROW_BYTES;  // + h*HN*128 + j*16*128 + chunk

    f32x4 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    s16x8 fa0[MIH][2], fa1[MIH][2], fb0[NIH][2], fb1[NIH][2];

    auto read_a = [&](int slot, int h, s16x8(&fa)[MIH][2]) {
        const char* base = smem + slot * SLOT + a_off + h * HM * ROW_BYTES;
#pragma unroll
        for (int i = 0; i < MIH; ++i) {
            fa[i][0] = *(const s16x8*)(base + i * 16 * ROW_BYTES + fch0);
            fa[i][1] = *(const s16x8*)(base + i * 16 * ROW_BYTES + fch1);
        }
    };
    auto read_b = [&](int slot, int h, s16x8(&fb)[NIH][2]) {
        const char* base = smem + slot * SLOT + b_off + h * HN * ROW_BYTES;
#pragma unroll
        for (int j = 0; j < NIH; ++j) {
            fb[j][0] = *(const s16x8*)(base + j * 16 * ROW_BYTES + fch0);
            fb[j][1] = *(const s16x8*)(base + j * 16 * ROW_BYTES + fch1);
        }
    };
    // MFMA section of one phase: quadrant (hm, hn) from the given register sets; `reads()` issues the ds_reads of the next
    // quadrant's missing operand(s) (NR of them), interleaved one per MFMA behind the first product.
    auto cluster = [&](auto hm_tag, auto hn_tag, const s16x8(&fa)[MIH][2], const s16x8(&fb)[NIH][2], auto nr_tag, auto&& reads) {
        constexpr int hm = decltype(hm_tag)::value, hn = decltype(hn_tag)::value, NR = decltype(nr_tag)::value;
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
        acc[hm * MIH][hn * NIH] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, fa[0][0]),
                                                                           __builtin_bit_cast(bf16x8_t, fb[0][0]), acc[hm * MIH][hn * NIH], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        reads();
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int i = 0; i < MIH; ++i)
#pragma unroll
                for (int j = 0; j < NIH; ++j)
                    if (ks + i + j > 0)
                        acc[hm * MIH + i][hn * NIH + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                            __builtin_bit_cast(bf16x8_t, fa[i][ks]), __builtin_bit_cast(bf16x8_t, fb[j][ks]),
                            acc[hm * MIH + i][hn * NIH + j], 0, 0, 0);
        constexpr int NM = 2 * MIH * NIH - 1;
        constexpr int NI_ = NR < NM ? NR : NM;
#pragma unroll
        for (int q = 0; q < NI_; ++q) {
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // one ds_read
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // one MFMA
        }
        __builtin_amdgcn_sched_group_barrier(0x008, NM - NI_, 0);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(0);
        raw_barrier();
        __builtin_amdgcn_sched_barrier(0);
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    using RA = std::integral_constant<int, 2 * MIH>;            // reads of one A half
    using RB = std::integral_constant<int, 2 * NIH>;            // reads of one B half
    using RAB = std::integral_constant<int, 2 * MIH + 2 * NIH>;
    auto no_reads = [] {};

    const int nk = g.K / BK;  // >= 2 (launcher)
    // prologue: tile 0 complete; tile 1: Bf = B half 1, Bs = B half 0, A half 0 (its A half 1 is staged in P1 of tile 0)
    stage_bh(0, 0, 0); stage_bh(0, 1, 0); stage_a0(0, 0); stage_a1(0, 0);
    stage_bh(1, 1, 1); stage_bh(1, 0, 1); stage_a0(1, 1);
    wait_vmcnt_barrier<G_BF + G_BS + G_A0>();
    read_a(0, 0, fa0);
    read_b(0, 0, fb0);
    if (wr == 1) raw_barrier();  // wave row 1 runs one barrier behind wave row 0 from here on

    // One K-tile = four phases; PAR = tile parity (slot, quadrant order). MODE 0: tile t+2 exists (full staging);
    // 1: t+1 is the last tile; 2: t is the last tile.
    auto ktile = [&](int t, auto par_tag, auto mode_tag) {
        constexpr int S = decltype(par_tag)::value, MODE = decltype(mode_tag)::value;
        constexpr int FH = S;      // B half of the tile's first quadrant pair (even tile: 0, odd tile: 1)
        constexpr int SH = S ^ 1;  // B half of the second pair
        auto& fbf = (FH == 0) ? fb0 : fb1;  // registers of Bf / Bs
        auto& fbs = (FH == 0) ? fb1 : fb0;
        // ---- P1: (a0, Bf); next quadrant needs Bs
        if constexpr (MODE <= 1) {
            wait_lgkm_vmcnt<G_BF + G_BS + G_A0>();  // A half 1 of this tile has landed (for every wave after the barrier)
            stage_a1(S ^ 1, t + 1);
        } else {
            wait_lgkm_vmcnt<0>();
        }
        raw_barrier();
        cluster(I0{}, std::integral_constant<int, FH>{}, fa0, fbf, RB{}, [&] { read_b(S, SH, fbs); });
        // ---- P2: (a0, Bs); next quadrant needs a1
        if constexpr (MODE == 0) stage_bh(S, (S == 0) ? 0 : 1, t + 2);  // Bf(t+2): same parity -> same half as this tile's Bf
        wait_lgkm_barrier();
        cluster(I0{}, std::integral_constant<int, SH>{}, fa0, fbs, RA{}, [&] { read_a(S, 1, fa1); });
        // ---- P3: (a1, Bs); nothing new to read for P4 = (a1, Bf)
        if constexpr (MODE == 0) {
            wait_lgkm_vmcnt<G_A1 + G_BF>();  // A half 0 and Bf of tile t+1 have landed
            stage_bh(S, (S == 0) ? 1 : 0, t + 2);  // Bs(t+2)
        } else {
            wait_lgkm_vmcnt<0>();
        }
        raw_barrier();
        cluster(I1{}, std::integral_constant<int, SH>{}, fa1, fbs, I0{}, no_reads);
        // ---- P4: (a1, Bf); next tile's first quadrant needs a0 and ITS Bf (= the half this tile calls Bs)
        if constexpr (MODE == 0) stage_a0(S, t + 2);
        wait_lgkm_barrier();
        if constexpr (MODE <= 1)
            cluster(I1{}, std::integral_constant<int, FH>{}, fa1, fbf, RAB{}, [&] { read_a(S ^ 1, 0, fa0); read_b(S ^ 1, SH, fbs); });
        else
            cluster(I1{}, std::integral_constant<int, FH>{}, fa1, fbf, I0{}, no_reads);
    };
    int t = 0;
    for (; t + 3 < nk; t += 2) {
        ktile(t, I0{}, I0{});
        ktile(t + 1, I1{}, I0{});
    }
    // 2 or 3 tiles left, t even
    if (t + 3 == nk) {
        ktile(t, I0{}, I0{});
        ktile(t + 1, I1{}, I1{});
        ktile(t + 2, I0{}, I2{});
    } else {
        ktile(t, I0{}, I1{});
        ktile(t + 1, I1{}, I2{});
    }
    if (wr == 0) raw_barrier();  // re-align the two wave rows
    __syncthreads();
    gemm_epilogue<BM, BN, WGM, WGN>(acc, g, m0, n0, wr, wc, lane, wave, smem);
}

// ---------------------------------------------------------------------------------------------------------------
// One wave per SIMD, assembly main loop (generated by tools/gen_gemm_asm.py; schedule and register map in that script's header).
// Workgroup tile 192 x 256, four waves as 2 x 2 (96 x 128 per wave), dense A.B^T only, M % 192 == 0, N % 256 == 0, K % 64 == 0.
// C++ prepares the per-lane offsets / LDS addresses (the ring kernel's LDS image) and runs the shared epilogue on the accumulators
// the assembly leaves in a[0:191].
// ---------------------------------------------------------------------------------------------------------------
template <int BN, int RING = 0>  // RING: 0 register-staged (71/72), 1 LDS-DMA ring (73), 2 A through the ring + B straight to registers (74)
__global__ __launch_bounds__(256, 1) void gemm_bf16_kernel_asm(const GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    static_assert(BN == 256 || BN == 128, "generated main loops exist for 192x256 and 192x128");
    static_assert(RING == 0 || BN == 128, "the LDS-DMA ring variants exist for 192x128");
    constexpr int BM = 192, WGM = 2, WGN = 2, NW = 4;
    constexpr int WM = BM / WGM, WN = BN / WGN, MI = WM / 16, NI = WN / 16;
    constexpr int A_BYTES = BM * ROW_BYTES;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / WGN, wc = wave % WGN;
    const int tiles_m = g.M / BM;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    int tm, tn;
    tile_coords(g, bid, tiles_m, BN, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;
    // piece i of this wave = rows (wave + 4 i) * 8 .. +7 of the tile: the per-lane part of its address (row inside the piece, swizzled
    // 16-byte column) does not depend on i ((row >> 1) & 7 is the same for rows 32 apart), the i part is a scalar offset
    const int srow = lane >> 3, pch = lane & 7;
    const int row0 = wave * 8 + srow;
    const int ao = (row0 * (int)g.lda + ((pch ^ ((row0 >> 1) & 7)) << 3)) * 2;
    const int bo = (row0 * (int)g.ldb + ((pch ^ ((row0 >> 1) & 7)) << 3)) * 2;
    const uint32_t sa = (uint32_t)(32 * g.lda * 2), sb = (uint32_t)(32 * g.ldb * 2);
    const bf16_t* At = g.A + (long)m0 * g.lda;
    const bf16_t* Bt = g.B + (long)n0 * g.ldb;
    const uint32_t alo = (uint32_t)(uintptr_t)At, ahi = (uint32_t)((uintptr_t)At >> 32);
    const uint32_t blo = (uint32_t)(uintptr_t)Bt, bhi = (uint32_t)((uintptr_t)Bt >> 32);
    const uint32_t arec = (uint32_t)(((long)(BM - 1) * g.lda + g.K) * 2), brec = (uint32_t)(((long)(BN - 1) * g.ldb + g.K) * 2);
    const uint32_t nk = (uint32_t)(g.K / BK);
    const int wb = wave * 1024 + lane * 16;
    const int frow = lane & 15, fsw = (lane >> 1) & 7;
    const int foff0 = frow * ROW_BYTES + ((((lane >> 4) + 0) ^ fsw) << 4);
    const int foff1 = frow * ROW_BYTES + ((((lane >> 4) + 4) ^ fsw) << 4);
    const int a_wave_off = (wr * WM) * ROW_BYTES, b_wave_off = A_BYTES + (wc * WN) * ROW_BYTES;
    const int fa0 = a_wave_off + foff0, fa1 = a_wave_off + foff1, fb0 = b_wave_off + foff0, fb1 = b_wave_off + foff1;
#ifdef GEMM_ASM_STAMPS  // tools/ubench/gemm_stamps.hip
    unsigned long long* dbg = (blockIdx.x == 7) ? &g_gemm_stamps[wave][0] : &g_gemm_stamps[4][0];
    const unsigned long long t_before = __builtin_readcyclecounter();
#endif
#define GEMM_ASM_OPERANDS                                                                                                           \
    [alo] "s"(alo), [ahi] "s"(ahi), [arec] "s"(arec), [blo] "s"(blo), [bhi] "s"(bhi), [brec] "s"(brec), [nk] "s"(nk), [sa] "s"(sa), \
        [sb] "s"(sb), [ao] "v"(ao), [bo] "v"(bo), [wb] "v"(wb), [fa0] "v"(fa0), [fa1] "v"(fa1), [fb0] "v"(fb0), [fb1] "v"(fb1)
    if constexpr (RING == 2) {
        // tile_cfg 74: A by LDS-DMA into four 24 KB slots, B never touches LDS: each lane loads its 16 bytes of every B fragment
        // (row 16 ni + (lane & 15) of this wave's 64 columns, k = 8 (lane >> 4) ..+7 of the k-step) four K-tiles ahead
        // (tools/gen_gemm_asm_ring.py --bdirect)
        const uint32_t wlds = (uint32_t)wave * 1024u;
#ifdef GEMM_HYBRID_PACKED_TIMING  // tools/ubench/gemm_stamps.hip: address pattern of fragment-ordered weights (timing only, wrong results)
        const int bfo = wc * 8192 + lane * 16;
        const uint32_t sb16 = 2048u;
#else
        const int bfo = ((wc * WN + (lane & 15)) * (int)g.ldb + 8 * (lane >> 4)) * 2;
        const uint32_t sb16 = (uint32_t)(16 * g.ldb * 2);
#endif
        asm volatile(
#ifdef GEMM_HYBRID_PACKED_TIMING
#include "gemm_asm_hybrid_192x128_stamps.inc"
#else
#include "gemm_asm_hybrid_192x128.inc"
#endif
            :
            : [alo] "s"(alo), [ahi] "s"(ahi), [arec] "s"(arec), [blo] "s"(blo), [bhi] "s"(bhi), [brec] "s"(brec), [nk] "s"(nk),
              [sa] "s"(sa), [sb16] "s"(sb16), [wlds] "s"(wlds), [ao] "v"(ao), [bfo] "v"(bfo), [fa0] "v"(fa0), [fa1] "v"(fa1)
            :
#include "gemm_asm_hybrid_192x128_clobbers.inc"
        );
    } else if constexpr (RING == 1) {
        // tile_cfg 73: the same wave tile, K-tiles staged by LDS-DMA into four 40 KB slots (tools/gen_gemm_asm_ring.py)
        const uint32_t wlds = (uint32_t)wave * 1024u;
        asm volatile(
#ifdef GEMM_ASM_STAMPS
#include "gemm_asm_ring_192x128_stamps.inc"
#else
#include "gemm_asm_ring_192x128.inc"
#endif
            :
            : [alo] "s"(alo), [ahi] "s"(ahi), [arec] "s"(arec), [blo] "s"(blo), [bhi] "s"(bhi), [brec] "s"(brec), [nk] "s"(nk),
              [sa] "s"(sa), [sb] "s"(sb), [wlds] "s"(wlds), [ao] "v"(ao), [bo] "v"(bo), [fa0] "v"(fa0), [fa1] "v"(fa1),
              [fb0] "v"(fb0), [fb1] "v"(fb1)
#ifdef GEMM_ASM_STAMPS
              , [dbg] "s"(dbg)
#endif
            :
#include "gemm_asm_ring_192x128_clobbers.inc"
        );
    } else if constexpr (BN == 256) {
        asm volatile(
#ifdef GEMM_ASM_STAMPS
#include "gemm_asm_192x256_stamps.inc"
#else
#include "gemm_asm_192x256.inc"
#endif
            :
            : GEMM_ASM_OPERANDS
#ifdef GEMM_ASM_STAMPS
              , [dbg] "s"(dbg)
#endif
            :
#include "gemm_asm_192x256_clobbers.inc"
        );
    } else {
        asm volatile(
#include "gemm_asm_192x128.inc"
            :
            : GEMM_ASM_OPERANDS
            :
#include "gemm_asm_192x128_clobbers.inc"
        );
    }
#undef GEMM_ASM_OPERANDS
#ifdef GEMM_ASM_STAMPS
    const unsigned long long t_after = __builtin_readcyclecounter();
#endif
    __syncthreads();  // every wave is done with the K-tile slots before the epilogue scratch reuses them
    // Epilogue: 32 rows x WN columns at a time through the wave's LDS scratch (assembly dump, see the generator), then a rolled loop:
    // one 16-byte column group per lane, 256 / WN rows per iteration.
    constexpr int LPR = WN / 4, RPI = 64 / LPR;  // lanes per row, rows per iteration
    float* scr = (float*)(smem + wave * (32 * WN * 4));
    // LDS byte address of this lane's first scratch element (the dynamic LDS of this kernel starts at 0, as the main loop assumes)
    const unsigned scr_lane = (unsigned)(wave * (32 * WN * 4) + ((((lane >> 4) * 4) * WN + (lane & 15)) * 4));
    const GemmEpilogue& ep = g.ep;
    const int gn = n0 + wc * WN + (lane % LPR) * 4;
    const f32x4 bias = ep.bias_n ? *(const f32x4*)(ep.bias_n + gn) : f32x4{0.f, 0.f, 0.f, 0.f};
    const float* rbase = ep.resid_src ? ep.resid_src : ep.out_f32;
    const long rld = ep.resid_src ? ep.ld_resid : ep.ld_f32;
    static_for<0, 3>([&](auto grp_c) {
        constexpr int grp = decltype(grp_c)::value;
        if constexpr (BN == 256) {
#include "gemm_asm_192x256_dump.inc"
        } else {
#include "gemm_asm_192x128_dump.inc"
        }
#pragma unroll 2
        for (int it = 0; it < 32 / RPI; ++it) {
            const int row = it * RPI + lane / LPR;
            const int gm = m0 + wr * WM + grp * 32 + row;
            f32x4 v = *(const f32x4*)(scr + row * WN + (lane % LPR) * 4);
            v += bias;
            if (ep.bias_m) {
                const float bm = ep.bias_m[gm];
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
            if (ep.resid) {
                const f32x4 rs = *(const f32x4*)(rbase + (long)gm * rld + gn);
                f32x4 gt = f32x4{ep.gate_scalar, ep.gate_scalar, ep.gate_scalar, ep.gate_scalar};
                if (ep.gate) gt = *(const f32x4*)(ep.gate + (long)(ep.gate_rowmap ? ep.gate_rowmap[gm] : gm / ep.rows_per_batch) * ep.gate_bstride + gn);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = rs[e] + gt[e] * v[e];
            }
            if (ep.out_f32) *(f32x4*)(ep.out_f32 + (long)gm * ep.ld_f32 + gn) = v;
            if (ep.out_bf16) {
                uint2 pk;
                pk.x = pack_bf16x2(v[0], v[1]);
                pk.y = pack_bf16x2(v[2], v[3]);
                *(uint2*)(ep.out_bf16 + (long)gm * ep.ld_bf16 + gn) = pk;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the scratch is rewritten by the next dump
    });
#ifdef GEMM_ASM_STAMPS
    if (blockIdx.x == 7 && lane == 0) {
        g_gemm_stamps[wave][6] = t_after - t_before;
        g_gemm_stamps[wave][7] = __builtin_readcyclecounter() - t_after;
    }
#endif
}

template <int BM, int BN>
void launch_v4(const GemmArgs& a, hipStream_t stream) {
    constexpr int smem = 2 * (BM + BN) * ROW_BYTES;
    static_assert(smem >= 8 * 16 * (BN / 4) * 4, "epilogue scratch must fit in the ring");
    static PerDeviceOnce attr_set;
    attr_set.run([&] {
        HIP_CHECK(hipFuncSetAttribute((const void*)gemm_bf16_kernel_v4<BM, BN>, hipFuncAttributeMaxDynamicSharedMemorySize, smem));
    });
    LTX_REQUIRE(!a.conv, "gemm v4: dense operands only");
    LTX_REQUIRE(a.K % BK == 0 && a.K >= 2 * BK, "gemm v4: K=%d must be a multiple of %d and >= %d", a.K, BK, 2 * BK);
    const int tiles = ((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN);
    hipLaunchKernelGGL((gemm_bf16_kernel_v4<BM, BN>), dim3(tiles), dim3(512), smem, stream, a);
    HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------------------------
// Weight-streaming GEMM for few rows (M <= 128; tile_cfg 90): C[M][N] = A[M][K] . W[N][K]^T with W read ONCE across the chip.
// At 128 tokens the DiT is HBM-bound (26 GB of weights, 6 TFLOP): what matters is bytes in flight per CU and that no weight byte is
// fetched twice, not MFMA issue. Workgroup = 128 rows x 64 columns x a K range; its four waves split the K-tiles of that range
// (wave w takes tiles w, w+4, ...), each wave holds the FULL 128 x 64 tile in 32 accumulators and loads its operands straight from
// global memory into MFMA fragment registers - no LDS on the way in, two K-tiles (48 KB per wave, 192 KB per CU) in flight.
// Fragment addressing: a lane (r = lane & 15, q = lane >> 4) reads 16 consecutive k of row r per K-tile, k = 64 kt + 16 q + [0,16):
// the first 8 feed k-step 0, the last 8 k-step 1. That is a permutation of the K-tile's 64 k against the usual fragment order,
// applied to A and W alike, so the products are the same set; a wave instruction then covers 16 rows x 128 contiguous bytes (bf16)
// or 16 x 64 (8-bit codes): whole lines, where the usual order touches half lines. QBITS = 8: W arrives as 8-bit codes + bf16
// group scale / bias (group = 64 along K = one K-tile) and is de-quantised in registers, w' = bf16(q * scale + bias) - half the
// HBM bytes of the bf16 matrix. The four waves' partial tiles are summed through LDS in wave order (deterministic), wave w then
// owns rows [32 w, 32 w + 32) and runs the shared epilogue; a K split over workgroups (grid.y) goes through the same workspace +
// finish pass as the ring kernel's.
// ---------------------------------------------------------------------------------------------------------------
template <int QBITS>
__global__ __launch_bounds__(256, 1) void gemm_stream_kernel(const GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int BM = 128, BN = 64, MI = 8, NI = 4;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int n0 = blockIdx.x * BN;
    int nk = g.K / BK, kt0 = 0;
    if (g.split_k > 1) {
        const int z = blockIdx.y;
        kt0 = (int)((long)nk * z / g.split_k);
        nk = (int)((long)nk * (z + 1) / g.split_k) - kt0;
    }
    const int my = (nk - wave + 3) / 4;  // K-tiles of this wave: kt0 + wave + 4 i
    // per-lane row bases (rows past M / N are clamped: their products are never stored)
    const bf16_t* arow[MI];
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        int m = i * 16 + r;
        m = m < g.M ? m : g.M - 1;
        arow[i] = g.A + (long)m * g.lda + q * 16;
    }
    long brow[NI];  // element offset of (row, k = 16 q) in W
    int bn[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
        int n = n0 + j * 16 + r;
        n = n < g.N ? n : g.N - 1;
        bn[j] = n;
        brow[j] = (long)n * g.ldb + q * 16;
    }
    f32x4 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    struct Stage {
        s16x8 a[MI][2];
        s16x8 b[NI][2];   // QBITS == 16: the fragments; QBITS == 8: b[j][0] holds the 16 codes of the K-tile (raw)
        float sc[NI], bi[NI];
    };
    auto load = [&](Stage& st, int kt) {
        const long ko = (long)kt * BK;
#pragma unroll
        for (int j = 0; j < NI; ++j) {   // the weights first: they are the HBM-cold operand
            if constexpr (QBITS == 16) {
                st.b[j][0] = *(const s16x8*)(g.B + brow[j] + ko);
                st.b[j][1] = *(const s16x8*)(g.B + brow[j] + ko + 8);
            } else {
                st.b[j][0] = *(const s16x8*)(g.Bq + brow[j] + ko);
                st.sc[j] = bf16_to_f32(g.Bqs[(long)bn[j] * (g.K / BK) + kt]);
                st.bi[j] = bf16_to_f32(g.Bqb[(long)bn[j] * (g.K / BK) + kt]);
            }
        }
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            st.a[i][0] = *(const s16x8*)(arow[i] + ko);
            st.a[i][1] = *(const s16x8*)(arow[i] + ko + 8);
        }
    };
    auto compute = [&](Stage& st) {
        if constexpr (QBITS == 8) {
#pragma unroll
            for (int j = 0; j < NI; ++j) {
                const uint4 raw = __builtin_bit_cast(uint4, st.b[j][0]);
                const uint32_t wd[4] = {raw.x, raw.y, raw.z, raw.w};
                uint32_t o[8];
#pragma unroll
                for (int w = 0; w < 4; ++w)
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const float q0 = (float)((wd[w] >> (16 * h)) & 0xffu), q1 = (float)((wd[w] >> (16 * h + 8)) & 0xffu);
                        o[w * 2 + h] = pack_bf16x2(q0 * st.sc[j] + st.bi[j], q1 * st.sc[j] + st.bi[j]);
                    }
                st.b[j][0] = __builtin_bit_cast(s16x8, uint4{o[0], o[1], o[2], o[3]});
                st.b[j][1] = __builtin_bit_cast(s16x8, uint4{o[4], o[5], o[6], o[7]});
            }
        }
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, st.a[i][s]),
                                                                        __builtin_bit_cast(bf16x8_t, st.b[j][s]), acc[i][j], 0, 0, 0);
    };
    // two K-tiles of this wave in flight: ping-pong between two named register stages (static indexing only)
    Stage s0, s1;
    const int kbase = kt0 + wave;
    if (my > 0) load(s0, kbase);
    int i = 0;
    for (; i + 1 < my; i += 2) {
        load(s1, kbase + 4 * (i + 1));
        compute(s0);
        if (i + 2 < my) load(s0, kbase + 4 * (i + 2));
        compute(s1);
    }
    if (i < my) compute(s0);

    // sum the four waves' tiles in wave order; wave w keeps row blocks 2w, 2w+1
    f32x4* red = (f32x4*)smem;  // [wave][mi][ni][lane]
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) red[((wave * MI + mi) * NI + ni) * 64 + lane] = acc[mi][ni];
    __syncthreads();
    f32x4 out[2][NI];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
            f32x4 v = red[((0 * MI + 2 * wave + h) * NI + ni) * 64 + lane];
#pragma unroll
            for (int w = 1; w < 4; ++w) v += red[((w * MI + 2 * wave + h) * NI + ni) * 64 + lane];
            out[h][ni] = v;
        }
    __syncthreads();  // the epilogue's transpose scratch reuses this LDS
    if (g.split_k > 1) {
        GemmArgs gs = g;  // raw partial tile -> workspace slice of this split
        gs.ep = GemmEpilogue{};
        gs.ep.out_f32 = g.split_ws + (long)blockIdx.y * g.M * g.N;
        gs.ep.ld_f32 = g.N;
        gemm_epilogue<BM, BN, 4, 1>(out, gs, 0, n0, wave, 0, lane, wave, smem);
        return;
    }
    gemm_epilogue<BM, BN, 4, 1>(out, g, 0, n0, wave, 0, lane, wave, smem);
}


// ---------------------------------------------------------------------------------------------------------------
// Few-row launches (M <= 128: the DiT at 256x256x9 = 128 tokens), round 3. Such a GEMM streams its weights once and is bound by
// how many bytes a CU keeps in flight against the HBM latency, not by MFMAs (16 per wave and K-tile). The ring kernel above stages
// activations and weights through ONE ring with one in-order counter: three K-tiles = 72 KB in flight, two thirds of them the
// activation tile, which comes from L2 and needs no such cover. Here the two operands have rings of their own and waves of their own:
//   waves 0, 1 stage the activation tile (128 x 64 bf16 = 16 pieces) two K-tiles ahead: 3 slots, 48 KB;
//   waves 2, 3 stage the weights in MACRO-tiles of four K-tiles, two macro-tiles ahead: a piece is 2 rows x 512 contiguous bytes
//              (8 rows x 128 B pieces fetch a quarter of a DRAM page per row visit: the ring kernel streams weights at ~3 TB/s);
//              3 slots of 32 KB - or, QB, the 8-bit codes of a quantised Linear: pieces of 4 rows x 256 B, 4 slots of 16 KB, three
//              macro-tiles ahead, plus the group scales / biases of the macro-tile (two dwords per row and wave);
// each role waits on its own vmcnt (the counter is per wave), one workgroup barrier per K-tile publishes both. All four waves run the
// MFMAs (wave tile 64 x 32). QB: the codes of tile t+1 are converted to the bf16 image (two slots) during K-tile t, w' = bf16(q * scale
// + bias) - quant_decode_kernel's arithmetic, bit-identical to the scratch path - so a quantised few-row GEMM reads half the bytes.
// Split-K (grid.y) and the epilogue are the ring kernel's.
// MEASURED, NOT SELECTED (tile_cfg 30, experiments build): bit-exact (tests/test_experiments_gpu.py), and 9 % SLOWER than the 128x64
// ring kernel at 128 tokens - 22.9 / 25.9 / 45.0 us against 20.95 / 23.3 / 41.1 us for the N = 4096 / 8192 / 16384 launches of a block
// (rocprofv3, profiles/r03_config1_fewrow.txt); forward 12.7 against 11.9 ms. Both kernels stream the weights at ~3 TB/s whatever the
// run length per DRAM row (128 B or 512 B). The activation tile's re-fetch (16 KB per K-tile from L2 beside 8 KB of weights) was this
// kernel's premise and is NOT the bound: 16-row launches of the ring kernel are only 7 % faster than 128-row ones
// (profiles/r03_fewrow_bounds.txt); a six-slot ring there gained 5 % and is what the product now runs.
// ---------------------------------------------------------------------------------------------------------------
template <int N>
LTX_DEVFN void wait_vmcnt_only() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// s_waitcnt vmcnt(n) for a run-time n (immediates only): n is wave-uniform, <= 45
LTX_DEVFN void wait_vmcnt_dyn(int n) {
    switch (n) {
#define LTX_W(K) case K: wait_vmcnt_only<K>(); break;
        LTX_W(0) LTX_W(1) LTX_W(2) LTX_W(3) LTX_W(4) LTX_W(5) LTX_W(6) LTX_W(7) LTX_W(8) LTX_W(9) LTX_W(10) LTX_W(11) LTX_W(12) LTX_W(13) LTX_W(14)
        LTX_W(15) LTX_W(16) LTX_W(17) LTX_W(18) LTX_W(19) LTX_W(20) LTX_W(21) LTX_W(22) LTX_W(23) LTX_W(24) LTX_W(25) LTX_W(26) LTX_W(27) LTX_W(28)
        LTX_W(29) LTX_W(30) LTX_W(31) LTX_W(32) LTX_W(33) LTX_W(34) LTX_W(35) LTX_W(36) LTX_W(37) LTX_W(38) LTX_W(39) LTX_W(40) LTX_W(41) LTX_W(42)
        LTX_W(43) LTX_W(44) LTX_W(45)
#undef LTX_W
        default: wait_vmcnt_only<0>(); break;
    }
}

template <bool QB>
__global__ __launch_bounds__(256, 1) void gemm_fewrow_kernel(const GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int BM = 128, BN = 64, WGM = 2, WGN = 2, WM = 64, WN = 32, MI = 4, NI = 2;
    constexpr int A_BYTES = BM * ROW_BYTES, B_BYTES = BN * ROW_BYTES;
    constexpr int NA = 3, PA = NA - 1;                       // activation ring (K-tiles)
    constexpr int MT = 4;                                    // K-tiles per weight macro-tile: 256 elements = 512 B (256 B of codes) of a row
    constexpr int NBM = QB ? 4 : 3, PBM = NBM - 1;           // weight ring (macro-tiles)
    constexpr int BM_BYTES = QB ? BN * MT * 64 : BN * MT * ROW_BYTES;   // 16 KB of codes / 32 KB of bf16 weights
    constexpr int SB_BYTES = 1024;                           // QB: [scale dword 0][scale dword 1][bias dword 0][bias dword 1] x 64 rows
    constexpr int A_OFF = 0, B_OFF = NA * A_BYTES;           // bf16 macro ring, or (QB) the two-slot bf16 image of single K-tiles
    constexpr int Q_OFF = B_OFF + 2 * B_BYTES, SB_OFF = Q_OFF + NBM * BM_BYTES;
    constexpr int APW = 8;                                   // LDS-DMA pieces per K-tile of an activation wave
    constexpr int BPW = QB ? 10 : 16;                        // ... per MACRO-tile of a weight wave
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / WGN, wc = wave % WGN;
    const bool a_role = wave < 2;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int n0 = bid * BN, m0 = 0;
    int nk = g.K / BK, kt0 = 0;
    const int groups = g.K / BK;
    if (g.split_k > 1) {  // the launcher guarantees whole macro-tiles per split
        const int z = blockIdx.y;
        kt0 = (int)((long)nk * z / g.split_k);
        nk = (int)((long)nk * (z + 1) / g.split_k) - kt0;
    }
    const int nm = nk / MT;  // macro-tiles of this workgroup
    // ---- staging sources ----
    const bf16_t* asrc[APW];
    const char* bsrc = nullptr;   // weight wave: this lane's 16 bytes of piece 0 of macro-tile 0; piece i is `bstep` rows further down
    long bstep = 0;
    const bf16_t* sbsrc = nullptr;
    if (a_role) {
        const int srow = lane >> 3, pch = lane & 7;
#pragma unroll
        for (int i = 0; i < APW; ++i) {
            const int row = (wave + 2 * i) * 8 + srow;
            const int gm = row < g.M ? row : g.M - 1;
            asrc[i] = g.A + (long)gm * g.lda + (pch ^ ((row >> 1) & 7)) * 8;
        }
    } else {
#pragma unroll
        for (int i = 0; i < APW; ++i) asrc[i] = nullptr;
        if constexpr (QB) {
            // piece = 4 rows x 256 B of codes; wave w-2 takes pieces (w-2), (w-2)+2, ...: rows 4 piece + lane / 16, chunk lane % 16
            const int row = (wave - 2) * 4 + (lane >> 4);
            int gn = n0 + row;
            gn = gn < g.N ? gn : g.N - 1;
            bsrc = (const char*)(g.Bq + (long)gn * g.K + (long)kt0 * BK + (lane & 15) * 16);
            bstep = 8L * g.K;   // two pieces = 8 rows further (ragged N is handled by the caller: N % 64 == 0 for this instance)
            int gs = n0 + lane;
            gs = gs < g.N ? gs : g.N - 1;
            sbsrc = (wave == 2 ? g.Bqs : g.Bqb) + (long)gs * groups + kt0;
        } else {
            // piece = 2 rows x 512 B; physical chunk p of row r holds logical chunk p ^ (r & 15) (fragment reads: 16 rows, one chunk);
            // the source addresses are formed in stage_b
        }
    }
    auto stage_a = [&](int j) {  // relative K-tile j -> activation slot j % NA
        char* base = smem + A_OFF + (j % NA) * A_BYTES;
#pragma unroll
        for (int i = 0; i < APW; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(asrc[i] + (long)(kt0 + j) * BK),
                                             (__attribute__((address_space(3))) void*)(base + (wave + 2 * i) * 1024), 16, 0, 0);
    };
    auto stage_b = [&](int m) {  // relative macro-tile m -> weight slot m % NBM
        if constexpr (QB) {
            char* base = smem + Q_OFF + (m % NBM) * BM_BYTES;
#pragma unroll
            for (int i = 0; i < 8; ++i)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(bsrc + i * bstep + (long)m * MT * BK),
                                                 (__attribute__((address_space(3))) void*)(base + ((wave - 2) + 2 * i) * 1024), 16, 0, 0);
            char* sb = smem + SB_OFF + (m % NBM) * SB_BYTES + (wave - 2) * 512;
#pragma unroll
            for (int i = 0; i < 2; ++i)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(sbsrc + m * MT + 2 * i),
                                                 (__attribute__((address_space(3))) void*)(sb + i * 256), 4, 0, 0);
        } else {
            char* base = smem + B_OFF + (m % NBM) * BM_BYTES;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                // piece (wave - 2) + 2 i = rows 2 piece, 2 piece + 1; the swizzle term (row & 15) changes from piece to piece
                const int row = ((wave - 2) + 2 * i) * 2 + (lane >> 5);
                const bf16_t* src = g.B + (long)(n0 + row) * g.ldb + (long)(kt0 + m * MT) * BK + (((lane & 31) ^ (row & 15)) * 8);
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                 (__attribute__((address_space(3))) void*)(base + ((wave - 2) + 2 * i) * 1024), 16, 0, 0);
            }
        }
    };
    // QB: codes of relative K-tile j -> bf16 image slot j & 1. Thread = (row tid / 4, 16 codes tid % 4).
    auto convert_q = [&](int j) {
        if constexpr (QB) {
            const int row = tid >> 2, c4 = tid & 3;
            const int m = j / MT, sub = j % MT;
            const uint4 raw = *(const uint4*)(smem + Q_OFF + (m % NBM) * BM_BYTES + row * 256 + sub * 64 + c4 * 16);
            const char* sbp = smem + SB_OFF + (m % NBM) * SB_BYTES + (sub >> 1) * 256 + row * 4;
            const uint32_t sw_ = *(const uint32_t*)sbp, bw_ = *(const uint32_t*)(sbp + 512);
            const float scale = bf16_to_f32((bf16_t)((sub & 1) ? (sw_ >> 16) : (sw_ & 0xffffu)));
            const float bias = bf16_to_f32((bf16_t)((sub & 1) ? (bw_ >> 16) : (bw_ & 0xffffu)));
            const uint32_t wd[4] = {raw.x, raw.y, raw.z, raw.w};
            uint32_t out[8];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const float q0 = (float)((wd[i] >> (16 * jj)) & 0xffu), q1 = (float)((wd[i] >> (16 * jj + 8)) & 0xffu);
                    out[i * 2 + jj] = pack_bf16x2(q0 * scale + bias, q1 * scale + bias);
                }
            char* brow = smem + B_OFF + (j & 1) * B_BYTES + row * ROW_BYTES;
            const int sw = (row >> 1) & 7;
            *(uint4*)(brow + (((2 * c4) ^ sw) << 4)) = uint4{out[0], out[1], out[2], out[3]};
            *(uint4*)(brow + (((2 * c4 + 1) ^ sw) << 4)) = uint4{out[4], out[5], out[6], out[7]};
        }
    };
    auto role_wait = [&](int need_through, int issued_through, int per) {
        int keep = issued_through - need_through;
        keep = keep < 0 ? 0 : keep;
        wait_vmcnt_dyn(keep * per);
    };

    const int frow = lane & 15;
    const int fsw = (lane >> 1) & 7;
    const int foff0 = frow * ROW_BYTES + ((((lane >> 4) + 0) ^ fsw) << 4);
    const int foff1 = frow * ROW_BYTES + ((((lane >> 4) + 4) ^ fsw) << 4);
    const int a_wave_off = (wr * WM) * ROW_BYTES;
    f32x4 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- prologue ----
    int a_issued = -1, b_issued = -1;  // last relative K-tile / macro-tile this role has staged
    if (a_role) {
        for (int j = 0; j < PA && j < nk; ++j) { stage_a(j); a_issued = j; }
    } else {
        for (int m = 0; m < PBM && m < nm; ++m) { stage_b(m); b_issued = m; }
    }
    if constexpr (QB) {  // the first tile's image needs a barrier of its own
        if (!a_role) role_wait(0, b_issued, BPW);
        raw_barrier();
        convert_q(0);
        wait_lgkm_barrier();
    }
    ResidualTile<BM, BN, WGM, WGN> rt;
    for (int t = 0; t < nk; ++t) {
        const int m = t / MT, sub = t % MT;
        // K-tile t of the activations and macro-tile m of the weights (QB: the macro-tile of K-tile t+1, converted below) must have landed
        if (a_role) role_wait(t, a_issued, APW);
        else role_wait(QB ? ((t + 1 < nk ? t + 1 : t) / MT) : m, b_issued, BPW);
        if constexpr (QB) wait_lgkm_barrier(); else raw_barrier();   // QB: also publishes the image converted during K-tile t-1
        // refill what K-tile t-1 / macro-tile m-1 occupied: every wave is past its reads (QB: past the conversion of its last K-tile)
        if (a_role) {
            if (t + PA < nk) { stage_a(t + PA); a_issued = t + PA; }
        } else if (sub == (QB ? 1 : 0)) {
            if (m + PBM < nm) { stage_b(m + PBM); b_issued = m + PBM; }
        }
        if (t == nk - 1 && !g.ep.d2s && g.split_k <= 1 && n0 + BN <= g.N) {  // residual / bias under the last tile's MFMAs
            gemm_bias_prefetch(g, n0, wc, lane, rt);
            if (g.ep.resid) gemm_residual_prefetch(g, m0, n0, wr, wc, lane, rt);
        }
        const char* abase = smem + A_OFF + (t % NA) * A_BYTES + a_wave_off;
        s16x8 fa[2][MI], fb[2][NI];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
#pragma unroll
            for (int i = 0; i < MI; ++i) fa[k][i] = *(const s16x8*)(abase + i * 16 * ROW_BYTES + (k ? foff1 : foff0));
#pragma unroll
            for (int j = 0; j < NI; ++j) {
                if constexpr (QB) {
                    fb[k][j] = *(const s16x8*)(smem + B_OFF + (t & 1) * B_BYTES + (wc * WN + j * 16) * ROW_BYTES + (k ? foff1 : foff0));
                } else {
                    // macro image: row stride 512 B, logical chunk sub*8 + 4k + (lane >> 4) at physical chunk ^ (row & 15)
                    const int row = wc * WN + j * 16 + frow;
                    fb[k][j] = *(const s16x8*)(smem + B_OFF + (m % NBM) * BM_BYTES + row * (MT * ROW_BYTES) +
                                               (((sub * 8 + 4 * k + (lane >> 4)) ^ frow) << 4));
                }
            }
        }
        if constexpr (QB) {
            if (t + 1 < nk) convert_q(t + 1);
        }
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, fa[k][i]), __builtin_bit_cast(bf16x8_t, fb[k][j]),
                                                                        acc[i][j], 0, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");  // the epilogue reuses the LDS
    if (g.split_k > 1) {
        GemmArgs gs = g;  // raw partial tile -> workspace slice of this split
        gs.ep = GemmEpilogue{};
        gs.ep.out_f32 = g.split_ws + (long)blockIdx.y * g.M * g.N;
        gs.ep.ld_f32 = g.N;
        gemm_epilogue<BM, BN, WGM, WGN>(acc, gs, m0, n0, wr, wc, lane, wave, smem);
        return;
    }
    gemm_epilogue<BM, BN, WGM, WGN>(acc, g, m0, n0, wr, wc, lane, wave, smem, &rt);
}

// ---------------------------------------------------------------------------------------------------------------
// The ring kernel on v_mfma_f32_32x32x16_bf16 (dense launches). Same LDS ring, counted waits and skewed fragment pipeline as _v2;
// what changes is the issue budget: an MFMA holds the SIMD's vector issue port for 8 cycles whether it computes for 16 or for 32
// (MI355X_MICROARCH.md, 'vector-instruction ISSUE cost'), so the 12 MFMAs of a K-tile leave 24 free cycles per gap where the 24 of
// the 16x16x32 form leave 8 - and the LDS-DMA pieces and fragment reads that the 16x16x32 loop cannot hide fit. Waves 2 x 4, per
// wave 96 x 32 = 3 x 1 blocks of 32 x 32 (48 accumulator registers, as before).
// MEASURED, NOT SELECTED (tile_cfg 31, experiments build): bit-identical to the 16x16x32 ring kernel on integer data, and slower -
// 1536x4096x4096 951 against 1021 TFLOP/s, K = 16384 1083 against 1178 (HBM-cold weights, same process): a 96 x 32 wave tile reads
// 16 KB of fragments per K-tile where 48 x 64 reads 14, and the compiler bunches the LDS-DMA pieces in one gap.
//   operands: lane l holds row (l & 31), k = 8 (l >> 5) .. +7 of the 16-deep k-step  -> one ds_read_b128 per block and k-step
//   result:   lane l holds column (l & 31), rows 8 (v / 4) + 4 (l >> 5) + (v % 4), v = 0..15
// ---------------------------------------------------------------------------------------------------------------
template <int BM, int BN, int NSTAGE>
__global__ __launch_bounds__(512) void gemm_bf16_kernel_m32(const GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int WGM = 2, WGN = 4, NW = 8;
    constexpr int WM = BM / WGM, WN = BN / WGN, MI = WM / 32, NI = WN / 32;
    static_assert(WM % 32 == 0 && WN % 32 == 0, "32x32 blocks");
    constexpr int A_BYTES = BM * ROW_BYTES, B_BYTES = BN * ROW_BYTES, STAGE = A_BYTES + B_BYTES;
    constexpr int A_PER_WAVE = BM / 8 / NW, B_PER_WAVE = BN / 8 / NW;
    static_assert(A_PER_WAVE * 8 * NW == BM && B_PER_WAVE * 8 * NW == BN, "tile rows must split evenly over the waves");
    constexpr int LPT = A_PER_WAVE + B_PER_WAVE;
    constexpr int PD = NSTAGE - 1;
    constexpr int NF = 2 * (MI + NI);  // fragment reads per half K-tile (two 16-deep k-steps)
    constexpr int NM = 2 * MI * NI;    // MFMAs per half K-tile
    static_assert(NSTAGE >= 3, "ring needs >= 3 slots");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / WGN, wc = wave % WGN;
    const int tiles_m = (g.M + BM - 1) / BM;
    const int bid = xcd_remap(blockIdx.x, gridDim.x) + g.tile0;
    int tm, tn;
    tile_coords(g, bid, tiles_m, BN, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN;

    const int srow = lane >> 3, pch = lane & 7;
    const bf16_t* a_src[A_PER_WAVE];
    const bf16_t* b_src[B_PER_WAVE];
#pragma unroll
    for (int i = 0; i < A_PER_WAVE; ++i) {
        const int row = (wave + NW * i) * 8 + srow;
        int gm = m0 + row;
        gm = gm < g.M ? gm : g.M - 1;
        a_src[i] = g.A + (long)gm * g.lda + (pch ^ ((row >> 1) & 7)) * 8;
    }
#pragma unroll
    for (int i = 0; i < B_PER_WAVE; ++i) {
        const int row = (wave + NW * i) * 8 + srow;
        int gn = n0 + row;
        gn = gn < g.N ? gn : g.N - 1;
        b_src[i] = g.B + (long)gn * g.ldb + (pch ^ ((row >> 1) & 7)) * 8;
    }
    int nk = g.K / BK, kt0 = 0;
    if (g.split_k > 1) {
        const int z = blockIdx.y;
        kt0 = (int)((long)nk * z / g.split_k);
        nk = (int)((long)nk * (z + 1) / g.split_k) - kt0;
    }
    auto stage = [&](int slot, int kt) {
        char* base = smem + slot * STAGE;
#pragma unroll
        for (int i = 0; i < A_PER_WAVE; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a_src[i] + (long)kt * BK),
                                             (__attribute__((address_space(3))) void*)(base + (wave + NW * i) * 1024), 16, 0, 0);
#pragma unroll
        for (int i = 0; i < B_PER_WAVE; ++i)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(b_src[i] + (long)kt * BK),
                                             (__attribute__((address_space(3))) void*)(base + A_BYTES + (wave + NW * i) * 1024), 16, 0, 0);
    };

    // fragment read offsets: row (lane & 31) of a 32-row block, 16-byte chunk (lane >> 5) + 2 ks of the row, XOR-swizzled by the row
    const int frow = lane & 31;
    const int fsw = (lane >> 1) & 7;  // ((row >> 1) & 7) for row = 32 k + (lane & 31)
    int foff[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) foff[ks] = frow * ROW_BYTES + ((((lane >> 5) + 2 * ks) ^ fsw) << 4);
    const int a_wave_off = (wr * WM) * ROW_BYTES;
    const int b_wave_off = A_BYTES + (wc * WN) * ROW_BYTES;

    f32x16 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[i][j][v] = 0.f;

    // two fragment sets (a half K-tile each = two k-steps): [k-step within the half][block]
    s16x8 fa0[2][MI], fb0[2][NI], fa1[2][MI], fb1[2][NI];
    auto load_frags = [&](int slot, int half, s16x8(&fa)[2][MI], s16x8(&fb)[2][NI]) {
        const char* base = smem + slot * STAGE;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
#pragma unroll
            for (int i = 0; i < MI; ++i) fa[k][i] = *(const s16x8*)(base + a_wave_off + i * 32 * ROW_BYTES + foff[2 * half + k]);
#pragma unroll
            for (int j = 0; j < NI; ++j) fb[k][j] = *(const s16x8*)(base + b_wave_off + j * 32 * ROW_BYTES + foff[2 * half + k]);
        }
    };
    auto mfma_one = [&](const s16x8(&fa)[2][MI], const s16x8(&fb)[2][NI], int k, int i, int j) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, fa[k][i]), __builtin_bit_cast(bf16x8_t, fb[k][j]),
                                                            acc[i][j], 0, 0, 0);
    };
    auto mfma_first = [&](const s16x8(&fa)[2][MI], const s16x8(&fb)[2][NI]) { mfma_one(fa, fb, 0, 0, 0); };
    auto mfma_rest = [&](const s16x8(&fa)[2][MI], const s16x8(&fb)[2][NI]) {
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j)
                    if (k + i + j > 0) mfma_one(fa, fb, k, i, j);
    };

#pragma unroll
    for (int s = 0; s < PD; ++s)
        if (s < nk) stage(s, kt0 + s);
    if (nk >= PD) wait_vmcnt_barrier<(PD - 1) * LPT>(); else wait_vmcnt_barrier<0>();
    load_frags(0, 0, fa0, fb0);

    int slot = 0;
    bool drained = false;
    auto ktile = [&](int kt, auto steady_tag) {
        constexpr bool STEADY = decltype(steady_tag)::value;
        int nslot = slot + 1;
        nslot = nslot == NSTAGE ? 0 : nslot;
        int pslot = slot - 1;
        pslot = pslot < 0 ? NSTAGE - 1 : pslot;
        // ---- first half: MFMAs of k-steps 0, 1; the fragment reads of k-steps 2, 3 go two per MFMA gap
        mfma_first(fa0, fb0);
        __builtin_amdgcn_sched_barrier(0);
        load_frags(slot, 1, fa1, fb1);
        mfma_rest(fa0, fb0);
#pragma unroll
        for (int q = 0; q < (NF + 1) / 2; ++q) {
            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);  // two ds_reads
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // one MFMA
        }
        __builtin_amdgcn_sched_group_barrier(0x008, NM - 1 - (NF + 1) / 2, 0);
        if constexpr (STEADY) wait_vmcnt_barrier<(PD - 2) * LPT>(); else if (!drained) wait_vmcnt_barrier<0>();
        // ---- second half
        mfma_first(fa1, fb1);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (STEADY) {
            stage(pslot, kt0 + kt + PD);
            load_frags(nslot, 0, fa0, fb0);
            mfma_rest(fa1, fb1);
            // five MFMAs to go: each gap takes one LDS-DMA piece and two of the next tile's fragment reads
#pragma unroll
            for (int q = 0; q < NM - 1; ++q) {
                __builtin_amdgcn_sched_group_barrier(0x020, (LPT + NM - 2) / (NM - 1), 1);
                __builtin_amdgcn_sched_group_barrier(0x100, (NF + NM - 2) / (NM - 1), 1);
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 1);
            }
        } else {
            if (kt + 1 < nk) load_frags(nslot, 0, fa0, fb0);
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
        if (!g.ep.d2s && g.split_k <= 1 && n0 + BN <= g.N && kt < nk) {
            gemm_bias_prefetch(g, n0, wc, lane, rt);
            if (g.ep.resid) gemm_residual_prefetch(g, m0, n0, wr, wc, lane, rt);
        }
    }
    for (; kt < nk; ++kt) ktile(kt, std::false_type{});
    __syncthreads();
    // the 16-row slab s of this wave's tile = half (s & 1) of block s / 2: values v = 8 (s & 1) + t, t = 0..7, at row
    // 8 (t / 4) + 4 (lane >> 5) + (t % 4) of the slab, column 32 j + (lane & 31)
    auto put = [&](auto s_c, float* scr) {
        constexpr int sidx = decltype(s_c)::value;
        constexpr int blk = sidx / 2, h = sidx % 2;
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int t = 0; t < 8; ++t)
                scr[(8 * (t / 4) + 4 * (lane >> 5) + (t % 4)) * WN + 32 * j + (lane & 31)] = acc[blk][j][8 * h + t];
    };
    if (g.split_k > 1) {
        GemmArgs gs = g;
        gs.ep = GemmEpilogue{};
        gs.ep.out_f32 = g.split_ws + ((long)blockIdx.y * (g.win_rows ? g.win_rows : g.M) - g.win_row0) * g.N;
        gs.ep.ld_f32 = g.N;
        gemm_epilogue_with<BM, BN, WGM, WGN, false, true>(put, gs, m0, n0, wr, wc, lane, wave, smem);
        return;
    }
    gemm_epilogue_with<BM, BN, WGM, WGN, false, true>(put, g, m0, n0, wr, wc, lane, wave, smem, &rt);
}

#elif LTX_GEMM_EXPERIMENTS_PART == 2
namespace {

template <int BM, int BN, int NSTAGE>
void launch_m32(const GemmArgs& a, hipStream_t stream) {
    constexpr int smem = NSTAGE * (BM + BN) * ROW_BYTES;
    static PerDeviceOnce attr_set;
    attr_set.run([&] {
        HIP_CHECK(hipFuncSetAttribute((const void*)gemm_bf16_kernel_m32<BM, BN, NSTAGE>, hipFuncAttributeMaxDynamicSharedMemorySize, smem));
    });
    LTX_REQUIRE(!a.conv && !a.ep.out_bf16_t && !a.ep.pn_out && !a.tile_count, "gemm: the 32x32x16 ring kernel takes dense launches without a transposed output");
    const int tiles = ((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN);
    if (a.split_k > 1) {
        LTX_REQUIRE(a.split_ws && a.N % 4 == 0 && !a.ep.d2s && a.split_k <= a.K / BK, "gemm split-K: workspace, N %% 4 == 0, no depth-to-space");
    }
    hipLaunchKernelGGL((gemm_bf16_kernel_m32<BM, BN, NSTAGE>), dim3(tiles, a.split_k > 1 ? a.split_k : 1), dim3(512), smem, stream, a);
    HIP_CHECK(hipGetLastError());
    if (a.split_k > 1) launch_splitk_finish(a, a.M, a.ep, 0, stream);
}

template <bool QB>
void launch_fewrow(const GemmArgs& a, hipStream_t stream) {
    constexpr int smem = 3 * 128 * ROW_BYTES + (QB ? 2 * 64 * ROW_BYTES + 4 * (64 * 256 + 1024) : 3 * 64 * 4 * ROW_BYTES);
    static PerDeviceOnce attr_set;
    attr_set.run([&] { HIP_CHECK(hipFuncSetAttribute((const void*)gemm_fewrow_kernel<QB>, hipFuncAttributeMaxDynamicSharedMemorySize, smem)); });
    LTX_REQUIRE(QB == (a.Bq != nullptr), "gemm: quantised codes need the de-quantising instance of the few-row kernel");
    LTX_REQUIRE(gemm_fewrow_takes(a.M, a.N, a.K, a.split_k) && !a.conv && !a.tile_count && !a.win_rows && !a.ep.d2s && !a.ep.pn_out,
                "gemm: the few-row kernel takes dense launches with M <= 128, N %% 64 == 0 and whole 256-wide macro-tiles of K per split "
                "(M=%d N=%d K=%d splits=%d)", a.M, a.N, a.K, a.split_k);
    const int tiles = (a.N + 63) / 64;
    if (a.split_k > 1) LTX_REQUIRE(a.split_ws && a.N % 4 == 0 && a.split_k <= a.K / BK, "gemm split-K: needs a workspace and N %% 4 == 0");
    hipLaunchKernelGGL(gemm_fewrow_kernel<QB>, dim3(tiles, a.split_k > 1 ? a.split_k : 1), dim3(256), smem, stream, a);
    HIP_CHECK(hipGetLastError());
    if (a.split_k > 1) launch_splitk_finish(a, a.M, a.ep, 0, stream);
}

}  // namespace

template <int BN>
static bool gemm_asm_takes(const GemmArgs& a) {
    return !a.conv && a.split_k <= 1 && a.M % 192 == 0 && a.N % BN == 0 && a.K % 64 == 0 && a.K >= 64 && !a.ep.d2s;
}
template <int BN, int RING = 0>
static void launch_asm(const GemmArgs& a, hipStream_t stream) {
    LTX_REQUIRE(gemm_asm_takes<BN>(a), "gemm: the assembly kernel needs a dense A.B^T with M %% 192 == 0, N %% %d == 0, K %% 64 == 0 (M=%d N=%d K=%d)",
                BN, a.M, a.N, a.K);
    constexpr int smem = RING == 2 ? 4 * 192 * ROW_BYTES : (RING ? 4 : 2) * (192 + BN) * ROW_BYTES;
    static PerDeviceOnce attr_set;
    attr_set.run([&] {
        HIP_CHECK(hipFuncSetAttribute((const void*)gemm_bf16_kernel_asm<BN, RING>, hipFuncAttributeMaxDynamicSharedMemorySize, smem));
    });
    hipLaunchKernelGGL((gemm_bf16_kernel_asm<BN, RING>), dim3((a.M / 192) * (a.N / BN)), dim3(256), smem, stream, a);
    HIP_CHECK(hipGetLastError());
}

bool gemm_stream_takes(const GemmArgs& a) {
    const GemmEpilogue& e = a.ep;
    return !a.conv && a.M >= 1 && a.M <= 128 && a.K % 64 == 0 && a.K >= 64 && a.N >= 16 && a.N % 4 == 0 && !e.d2s && a.lda % 8 == 0 &&
           (a.Bq ? a.ldb % 16 == 0 : a.ldb % 8 == 0);
}
// K split of the weight-streaming kernel: aim at one to two workgroups per CU, each wave with >= 4 K-tiles
static int stream_split_k(const GemmArgs& a) {
    const int tiles_n = (a.N + 63) / 64, nk = a.K / BK;
    int s = 1;
    while (tiles_n * s * 2 <= 512 && nk / (s * 2) >= 16 && s < 8) s *= 2;
    return s;
}
static void launch_stream(const GemmArgs& a_in, hipStream_t stream) {
    GemmArgs a = a_in;
    LTX_REQUIRE(gemm_stream_takes(a), "gemm: the weight-streaming kernel needs M <= 128, K %% 64 == 0, N %% 4 == 0 (M=%d N=%d K=%d)", a.M, a.N, a.K);
    if (a.split_k == 0) {  // workspace given, split left to the launcher
        a.split_k = stream_split_k(a);
        while (a.split_k > 1 && (long)a.split_k * a.M * a.N > a.split_ws_elems) a.split_k /= 2;
    }
    if (a.split_k < 1 || !a.split_ws) a.split_k = 1;
    constexpr int smem = 4 * 8 * 4 * 64 * 16;  // the four waves' 128 x 64 f32 tiles
    static PerDeviceOnce attr_set;
    attr_set.run([&] {
        HIP_CHECK(hipFuncSetAttribute((const void*)gemm_stream_kernel<16>, hipFuncAttributeMaxDynamicSharedMemorySize, smem));
        HIP_CHECK(hipFuncSetAttribute((const void*)gemm_stream_kernel<8>, hipFuncAttributeMaxDynamicSharedMemorySize, smem));
    });
    const dim3 grid((a.N + 63) / 64, a.split_k);
    if (a.Bq)
        hipLaunchKernelGGL(gemm_stream_kernel<8>, grid, dim3(256), smem, stream, a);
    else
        hipLaunchKernelGGL(gemm_stream_kernel<16>, grid, dim3(256), smem, stream, a);
    HIP_CHECK(hipGetLastError());
    if (a.split_k > 1) launch_splitk_finish(a, a.M, a.ep, 0, stream);
}

// ---- the hooks of gemm.hip's launch flow ----
// tile cfgs that only this build knows: the `default:` of launch_cfg's two switches asks here (true = launched)
static bool gemm_experiments_cfg(const GemmArgs& a, int cfg, const GemmOpts& o, hipStream_t stream) {
    if (a.conv) {
        switch (cfg) {  // measured, not selected for convs (VAE decode 19.4 ms with the 256x128 ring, 22.8 with the two-stage kernel, against 17.0)
            case 0: launch_one<128, 128, true>(a, stream); break;
            case 1: launch_one<192, 128, true>(a, stream); break;
            case 3: launch_one<96, 128, true>(a, stream); break;
            case 4: launch_one<128, 96, true>(a, stream); break;
            case 23: launch_v2<256, 128, 3, true, 4, 2>(a, o, stream); break;  // 8 waves, per-wave 64x64
            case 25: launch_v2<128, 192, 4, true, 2, 4>(a, o, stream); break;
            default: return false;
        }
    } else {
        switch (cfg) {
            case 28: launch_v2<128, 64, 4, false, 2, 2>(a, o, stream); break;  // cfg 29 with the 4-slot ring it had until round 3 (A/B)
            case 30:  // few rows (M <= 128), operand rings of their own, weights in macro-tiles: measured, not selected
                if (a.Bq) launch_fewrow<true>(a, stream); else launch_fewrow<false>(a, stream);
                break;
            case 31: launch_m32<192, 128, 4>(a, stream); break;  // the 192x128 ring tile on 32x32x16 MFMAs (2 x 4 waves of 96 x 32): 951 vs 1021 TFLOP/s
            case 90: launch_stream(a, stream); break;  // weight-streaming kernel for M <= 128 (bf16 weights or 8-bit codes): 1.4x slower than the ring split-K path
            case 71: launch_asm<256>(a, stream); break;      // one wave per SIMD, assembly main loop, 192x256
            case 72: launch_asm<128>(a, stream); break;      // the same, 192x128
            case 73: launch_asm<128, 1>(a, stream); break;  // 192x128, one wave per SIMD, LDS-DMA ring of four slots
            case 74: launch_asm<128, 2>(a, stream); break;  // the same with B as fragment-layout loads straight to registers
            case 41: launch_v4<192, 256>(a, stream); break;  // ping-pong, 8 waves (2x4), per-wave 96x64
            case 42: launch_v4<256, 256>(a, stream); break;  // ping-pong, per-wave 128x64
            default: return false;
        }
    }
    return true;
}

// string-valued tile experiments stay environment hooks of the experiments build only
// A/B hook: LTX_GEMM_GROUP_M="N:g,..." overrides the supertile height of dense launches with that N (tile_coords)
static void gemm_experiments_group_m(GemmArgs& a) {
    if (const char* f = getenv("LTX_GEMM_GROUP_M")) {
        for (const char* q = f; *q;) {
            const long n = strtol(q, (char**)&q, 10);
            if (*q != ':') break;
            const long gm = strtol(q + 1, (char**)&q, 10);
            if (n == a.N && !a.conv) a.group_m = (int)gm;
            if (*q == ',') ++q;
        }
    }
}

// a plain dense launch (no split count left to the launcher) that the environment sends to a tile cfg of its own (true = launched)
static bool gemm_experiments_forced(const GemmArgs& a, const GemmOpts& o, hipStream_t stream) {
    // The assembly kernel (tile_cfg 71: 192 x 256 tile, one wave per SIMD, generated main loop) is NOT in the default choice.
    // Measured on MI355X, HBM-cold weights, random data, same process (tools/bench_gemm.py --cold --cfgs=-1,21,1,71), TFLOP/s:
    // 1536x16384x4096 1057 vs 1009 (two-stage) / 987 (ring); 6144x4096x4096 1069 vs 1053 / 1015; 1536x8192x4096 895 vs 930 (ring);
    // but inside the DiT step (same-box A/B of bench.py) routing the FFN's first GEMM to it costs 0.3 ms per step (41.6 vs 41.3).
    // Its loop runs 2380 cycles per K-tile against 1730 of MFMA issue (14 buffer loads + 14 ds_write_b128 per wave and tile are
    // not free) and its epilogue (10 us for 50 MB of output, every workgroup at the same time) is exposed once per launch.
    // LTX_GEMM_ASM=1 opts in for launches that fill the chip at least twice with 192x256 tiles (A/B runs).
    static const bool asm_on = getenv("LTX_GEMM_ASM") && getenv("LTX_GEMM_ASM")[0] == '1';
    if (asm_on && gemm_asm_takes<256>(a)) {
        const long tiles_asm = (long)(a.M / 192) * (a.N / 256);
        if (tiles_asm >= 512 && tiles_asm % 256 == 0 && a.K <= 8192) {
            launch_cfg(a, 71, o, 0, stream);
            return true;
        }
    }
    // A/B hook for in-pipeline tile experiments (experiments build only): LTX_GEMM_FORCE="8192:21,16384:21" forces a tile cfg for dense launches by N
    if (const char* f = getenv("LTX_GEMM_FORCE")) {
        for (const char* q = f; *q;) {
            const long n = strtol(q, (char**)&q, 10);
            if (*q != ':') break;
            const long c = strtol(q + 1, (char**)&q, 10);
            const bool takes = c == 71 ? gemm_asm_takes<256>(a) : (c >= 72 && c <= 74) ? gemm_asm_takes<128>(a) : c == 75 ? gemm_dtl_takes(a) : true;
            if (n == a.N && takes) {
                launch_cfg(a, (int)c, o, 0, stream);
                return true;
            }
            if (*q == ',') ++q;
        }
    }
    return false;
}
#endif
#undef LTX_GEMM_EXPERIMENTS_PART
