// gemm_tall_stamps.hip - cycle stamps inside one K-tile body of the 384x256 GEMM kernel (tile_cfg 76), all four waves of one
// workgroup, the clock held in the loop, prologue / loop / epilogue of the launch, and launch timing against tile_cfg 75 for schedule
// variants (TALL_KNOBS of tools/gen_gemm_asm_tall.py). Build from the repo root:
//   python3 tools/gen_gemm_asm_tall.py --stamps      (or: TALL_KNOBS=bar1=20,bdma0=30 python3 tools/gen_gemm_asm_tall.py)
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -DTALL_STAMPS -Iinclude -Iltx-video-swift-mlx_amd/csrc -o tools/ubench/gemm_tall_stamps tools/ubench/gemm_tall_stamps.hip ltx-video-swift-mlx_amd/csrc/options.cpp
// s_memtime counts shader-clock cycles. The launch is timed at K and K / 2: the difference is K / 128 K-tiles of pure loop, the rest is
// prologue + epilogue; (cycles per K-tile from the stamps) / (us per K-tile from the timing) is the clock held in the loop.
#include "../../ltx-video-swift-mlx_amd/csrc/gemm.hip"

#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <vector>

Profiler* prof_current() { return nullptr; }
ProfRec* Profiler::begin(int, double, hipStream_t) { return nullptr; }
void Profiler::end(ProfRec*, hipStream_t) {}
// (the row pass behind a GEMM lives in elementwise.hip; nothing here launches it)
void launch_norm_mod(const NormModArgs&, hipStream_t) {}

static float time_cfg(GemmArgs g, bf16_t* const* b, int nb, int cfg, int& it) {
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    std::vector<float> us;
    for (int r = 0; r < 5; ++r) {
        (void)hipEventRecord(e0);
        for (int i = 0; i < 8; ++i) { g.B = b[it++ % nb]; launch_gemm_bf16_cfg(g, cfg, 0); }
        (void)hipEventRecord(e1);
        (void)hipEventSynchronize(e1);
        float ms; (void)hipEventElapsedTime(&ms, e0, e1);
        us.push_back(ms * 1000 / 8);
    }
    std::sort(us.begin(), us.end());
    return us[2];
}

int main() {
    const int M = getenv("GEMM_M") ? atoi(getenv("GEMM_M")) : 1536, N = getenv("GEMM_N") ? atoi(getenv("GEMM_N")) : 16384, K = getenv("GEMM_K") ? atoi(getenv("GEMM_K")) : 4096;
    const int NB = 6;  // rotate through distinct weight matrices: HBM-cold B operand, as in the DiT
    std::vector<bf16_t> ha((size_t)M * K), hb((size_t)N * K);
    for (size_t i = 0; i < ha.size(); ++i) ha[i] = host_f32_to_bf16((float)((i * 2654435761u >> 20) & 255) / 256.f - 0.5f);
    for (size_t i = 0; i < hb.size(); ++i) hb[i] = host_f32_to_bf16((float)((i * 40503u >> 12) & 255) / 256.f - 0.5f);
    bf16_t *a, *b[NB];
    bf16_t* c;
    float* bias;
    (void)hipMalloc(&a, ha.size() * 2); (void)hipMalloc(&c, (size_t)M * N * 2); (void)hipMalloc(&bias, (size_t)N * 4);
    (void)hipMemset(bias, 0, (size_t)N * 4);
    (void)hipMemcpy(a, ha.data(), ha.size() * 2, hipMemcpyHostToDevice);
    for (int i = 0; i < NB; ++i) {
        (void)hipMalloc(&b[i], hb.size() * 2);
        (void)hipMemcpy(b[i], hb.data(), hb.size() * 2, hipMemcpyHostToDevice);
    }
    GemmArgs g;
    g.A = a; g.lda = K; g.ldb = K; g.M = M; g.N = N; g.K = K;
    g.ep.bias_n = bias; g.ep.act = LTX_ACT_GELU_TANH;  // the FFN-up epilogue
    g.ep.out_bf16 = c; g.ep.ld_bf16 = N;
    int it = 0;
    for (int i = 0; i < 6; ++i) { g.B = b[it++ % NB]; launch_gemm_bf16_cfg(g, i & 1 ? 75 : 76, 0); }
    float full[2][3], half[2][3];
    GemmArgs h = g;
    h.K = K / 2;  // same leading dimensions: half the K-tiles of the same matrices
    for (int r = 0; r < 3; ++r)  // alternating, same process
        for (int k = 0; k < 2; ++k) {
            full[k][r] = time_cfg(g, b, NB, 75 + k, it);
            half[k][r] = time_cfg(h, b, NB, 75 + k, it);
        }
    double tile_us = 0;
    for (int k = 0; k < 2; ++k) {
        std::sort(full[k], full[k] + 3);
        std::sort(half[k], half[k] + 3);
        const double loop = 2.0 * (full[k][1] - half[k][1]), fixed = full[k][1] - loop;
        const int rounds = k == 0 ? (M / 192) * (N / 256) / 256 : (M / 384) * (N / 256) / 256;
        printf("cfg %d %dx%dx%d: %.1f us per launch [%.1f .. %.1f], %.0f TFLOP/s | loop %.1f us = %.3f us per K-tile and round, prologue + epilogue %.1f us\n",
               75 + k, M, N, K, full[k][1], full[k][0], full[k][2], 2.0 * M * N * K / (full[k][1] * 1e-6) / 1e12, loop,
               loop / (K / 64) / (rounds > 0 ? rounds : 1), fixed);
        if (k == 1) tile_us = loop / (K / 64) / (rounds > 0 ? rounds : 1);
    }
    g.B = b[0];
    launch_gemm_bf16_cfg(g, 76, 0);
    (void)hipDeviceSynchronize();
    unsigned long long st[5][8];
    (void)hipMemcpyFromSymbol(st, HIP_SYMBOL(g_gemm_stamps), sizeof(st));
    printf("one K-tile body (slot 0, last pass), cycles:\nwave | to BAR1 (MFMA + B reads + A pieces) | lgkmcnt | barrier 1 | BAR1 .. BAR2 (MFMA + 8 B pieces) | vmcnt wait | barrier 2 | tail (next tile's reads) | tile\n");
    for (int w = 0; w < 4; ++w)
        printf("  %d  | %8llu %20llu %10llu %18llu %18llu %10llu %14llu          | %llu\n", w, (st[w][1] - st[w][0]), (st[w][2] - st[w][1]),
               (st[w][3] - st[w][2]), (st[w][4] - st[w][3]), (st[w][5] - st[w][4]), (st[w][6] - st[w][5]), (st[w][7] - st[w][6]),
               (st[w][7] - st[w][0]));
    const double cyc = (double)(st[0][7] - st[0][0]);
    printf("wave 0: %.0f cycles per K-tile, MFMA duty %.1f %% (192 MFMAs x 16 issue cycles = 3072), clock in the loop %.0f MHz (%.3f us per K-tile)\n", cyc,
           100.0 * 3072 / cyc, tile_us > 0 ? cyc / tile_us : 0.0, tile_us);
    // the epilogue of the same launch (GELU-tanh -> bf16, the FFN-up form): ASM_EPI_STAMP points of gemm_asm_tiles.inc
    unsigned long long ep[5][16];
    (void)hipMemcpyFromSymbol(ep, HIP_SYMBOL(g_gemm_epi_stamps), sizeof(ep));
    printf("epilogue, cycles from the stream's exit; groups in store order 4 5 0 1 2 3: [dump done | last store issued] x 6, final vmcnt(0)\n");
    for (int w = 0; w < 4; ++w) {
        printf("  %d  |", w);
        for (int i = 1; i <= 13; ++i) printf(" %6llu%s", ep[w][i] - ep[w][0], (i & 1) ? "" : " |");
        printf("\n");
    }
    double dump = 0, store = 0;
    for (int i = 0; i < 6; ++i) { dump += (double)(ep[0][1 + 2 * i] - ep[0][2 * i]); store += (double)(ep[0][2 + 2 * i] - ep[0][1 + 2 * i]); }
    printf("wave 0: dumps %.0f cycles, reads + arithmetic + store issue %.0f, drain %.0f, epilogue %.0f\n", dump, store, (double)(ep[0][13] - ep[0][12]),
           (double)(ep[0][13] - ep[0][0]));
    return 0;
}
