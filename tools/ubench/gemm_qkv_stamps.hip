// gemm_qkv_stamps.hip - cycle stamps inside one K-tile body of the fused q|k + V GEMM kernel (gemm_bf16_kernel_qkv, 192 x 384 tiles),
// all four waves of one workgroup, plus launch timing with HBM-cold weights for schedule variants (QKV_KNOBS of
// tools/gen_gemm_asm_qkv.py). Build from the repo root:
//   python3 tools/gen_gemm_asm_qkv.py --stamps      (or: QKV_KNOBS=bar1=30,dma0=31 python3 tools/gen_gemm_asm_qkv.py)
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -DQKV_STAMPS -Iinclude -Iltx-video-swift-mlx_amd/csrc -o tools/ubench/gemm_qkv_stamps tools/ubench/gemm_qkv_stamps.hip
#include "../../ltx-video-swift-mlx_amd/csrc/gemm.hip"
#include "../../ltx-video-swift-mlx_amd/csrc/options.cpp"   // the launchers' switch table (defaults; nothing here moves it)

#include <stdio.h>
#include <stdlib.h>
#include <vector>

Profiler* prof_current() { return nullptr; }
ProfRec* Profiler::begin(int, double, hipStream_t) { return nullptr; }
void Profiler::end(ProfRec*, hipStream_t) {}
void launch_norm_mod(const NormModArgs&, hipStream_t) { abort(); }

int main() {
    const int M = getenv("GEMM_M") ? atoi(getenv("GEMM_M")) : 1536, D = getenv("GEMM_D") ? atoi(getenv("GEMM_D")) : 4096, K = getenv("GEMM_K") ? atoi(getenv("GEMM_K")) : 4096;
    const int NB = 8;  // rotate through distinct weight sets (8 x 100 MB): HBM-cold B operands, as in the DiT
    std::vector<bf16_t> ha((size_t)M * K), hb((size_t)3 * D * K);
    for (size_t i = 0; i < ha.size(); ++i) ha[i] = host_f32_to_bf16((float)((i * 2654435761u >> 20) & 255) / 256.f - 0.5f);
    for (size_t i = 0; i < hb.size(); ++i) hb[i] = host_f32_to_bf16((float)((i * 40503u >> 12) & 255) / 256.f - 0.5f);
    bf16_t *a, *b[NB], *qk, *vt;
    (void)hipMalloc(&a, ha.size() * 2); (void)hipMalloc(&qk, (size_t)M * 2 * D * 2); (void)hipMalloc(&vt, (size_t)D * M * 2);
    (void)hipMemcpy(a, ha.data(), ha.size() * 2, hipMemcpyHostToDevice);
    for (int i = 0; i < NB; ++i) {
        (void)hipMalloc(&b[i], hb.size() * 2);
        (void)hipMemcpy(b[i], hb.data(), hb.size() * 2, hipMemcpyHostToDevice);
    }
    GemmQkvArgs g;
    g.X = a; g.ldx = K; g.M = M; g.rows_per_batch = M; g.ldwqk = K; g.ldwv = K; g.Nqk = 2 * D; g.K = K;
    g.qk = qk; g.ld_qk = 2 * D; g.vt = vt; g.ldvt = M; g.vt_bstride = (long)D * M;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    auto launch = [&](int it) { g.Wqk = b[it % NB]; g.Wv = b[it % NB] + (size_t)2 * D * K; launch_gemm_qkv(g, 0); };
    for (int it = 0; it < 6; ++it) launch(it);
    (void)hipEventRecord(e0);
    for (int it = 0; it < 24; ++it) launch(it);
    (void)hipEventRecord(e1);
    (void)hipDeviceSynchronize();
    float ms; (void)hipEventElapsedTime(&ms, e0, e1);
    printf("fused q|k + V %d x (%d + %d) x %d: %.1f us per launch, %.0f TFLOP/s\n", M, 2 * D, D, K, ms * 1000 / 24, 2.0 * M * 3 * D * K / (ms / 24 * 1e-3) / 1e12);
    unsigned long long st[5][8];
    (void)hipMemcpyFromSymbol(st, HIP_SYMBOL(g_gemm_stamps), sizeof(st));
    printf("one K-tile body (slot 0, last pass), cycles:\nwave | MFMA 1..26 + k1 reads | lgkmcnt(0) | barrier 1 | MFMA 27..126 + 18 LDS-DMA | vmcnt wait | barrier 2 | MFMA 127..144 + entry reads | tile\n");
    for (int w = 0; w < 4; ++w)
        printf("  %d  | %12llu %16llu %10llu %18llu %18llu %10llu %18llu          | %llu\n", w, st[w][1] - st[w][0], st[w][2] - st[w][1], st[w][3] - st[w][2],
               st[w][4] - st[w][3], st[w][5] - st[w][4], st[w][6] - st[w][5], st[w][7] - st[w][6], st[w][7] - st[w][0]);
    // the epilogue of the same launch: ASM_EPI_STAMP points of gemm_asm_tiles.inc
    unsigned long long ep[5][16];
    (void)hipMemcpyFromSymbol(ep, HIP_SYMBOL(g_gemm_epi_stamps), sizeof(ep));
    printf("epilogue, cycles from the stream's exit: V^T stores issued | [dump done | last store issued] x 3 q|k groups, final vmcnt(0)\n");
    for (int w = 0; w < 4; ++w) {
        printf("  %d  | %6llu |", w, ep[w][1] - ep[w][0]);
        for (int i = 2; i <= 8; ++i) printf(" %6llu%s", ep[w][i] - ep[w][0], (i & 1) ? " |" : "");
        printf("\n");
    }
    return 0;
}
