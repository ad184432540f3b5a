// attention_experiments.inc - attention kernels that were built, measured and NOT selected, and their launch blocks. Compiled only with
// -DLTX_EXPERIMENTS (make EXPERIMENTS=1; tools/ and the `experiments`-marked tests load that library); the product library does not
// contain them. attention.hip includes this file twice, LTX_ATTN_EXPERIMENTS_PART selects what it gets:
//   1  inside the anonymous namespace, behind the 48-query layout helpers and the 4-wave kernel: the kernels
//   2  in front of launch_attention: launch_attention_experiment, the hook that runs them for option "attn_impl" = 3 / 5
#if LTX_ATTN_EXPERIMENTS_PART == 1
// plain-HIP layout reference of the 48-query kernel ("attn_impl" = 3): pins the LDS images and the MFMA operand mapping
__global__ __launch_bounds__(256, 1) void attn_fwd_kernel_w48_ref(const AttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c16 = lane & 15, g = lane >> 4;
    const int head = blockIdx.y, b = blockIdx.z;
    const bf16_t* Qb = a.Q + (long)b * a.q_bstride + head * 128;
    const bf16_t* Kb = a.K + (long)b * a.k_bstride + head * 128;
    const bf16_t* Vb = a.Vt + (long)b * a.vt_bstride + (long)head * 128 * a.ldvt;
    const int q0 = blockIdx.x * W48_Q + wave * 48;
    const int nt = a.Tk / KV_TILE;
    const W48Lane L = w48_lane(lane, wave, a.ldk, a.ldvt);
    s16x8 qf[3][4];
    for (int qb = 0; qb < 3; ++qb)
        for (int ks = 0; ks < 4; ++ks) qf[qb][ks] = *(const s16x8*)(Qb + (long)(q0 + 16 * qb + c16) * a.ldq + ks * 32 + g * 8);
    const __amdgpu_buffer_rsrc_t k_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)Kb, 0, (int)(((long)(a.Tk - 1) * a.ldk + 128) * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t v_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)Vb, 0, (int)((long)128 * a.ldvt * 2), 0x00020000);
    f32x4 o[8][3];
    for (int db = 0; db < 8; ++db)
        for (int qb = 0; qb < 3; ++qb) o[db][qb] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run[3] = {-INFINITY, -INFINITY, -INFINITY}, l_run[3] = {0.f, 0.f, 0.f};
    const float c = a.scale * 1.4426950408889634f;
    for (int t = 0; t < nt; ++t) {  // single-buffered, fully synchronous: a layout check, not a fast kernel
        __syncthreads();
        for (int i = 0; i < 4; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(k_rsrc, (__attribute__((address_space(3))) void*)(smem + (wave + 4 * i) * 1024), 16, L.koff[i], t * KV_TILE * (int)a.ldk * 2, 0, 0);
        for (int i = 0; i < 4; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(v_rsrc, (__attribute__((address_space(3))) void*)(smem + K_TILE_BYTES + (wave + 4 * i) * 1024), 16, L.voff[i], t * KV_TILE * 2, 0, 0);
        __syncthreads();
        f32x4 s[4][3];
        for (int kb = 0; kb < 4; ++kb)
            for (int qb = 0; qb < 3; ++qb) s[kb][qb] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int kb = 0; kb < 4; ++kb)
            for (int ks = 0; ks < 4; ++ks) {
                const s16x8 kf = *(const s16x8*)(smem + L.kaddr[ks] + w48_kblock_off(kb));
                for (int qb = 0; qb < 3; ++qb)
                    s[kb][qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, kf), __builtin_bit_cast(bf16x8_t, qf[qb][ks]), s[kb][qb], 0, 0, 0);
            }
        s16x8 pf[3][2];
        for (int qb = 0; qb < 3; ++qb) {
            float mloc = s[0][qb][0];
            for (int kb = 0; kb < 4; ++kb)
                for (int j = 0; j < 4; ++j) mloc = fmaxf(mloc, s[kb][qb][j]);
            mloc = fmaxf(mloc, __shfl_xor(mloc, 16, 64));
            mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
            const float m_new = fmaxf(m_run[qb], mloc);
            const float alpha = __builtin_amdgcn_exp2f((m_run[qb] - m_new) * c);
            m_run[qb] = m_new;
            float psum = 0.f;
            for (int i = 0; i < 2; ++i) {
                s16x8 pk;
                for (int hh = 0; hh < 2; ++hh)
                    for (int j = 0; j < 4; ++j) {
                        const float p = __builtin_amdgcn_exp2f(s[2 * i + hh][qb][j] * c - m_new * c);
                        psum += p;
                        pk[4 * hh + j] = (short)f32_to_bf16(p);
                    }
                pf[qb][i] = pk;
            }
            l_run[qb] = l_run[qb] * alpha + psum;
            for (int db = 0; db < 8; ++db) o[db][qb] *= alpha;
        }
        for (int db = 0; db < 8; ++db)
            for (int i = 0; i < 2; ++i) {
                const s16x8 vf = *(const s16x8*)(smem + L.vaddr[i] + w48_vblock_off(db));
                for (int qb = 0; qb < 3; ++qb)
                    o[db][qb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, vf), __builtin_bit_cast(bf16x8_t, pf[qb][i]), o[db][qb], 0, 0, 0);
            }
    }
    for (int qb = 0; qb < 3; ++qb) {
        float l = l_run[qb];
        l += __shfl_xor(l, 16, 64);
        l += __shfl_xor(l, 32, 64);
        const float inv = 1.0f / l;
        bf16_t* orow = a.O + (long)b * a.o_bstride + (long)(q0 + 16 * qb + c16) * a.ldo + head * 128;
        for (int db = 0; db < 8; ++db) {
            uint2 pk;
            pk.x = pack_bf16x2(o[db][qb][0] * inv, o[db][qb][1] * inv);
            pk.y = pack_bf16x2(o[db][qb][2] * inv, o[db][qb][3] * inv);
            *(uint2*)(orow + db * 16 + g * 4) = pk;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// 32x32x16 stream, 48 queries per wave (round 3): one 32-query block per wave + half of a block shared by a wave pair, split by
// keys (tools/gen_attn_x32.py: layout, register map, pipeline). The LDS images and the K-row permutation are those of
// attn_fwd_kernel above (the plain-HIP 32x32 kernel pins them through the parity tests); C++ only prepares per-lane offsets.
// Takes unmasked launches with prescaled Q and Tk % 64 == 0; any Tq (rows past Tq are clamped on load and dropped by the O
// descriptor). MEASURED, NOT SELECTED (experiments build, option "attn_impl" = 5): its tile step takes 2071 cycles against 2428 of the
// 16x16x32 stream, but the part holds 1.47 GHz under it against 1.86 GHz (32x32x16 MFMAs draw more per FLOP): 495 vs 459 us at
// T = 6144, 40.2 vs 38.5 us at T = 1536, 3.65 vs 3.40 ms per DiT step (profiles/r03_attn_x32_stamps.txt).
// ---------------------------------------------------------------------------------------------------------------
constexpr int X32_Q = 192;
constexpr int X32_LDS = 4 * STAGE_BYTES;
constexpr int X32_XSZ = 0x2400;  // epilogue exchange area per wave (gen_attn_x32.py XSZ)
#ifdef X32_STAMPS
__device__ unsigned long long g_x32_stamps[8][16];
#endif

__global__ __launch_bounds__(256, 1) void attn_fwd_kernel_x32_asm(const AttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int hwv = wave & 1, pair = wave >> 1;
    const AttnBlock blk = attn_block((a.Tq + X32_Q - 1) / X32_Q, a.H, a.B, a.plain_order);
    const int head = blk.head, b = blk.b;
    const bf16_t* Qb = a.Q + (long)b * a.q_bstride + head * 128;
    const bf16_t* Kb = a.K + (long)b * a.k_bstride + head * 128;
    const bf16_t* Vb = a.Vt + (long)b * a.vt_bstride + (long)head * 128 * a.ldvt;
    bf16_t* Ob = a.O + (long)b * a.o_bstride + head * 128;
    const int q0 = blk.x * X32_Q;
    const int qi_own = q0 + 32 * wave + r, qi_sh = q0 + 128 + 32 * pair + r;
    const int qoo = ((qi_own < a.Tq ? qi_own : a.Tq - 1) * (int)a.ldq + h * 8) * 2;
    const int qos = ((qi_sh < a.Tq ? qi_sh : a.Tq - 1) * (int)a.ldq + h * 8) * 2;
    const int oow = (qi_own * (int)a.ldo + h * 4) * 2, oos = (qi_sh * (int)a.ldo + h * 4) * 2;
    // LDS-DMA pieces: wave w stages pieces w, w+4, w+8, w+12 of each image (1 KB each: 4 keys x 256 B / 8 d-rows x 128 B); the bank
    // swizzle sits on the SOURCE address: physical chunk p of key k holds logical chunk p ^ (k & 15), of d-row d chunk p ^ ((d>>1)&7)
    int ko[4], vo[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int kl = (wave + 4 * i) * 4 + (lane >> 4);
        ko[i] = (kl * (int)a.ldk + (((lane & 15) ^ (kl & 15)) << 3)) * 2;
        const int d = (wave + 4 * i) * 8 + (lane >> 3);
        vo[i] = (d * (int)a.ldvt + (((lane & 7) ^ ((d >> 1) & 7)) << 3)) * 2;
    }
    // fragment addresses. K: MFMA row r reads key pi(r) (bits 2 and 3 swapped) of a 32-key half; half A = this wave's own (hw)
    const int pr = (r & ~12) | ((r & 4) << 1) | ((r & 8) >> 1);
    const int ksw = pr & 15;
    const int kbase = pr * 256 + ((h ^ (ksw & 1)) << 4);
    const int kbA = kbase + hwv * 8192, kbB = kbase + (1 - hwv) * 8192;
    const int kx5 = (ksw >> 1) << 5;
    const int vsw = (r >> 1) & 7;
    int va[4];  // A0 A1 B0 B1: k-step (2 * half + s2) of the PV product
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int half = (i >> 1) ? 1 - hwv : hwv;
        const int kst = 2 * half + (i & 1);
        va[i] = K_TILE_BYTES + r * 128 + ((((kst << 1) + h) ^ vsw) << 4);
    }
    const int xout = wave * X32_XSZ + lane * 16, xin = (wave ^ 1) * X32_XSZ + lane * 16;
    const uint32_t nt = (uint32_t)(a.Tk / KV_TILE);
    const uint32_t oblo = (uint32_t)(uintptr_t)Ob, obhi = (uint32_t)((uintptr_t)Ob >> 32);
    const uint32_t orec = (uint32_t)(((long)(a.Tq - 1) * a.ldo + 128) * 2);
    const uint32_t kblo = (uint32_t)(uintptr_t)Kb, kbhi = (uint32_t)((uintptr_t)Kb >> 32);
    const uint32_t vblo = (uint32_t)(uintptr_t)Vb, vbhi = (uint32_t)((uintptr_t)Vb >> 32);
    const uint32_t krec = (uint32_t)(((long)(a.Tk - 1) * a.ldk + 128) * 2), vrec = (uint32_t)((long)128 * a.ldvt * 2);
    const uint32_t ktb = (uint32_t)(KV_TILE * a.ldk * 2);
    const uint32_t wlds = (uint32_t)wave * 1024u;
    const uint32_t hws = (uint32_t)hwv;
    const float tau = 8.0f;
#ifdef X32_STAMPS
    unsigned long long* dbg = (blk.x == 1 && head == 3) ? &g_x32_stamps[wave][0] : &g_x32_stamps[4 + (wave & 3)][0];
#endif
    asm volatile(
#ifdef X32_STAMPS
#include "attention_x32_asm_stamps.inc"
#else
#include "attention_x32_asm.inc"
#endif
        :
        : [qbase] "s"(Qb), [oblo] "s"(oblo), [obhi] "s"(obhi), [orec] "s"(orec), [kblo] "s"(kblo), [kbhi] "s"(kbhi), [vblo] "s"(vblo),
          [vbhi] "s"(vbhi), [krec] "s"(krec), [vrec] "s"(vrec), [ktb] "s"(ktb), [nt] "s"(nt), [tau] "s"(tau), [wlds] "s"(wlds),
          [hw] "s"(hws), [qoo] "v"(qoo), [qos] "v"(qos), [oow] "v"(oow), [oos] "v"(oos), [ko0] "v"(ko[0]), [ko1] "v"(ko[1]),
          [ko2] "v"(ko[2]), [ko3] "v"(ko[3]), [vo0] "v"(vo[0]), [vo1] "v"(vo[1]), [vo2] "v"(vo[2]), [vo3] "v"(vo[3]), [kbA] "v"(kbA),
          [kbB] "v"(kbB), [kx5] "v"(kx5), [vaA0] "v"(va[0]), [vaA1] "v"(va[1]), [vaB0] "v"(va[2]), [vaB1] "v"(va[3]), [xout] "v"(xout),
          [xin] "v"(xin)
#ifdef X32_STAMPS
          , [dbg] "s"(dbg)
#endif
        :
#include "attention_x32_clobbers.inc"
    );
    (void)smem;
}

#elif LTX_ATTN_EXPERIMENTS_PART == 2
static bool launch_attention_experiment(const AttnArgs& a, int impl, bool w48_ok, hipStream_t stream) {
    if (impl == 3) {
        LTX_REQUIRE(w48_ok, "attention: attn_impl = 3 needs Tq %% 192 == 0, Tk %% 256 == 0 and no mask (Tq=%d Tk=%d)", a.Tq, a.Tk);
        static PerDeviceOnce attr3_set;
        attr3_set.run([&] {
            HIP_CHECK(hipFuncSetAttribute((const void*)attn_fwd_kernel_w48_ref, hipFuncAttributeMaxDynamicSharedMemorySize, W48_LDS));
        });
        hipLaunchKernelGGL(attn_fwd_kernel_w48_ref, dim3(a.Tq / W48_Q, a.H, a.B), dim3(256), W48_LDS, stream, a);
        HIP_CHECK(hipGetLastError());
        return true;
    }
    // the 32x32 stream ("attn_impl" = 5 only: measured slower than the 16x16 stream on every BASELINE shape)
    if (impl == 5) {
        const bool x32_ok = !a.bias && a.q_prescaled && a.Tk % KV_TILE == 0;
        LTX_REQUIRE(x32_ok, "attention: attn_impl = 5 takes unmasked launches with prescaled Q and Tk %% 64 == 0 (Tq=%d Tk=%d)", a.Tq, a.Tk);
        static PerDeviceOnce attr5_set;
        attr5_set.run([&] { HIP_CHECK(hipFuncSetAttribute((const void*)attn_fwd_kernel_x32_asm, hipFuncAttributeMaxDynamicSharedMemorySize, X32_LDS)); });
        hipLaunchKernelGGL(attn_fwd_kernel_x32_asm, dim3(((a.Tq + X32_Q - 1) / X32_Q) * a.H * a.B), dim3(256), X32_LDS, stream, a);
        HIP_CHECK(hipGetLastError());
        return true;
    }
    return false;
}
#endif
#undef LTX_ATTN_EXPERIMENTS_PART
