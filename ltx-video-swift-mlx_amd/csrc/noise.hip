// noise.hip - see noise.h.
#include "noise.h"

#include <cmath>

namespace {

constexpr int kNoiseBlock = 256;  // 4 waves; the kernel is ALU work on a few registers, so any multiple of 64 fills the CUs

struct NoiseGroup {  // the kernel's argument: the jobs by value, the prefix table of their workgroups, the host's f32 constants
    ltx_noise_job job[kNoiseJobsPerLaunch];
    int wg_end[kNoiseJobsPerLaunch];
    int n_jobs;
    float lo, range, upper, maxval, sqrt2;  // computed by the host expressions of mlx_random_normal, so both sides hold the same bits
};

LTX_DEVFN void threefry2x32_dev(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t& r0, uint32_t& r1) {
    const uint32_t ks[3] = {k0, k1, k0 ^ k1 ^ 0x1BD11BDAu};
    uint32_t x0 = c0 + ks[0], x1 = c1 + ks[1];
#define LTX_TF_ROUND(R)                   \
    x0 += x1;                             \
    x1 = (x1 << (R)) | (x1 >> (32 - (R))); \
    x1 ^= x0;
#define LTX_TF_EVEN LTX_TF_ROUND(13) LTX_TF_ROUND(15) LTX_TF_ROUND(26) LTX_TF_ROUND(6)
#define LTX_TF_ODD LTX_TF_ROUND(17) LTX_TF_ROUND(29) LTX_TF_ROUND(16) LTX_TF_ROUND(24)
    LTX_TF_EVEN x0 += ks[1]; x1 += ks[2] + 1u;
    LTX_TF_ODD  x0 += ks[2]; x1 += ks[0] + 2u;
    LTX_TF_EVEN x0 += ks[0]; x1 += ks[1] + 3u;
    LTX_TF_ODD  x0 += ks[1]; x1 += ks[2] + 4u;
    LTX_TF_EVEN x0 += ks[2]; x1 += ks[0] + 5u;
#undef LTX_TF_EVEN
#undef LTX_TF_ODD
#undef LTX_TF_ROUND
    r0 = x0;
    r1 = x1;
}

LTX_DEVFN float mlx_erfinv_dev(float a) {  // mlx_erfinv (hostmath.cpp), every fma explicit
    float t = fmaf(a, 0.0f - a, 1.0f);
    t = logf(t);
    float p;
    if (fabsf(t) > 6.125f) {
        p = 3.03697567e-10f;
        p = fmaf(p, t, 2.93243101e-8f);
        p = fmaf(p, t, 1.22150334e-6f);
        p = fmaf(p, t, 2.84108955e-5f);
        p = fmaf(p, t, 3.93552968e-4f);
        p = fmaf(p, t, 3.02698812e-3f);
        p = fmaf(p, t, 4.83185798e-3f);
        p = fmaf(p, t, -2.64646143e-1f);
        p = fmaf(p, t, 8.40016484e-1f);
    } else {
        p = 5.43877832e-9f;
        p = fmaf(p, t, 1.43285448e-7f);
        p = fmaf(p, t, 1.22774793e-6f);
        p = fmaf(p, t, 1.12963626e-7f);
        p = fmaf(p, t, -5.61530760e-5f);
        p = fmaf(p, t, -1.47697632e-4f);
        p = fmaf(p, t, 2.31468678e-3f);
        p = fmaf(p, t, 1.15392581e-2f);
        p = fmaf(p, t, -2.32015476e-1f);
        p = fmaf(p, t, 8.86226892e-1f);
    }
    return a * p;
}

LTX_DEVFN float bits_to_normal(uint32_t bits, const NoiseGroup& g, float scale) {
// hipcc's device default (-ffp-contract=fast-honor-pragmas) fuses a multiply and an add into one fma, and HIP's __fmul_rn / __fadd_rn
// are a plain * and + compiled under that default in their header, so they fuse too: the pragma on this function's own operators is
// what keeps the two roundings of the host build
#pragma clang fp contract(off)
    float u = (float)bits / g.maxval;  // correctly rounded (no fast-math flag on this build)
    u = u < g.upper ? u : g.upper;
    const float scaled = g.range * u;
    u = scaled + g.lo;
    return (g.sqrt2 * mlx_erfinv_dev(u)) * scale;  // the last multiply is the reference's separate noise * sigmas[0]
}

__global__ __launch_bounds__(kNoiseBlock) void mlx_normal_group_kernel(const NoiseGroup g) {
    // the job of this workgroup: uniform, from the prefix table (an empty job owns no workgroup and is stepped over)
    int j = 0;
    while (j < g.n_jobs - 1 && (int)blockIdx.x >= g.wg_end[j]) ++j;
    const ltx_noise_job& job = g.job[j];
    const int wg0 = j ? g.wg_end[j - 1] : 0;
    const long n = job.n;
    const long half = n >> 1, second = half + (n & 1);  // mlx_random_bits: where the second words of the pairs go
    const long i = (long)((int)blockIdx.x - wg0) * kNoiseBlock + threadIdx.x;
    if (i >= second) return;  // second = ceil(n / 2) counters in all
    const bool middle = i >= half;  // odd n only: counter (half, 0), word 0 alone
    uint32_t r0, r1;
    threefry2x32_dev(job.key[0], job.key[1], (uint32_t)i, middle ? 0u : (uint32_t)(second + i), r0, r1);
    if (job.raw_bits) {
        uint32_t* __restrict__ out = (uint32_t*)job.dst;
        out[i] = r0;
        if (!middle) out[second + i] = r1;
    } else {
        float* __restrict__ out = job.dst;
        out[i] = bits_to_normal(r0, g, job.scale);
        if (!middle) out[second + i] = bits_to_normal(r1, g, job.scale);
    }
}

}  // namespace

void mlx_normal_group_check(const ltx_noise_job* jobs, int n_jobs) {
    LTX_REQUIRE(n_jobs >= 0 && (jobs || n_jobs == 0), "mlx normal group: %d jobs, or a null job array", n_jobs);
    for (int j = 0; j < n_jobs; ++j) {
        LTX_REQUIRE(jobs[j].n >= 0 && jobs[j].n < (1L << 31), "mlx normal group: job %d has n=%ld outside 0 .. 2^31 - 1 (the counters are 32 bit)", j,
                    jobs[j].n);
        LTX_REQUIRE(jobs[j].n == 0 || jobs[j].dst, "mlx normal group: job %d has a null dst", j);
    }
}

int launch_mlx_normal_group(const ltx_noise_job* jobs, int n_jobs, hipStream_t stream) {
    mlx_normal_group_check(jobs, n_jobs);  // every check comes before the first launch: a refused call writes nothing
    int launches = 0;
    for (int first = 0; first < n_jobs; first += kNoiseJobsPerLaunch) {
        NoiseGroup g;
        g.n_jobs = n_jobs - first < kNoiseJobsPerLaunch ? n_jobs - first : kNoiseJobsPerLaunch;
        // the constants of mlx_random_normal (hostmath.cpp), by its expressions
        g.lo = std::nextafter(-1.0f, 0.0f);
        g.range = 1.0f - g.lo;
        g.upper = std::nextafter(1.0f, 0.0f);
        g.maxval = float(UINT32_MAX);
        g.sqrt2 = float(std::sqrt(2.0));
        long wgs = 0;
        double elems = 0;
        for (int j = 0; j < kNoiseJobsPerLaunch; ++j) {
            g.job[j] = j < g.n_jobs ? jobs[first + j] : ltx_noise_job{};
            const long counters = (g.job[j].n + 1) / 2;
            wgs += (counters + kNoiseBlock - 1) / kNoiseBlock;
            elems += (double)g.job[j].n;
            g.wg_end[j] = (int)wgs;
        }
        // n < 2^31 gives at most 2^22 workgroups per job and 2^28 per launch: the grid and the int table hold them
        if (wgs == 0) continue;
        ProfScope prof(PROF_ELEM, elems * 4, stream);  // algorithmic bytes: the f32 values written
        hipLaunchKernelGGL(mlx_normal_group_kernel, dim3((unsigned)wgs), dim3(kNoiseBlock), 0, stream, g);
        HIP_CHECK(hipGetLastError());
        ++launches;
    }
    return launches;
}
