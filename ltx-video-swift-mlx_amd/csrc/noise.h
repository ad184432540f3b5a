// noise.h - the MLX-compatible normal draws of a run, made on the device (hostmath.h has the algorithm and its host restatement).
// One launch fills any number of draws: a workgroup finds its job through a prefix table of per-job workgroup counts in the kernel
// arguments (as gemv_group_kernel does), one thread hashes one counter pair (i, second + i) with threefry2x32-20 and writes word 0 to
// element i and word 1 to element second + i (both stores coalesced over the wave); for an odd n the thread of the middle element hashes
// (half, 0) and keeps word 0. The bits -> normal tail restates mlx_random_normal operation by operation: a correctly rounded division,
// a separate multiply and add for range * u + lo (the host build does not contract it), fmaf for every fma of the erfinv polynomial,
// logf. Host and device can therefore differ only in the last place of logf. No LDS, no scratch.
#pragma once
#include "../../include/ltxhip.h"
#include "runtime.h"

constexpr int kNoiseJobsPerLaunch = 64;  // jobs of one launch (they travel by value in the kernel arguments); more are sent in chunks

// every check of launch_mlx_normal_group and nothing else: for a caller that must refuse before a launch of its own
void mlx_normal_group_check(const ltx_noise_job* jobs, int n_jobs);
// jobs: HOST array, dst DEVICE. Throws before any launch on n_jobs < 0, n < 0, n >= 2^31 or a null dst with n > 0; empty jobs and
// n_jobs == 0 do nothing. Returns the number of launches made.
int launch_mlx_normal_group(const ltx_noise_job* jobs, int n_jobs, hipStream_t stream);
