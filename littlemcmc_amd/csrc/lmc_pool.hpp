// Host-callable launchers of the pooled second-moment kernels (lmc_pool.hip); called by the C ABI in lmc_engine.hip.
// The statistic a shared dense mass matrix is adapted from: one SNAPSHOT adds the current position of every chain,
// q [C][dpad], to   n,  s = sum (q - shift),  S = sum (q - shift)(q - shift)^T   (float64, lower triangle of 16 x 16 tiles).
// Return value of the launchers: that of launch() (lmc_dispatch.hpp).
#pragma once
#include <hip/hip_runtime.h>

namespace lmc {

constexpr int kPoolChunk = 32;        // chains a workgroup stages through LDS at a time (8 k-blocks of v_mfma_f64_16x16x4_f64)
constexpr int kPoolWaves = 8;         // wavefronts of a workgroup: they deal the lower-triangle tiles among themselves
constexpr int kPoolMaxGroups = 512;   // workgroups the chains (the K dimension) are split over: two per compute unit, so that one
                                      // stages its next chunk while the other is in its products (dpad 256: 256, one per unit --
                                      // its accumulators leave room for one workgroup only)
constexpr int kPoolReduceSplit = 4;   // pool_reduce_kernel: quarters of the workgroup range summed side by side, then in order
constexpr int kPoolMaxDpad = 256;

struct PoolArrays {
    long long* n;      // [1] samples so far
    double* shift;     // [dpad] column mean of the first snapshot after a reset
    double* s;         // [dpad]
    double* S;         // [dpad][dpad] row-major; tiles above the diagonal are never written
    double* part;      // [groups][tiles][256]: every workgroup's share of S, tile by tile in the MFMA result layout
    double* spart;     // [groups][dpad]: every workgroup's share of s (or of the plain column sum, first snapshot)
    int dpad, groups, chunks_per_group;
};

__host__ __device__ inline int pool_tiles(int dpad) { return (dpad / 16) * (dpad / 16 + 1) / 2; }
// how the chains are split over workgroups: a function of the shape alone, so that the summation order -- and with it
// every bit of the result -- is the same from run to run and from engine to engine
inline void pool_plan(int chains, int dpad, int* groups, int* chunks_per_group) {
    const int chunks = (chains + kPoolChunk - 1) / kPoolChunk;
    const int max_groups = dpad > 128 ? kPoolMaxGroups / 2 : kPoolMaxGroups;
    *chunks_per_group = (chunks + max_groups - 1) / max_groups;
    *groups = (chunks + *chunks_per_group - 1) / *chunks_per_group;
}

// shift <- column mean of q (two kernels: per-workgroup column sums, then their sum in workgroup order)
int pool_launch_shift(hipStream_t stream, const PoolArrays& P, const double* q, int chains);
// n, s, S += this snapshot (the MFMA kernel writes partials, a second kernel adds them in workgroup order)
int pool_launch_accumulate(hipStream_t stream, const PoolArrays& P, const double* q, int chains);
// Stan's restart of dual averaging after a metric change, per chain: mu <- log(10 exp(log_step)), log_bar <- 0, hbar <- 0, count <- 1
int pool_launch_restart_da(hipStream_t stream, double* da, int* da_count, int chains);

}  // namespace lmc
