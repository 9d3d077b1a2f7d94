// Fourth translation unit of liblmc_hip.so: cross-chain convergence diagnostics on the draws where they live (HBM).
//
// The reference has no diagnostics (ArviZ appears only in a docs recipe, /root/reference/docs/tutorials/
// framework_cookbook.rst:201-213): the definitions are this build's own -- split R-hat and the
// Geyer initial-monotone-sequence ESS of the Stan reference manual -- pinned against oracle/diagnostics_oracle.py.
// Everything reduces to per-dimension SUFFICIENT STATISTICS THAT ADD OVER CHAINS
//     sum_c mean_c, sum_c mean_c^2, sum_c var_c, sum_c acov_c[k]   (k = lag0 .. lag0 + 15)
// which is what makes the multi-GPU version one small all-reduce per block of 16 lags (littlemcmc_amd/diagnostics.py).
//
// chain_stats_kernel: one wavefront walks the sub-series [t0, t0 + n) of one chain for 64 dimensions (lane = dimension:
// a draw row is read as one coalesced 512-byte segment), first for the mean, then for the centred lagged products. The
// 16 lags of a pass are formed from register-resident windows -- the current block of 16 centred draws and the two
// blocks of the delayed stream -- with static indices only: 16 FMAs per draw and dimension, no ring-buffer moves.
// Blocks loop over chains and keep running sums; a second kernel adds the per-block partials in a fixed order, so the
// result is bit-reproducible (no floating-point atomics). Bound: HBM (the trace is read twice per pass; 16 loads of
// 512 B in flight per wave); algorithmic bytes = 2 x 8 x chains x n x dim per pass.
//
// Groups (targets.Batched: many posteriors in one job): chain j of the JOB is in group j / chains_per_group
// (lmc_target_param_row), and the statistics are wanted per group. The block index is (group, chain block, slab); a block
// loops over ITS group's chains inside the trace block, and the reduction adds a group's chain blocks. The ~4096
// wavefronts of a launch are shared by the groups, so many small groups get one block each and the partial buffer stays
// at the size of the result. The ungrouped call is the one-group call of the same code. The entry point's checks of the trace
// view and of the grouping are trace_span (lmc_trace_pass.hpp), shared by every pass over the trace.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lmc_hip.h"
#include "lmc_trace_pass.hpp"

namespace lmc {

constexpr int kDiagLags = 16;                 // lags per pass
constexpr int kDiagRows = 3 + kDiagLags;      // sum mean, sum mean^2, sum var, sum acov[16]

__global__ __launch_bounds__(64) void chain_stats_kernel(const double* __restrict__ x, long long chains, long long draws_stride,
                                                         int dim, long long t0, long long n, int lag0, int nslab,
                                                         int chain_blocks, long long first_chain, long long per, long long g0,
                                                         double* __restrict__ partial) {
    const int lane = static_cast<int>(threadIdx.x);
    const int slab = static_cast<int>(blockIdx.x) % nslab;
    const int gcb = static_cast<int>(blockIdx.x) / nslab;   // (group, chain block): the order of the partials
    const int cb = gcb % chain_blocks;
    // the chains of this block's group inside the trace block: the job's chains [g * per, (g + 1) * per), counted from
    // first_chain and clipped to [0, chains). All of it is the same in every lane (scalars, computed once per block).
    const long long g = g0 + gcb / chain_blocks;
    long long c_lo = g * per - first_chain, c_hi = c_lo + per;
    if (c_lo < 0) c_lo = 0;
    if (c_hi > chains) c_hi = chains;
    const int j = slab * 64 + lane;             // this lane's dimension
    const bool live = j < dim;
    double s_mean = 0.0, s_mean_sq = 0.0, s_var = 0.0;
    double s_acov[kDiagLags];
#pragma unroll
    for (int k = 0; k < kDiagLags; ++k) s_acov[k] = 0.0;
    const double inv_n = 1.0 / static_cast<double>(n);

    for (long long c = c_lo + cb; c < c_hi; c += chain_blocks) {
        const double* base = x + (c * draws_stride + t0) * dim + j;
        // ---- pass 1: mean (16 independent loads in flight)
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        long long t = 0;
        for (; t + 16 <= n; t += 16) {
            double v[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) v[i] = live ? base[(t + i) * dim] : 0.0;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i & 3] += v[i];
        }
        for (; t < n; ++t) acc[0] += live ? base[t * dim] : 0.0;
        const double mean = ((acc[0] + acc[1]) + (acc[2] + acc[3])) * inv_n;
        // ---- pass 2: centred lagged products, 16 draws per block
        double acov[kDiagLags];
#pragma unroll
        for (int k = 0; k < kDiagLags; ++k) acov[k] = 0.0;
        double w[kDiagLags];   // delayed stream, previous block: centred x at t = b*16 - lag0 - 16 + i (before block 0: zeros)
#pragma unroll
        for (int i = 0; i < kDiagLags; ++i) w[i] = 0.0;
        for (long long b = 0; b < n; b += kDiagLags) {
            double cur[kDiagLags], e[kDiagLags];   // e: delayed stream, current block: centred x at t = b - lag0 + i
#pragma unroll
            for (int i = 0; i < kDiagLags; ++i) {
                const long long tt = b + i;
                cur[i] = (live && tt < n) ? base[tt * dim] - mean : 0.0;
            }
            if (lag0 == 0) {
#pragma unroll
                for (int i = 0; i < kDiagLags; ++i) e[i] = cur[i];
            } else {
#pragma unroll
                for (int i = 0; i < kDiagLags; ++i) {
                    const long long tt = b - lag0 + i;
                    e[i] = (live && tt >= 0 && tt < n) ? base[tt * dim] - mean : 0.0;
                }
            }
            // acov[lag0 + k] += sum_i cur[i] * x(t_i - lag0 - k), the delayed value being e[i - k] or w[16 + i - k]
#pragma unroll
            for (int k = 0; k < kDiagLags; ++k) {
                double a = acov[k];
#pragma unroll
                for (int i = 0; i < kDiagLags; ++i) a = __builtin_fma(cur[i], (i >= k) ? e[i - k] : w[kDiagLags + i - k], a);
                acov[k] = a;
            }
#pragma unroll
            for (int i = 0; i < kDiagLags; ++i) w[i] = e[i];
        }
        s_mean += mean;
        s_mean_sq += mean * mean;
        if (lag0 == 0) s_var += acov[0] / static_cast<double>(n - 1);   // unbiased within-chain variance
#pragma unroll
        for (int k = 0; k < kDiagLags; ++k) s_acov[k] += acov[k] * inv_n;   // biased (1/n) autocovariance
    }
    double* out = partial + (static_cast<long long>(gcb) * nslab + slab) * kDiagRows * 64 + lane;
    out[0] = s_mean;
    out[64] = s_mean_sq;
    out[128] = s_var;
#pragma unroll
    for (int k = 0; k < kDiagLags; ++k) out[(3 + k) * 64] = s_acov[k];
}

// out[group][row][dim] = sum over the group's chain blocks, in block order (deterministic)
__global__ void chain_stats_reduce_kernel(const double* __restrict__ partial, int nslab, int chain_blocks, int dim,
                                          long long groups, double* __restrict__ out) {
    const long long idx = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    const long long block = static_cast<long long>(kDiagRows) * dim;   // one group's statistics block
    if (idx >= groups * block) return;
    const long long gi = idx / block;
    const int row = static_cast<int>((idx % block) / dim), j = static_cast<int>(idx % dim);
    const int slab = j / 64, lane = j % 64;
    double acc = 0.0;
    for (int cb = 0; cb < chain_blocks; ++cb)
        acc += partial[(((gi * chain_blocks + cb) * nslab + slab) * kDiagRows + row) * 64 + lane];
    out[idx] = acc;
}

}  // namespace lmc

extern "C" int lmc_diag_lags_per_pass(void) { return lmc::kDiagLags; }

// See include/lmc_hip.h. x and out are DEVICE pointers on the current device; the work is enqueued on `stream`.
extern "C" int lmc_diag_chain_stats_grouped(const double* x, int64_t chains, int64_t draws_stride, int32_t dim, int64_t t0,
                                            int64_t n, int32_t lag0, int64_t first_chain, int64_t chains_per_group, double* out,
                                            void* stream) {
    using namespace lmc;
    const int64_t lim = int64_t(1) << 31;
    TraceSpan span;
    if (!out || n < 2 || lag0 < 0 || trace_span(x, chains, draws_stride, dim, t0, n, first_chain, chains_per_group, &span) != LMC_OK)
        return LMC_ERR_INVALID;
    const int64_t per = span.per, g0 = span.g0, groups = span.groups;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int nslab = (dim + 63) / 64;
    long long cbl = (4096 / nslab) / groups;            // ~16 wavefronts per CU, each looping over chains: shared by the groups
    if (cbl > per) cbl = per;
    if (cbl > chains) cbl = chains;
    if (cbl < 1) cbl = 1;
    const int chain_blocks = static_cast<int>(cbl);
    const long long blocks = groups * chain_blocks * nslab;
    const long long total = groups * kDiagRows * dim;
    if (blocks >= lim || (total + 255) / 256 >= lim) return LMC_ERR_INVALID;
    double* partial = nullptr;
    const size_t bytes = static_cast<size_t>(blocks) * kDiagRows * 64 * sizeof(double);
    if (hipMallocAsync(reinterpret_cast<void**>(&partial), bytes, s) != hipSuccess) return LMC_ERR_HIP;
    (void)hipGetLastError();
    hipLaunchKernelGGL(chain_stats_kernel, dim3(static_cast<unsigned>(blocks)), dim3(64), 0, s, x, static_cast<long long>(chains),
                       static_cast<long long>(draws_stride), dim, static_cast<long long>(t0), static_cast<long long>(n), lag0,
                       nslab, chain_blocks, static_cast<long long>(first_chain), static_cast<long long>(per),
                       static_cast<long long>(g0), partial);
    hipLaunchKernelGGL(chain_stats_reduce_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, s, partial, nslab,
                       chain_blocks, dim, static_cast<long long>(groups), out);
    const hipError_t err = hipGetLastError();
    (void)hipFreeAsync(partial, s);
    return err == hipSuccess ? LMC_OK : LMC_ERR_HIP;
}

// One group that holds every chain of the block.
extern "C" int lmc_diag_chain_stats(const double* x, int64_t chains, int64_t draws_stride, int32_t dim, int64_t t0, int64_t n,
                                    int32_t lag0, double* out, void* stream) {
    return lmc_diag_chain_stats_grouped(x, chains, draws_stride, dim, t0, n, lag0, 0, chains, out, stream);
}
