// Translation unit of liblmc_hip.so: threshold counts over the draws where they live (HBM) -- per (posterior, coefficient,
// threshold) the number of draws below and equal to the threshold, and per (posterior, coefficient) the number of NaN draws
// (littlemcmc_amd/diagnostics.py: threshold_counts, prob, direction, rope; predictive.exceedance; sbc.sbc_glm). include/lmc_hip.h
// states the definition (lmc_diag_threshold_counts). It is the inverse question of lmc_select.hip: which rank a value has.
//
// The statistic is a set of INTEGER COUNTS THAT ADD over chains, chain blocks and GPUs. The comparisons are IEEE numeric
// comparisons (v_cmp_lt_f64, v_cmp_eq_f64, v_cmp_u_f64), not the select's total order on the bits.
//
// threshold_count_kernel<W, KT>: the geometry of select_count_kernel<W> -- lane = dimension in slabs of W = 16 / 32 / 64
// columns, the lanes beyond W taking the next row (next three rows) so that a wavefront stays full at small dim, a workgroup
// counting its share (every chain_blocks-th chain) of ONE group's chains for one slab, kThrRows rows in flight per lane. In
// contrast to the select a lane holds its KT thresholds (2 KT VGPRs) and its 2 KT + 1 counters (32-bit) in REGISTERS: KT is a
// template parameter (1, 2, 4, 8, 16; the thresholds beyond n_thresholds are NaN, which count nothing) so that every index
// is a compile-time constant and nothing lives in scratch. The trace is read ONCE whatever K is. LDS is touched once, after
// the loop: one table tbl[2 KT + 1][W] of 32-bit counters per workgroup, zeroed, added to with LDS integer atomics, and its
// non-zero sums added to the result with 64-bit integer global atomics (the result is zeroed first; integer addition is exact
// in any order, so the counts are reproducible).
// A 32-bit counter cannot wrap: the host gives a block at most (2^32 - 1) / n chains, so no block counts 2^32 draws.
// The entry point's checks of the trace view and of the grouping are trace_span (lmc_trace_pass.hpp).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lmc_hip.h"
#include "lmc_trace_pass.hpp"

namespace lmc {

constexpr int kThrThreads = 256;                    // 4 wavefronts share one table
constexpr int kThrWaves = kThrThreads / 64;
constexpr int kThrRows = 8;                         // loads a lane has in flight
constexpr int kThrBlocks = 1024;                    // workgroups aimed at: four per CU, each looping over chains

template <int W, int KT>
__global__ __launch_bounds__(kThrThreads) void threshold_count_kernel(const double* __restrict__ x, long long chains,
                                                                      long long draws_stride, int dim, long long t0, long long n,
                                                                      int nslab, int chain_blocks, long long first_chain,
                                                                      long long per, long long g0, int n_thr,
                                                                      const double* __restrict__ thr,
                                                                      unsigned long long* __restrict__ counts) {
    constexpr int RP = 64 / W;                      // rows a wavefront reads at once
    constexpr int NC = 2 * KT + 1;                  // counters of a lane
    __shared__ unsigned tbl[NC * W];
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    unsigned bid = blockIdx.x;                      // (group, chain block, slab)
    const int slab = static_cast<int>(bid % static_cast<unsigned>(nslab));
    bid /= static_cast<unsigned>(nslab);
    const int cb = static_cast<int>(bid % static_cast<unsigned>(chain_blocks));
    const long long gi = bid / static_cast<unsigned>(chain_blocks);
    // the chains of this block's group inside the trace block, as in select_count_kernel
    long long c_lo = (g0 + gi) * per - first_chain, c_hi = c_lo + per;
    if (c_lo < 0) c_lo = 0;
    if (c_hi > chains) c_hi = chains;
    const long long nc = (c_hi > c_lo + cb) ? (c_hi - c_lo - cb + chain_blocks - 1) / chain_blocks : 0;   // chains of this block

    const int col = lane % W, sub = lane / W;
    const int j = slab * W + col;                   // this lane's dimension
    const bool live = j < dim;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    double c[KT];
    unsigned cnt[NC];
#pragma unroll
    for (int k = 0; k < KT; ++k) c[k] = (live && k < n_thr) ? thr[(gi * n_thr + k) * dim + j] : qnan;
#pragma unroll
    for (int s = 0; s < NC; ++s) cnt[s] = 0u;

    constexpr int kTileRows = kThrRows * RP;
    const long long tiles = (n + kTileRows - 1) / kTileRows;
    for (long long item = wave; item < nc * tiles; item += kThrWaves) {
        const long long ch = c_lo + cb + (item / tiles) * chain_blocks;
        const long long tf = (item % tiles) * kTileRows + sub;
        const double* base = x + (ch * draws_stride + t0) * dim + j;
        double v[kThrRows];
        bool ok[kThrRows];
#pragma unroll
        for (int i = 0; i < kThrRows; ++i) {
            const long long t = tf + i * RP;
            ok[i] = live && t < n;
            v[i] = ok[i] ? base[t * dim] : qnan;    // a row that is not there counts nothing below or equal
        }
#pragma unroll
        for (int i = 0; i < kThrRows; ++i) {
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                cnt[2 * k] += (v[i] < c[k]) ? 1u : 0u;
                cnt[2 * k + 1] += (v[i] == c[k]) ? 1u : 0u;
            }
            cnt[2 * KT] += (ok[i] && v[i] != v[i]) ? 1u : 0u;
        }
    }
    for (int i = tid; i < NC * W; i += kThrThreads) tbl[i] = 0u;
    __syncthreads();
#pragma unroll
    for (int s = 0; s < NC; ++s)
        if (cnt[s] != 0u) atomicAdd(&tbl[s * W + col], cnt[s]);
    __syncthreads();
    const int nlive = 2 * n_thr + 1;                // the counters of the result: 2k, 2k + 1 for k < n_thr, then the NaN count
    for (int i = tid; i < nlive * W; i += kThrThreads) {
        const int s = i / W, jj = slab * W + i % W;
        const unsigned u = tbl[(s == nlive - 1 ? NC - 1 : s) * W + i % W];
        if (u != 0u && jj < dim) atomicAdd(&counts[(gi * nlive + s) * dim + jj], static_cast<unsigned long long>(u));
    }
}

template <int W>
static void threshold_launch(int kt, unsigned blocks, hipStream_t s, const double* x, long long chains, long long draws_stride,
                             int dim, long long t0, long long n, int nslab, int cbl, long long first_chain, long long per,
                             long long g0, int n_thr, const double* thr, unsigned long long* out) {
#define LMC_THRESHOLD_LAUNCH(KT)                                                                                              \
    hipLaunchKernelGGL((threshold_count_kernel<W, KT>), dim3(blocks), dim3(kThrThreads), 0, s, x, chains, draws_stride, dim,  \
                       t0, n, nslab, cbl, first_chain, per, g0, n_thr, thr, out)
    if (kt <= 1) LMC_THRESHOLD_LAUNCH(1);
    else if (kt <= 2) LMC_THRESHOLD_LAUNCH(2);
    else if (kt <= 4) LMC_THRESHOLD_LAUNCH(4);
    else if (kt <= 8) LMC_THRESHOLD_LAUNCH(8);
    else LMC_THRESHOLD_LAUNCH(16);
#undef LMC_THRESHOLD_LAUNCH
}

}  // namespace lmc

// See include/lmc_hip.h. x, thresholds and counts are DEVICE pointers on the current device; the work is enqueued on `stream`.
extern "C" int lmc_diag_threshold_counts(const double* x, int64_t chains, int64_t draws_stride, int32_t dim, int64_t t0,
                                         int64_t n, int64_t first_chain, int64_t chains_per_group, int32_t n_thresholds,
                                         const double* thresholds, int64_t* counts, void* stream) {
    using namespace lmc;
    const int64_t lim = int64_t(1) << 31;
    TraceSpan span;
    if (!thresholds || !counts || n_thresholds < 1 || n_thresholds > LMC_THRESHOLD_MAX || n >= lim ||
        trace_span(x, chains, draws_stride, dim, t0, n, first_chain, chains_per_group, &span) != LMC_OK)
        return LMC_ERR_INVALID;
    const int64_t per = span.per, g0 = span.g0, groups = span.groups;
    const int w = dim <= 16 ? 16 : (dim <= 32 ? 32 : 64);
    const int nslab = (dim + w - 1) / w;
    const int64_t in_group = per < chains ? per : chains;           // the most chains one group has in the block
    const int64_t fit = ((int64_t(1) << 32) - 1) / n;               // chains whose draws one 32-bit counter holds (>= 2)
    int64_t cbl = kThrBlocks / (groups * nslab);
    if (cbl > in_group) cbl = in_group;
    if (cbl < (in_group + fit - 1) / fit) cbl = (in_group + fit - 1) / fit;
    if (cbl < 1) cbl = 1;
    const int64_t blocks = groups * cbl * nslab;
    const int64_t total = groups * (2 * int64_t(n_thresholds) + 1) * dim;
    if (cbl >= lim || blocks >= lim || total >= (int64_t(1) << 39)) return LMC_ERR_INVALID;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(counts, 0, static_cast<size_t>(total) * sizeof(int64_t), s) != hipSuccess) return LMC_ERR_HIP;
    (void)hipGetLastError();
    unsigned long long* out = reinterpret_cast<unsigned long long*>(counts);
#define LMC_THRESHOLD_W(W)                                                                                                     \
    threshold_launch<W>(n_thresholds, static_cast<unsigned>(blocks), s, x, static_cast<long long>(chains),                     \
                        static_cast<long long>(draws_stride), dim, static_cast<long long>(t0), static_cast<long long>(n), nslab, \
                        static_cast<int>(cbl), static_cast<long long>(first_chain), static_cast<long long>(per),               \
                        static_cast<long long>(g0), n_thresholds, thresholds, out)
    if (w == 16) LMC_THRESHOLD_W(16);
    else if (w == 32) LMC_THRESHOLD_W(32);
    else LMC_THRESHOLD_W(64);
#undef LMC_THRESHOLD_W
    return hipGetLastError() == hipSuccess ? LMC_OK : LMC_ERR_HIP;
}
