// Seventh translation unit of liblmc_hip.so: one pass of a radix select over the draws where they live (HBM) -- exact
// posterior quantiles, credible intervals and tail-ESS (littlemcmc_amd/diagnostics.py: order_statistics, quantiles,
// intervals, tail_ess). include/lmc_hip.h states the key and the count (lmc_select_digit_counts).
//
// The statistic is an INTEGER HISTOGRAM THAT ADDS over chains, chain blocks and GPUs: for up to 16 rank slots at once, how
// many draws of a (group, dimension) carry digit b at `shift` among those that agree with the slot's prefix above it. Eight
// passes (shift 56, 48, .., 0), the host choosing a bucket after each, leave the key of the wanted order statistic, and the
// key decodes to the draw itself.
//
// select_count_kernel<W>: a workgroup of 16 wavefronts counts its share of ONE group's chains for one slab of W dimensions
// and one tile of rank slots into an LDS table tbl[slot][256 digits][W columns] of 32-bit counters (128 KiB: 2 slots at
// W = 64, 4 at W = 32, 8 at W = 16), then adds the non-zero counters to the result with 64-bit integer global atomics (the
// result is zeroed first; integer addition is exact in any order, so the counts are reproducible). lane = dimension: with
// W = 64 a wavefront reads a draw row as one coalesced 512-byte segment, as chain_stats_kernel does; at dim <= 32 (<= 16)
// the lanes beyond W take the next row (next three rows) of the same columns, so the wavefront stays full and a table column
// is half (a quarter) as wide. A lane's counter column (a / 4) % 32 is its own in every 32-lane group at W >= 32 -- no bank
// conflict whatever the digits; at W = 16 lanes l and l + 16 share a column (a two-way conflict, or the same address). All
// counters are shared by the block's 16 wavefronts: LDS integer atomics (ds_add_u32, no return value).
// The trace is read ceil(n_ranks / slots per block) times per pass (the slot tiles are neighbouring blocks, so the re-reads
// of a pass run together): once at shift 56, and e.g. twice at W = 32 with 8 ranks -- three probabilities' lo / hi ranks,
// the minimum and the maximum. Algorithmic bytes of a pass: 8 x chains x n x dim x that factor.
// A 32-bit counter cannot wrap: the host gives a block at most (2^32 - 1) / n chains, so no block counts 2^32 draws.
// The entry point's checks of the trace view and of the grouping are trace_span (lmc_trace_pass.hpp).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lmc_hip.h"
#include "lmc_trace_pass.hpp"

namespace lmc {

constexpr int kSelThreads = 1024;                   // 16 wavefronts share one table
constexpr int kSelWaves = kSelThreads / 64;
constexpr int kSelTable = 2 * 256 * 64;             // 32-bit counters: 128 KiB of the CU's 160 KiB
constexpr int kSelRows = 8;                         // loads a lane has in flight
static_assert(kSelTable * 4 == 131072, "the table plan");

// the IEEE total order on the bits: -NaN < -inf < .. < -0 < +0 < .. < +inf < +NaN
__device__ __forceinline__ unsigned long long select_key(unsigned long long u) {
    return (u >> 63) ? ~u : (u | (1ull << 63));
}

template <int W>
__global__ __launch_bounds__(kSelThreads) void select_count_kernel(const unsigned long long* __restrict__ x, long long chains,
                                                                   long long draws_stride, int dim, long long t0, long long n,
                                                                   int nslab, int ntile, int chain_blocks, long long first_chain,
                                                                   long long per, long long g0, int shift, int n_ranks,
                                                                   const unsigned long long* __restrict__ prefix,
                                                                   unsigned long long* __restrict__ counts) {
    constexpr int RP = 64 / W;                      // rows a wavefront reads at once
    constexpr int SL = kSelTable / (256 * W);       // rank slots of a block
    __shared__ unsigned tbl[kSelTable];
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    unsigned bid = blockIdx.x;                      // (group, chain block, slab, slot tile): the tiles of one read are neighbours
    const int tile = static_cast<int>(bid % static_cast<unsigned>(ntile));
    bid /= static_cast<unsigned>(ntile);
    const int slab = static_cast<int>(bid % static_cast<unsigned>(nslab));
    bid /= static_cast<unsigned>(nslab);
    const int cb = static_cast<int>(bid % static_cast<unsigned>(chain_blocks));
    const long long gi = bid / static_cast<unsigned>(chain_blocks);
    // the chains of this block's group inside the trace block, as in chain_stats_kernel
    long long c_lo = (g0 + gi) * per - first_chain, c_hi = c_lo + per;
    if (c_lo < 0) c_lo = 0;
    if (c_hi > chains) c_hi = chains;
    const long long nc = (c_hi > c_lo + cb) ? (c_hi - c_lo - cb + chain_blocks - 1) / chain_blocks : 0;   // chains of this block
    const int r0 = tile * SL;
    const int nr = (n_ranks - r0 < SL) ? n_ranks - r0 : SL;
    for (int i = tid; i < kSelTable; i += kSelThreads) tbl[i] = 0u;
    __syncthreads();

    const int col = lane % W, sub = lane / W;
    const int j = slab * W + col;                   // this lane's dimension
    const bool live = j < dim;
    const int hs = shift + 8;                       // the prefix's digits lie at and above this bit
    unsigned long long pf[SL];
#pragma unroll
    for (int r = 0; r < SL; ++r)
        pf[r] = (live && r < nr && hs < 64) ? prefix[(gi * n_ranks + r0 + r) * dim + j] : 0ull;

    constexpr int kTileRows = kSelRows * RP;
    const long long tiles = (n + kTileRows - 1) / kTileRows;
    for (long long item = wave; item < nc * tiles; item += kSelWaves) {
        const long long c = c_lo + cb + (item / tiles) * chain_blocks;
        const long long tf = (item % tiles) * kTileRows + sub;
        const unsigned long long* base = x + (c * draws_stride + t0) * dim + j;
        unsigned long long u[kSelRows];
#pragma unroll
        for (int i = 0; i < kSelRows; ++i) {
            const long long t = tf + i * RP;
            u[i] = (live && t < n) ? base[t * dim] : 0ull;
        }
#pragma unroll
        for (int i = 0; i < kSelRows; ++i) {
            if (!(live && tf + i * RP < n)) continue;
            const unsigned long long k = select_key(u[i]);
            const unsigned b = static_cast<unsigned>(k >> shift) & 255u;
#pragma unroll
            for (int r = 0; r < SL; ++r)
                if (r < nr && (hs >= 64 || ((k ^ pf[r]) >> (hs & 63)) == 0ull)) atomicAdd(&tbl[(r * 256 + b) * W + col], 1u);
        }
    }
    __syncthreads();
    for (int i = tid; i < nr * 256 * W; i += kSelThreads) {
        const unsigned v = tbl[i];
        const int jj = slab * W + i % W;
        if (v != 0u && jj < dim)
            atomicAdd(&counts[((gi * n_ranks + r0) * 256 + i / W) * dim + jj], static_cast<unsigned long long>(v));
    }
}

}  // namespace lmc

// See include/lmc_hip.h. x, prefix and counts are DEVICE pointers on the current device; the work is enqueued on `stream`.
extern "C" int lmc_select_digit_counts(const double* x, int64_t chains, int64_t draws_stride, int32_t dim, int64_t t0, int64_t n,
                                       int64_t first_chain, int64_t chains_per_group, int32_t shift, int32_t n_ranks,
                                       const uint64_t* prefix, int64_t* counts, void* stream) {
    using namespace lmc;
    const int64_t lim = int64_t(1) << 31;
    TraceSpan span;
    if (!counts || n >= lim || trace_span(x, chains, draws_stride, dim, t0, n, first_chain, chains_per_group, &span) != LMC_OK)
        return LMC_ERR_INVALID;
    if (shift < 0 || shift > 56 || shift % 8 != 0 || n_ranks < 1 || n_ranks > LMC_SELECT_MAX_RANKS) return LMC_ERR_INVALID;
    if (shift == 56 ? n_ranks != 1 : !prefix) return LMC_ERR_INVALID;
    const int64_t per = span.per, g0 = span.g0, groups = span.groups;
    const int w = dim <= 16 ? 16 : (dim <= 32 ? 32 : 64);
    const int slots = kSelTable / (256 * w);
    const int nslab = (dim + w - 1) / w, ntile = (n_ranks + slots - 1) / slots;
    const int64_t in_group = per < chains ? per : chains;           // the most chains one group has in the block
    const int64_t fit = ((int64_t(1) << 32) - 1) / n;               // chains whose draws one 32-bit counter holds (>= 2)
    int64_t cbl = 512 / (groups * nslab * ntile);                   // about two workgroups per CU, each looping over chains
    if (cbl > in_group) cbl = in_group;
    if (cbl < (in_group + fit - 1) / fit) cbl = (in_group + fit - 1) / fit;
    if (cbl < 1) cbl = 1;
    const int64_t blocks = groups * cbl * nslab * ntile;
    const int64_t total = groups * n_ranks * 256 * dim;
    if (cbl >= lim || blocks >= lim || (total + 255) / 256 >= lim) return LMC_ERR_INVALID;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(counts, 0, static_cast<size_t>(total) * sizeof(int64_t), s) != hipSuccess) return LMC_ERR_HIP;
    (void)hipGetLastError();
    const unsigned long long* xb = reinterpret_cast<const unsigned long long*>(x);
    const unsigned long long* pb = reinterpret_cast<const unsigned long long*>(prefix);
    unsigned long long* out = reinterpret_cast<unsigned long long*>(counts);
#define LMC_SELECT_LAUNCH(W)                                                                                                   \
    hipLaunchKernelGGL(select_count_kernel<W>, dim3(static_cast<unsigned>(blocks)), dim3(kSelThreads), 0, s, xb,               \
                       static_cast<long long>(chains), static_cast<long long>(draws_stride), dim, static_cast<long long>(t0),  \
                       static_cast<long long>(n), nslab, ntile, static_cast<int>(cbl), static_cast<long long>(first_chain),    \
                       static_cast<long long>(per), static_cast<long long>(g0), shift, n_ranks, pb, out)
    if (w == 16) LMC_SELECT_LAUNCH(16);
    else if (w == 32) LMC_SELECT_LAUNCH(32);
    else LMC_SELECT_LAUNCH(64);
#undef LMC_SELECT_LAUNCH
    return hipGetLastError() == hipSuccess ? LMC_OK : LMC_ERR_HIP;
}
