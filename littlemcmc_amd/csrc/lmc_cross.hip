// Translation unit of liblmc_hip.so: the co-moment matrix of every posterior of a job, from the draws where they lie (HBM)
// -- posterior covariance and correlation, the sd of a contrast, a dense mass matrix for the next run
// (littlemcmc_amd/diagnostics.py: cross_moments, covariance, contrasts). include/lmc_hip.h states the result
// (lmc_diag_cross_moments).
//
// Per group the statistic is the contraction  S = X^T X  with X = x - shift over the group's (chain, draw) rows inside the
// block, the contraction lmc_pool.hip makes for one snapshot of positions, on the same instruction: 16 x 16 tiles of the
// lower triangle, each the sum of v_mfma_f64_16x16x4_f64 with A[i][k] = X[k][16 ti + i], B[k][j] = X[k][16 tj + j].
//
// Rows. A group's rows are its present chains' draws [t0, t0 + n): chains lie draws_stride * dim doubles apart, the draws
// of one chain follow each other, dim unpadded doubles each (8-byte aligned only). The unit of work is an ITEM: up to KC
// consecutive draws of one chain, contiguous in memory. The items of a group -- (chain, chunk) in that order -- are dealt to
// the group's wpg workgroups in contiguous ranges of ipw items (cross_plan: a function of the shapes alone), so a
// workgroup's rows never cross a group boundary. A workgroup stages an item centred into LDS, thread = (row, column) with
// the column fastest (a row segment of a panel is read as one contiguous run), columns beyond dim and rows beyond the item
// staged as ZEROS (never as -shift: they contribute exact zeros, and a non-finite shift stays in its own column).
// Tiles. dp16 = dim rounded up to 16, NT = dp16 / 16 tile rows. The geometry class is NTL, the tile columns a workgroup
// stages per side, chosen at compile time (with_int):
//     NTL 1 (dim <= 16):   1 tile,   KC 128, every wave the same tile over its own 16 of the 128 rows
//     NTL 2 (dim <= 32):   3 tiles,  KC 128, every wave the three tiles over its own 16 rows
//     NTL 4 (dim <= 64):  10 tiles,  KC 64,  two waves deal the tiles, four row quarters of 16 rows
//     NTL 8 (dim <= 512): panels of 8 x 8 tiles over the second grid dimension, KC 32, the eight waves deal a panel's tiles
//                         (36 live on a diagonal panel, 64 below); a panel stages only its own 128 + 128 columns
// The row sub-ranges of a workgroup are added in LDS in their order before the tiles are written; every workgroup writes
// its tiles and (diagonal panels) its column sums as partials, and cross_finish_kernel adds them in workgroup order, then
// forms  mean = shift + s / n_g,  m2 = S - s s^T / n_g  and mirrors the lower triangle. The shift itself is the column mean
// from a first kernel pair over the same split (per-workgroup column sums, added in workgroup order): column i's shift
// reads column i only. No floating-point atomics anywhere: the same draws give the same bits.
//
// Bound from shapes: two reads of the sub-series, 2 * 8 * rows * dim bytes (at NTL 8 a panel re-reads its columns: the 10
// panels of dim 512 read 5 x the columns, from L2 for the most part) and rows * dp16^2 / 2 FMA on the matrix pipe (the
// diagonal tiles are formed whole, NT / 2 tiles more than the half). On an MI355X -- about 6.3 TB/s achievable of the 8 TB/s
// of its HBM, and 78.6 TFLOP/s of FP64 on the matrix pipe by the public specification, half the f32-input rate -- 16 dim
// bytes against dim^2 FLOP per row balance at dim = 16 * 78.6 / 6.3 = 200: the pass is HBM-bound below dim ~ 200 and bound by
// the matrix pipe above.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lmc_hip.h"
#include "lmc_trace_pass.hpp"
#include "lmc_dispatch.hpp"

namespace lmc {

typedef double cross_v4d __attribute__((ext_vector_type(4)));   // (v4d of lmc_pool.hip, restated)

constexpr int kCrossThreads = 512;        // eight wavefronts
constexpr int kCrossWaves = kCrossThreads / 64;
constexpr int kCrossBudget = 1024;        // workgroups of a launch (groups x panels x wpg) while a group has items to split:
                                          // four per compute unit, so that some stage while others multiply
constexpr int kCrossPanel = 8;            // tile rows of a panel at NTL 8
constexpr int kCrossSumThreads = 256;

// geometry class of a dimension, and the draws of an item in that class
__host__ __device__ constexpr int cross_ntl(int dim) { return dim <= 16 ? 1 : (dim <= 32 ? 2 : (dim <= 64 ? 4 : 8)); }
__host__ __device__ constexpr int cross_kc(int ntl) { return ntl <= 2 ? 128 : (ntl == 4 ? 64 : 32); }

struct CrossArgs {
    long long chains, stride, t0, n, first_chain, per, g0;
    long long chunks, ipw;   // items of one chain; items of one workgroup
    int dim, dp16, wpg, ttot;
    double* part;    // [groups][wpg][ttot][256]: every workgroup's share of S, tile by tile in the MFMA result layout
    double* spart;   // [groups][wpg][dp16]: every workgroup's column sums (first of x, then of x - shift)
    double* shift;   // [groups][dp16]
};

// How a group's items are split over its workgroups: a function of the shapes alone (the summation order is fixed by it).
// in_group: the most chains one group has in the block.
inline void cross_plan(int64_t groups, int64_t in_group, int64_t n, int dim, int64_t* chunks, int64_t* ipw, int64_t* wpg, int* panels) {
    const int ntl = cross_ntl(dim), nt = (dim + 15) / 16;
    const int mb = ntl == 8 ? (nt + kCrossPanel - 1) / kCrossPanel : 1;
    *panels = mb * (mb + 1) / 2;
    *chunks = (n + cross_kc(ntl) - 1) / cross_kc(ntl);
    const int64_t items = in_group * *chunks;
    int64_t w = kCrossBudget / (groups * *panels);
    if (w > items) w = items;
    if (w < 1) w = 1;
    *ipw = (items + w - 1) / w;
    *wpg = (items + *ipw - 1) / *ipw;
}

// tile t of the lower triangle, row by row: t = ti (ti + 1) / 2 + tj, tj <= ti   (pool_tile_of of lmc_pool.hip, restated)
__device__ __forceinline__ void cross_tile_of(int t, int& ti, int& tj) {
    int i = 0;
    while ((i + 1) * (i + 2) / 2 <= t) ++i;
    ti = i;
    tj = t - i * (i + 1) / 2;
}

// the chains [c_lo, c_hi) of touched group gi inside the block (as chain_stats_kernel clips them)
__device__ __forceinline__ void cross_group_chains(const CrossArgs& A, long long gi, long long& c_lo, long long& c_hi) {
    c_lo = (A.g0 + gi) * A.per - A.first_chain;
    c_hi = c_lo + A.per;
    if (c_lo < 0) c_lo = 0;
    if (c_hi > A.chains) c_hi = A.chains;
}

// sum over k in [0, count) of p[k * stride], in order, eight loads in flight (pool_sum_groups)
__device__ __forceinline__ double cross_sum_in_order(const double* __restrict__ p, size_t stride, int count) {
    double a = 0.0;
    int g = 0;
    for (; g + 8 <= count; g += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = p[static_cast<size_t>(g + u) * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) a += v[u];
    }
    for (; g < count; ++g) a += p[static_cast<size_t>(g) * stride];
    return a;
}

// spart[group][workgroup][column] = the plain column sums of the workgroup's items. Up to 256 columns at a time, thread =
// (row, column) with 256 / w rows side by side; the rows of a column are added in LDS in row-lane order.
__global__ __launch_bounds__(kCrossSumThreads) void cross_colsum_kernel(const double* __restrict__ x, CrossArgs A, int kc) {
    __shared__ double cs[kCrossSumThreads];
    const int tid = static_cast<int>(threadIdx.x);
    const long long gi = blockIdx.x / static_cast<unsigned>(A.wpg), wb = blockIdx.x % static_cast<unsigned>(A.wpg);
    long long c_lo, c_hi;
    cross_group_chains(A, gi, c_lo, c_hi);
    const long long items = (c_hi > c_lo ? c_hi - c_lo : 0) * A.chunks;
    const long long it0 = wb * A.ipw;
    long long it1 = it0 + A.ipw;
    if (it1 > items) it1 = items;
    for (int cb = 0; cb < A.dim; cb += kCrossSumThreads) {
        const int w = A.dim - cb < kCrossSumThreads ? A.dim - cb : kCrossSumThreads;
        const int col = tid % w, r0 = tid / w, rstep = kCrossSumThreads / w;
        const bool active = r0 < rstep;
        double sum = 0.0;
        for (long long it = it0; it < it1; ++it) {
            const long long t_lo = (it % A.chunks) * kc;
            const int rows = static_cast<int>(A.n - t_lo < kc ? A.n - t_lo : kc);
            const double* base = x + ((c_lo + it / A.chunks) * A.stride + A.t0 + t_lo) * A.dim + cb + col;
            if (!active) continue;
            int r = r0;
            for (; r + 3 * rstep < rows; r += 4 * rstep) {
                double v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = base[static_cast<long long>(r + u * rstep) * A.dim];
#pragma unroll
                for (int u = 0; u < 4; ++u) sum += v[u];
            }
            for (; r < rows; r += rstep) sum += base[static_cast<long long>(r) * A.dim];
        }
        cs[tid] = active ? sum : 0.0;
        __syncthreads();
        if (tid < w) {
            double a = cs[tid];
            for (int k = 1; k < rstep; ++k) a += cs[tid + k * w];
            A.spart[static_cast<size_t>(blockIdx.x) * A.dp16 + cb + tid] = a;
        }
        __syncthreads();
    }
}

// shift[group][column] = (the workgroups' column sums, added in workgroup order) / n_g
__global__ __launch_bounds__(kCrossSumThreads) void cross_shift_kernel(CrossArgs A) {
    const long long gi = blockIdx.x;
    long long c_lo, c_hi;
    cross_group_chains(A, gi, c_lo, c_hi);
    const double ng = static_cast<double>((c_hi - c_lo) * A.n);
    for (int j = static_cast<int>(threadIdx.x); j < A.dim; j += kCrossSumThreads)
        A.shift[gi * A.dp16 + j] = cross_sum_in_order(A.spart + static_cast<size_t>(gi) * A.wpg * A.dp16 + j, A.dp16, A.wpg) / ng;
}

template <int NTL>
struct CrossGeom {
    static constexpr int W = 16 * NTL;                         // columns staged per side
    static constexpr int XS = NTL == 1 ? 16 : W + 16;          // row pitch in LDS: the k-rows a half-wave reads on disjoint banks
    static constexpr int KC = cross_kc(NTL);                   // rows of an item
    static constexpr int RS = NTL <= 2 ? 8 : (NTL == 4 ? 4 : 1);   // row sub-ranges of a chunk, a set of waves each
    static constexpr int TW = kCrossWaves / RS;                // waves that deal the tiles among themselves
    static constexpr int T = NTL == 8 ? 64 : NTL * (NTL + 1) / 2;  // tiles of a panel (a diagonal panel: the first NTL (NTL + 1) / 2)
    static constexpr int TPW = (T + TW - 1) / TW;
    static constexpr int RPP = kCrossThreads / W;              // rows staged per pass
    static constexpr int PASSES = KC / RPP;
    static constexpr int KBW = KC / 4 / RS;                    // k-blocks of a wave per chunk
    static constexpr int kSides = NTL == 8 ? 2 : 1;
    static constexpr int kStage = kSides * KC * XS;
    static constexpr int kLds = kStage > T * 256 ? (kStage > kCrossThreads ? kStage : kCrossThreads)
                                                 : (T * 256 > kCrossThreads ? T * 256 : kCrossThreads);   // doubles
    static_assert(KC % RPP == 0 && (KC / 4) % RS == 0 && kCrossWaves % RS == 0, "the chunk plan");
};

// one side of a chunk: rows [0, rows) of `base` (row pitch dim), column c of the side -> xs[row][col] centred, zeros elsewhere
template <class G>
__device__ __forceinline__ void cross_stage(const double* __restrict__ base, int dim, int rows, bool live, int c, double sh,
                                            double* xs, int col, int r0, double& colsum) {
    double v[G::PASSES];
#pragma unroll
    for (int p = 0; p < G::PASSES; ++p) {
        const int r = r0 + p * G::RPP;
        v[p] = (live && r < rows) ? base[static_cast<long long>(r) * dim + c] : 0.0;
    }
#pragma unroll
    for (int p = 0; p < G::PASSES; ++p) {
        const int r = r0 + p * G::RPP;
        double d = 0.0;
        if (live && r < rows) {
            d = v[p] - sh;
            colsum += d;
        }
        xs[r * G::XS + col] = d;
    }
}

template <int NTL>
__global__ __launch_bounds__(kCrossThreads) void cross_accumulate_kernel(const double* __restrict__ x, CrossArgs A) {
    typedef CrossGeom<NTL> G;
    extern __shared__ double cross_lds[];
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int rs = wave / G::TW, tw = wave % G::TW;
    const long long gi = blockIdx.x / static_cast<unsigned>(A.wpg), wb = blockIdx.x % static_cast<unsigned>(A.wpg);
    int pi = 0, pj = 0;
    if (NTL == 8) cross_tile_of(static_cast<int>(blockIdx.y), pi, pj);
    const bool diag = pi == pj;
    double* xa = cross_lds;
    double* xb = diag ? xa : cross_lds + G::KC * G::XS;
    long long c_lo, c_hi;
    cross_group_chains(A, gi, c_lo, c_hi);
    const long long items = (c_hi > c_lo ? c_hi - c_lo : 0) * A.chunks;
    const long long it0 = wb * A.ipw;
    long long it1 = it0 + A.ipw;
    if (it1 > items) it1 = items;

    const int col = tid % G::W, r0 = tid / G::W;
    const int ca = G::W * pi + col, cb = G::W * pj + col;
    const bool live_a = ca < A.dim, live_b = cb < A.dim;
    const double sh_a = live_a ? A.shift[gi * A.dp16 + ca] : 0.0;
    const double sh_b = (!diag && live_b) ? A.shift[gi * A.dp16 + cb] : 0.0;
    double colsum = 0.0, unused = 0.0;

    int ti[G::TPW], tj[G::TPW];
    bool live[G::TPW];
    cross_v4d acc[G::TPW];
#pragma unroll
    for (int u = 0; u < G::TPW; ++u) {
        const int t = tw + G::TW * u;
        if (NTL == 8 && !diag) {
            ti[u] = (t & 63) >> 3;
            tj[u] = t & 7;
            live[u] = t < 64;
        } else {
            cross_tile_of(t < G::T ? t : 0, ti[u], tj[u]);
            live[u] = t < NTL * (NTL + 1) / 2;
        }
        live[u] = live[u] && G::W * pi + 16 * ti[u] < A.dp16 && G::W * pj + 16 * tj[u] < A.dp16;   // (the same in every lane of a wave)
        acc[u] = cross_v4d{0.0, 0.0, 0.0, 0.0};
    }

    for (long long it = it0; it < it1; ++it) {
        const long long t_lo = (it % A.chunks) * G::KC;
        const int rows = static_cast<int>(A.n - t_lo < G::KC ? A.n - t_lo : G::KC);
        const double* base = x + ((c_lo + it / A.chunks) * A.stride + A.t0 + t_lo) * A.dim;
        __syncthreads();   // the previous chunk has been read by every wave
        cross_stage<G>(base, A.dim, rows, live_a, ca, sh_a, xa, col, r0, colsum);
        if (!diag) cross_stage<G>(base, A.dim, rows, live_b, cb, sh_b, xb, col, r0, unused);
        __syncthreads();
        // operand layout of the instruction: A[i][k] on lane i + 16 k, B[k][j] on lane j + 16 k
        const double* ar = xa + (lane >> 4) * G::XS + (lane & 15);
        const double* br = xb + (lane >> 4) * G::XS + (lane & 15);
#pragma unroll
        for (int kk = 0; kk < G::KBW; ++kk) {
            const int kb = rs * G::KBW + kk;
            if (4 * kb < rows) {   // (a k-block of rows beyond the item holds zeros)
#pragma unroll
                for (int u = 0; u < G::TPW; ++u) {
                    if (live[u]) {
                        const double a = ar[4 * kb * G::XS + 16 * ti[u]];
                        const double b = br[4 * kb * G::XS + 16 * tj[u]];
                        acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[u], 0, 0, 0);
                    }
                }
            }
        }
    }
    // the row sub-ranges, added in their order onto sub-range 0 (result layout: D[(lane >> 4) + 4 r][lane & 15] in register r)
    for (int r = 1; r < G::RS; ++r) {
        __syncthreads();
        if (rs == r) {
#pragma unroll
            for (int u = 0; u < G::TPW; ++u)
                if (live[u])
#pragma unroll
                    for (int q = 0; q < 4; ++q) cross_lds[(tw + G::TW * u) * 256 + 64 * q + lane] = acc[u][q];
        }
        __syncthreads();
        if (rs == 0) {
#pragma unroll
            for (int u = 0; u < G::TPW; ++u)
                if (live[u])
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[u][q] += cross_lds[(tw + G::TW * u) * 256 + 64 * q + lane];
        }
    }
    if (rs == 0) {
#pragma unroll
        for (int u = 0; u < G::TPW; ++u) {
            if (live[u]) {
                const int gti = NTL * pi + ti[u], gtj = NTL * pj + tj[u];
                double* o = A.part + (static_cast<size_t>(blockIdx.x) * A.ttot + gti * (gti + 1) / 2 + gtj) * 256 + lane;
#pragma unroll
                for (int q = 0; q < 4; ++q) o[64 * q] = acc[u][q];
            }
        }
    }
    if (!diag) return;   // (the same for the whole workgroup) column sums come from the diagonal panels
    __syncthreads();
    cross_lds[tid] = colsum;
    __syncthreads();
    if (tid < G::W && live_a) {
        double a = cross_lds[tid];
#pragma unroll
        for (int k = 1; k < G::RPP; ++k) a += cross_lds[tid + k * G::W];
        A.spart[static_cast<size_t>(blockIdx.x) * A.dp16 + ca] = a;
    }
}

// Block (group, t): t < ttot adds tile t's partials in workgroup order, subtracts s s^T / n_g and writes the tile's entries of
// the lower triangle and their mirror images; t == ttot writes the mean and n_g.
__global__ __launch_bounds__(256) void cross_finish_kernel(CrossArgs A, double* __restrict__ n_out, double* __restrict__ mean_out,
                                                           double* __restrict__ m2_out) {
    __shared__ double s_rc[32];
    const long long gi = blockIdx.x / static_cast<unsigned>(A.ttot + 1);
    const int t = static_cast<int>(blockIdx.x % static_cast<unsigned>(A.ttot + 1)), e = static_cast<int>(threadIdx.x);
    long long c_lo, c_hi;
    cross_group_chains(A, gi, c_lo, c_hi);
    const double ng = static_cast<double>((c_hi - c_lo) * A.n);
    const double* sp = A.spart + static_cast<size_t>(gi) * A.wpg * A.dp16;
    if (t == A.ttot) {
        for (int j = e; j < A.dim; j += 256)
            mean_out[gi * A.dim + j] = A.shift[gi * A.dp16 + j] + cross_sum_in_order(sp + j, A.dp16, A.wpg) / ng;
        if (e == 0) n_out[gi] = ng;
        return;
    }
    int ti, tj;
    cross_tile_of(t, ti, tj);
    if (e < 32) {
        const int c = e < 16 ? 16 * ti + e : 16 * tj + e - 16;
        s_rc[e] = c < A.dim ? cross_sum_in_order(sp + c, A.dp16, A.wpg) : 0.0;
    }
    __syncthreads();
    const int i = 16 * ti + (e >> 4), j = 16 * tj + (e & 15);
    if (i >= A.dim || j > i) return;
    const double S = cross_sum_in_order(A.part + (static_cast<size_t>(gi) * A.wpg * A.ttot + t) * 256 + e,
                                        static_cast<size_t>(A.ttot) * 256, A.wpg);
    const double v = S - s_rc[e >> 4] * s_rc[16 + (e & 15)] / ng;
    double* o = m2_out + static_cast<size_t>(gi) * A.dim * A.dim;
    o[static_cast<size_t>(i) * A.dim + j] = v;
    o[static_cast<size_t>(j) * A.dim + i] = v;
}

typedef void (*CrossKernel)(const double*, CrossArgs);

}  // namespace lmc

// See include/lmc_hip.h. x and the outputs are DEVICE pointers on the current device; the work is enqueued on `stream`.
extern "C" int lmc_diag_cross_moments(const double* x, int64_t chains, int64_t draws_stride, int32_t dim, int64_t t0, int64_t n,
                                      int64_t first_chain, int64_t chains_per_group, double* n_out, double* mean_out,
                                      double* m2_out, void* stream) {
    using namespace lmc;
    const int64_t lim = int64_t(1) << 31;
    TraceSpan span;
    if (!n_out || !mean_out || !m2_out || dim > LMC_CROSS_MAX_DIM ||
        trace_span(x, chains, draws_stride, dim, t0, n, first_chain, chains_per_group, &span) != LMC_OK)
        return LMC_ERR_INVALID;
    const int ntl = cross_ntl(dim), nt = (dim + 15) / 16;
    int panels = 1;
    int64_t chunks = 0, ipw = 0, wpg = 0;
    cross_plan(span.groups, span.per < chains ? span.per : chains, n, dim, &chunks, &ipw, &wpg, &panels);
    const int ttot = nt * (nt + 1) / 2;
    if (span.groups * wpg >= lim || span.groups * (ttot + 1) >= lim) return LMC_ERR_INVALID;
    const size_t slots = static_cast<size_t>(span.groups) * static_cast<size_t>(wpg);
    const size_t n_part = slots * ttot * 256, n_spart = slots * 16 * nt, n_shift = static_cast<size_t>(span.groups) * 16 * nt;
    hipStream_t s = static_cast<hipStream_t>(stream);
    double* scratch = nullptr;
    if (hipMallocAsync(reinterpret_cast<void**>(&scratch), (n_part + n_spart + n_shift) * sizeof(double), s) != hipSuccess) {
        (void)hipGetLastError();
        return LMC_ERR_HIP;
    }
    CrossArgs A;
    A.chains = chains, A.stride = draws_stride, A.t0 = t0, A.n = n, A.first_chain = first_chain, A.per = span.per, A.g0 = span.g0;
    A.chunks = chunks, A.ipw = ipw;
    A.dim = dim, A.dp16 = 16 * nt, A.wpg = static_cast<int>(wpg), A.ttot = ttot;
    A.part = scratch, A.spart = scratch + n_part, A.shift = scratch + n_part + n_spart;
    const unsigned wgs = static_cast<unsigned>(slots);
    const CrossKernel kernel = with_int<1, 2, 4, 8>(ntl, [](auto NTL) -> CrossKernel { return &cross_accumulate_kernel<NTL>; });
    const int lds = with_int<1, 2, 4, 8>(ntl, [](auto NTL) -> int { return CrossGeom<NTL>::kLds; }) * static_cast<int>(sizeof(double));
    int rc = launch(cross_colsum_kernel, dim3(wgs), dim3(kCrossSumThreads), 0, s, x, A, cross_kc(ntl));
    if (rc == 0) rc = launch(cross_shift_kernel, dim3(static_cast<unsigned>(span.groups)), dim3(kCrossSumThreads), 0, s, A);
    if (rc == 0) rc = launch(kernel, dim3(wgs, static_cast<unsigned>(panels)), dim3(kCrossThreads), lds, s, x, A);
    if (rc == 0)
        rc = launch(cross_finish_kernel, dim3(static_cast<unsigned>(span.groups * (ttot + 1))), dim3(256), 0, s, A, n_out, mean_out,
                    m2_out);
    (void)hipFreeAsync(scratch, s);
    return rc == 0 ? LMC_OK : LMC_ERR_HIP;
}
