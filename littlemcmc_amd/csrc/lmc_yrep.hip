// Tenth translation unit of liblmc_hip.so: replicated responses y_rep ~ p(y | q_s) of the GLM family for every draw, from the
// draws where they live (HBM). include/lmc_hip.h: lmc_glm_yrep, lmc_glm_yrep_stats; littlemcmc_amd/predictive.py: replicate(),
// predict_response(), ppc().
//
// The value of one (draw, observation) is yrep_value (lmc_yrep.hpp): a pure function of (seed, job chain, draw row,
// observation) on top of the sampler's own eta and mu (glm_eta_tile / glm_link_of_eta, lmc_predict_tile.hpp). Two kernels call it
// through ONE device function, yrep_tile:
//
// yrep_kernel: the decomposition of linpred_kernel (lmc_linpred.hip) -- one wavefront per (chain, segment of kLinSeg draws,
// observation block), lane = observation, kPredT draws a tile -- which stores every draw's 64 values as one coalesced 512-byte
// row of y[chain][t][W], the [chains, draws, dim] layout of a trace with dim = W: the radix select (lmc_select.hip) takes the
// exact order statistics of a new response from it. The y section of the rows is not read. Padding observations hold 0.
//
// yrep_stats_kernel: one wavefront per (chain, segment of kYrepSeg draws). The wave walks its draws kYrepT at a time and, per
// tile, ALL observation blocks of the row ascending: a lane accumulates the seven statistics of its observations 64 ob + lane
// of each draw, and at the end of the tile one wave reduction per plane and draw (wave_sum, or the same tree with min / max)
// gives T[chain][t][7] -- a trace-shaped block again; y_rep is never written. kYrepT = 4: seven lane partials a draw are 14
// VGPRs, 56 at four draws (112 at kPredT = 8, next to a sampler that wants its own registers for log, lgamma and Philox);
// glm_eta_tile and glm_link_of_eta are instantiated at that width. A draw's statistics do not merge with any other draw's,
// so the segment length is free: 32 draws give a job of few chains enough wavefronts.
// No LDS, no atomics. Order: lane partials over ob ascending, then the tree of lmc_wave.hpp: wave_sum.
//
// The sampler's loops make lanes diverge (a poisson count of a small mean takes its own number of uniforms); to keep ONE
// inlined copy of it per kernel the draws of a tile are walked by a rolled loop whose wave-uniform index selects eta and mu
// from, and y into, the tile's registers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lmc_hip.h"
#include "lmc_predict_tile.hpp"
#include "lmc_targets.hpp"
#include "lmc_trace_pass.hpp"
#include "lmc_yrep.hpp"

namespace lmc {

constexpr int kYrepOutSeg = 256;   // draws of one wavefront of yrep_kernel: lmc_linpred.hip's kLinSeg
constexpr int kYrepT = 4;          // draws of a tile of yrep_stats_kernel
constexpr int kYrepSeg = 32;       // draws of one wavefront of yrep_stats_kernel
constexpr int kYrepPlanes = LMC_YREP_STATS;
static_assert(kYrepOutSeg % kPredT == 0 && kYrepSeg % kYrepT == 0 && kYrepT <= kPredT, "segments are whole tiles");
static_assert(kYrepPlanes == 7, "sum, sum of squares, min, max, zeros, two Pearson statistics");

// y[i] = y_rep of the tile's draw i < k (wave-uniform k <= T) at the lane's observation `obs`; real = false (a padding
// observation) gives 0 and draws nothing. y[i] for i >= k is 0. yrep_value asks eta itself for a NaN, so mu may be the link's.
template <int T>
__device__ __forceinline__ void yrep_tile(int lik, const double (&eta)[T], const double (&mu)[T], int k, double sigma,
                                          uint32_t seed, uint32_t chain, uint32_t r0, uint32_t obs, bool real, double (&y)[T]) {
#pragma unroll
    for (int j = 0; j < T; ++j) y[j] = 0.0;
#pragma unroll 1
    for (int i = 0; i < k; ++i) {
        double e = eta[0], m = mu[0];
#pragma unroll
        for (int j = 1; j < T; ++j) {
            e = (i == j) ? eta[j] : e;
            m = (i == j) ? mu[j] : m;
        }
        double v = 0.0;
        if (real) v = yrep_value(lik, e, m, sigma, seed, chain, r0 + static_cast<uint32_t>(i), obs);
#pragma unroll
        for (int j = 0; j < T; ++j) y[j] = (i == j) ? v : y[j];
    }
}

// y_out[chain][t][W]
__global__ __launch_bounds__(64) void yrep_kernel(const double* __restrict__ x, long long draws_stride, int dim, long long t0,
                                                  long long n, const double* __restrict__ rows, long long row_len, int npad,
                                                  int ob0, int nobr, long long segs, long long first_chain, long long per,
                                                  uint32_t seed, double* __restrict__ y_out) {
    const unsigned lane = threadIdx.x;
    const int obr = static_cast<int>(blockIdx.x % static_cast<unsigned>(nobr));
    const long long cs = blockIdx.x / static_cast<unsigned>(nobr);
    const long long c = cs / segs, seg = cs % segs;
    const GlmRowView row = glm_row_view(rows, row_len, npad, (first_chain + c) / per);   // its y section is never read
    const unsigned obs = static_cast<unsigned>(ob0 + obr) * 64u + lane;
    const unsigned col0 = obs * 8u;
    const bool real = obs < static_cast<unsigned>(row.nobs);
    const uint32_t chain = static_cast<uint32_t>(first_chain + c);
    const double* xc = x + (c * draws_stride + t0) * dim;
    const long long W = static_cast<long long>(nobr) * 64;
    double* o = y_out + c * n * W + obr * 64 + lane;

    const DrawWindow win = draw_window(seg, kYrepOutSeg, n);
    for (long long t = win.ta; t < win.tb; t += kPredT) {
        const int k = (win.tb - t < kPredT) ? static_cast<int>(win.tb - t) : kPredT;   // draws of this tile (wave-uniform)
        double eta[kPredT], l[kPredT], mu[kPredT], y[kPredT];
        glm_eta_tile(xc + t * dim, k, dim, row.xt, col0, row.row_bytes, eta);
        glm_link_of_eta(row.lik, 0.0, 0.0, eta, l, mu);   // mu alone: l is dropped, and yrep_value asks eta for a NaN itself
        yrep_tile<kPredT>(row.lik, eta, mu, k, row.sigma, seed, chain, static_cast<uint32_t>(t0 + t), obs, real, y);
#pragma unroll
        for (int i = 0; i < kPredT; ++i)
            if (i < k) o[(t + i) * W] = y[i];   // 64 lanes, 64 consecutive doubles: one 512-byte row
    }
}

// min / max that keep a NaN (fmin / fmax drop one), and their wave reductions: wave_sum's tree -- row_shr 1, 2, 4, 8, then
// row_bcast 15 and 31 -- with a lane that has no source keeping its own value; the result is lane 63's.
__device__ __forceinline__ double nan_min(double a, double b) { return (a != a) ? a : ((b != b || b < a) ? b : a); }
__device__ __forceinline__ double nan_max(double a, double b) { return (a != a) ? a : ((b != b || b > a) ? b : a); }
template <int CTRL>
__device__ __forceinline__ double dpp_keep_f64(double x) {
    const int xl = __double2loint(x), xh = __double2hiint(x);
    const int lo = __builtin_amdgcn_update_dpp(xl, xl, CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(xh, xh, CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
template <bool kMax>
__device__ __forceinline__ double wave_extreme(double x) {
#define LMC_YREP_STEP(CTRL)                                   \
    {                                                         \
        const double o = dpp_keep_f64<CTRL>(x);               \
        x = kMax ? nan_max(x, o) : nan_min(x, o);             \
    }
    LMC_YREP_STEP(0x111)
    LMC_YREP_STEP(0x112)
    LMC_YREP_STEP(0x114)
    LMC_YREP_STEP(0x118)
    LMC_YREP_STEP(0x142)
    LMC_YREP_STEP(0x143)
#undef LMC_YREP_STEP
    return readlane_f64(x, 63);
}

// T[chain][t][7]
__global__ __launch_bounds__(64) void yrep_stats_kernel(const double* __restrict__ x, long long draws_stride, int dim, long long t0,
                                                        long long n, const double* __restrict__ rows, long long row_len, int npad,
                                                        int nob, long long segs, long long first_chain, long long per,
                                                        uint32_t seed, const double* __restrict__ centre, double* __restrict__ T) {
    const unsigned lane = threadIdx.x;
    const long long c = blockIdx.x / segs, seg = blockIdx.x % segs;
    const long long g = (first_chain + c) / per;
    const GlmRowView row = glm_row_view(rows, row_len, npad, g);   // wave-uniform
    const double cen = centre[g];
    const uint32_t chain = static_cast<uint32_t>(first_chain + c);
    const double* xc = x + (c * draws_stride + t0) * dim;
    double* out = T + c * n * kYrepPlanes;

    const DrawWindow win = draw_window(seg, kYrepSeg, n);
    for (long long t = win.ta; t < win.tb; t += kYrepT) {
        const int k = (win.tb - t < kYrepT) ? static_cast<int>(win.tb - t) : kYrepT;   // draws of this tile (wave-uniform)
        double a_sum[kYrepT], a_sq[kYrepT], a_min[kYrepT], a_max[kYrepT], a_zero[kYrepT], a_rep[kYrepT], a_obs[kYrepT];
#pragma unroll
        for (int i = 0; i < kYrepT; ++i) {
            a_sum[i] = a_sq[i] = a_zero[i] = a_rep[i] = a_obs[i] = 0.0;
            a_min[i] = HUGE_VAL;
            a_max[i] = -HUGE_VAL;
        }
        for (int ob = 0; ob < nob; ++ob) {
            const unsigned obs = static_cast<unsigned>(ob) * 64u + lane;
            const unsigned col0 = obs * 8u;
            const bool real = obs < static_cast<unsigned>(row.nobs);
            const double yn = grow_at(row.y, col0);
            double eta[kYrepT], l[kYrepT], mu[kYrepT], y[kYrepT];
            glm_eta_tile(xc + t * dim, k, dim, row.xt, col0, row.row_bytes, eta);   // (a tile of kYrepT draws: the width is the array's)
            glm_mu_of_eta(row.lik, eta, l, mu);   // the Pearson sums below want a NaN draw's mu NaN
            yrep_tile<kYrepT>(row.lik, eta, mu, k, row.sigma, seed, chain, static_cast<uint32_t>(t0 + t), obs, real, y);
#pragma unroll
            for (int i = 0; i < kYrepT; ++i) {
                const double V = (row.lik == kGlmBernoulli) ? mu[i] * (1.0 - mu[i]) : (row.lik == kGlmPoisson) ? mu[i] : 1.0 / row.isig2;
                const double dc = y[i] - cen, dr = y[i] - mu[i], dy = yn - mu[i];
                a_sum[i] += real ? y[i] : 0.0;
                a_sq[i] += real ? dc * dc : 0.0;
                a_min[i] = real ? nan_min(a_min[i], y[i]) : a_min[i];
                a_max[i] = real ? nan_max(a_max[i], y[i]) : a_max[i];
                a_zero[i] += (real && y[i] == 0.0) ? 1.0 : 0.0;
                a_rep[i] += real ? (dr * dr) / V : 0.0;
                a_obs[i] += real ? (dy * dy) / V : 0.0;
            }
        }
#pragma unroll
        for (int i = 0; i < kYrepT; ++i) {
            const double s0 = wave_sum(a_sum[i]), s1 = wave_sum(a_sq[i]);
            const double s2 = wave_extreme<false>(a_min[i]), s3 = wave_extreme<true>(a_max[i]);
            const double s4 = wave_sum(a_zero[i]), s5 = wave_sum(a_rep[i]), s6 = wave_sum(a_obs[i]);
            const double v = lane == 0 ? s0 : lane == 1 ? s1 : lane == 2 ? s2 : lane == 3 ? s3 : lane == 4 ? s4 : lane == 5 ? s5 : s6;
            if (i < k && lane < static_cast<unsigned>(kYrepPlanes)) out[(t + i) * kYrepPlanes + lane] = v;
        }
    }
}

}  // namespace lmc

// See include/lmc_hip.h. x, rows and y are DEVICE pointers on the current device; the work is enqueued on `stream`.
extern "C" int lmc_glm_yrep(const double* x, int64_t chains, int64_t draws_stride, int32_t dim, int64_t t0, int64_t n,
                            const double* rows, int64_t row_len, int64_t n_rows, int64_t first_chain, int64_t chains_per_group,
                            int64_t ob0, int64_t ob1, uint32_t seed, double* y, void* stream) {
    using namespace lmc;
    const int64_t lim = int64_t(1) << 31;
    TraceSpan span;
    GlmSpan glm;
    if (!y || trace_span(x, chains, draws_stride, dim, t0, n, first_chain, chains_per_group, &span) != LMC_OK ||
        glm_span(rows, row_len, n_rows, dim, span, ob0, ob1, &glm) != LMC_OK)
        return LMC_ERR_INVALID;
    const int64_t nobr = ob1 - ob0, W = nobr * 64;
    // y[chains][n][W] of 2^40 elements or more is refused: chains < 2^31 and W < 2^29, so chains * W cannot overflow
    if (n > ((int64_t(1) << 40) - 1) / (chains * W)) return LMC_ERR_INVALID;
    const int64_t segs = (n + kYrepOutSeg - 1) / kYrepOutSeg;
    const int64_t blocks = chains * segs * nobr;
    if (blocks >= lim) return LMC_ERR_INVALID;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int hdr_rc = glm_check_headers(rows, row_len, span, glm.npad, dim, s);
    if (hdr_rc != LMC_OK) return hdr_rc;
    (void)hipGetLastError();
    hipLaunchKernelGGL(yrep_kernel, dim3(static_cast<unsigned>(blocks)), dim3(64), 0, s, x, static_cast<long long>(draws_stride), dim,
                       static_cast<long long>(t0), static_cast<long long>(n), rows, static_cast<long long>(row_len),
                       static_cast<int>(glm.npad), static_cast<int>(ob0), static_cast<int>(nobr), static_cast<long long>(segs),
                       static_cast<long long>(first_chain), static_cast<long long>(span.per), seed, y);
    return hipGetLastError() == hipSuccess ? LMC_OK : LMC_ERR_HIP;
}

// See include/lmc_hip.h. x, rows, centre and T are DEVICE pointers on the current device; the work is enqueued on `stream`.
extern "C" int lmc_glm_yrep_stats(const double* x, int64_t chains, int64_t draws_stride, int32_t dim, int64_t t0, int64_t n,
                                  const double* rows, int64_t row_len, int64_t n_rows, int64_t first_chain,
                                  int64_t chains_per_group, uint32_t seed, const double* centre, double* T, void* stream) {
    using namespace lmc;
    const int64_t lim = int64_t(1) << 31;
    TraceSpan span;
    GlmSpan glm;   // every block of 64 observations: [0, nob)
    if (!centre || !T || trace_span(x, chains, draws_stride, dim, t0, n, first_chain, chains_per_group, &span) != LMC_OK ||
        glm_span(rows, row_len, n_rows, dim, span, 0, glm_npad_of_row(row_len, dim) / 64, &glm) != LMC_OK)
        return LMC_ERR_INVALID;
    // T[chains][n][7] of 2^40 elements or more is refused (chains < 2^31: chains * 7 cannot overflow): chains * segs < 2^40
    if (n > ((int64_t(1) << 40) - 1) / (chains * kYrepPlanes)) return LMC_ERR_INVALID;
    const int64_t segs = (n + kYrepSeg - 1) / kYrepSeg;
    const int64_t blocks = chains * segs;
    if (blocks >= lim) return LMC_ERR_INVALID;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int hdr_rc = glm_check_headers(rows, row_len, span, glm.npad, dim, s);
    if (hdr_rc != LMC_OK) return hdr_rc;
    (void)hipGetLastError();
    hipLaunchKernelGGL(yrep_stats_kernel, dim3(static_cast<unsigned>(blocks)), dim3(64), 0, s, x,
                       static_cast<long long>(draws_stride), dim, static_cast<long long>(t0), static_cast<long long>(n), rows,
                       static_cast<long long>(row_len), static_cast<int>(glm.npad), static_cast<int>(glm.nob),
                       static_cast<long long>(segs), static_cast<long long>(first_chain), static_cast<long long>(span.per), seed,
                       centre, T);
    return hipGetLastError() == hipSuccess ? LMC_OK : LMC_ERR_HIP;
}
