// Fifth translation unit of liblmc_hip.so: the pointwise predictive passes over the draws where they live (HBM), for the
// GLM family (include/lmc_hip.h: lmc_glm_pointwise, lmc_glm_pointwise_loglik; littlemcmc_amd/predictive.py: lppd, WAIC,
// held-out scoring, and the array that loo() smooths).
//
// Wanted is, per observation n, a handful of statistics over the draws s of the pointwise log-likelihood l[s, n] -- the
// functor's l_n (lmc_targets.hpp: GLMTarget), additive constants dropped. The array l itself is N / d times the trace and is
// never written: every statistic MERGES over blocks of draws,
//     count n, m = max l, S = sum exp(l - m), mean l, M2 = sum (l - mean)^2, sum mu
//     merge(a, b):  m = max(ma, mb);  S = S_hi + S_lo exp(m_lo - m_hi);  Chan's update of (mean, M2);  sums;
//                   a side of count 0 is skipped by its count
// and the same pw_merge() serves a wavefront's tiles of draws, the reduce kernel's chain blocks and (restated in
// predictive.py) the host's devices.
//
// pointwise_kernel: the block index is (group, chain block, observation block), one wavefront a block, lane = observation.
// The wave walks the draws of its chains kPredT at a time through glm_link_tile (lmc_predict_tile.hpp states the tile: the
// functor's eta and link, bit for bit), then the tile's statistics (two-pass mean / M2, max, sum exp) and one merge into the
// running block. At d = 32 the link and the exponentials (a few tens of FP64 operations per draw and observation) outweigh
// the contraction; an FP64-MFMA eta would pay from d of a few hundred.
// No LDS, no scratch, no atomics: partial[group][chain block][obs block][6][64], merged per group in chain-block order by
// pointwise_reduce_kernel, so the same call on the same data gives the same bits.
//
// Non-finite l (include/lmc_hip.h says the same): a draw with l = -inf (an overflowing poisson exp(eta)) contributes
// exp(l - m) := 0 whatever m is, so m and S are those of the other draws and m + log S stays finite (all draws -inf:
// m = -inf, S = 0); mean and M2 are then non-finite (-inf or NaN) and sum mu = +inf. A NaN l makes planes 1..5 NaN.
//
// pointwise_loglik_kernel: one wavefront per (group, chain of the group, observation block), lane = observation; the same
// glm_link_tile (lmc_predict_tile.hpp), so the l written are the bits reduced above; every lane stores its tile's l as up to
// kPredT consecutive doubles of its row out[group][observation][chain * n + t], which lmc_psis_rows (lmc_psis.hip) smooths.
// The entry points' checks of the trace view, the grouping and the GLM table are trace_span, glm_span and glm_check_headers
// (lmc_trace_pass.hpp), shared by every pass over the trace.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lmc_hip.h"
#include "lmc_predict_tile.hpp"
#include "lmc_targets.hpp"
#include "lmc_trace_pass.hpp"

namespace lmc {

constexpr int kPredPlanes = 6;

struct PwStats {
    double m, S, mean, M2, smu;
};

// a <- merge(a, b); na, nb are the counts (as doubles; the caller adds them)
__device__ __forceinline__ void pw_merge(double na, PwStats& a, double nb, const PwStats& b) {
    if (nb == 0.0) return;
    if (na == 0.0) {
        a = b;
        return;
    }
    const double n = na + nb;
    const double hi = fmax(a.m, b.m), lo = fmin(a.m, b.m);
    const double e = (lo == -HUGE_VAL) ? 0.0 : exp_lane(lo - hi);   // (-inf) - (-inf) is never formed
    a.S = (a.m >= b.m) ? a.S + b.S * e : a.S * e + b.S;
    a.m = hi;
    chan_merge(nb / n, na * nb / n, a.mean, a.M2, b.mean, b.M2);
    a.smu = a.smu + b.smu;
}

__global__ __launch_bounds__(64) void pointwise_kernel(const double* __restrict__ x, long long chains, long long draws_stride,
                                                       int dim, long long t0, long long n, const double* __restrict__ rows,
                                                       long long row_len, int npad, int nob, int chain_blocks,
                                                       long long first_chain, long long per, long long g0,
                                                       double* __restrict__ partial) {
    const unsigned lane = threadIdx.x;
    const int ob = static_cast<int>(blockIdx.x) % nob;
    const int gcb = static_cast<int>(blockIdx.x) / nob;   // (group, chain block): the order of the partials
    const int cb = gcb % chain_blocks;
    const long long g = g0 + gcb / chain_blocks;
    long long c_lo = g * per - first_chain, c_hi = c_lo + per;   // this group's chains inside the trace block
    if (c_lo < 0) c_lo = 0;
    if (c_hi > chains) c_hi = chains;
    const GlmRowView row = glm_row_view(rows, row_len, npad, g);   // the group's row: wave-uniform
    const unsigned col0 = (static_cast<unsigned>(ob) * 64u + lane) * 8u;
    const double yn = grow_at(row.y, col0);   // padding observations: y = 0, X = 0 -> eta = 0, finite statistics

    PwStats acc = {-HUGE_VAL, 0.0, 0.0, 0.0, 0.0};
    double cnt = 0.0;
    bool bad = false;   // some l was NaN

    for (long long c = c_lo + cb; c < c_hi; c += chain_blocks) {
        const double* xc = x + (c * draws_stride + t0) * dim;
        for (long long t = 0; t < n; t += kPredT) {
            const int k = (n - t < kPredT) ? static_cast<int>(n - t) : kPredT;   // draws of this tile (wave-uniform)
            // a tile's missing draws repeat its last one and are deselected below
            double l[kPredT], mu[kPredT];
            glm_link_tile(xc + t * dim, k, dim, row.xt, col0, row.row_bytes, row.lik, yn, row.isig2, l, mu);
            // ---- the tile's statistics
            PwStats tile = {-HUGE_VAL, 0.0, 0.0, 0.0, 0.0};
            double sum = 0.0;
#pragma unroll
            for (int i = 0; i < kPredT; ++i) {
                const bool on = i < k;
                tile.m = fmax(tile.m, on ? l[i] : -HUGE_VAL);
                sum += on ? l[i] : 0.0;
                tile.smu += on ? mu[i] : 0.0;
                bad = bad || (on && l[i] != l[i]);
            }
            const double kd = static_cast<double>(k);
            tile.mean = sum / kd;
#pragma unroll
            for (int i = 0; i < kPredT; ++i) {
                const bool on = i < k;
                const double dv = on ? l[i] - tile.mean : 0.0;
                tile.M2 += dv * dv;
                const double w = exp_lane(l[i] - tile.m);
                tile.S += (on && l[i] != -HUGE_VAL) ? w : 0.0;
            }
            pw_merge(cnt, acc, kd, tile);
            cnt += kd;
        }
    }
    if (bad) acc.S = __builtin_nan("");   // carried through every merge; the reduce kernel spreads it to the other planes
    double* out = partial + (static_cast<long long>(gcb) * nob + ob) * kPredPlanes * 64 + lane;
    out[0] = cnt;
    out[64] = acc.m;
    out[128] = acc.S;
    out[192] = acc.mean;
    out[256] = acc.M2;
    out[320] = acc.smu;
}

// out[group][plane][npad] = the group's chain blocks merged in block order (deterministic)
__global__ void pointwise_reduce_kernel(const double* __restrict__ partial, int nob, int chain_blocks, int npad,
                                        long long groups, double* __restrict__ out) {
    const long long idx = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (idx >= groups * npad) return;
    const long long gi = idx / npad;
    const int j = static_cast<int>(idx % npad);
    const int ob = j / 64, lane = j % 64;
    PwStats acc = {-HUGE_VAL, 0.0, 0.0, 0.0, 0.0};
    double cnt = 0.0;
    for (int cb = 0; cb < chain_blocks; ++cb) {
        const double* p = partial + ((gi * chain_blocks + cb) * nob + ob) * kPredPlanes * 64 + lane;
        const double nb = p[0];
        const PwStats b = {p[64], p[128], p[192], p[256], p[320]};
        pw_merge(cnt, acc, nb, b);
        cnt += nb;
    }
    if (acc.S != acc.S) acc.m = acc.mean = acc.M2 = acc.smu = acc.S;   // a NaN l: every plane but the count
    double* o = out + gi * kPredPlanes * npad + j;
    o[0] = cnt;
    o[npad] = acc.m;
    o[2LL * npad] = acc.S;
    o[3LL * npad] = acc.mean;
    o[4LL * npad] = acc.M2;
    o[5LL * npad] = acc.smu;
}

__global__ __launch_bounds__(64) void pointwise_loglik_kernel(const double* __restrict__ x, long long draws_stride, int dim,
                                                              long long t0, long long n, const double* __restrict__ rows,
                                                              long long row_len, int npad, int ob0, int nobr, long long per,
                                                              long long g0, double* __restrict__ out) {
    const unsigned lane = threadIdx.x;
    const int ob = ob0 + static_cast<int>(blockIdx.x % static_cast<unsigned>(nobr));
    const long long gc = blockIdx.x / static_cast<unsigned>(nobr);   // chain of the block (whole groups: gi * per + cg)
    const long long gi = gc / per, cg = gc % per;
    const GlmRowView row = glm_row_view(rows, row_len, npad, g0 + gi);
    const unsigned col0 = (static_cast<unsigned>(ob) * 64u + lane) * 8u;
    const double yn = grow_at(row.y, col0);
    const double* xc = x + (gc * draws_stride + t0) * dim;
    const long long S = per * n;
    double* o = out + ((gi * nobr + (ob - ob0)) * 64 + lane) * S + cg * n;
    for (long long t = 0; t < n; t += kPredT) {
        const int k = (n - t < kPredT) ? static_cast<int>(n - t) : kPredT;   // draws of this tile (wave-uniform)
        double l[kPredT], mu[kPredT];
        glm_link_tile(xc + t * dim, k, dim, row.xt, col0, row.row_bytes, row.lik, yn, row.isig2, l, mu);
#pragma unroll
        for (int i = 0; i < kPredT; ++i)
            if (i < k) o[t + i] = l[i];
    }
}

}  // namespace lmc

// See include/lmc_hip.h. x, rows and out are DEVICE pointers on the current device; the work is enqueued on `stream`.
extern "C" int lmc_glm_pointwise(const double* x, int64_t chains, int64_t draws_stride, int32_t dim, int64_t t0, int64_t n,
                                 const double* rows, int64_t row_len, int64_t n_rows, int64_t first_chain,
                                 int64_t chains_per_group, double* out, void* stream) {
    using namespace lmc;
    const int64_t lim = int64_t(1) << 31;
    TraceSpan span;
    GlmSpan glm;   // every block of 64 observations: [0, nob)
    if (!out || trace_span(x, chains, draws_stride, dim, t0, n, first_chain, chains_per_group, &span) != LMC_OK ||
        glm_span(rows, row_len, n_rows, dim, span, 0, glm_npad_of_row(row_len, dim) / 64, &glm) != LMC_OK)
        return LMC_ERR_INVALID;
    const int64_t per = span.per, g0 = span.g0, groups = span.groups, npad = glm.npad, nob = glm.nob;
    long long cbl = (4096 / nob) / groups;   // one launch-wide budget of wavefronts, shared by the groups
    if (cbl > per) cbl = per;
    if (cbl > chains) cbl = chains;
    if (cbl < 1) cbl = 1;
    const int chain_blocks = static_cast<int>(cbl);
    const long long blocks = groups * chain_blocks * nob;
    const long long total = groups * npad;
    if (blocks >= lim || (total + 255) / 256 >= lim) return LMC_ERR_INVALID;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the headers of the touched rows: one strided copy, the call's only host look, before anything is launched
    const int hdr_rc = glm_check_headers(rows, row_len, span, npad, dim, s);
    if (hdr_rc != LMC_OK) return hdr_rc;
    double* partial = nullptr;
    const size_t bytes = static_cast<size_t>(blocks) * kPredPlanes * 64 * sizeof(double);
    if (hipMallocAsync(reinterpret_cast<void**>(&partial), bytes, s) != hipSuccess) return LMC_ERR_HIP;
    (void)hipGetLastError();
    hipLaunchKernelGGL(pointwise_kernel, dim3(static_cast<unsigned>(blocks)), dim3(64), 0, s, x, static_cast<long long>(chains),
                       static_cast<long long>(draws_stride), dim, static_cast<long long>(t0), static_cast<long long>(n), rows,
                       static_cast<long long>(row_len), static_cast<int>(npad), static_cast<int>(nob), chain_blocks,
                       static_cast<long long>(first_chain), static_cast<long long>(per), static_cast<long long>(g0), partial);
    hipLaunchKernelGGL(pointwise_reduce_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, s, partial,
                       static_cast<int>(nob), chain_blocks, static_cast<int>(npad), static_cast<long long>(groups), out);
    const hipError_t err = hipGetLastError();
    (void)hipFreeAsync(partial, s);
    return err == hipSuccess ? LMC_OK : LMC_ERR_HIP;
}

// See include/lmc_hip.h. x, rows and out are DEVICE pointers on the current device; the work is enqueued on `stream`.
extern "C" int lmc_glm_pointwise_loglik(const double* x, int64_t chains, int64_t draws_stride, int32_t dim, int64_t t0, int64_t n,
                                        const double* rows, int64_t row_len, int64_t n_rows, int64_t first_chain,
                                        int64_t chains_per_group, int64_t ob0, int64_t ob1, double* out, void* stream) {
    using namespace lmc;
    const int64_t lim = int64_t(1) << 31;
    TraceSpan span;
    GlmSpan glm;
    if (!out || trace_span(x, chains, draws_stride, dim, t0, n, first_chain, chains_per_group, &span) != LMC_OK) return LMC_ERR_INVALID;
    // whole groups: then chains_per_group <= chains < 2^31 (span.per is it), g0 = first_chain / per and groups = chains / per
    if (first_chain % chains_per_group != 0 || chains % chains_per_group != 0) return LMC_ERR_INVALID;
    if (glm_span(rows, row_len, n_rows, dim, span, ob0, ob1, &glm) != LMC_OK) return LMC_ERR_INVALID;
    const int64_t per = span.per, g0 = span.g0, npad = glm.npad;
    const int64_t nobr = ob1 - ob0;
    const int64_t blocks = chains * nobr;
    if (blocks >= lim) return LMC_ERR_INVALID;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int hdr_rc = glm_check_headers(rows, row_len, span, npad, dim, s);
    if (hdr_rc != LMC_OK) return hdr_rc;
    (void)hipGetLastError();
    hipLaunchKernelGGL(pointwise_loglik_kernel, dim3(static_cast<unsigned>(blocks)), dim3(64), 0, s, x,
                       static_cast<long long>(draws_stride), dim, static_cast<long long>(t0), static_cast<long long>(n), rows,
                       static_cast<long long>(row_len), static_cast<int>(npad), static_cast<int>(ob0), static_cast<int>(nobr),
                       static_cast<long long>(per), static_cast<long long>(g0), out);
    return hipGetLastError() == hipSuccess ? LMC_OK : LMC_ERR_HIP;
}
