// Fifth translation unit of liblmc_hip.so: the pointwise predictive pass over the draws where they live (HBM), for the
// GLM family (include/lmc_hip.h: lmc_glm_pointwise; littlemcmc_amd/predictive.py: lppd, WAIC, held-out scoring).
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
// pointwise_kernel: lane = observation (the Xt[e][n] section of the row: one coalesced 512-byte row per coefficient and
// block of 64 observations); the block index is (group, chain block, observation block), one wavefront a block. The wave
// walks the draws of its chains kPredT at a time: the trace row q is read through a wave-uniform address (the scalar unit,
// one load for 64 lanes) and NEVER beyond its d coefficients -- the trace is [.., d], the next doubles are the next draw --
// and every loaded X element feeds kPredT FMAs, eta[i] = fma(Xt[e][n], q_i[e], eta[i]) with e ascending: the functor's eta,
// bit for bit. Then the link (the functor's expressions), the tile's statistics (two-pass mean / M2, max, sum exp) and one
// merge into the running block. At d = 32 the link and the exponentials (a few tens of FP64 operations per draw and
// observation) outweigh the contraction; an FP64-MFMA eta would pay from d of a few hundred.
// No LDS, no scratch, no atomics: partial[group][chain block][obs block][6][64], merged per group in chain-block order by
// pointwise_reduce_kernel, so the same call on the same data gives the same bits.
//
// Non-finite l (include/lmc_hip.h says the same): a draw with l = -inf (an overflowing poisson exp(eta)) contributes
// exp(l - m) := 0 whatever m is, so m and S are those of the other draws and m + log S stays finite (all draws -inf:
// m = -inf, S = 0); mean and M2 are then non-finite (-inf or NaN) and sum mu = +inf. A NaN l makes planes 1..5 NaN.
// The entry point's checks of the trace view, the grouping and the GLM table are trace_span, glm_span and glm_check_headers
// (lmc_trace_pass.hpp), shared by every pass over the trace.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lmc_hip.h"
#include "lmc_predict_tile.hpp"
#include "lmc_targets.hpp"
#include "lmc_trace_pass.hpp"

namespace lmc {

constexpr int kPredPlanes = 6;

static_assert(kGlmHeader == LMC_GLM_HEADER && kGlmMaxDim == LMC_GLM_MAX_DIM, "lmc_targets.hpp and lmc_hip.h agree");

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
    const double delta = b.mean - a.mean;
    a.mean = a.mean + delta * (nb / n);
    a.M2 = (a.M2 + b.M2) + (delta * delta) * (na * nb / n);
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
    // the group's row: wave-uniform (the header is read on the scalar unit)
    const double* row = rows + g * row_len;
    const int lik = first_i32(static_cast<int>(row[0]));
    const double isig2 = row[4];
    const GRow y = reinterpret_cast<GRow>(reinterpret_cast<unsigned long long>(row + kGlmHeader));
    const GRow xt = y + npad;
    const unsigned row_bytes = static_cast<unsigned>(npad) * 8u;
    const unsigned col0 = (static_cast<unsigned>(ob) * 64u + lane) * 8u;
    const double yn = grow_at(y, col0);   // padding observations: y = 0, X = 0 -> eta = 0, finite statistics

    PwStats acc = {-HUGE_VAL, 0.0, 0.0, 0.0, 0.0};
    double cnt = 0.0;
    bool bad = false;   // some l was NaN

    for (long long c = c_lo + cb; c < c_hi; c += chain_blocks) {
        const double* xc = x + (c * draws_stride + t0) * dim;
        for (long long t = 0; t < n; t += kPredT) {
            const int k = (n - t < kPredT) ? static_cast<int>(n - t) : kPredT;   // draws of this tile (wave-uniform)
            // eta and the link of the tile's draws (lmc_predict_tile.hpp: shared with pointwise_loglik_kernel); a tile's
            // missing draws repeat its last one and are deselected below
            double l[kPredT], mu[kPredT];
            glm_link_tile(xc + t * dim, k, dim, xt, col0, row_bytes, lik, yn, isig2, l, mu);
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
