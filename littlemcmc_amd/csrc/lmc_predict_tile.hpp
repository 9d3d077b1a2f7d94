// What the GLM passes over the trace share on the device, stated ONCE: the view of a parameter row (glm_row_view), a
// wavefront's segment of draws (draw_window), Chan's update of a (mean, M2) pair (chan_merge) and the eta / link tile.
// pointwise_kernel reduces the l[], mu[] that glm_link_tile returns to the six planes, pointwise_loglik_kernel (both in
// lmc_predict.hip) writes the same l[] out -- the same instructions on the same operands, so the written array holds the bits
// the planes were reduced from. The contraction alone is glm_eta_tile, which linpred_kernel (lmc_linpred.hip) writes out and
// the kernels of lmc_yrep.hip sample from: the eta of a prediction is the eta of the score.
//
// One wavefront, lane = observation (the Xt[e][n] section of the GLM row: one coalesced 512-byte row per coefficient and
// block of 64 observations). A tile is kPredT consecutive draws of one chain: the trace row q is read through a wave-uniform
// address (the scalar unit, one load for 64 lanes) and NEVER beyond its d coefficients -- the trace is [.., d], the next
// doubles are the next draw -- and every loaded X element feeds kPredT FMAs, eta[i] = fma(Xt[e][n], q_i[e], eta[i]) with e
// ascending: the functor's eta (lmc_targets.hpp: GLMTarget), bit for bit. Then the link, the functor's expressions.
// Device code only: the entry points' host-side checks of a GLM table are in lmc_trace_pass.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lmc_hip.h"
#include "lmc_targets.hpp"

namespace lmc {

constexpr int kPredT = 8;        // draws per loaded X element (accumulators eta[kPredT])
constexpr int kPredBatch = 8;    // rows of Xt in flight: the 8 its rows are padded to

typedef const __attribute__((address_space(1))) double* GRow;
__device__ __forceinline__ double grow_at(GRow base, unsigned bytes) {
    return *reinterpret_cast<GRow>(reinterpret_cast<const __attribute__((address_space(1))) char*>(base) + bytes);
}

static_assert(kGlmHeader == LMC_GLM_HEADER && kGlmMaxDim == LMC_GLM_MAX_DIM, "lmc_targets.hpp and lmc_hip.h agree");

// The parameter row of a wave-uniform `group` (targets.glm_row_layout): header fields through the scalar unit, the y section,
// the Xt section npad doubles behind it, the bytes of a row of Xt. A kernel pays for the fields it uses. sigma is formed here,
// between the header loads and the sections, because that is where the lmc_yrep.hip kernels formed it: their ISA stays.
struct GlmRowView {
    int lik, nobs;
    double isig2, sigma;
    GRow y, xt;
    unsigned row_bytes;
};
__device__ __forceinline__ GlmRowView glm_row_view(const double* rows, long long row_len, int npad, long long group) {
    const double* row = rows + group * row_len;
    GlmRowView v;
    v.lik = first_i32(static_cast<int>(row[0]));
    v.nobs = first_i32(static_cast<int>(row[1]));
    v.isig2 = row[4];
    v.sigma = 1.0 / sqrt(v.isig2);
    v.y = reinterpret_cast<GRow>(reinterpret_cast<unsigned long long>(row + kGlmHeader));
    v.xt = v.y + npad;
    v.row_bytes = static_cast<unsigned>(npad) * 8u;
    return v;
}

// The draws [ta, tb) of segment `seg` of a chain's n draws, `len` draws a segment; the last one may be short.
struct DrawWindow {
    long long ta, tb;
};
__device__ __forceinline__ DrawWindow draw_window(long long seg, int len, long long n) {
    const long long ta = seg * len;
    return {ta, (n - ta < len) ? n : ta + len};
}

// Chan's update of a (mean, M2) pair over na and nb > 0 draws, n = na + nb: w = nb / n, cross = na * nb / n, the caller's.
__device__ __forceinline__ void chan_merge(double w, double cross, double& mean_a, double& M2_a, double mean_b, double M2_b) {
    const double delta = mean_b - mean_a;
    mean_a = mean_a + delta * w;
    M2_a = (M2_a + M2_b) + (delta * delta) * cross;
}

// The contraction alone: eta[i] of the tile's draws. qt: the tile's first draw (dim doubles a draw), k <= T draws of it
// exist (wave-uniform; T, the tile's width, is kPredT everywhere but in yrep_stats_kernel, lmc_yrep.hip); xt: the row's Xt section, col0 the lane's byte offset in a row of it, row_bytes = npad * 8. eta[i] for
// i >= k repeats draw k - 1. The y section of the row is not touched (lmc_linpred.hip predicts where no y is known).
template <int T>
__device__ __forceinline__ void glm_eta_tile(const double* qt, int k, int dim, GRow xt, unsigned col0, unsigned row_bytes,
                                             double (&eta)[T]) {
    // a tile's missing draws repeat its last one (a valid row; the callers deselect their values)
    int qoff[T];
#pragma unroll
    for (int i = 0; i < T; ++i) qoff[i] = (i < k ? i : k - 1) * dim;
#pragma unroll
    for (int i = 0; i < T; ++i) eta[i] = 0.0;
    unsigned col = col0;
    int e0 = 0;
    for (; e0 + kPredBatch <= dim; e0 += kPredBatch) {
        double xv[kPredBatch];
#pragma unroll
        for (int j = 0; j < kPredBatch; ++j) xv[j] = grow_at(xt, col + static_cast<unsigned>(j) * row_bytes);
#pragma unroll
        for (int j = 0; j < kPredBatch; ++j)
#pragma unroll
            for (int i = 0; i < T; ++i) eta[i] = __builtin_fma(xv[j], qt[qoff[i] + e0 + j], eta[i]);
        col += kPredBatch * row_bytes;
    }
    if (e0 < dim) {   // the last rows: Xt is padded to 8 rows (zeros), the trace row is NOT: q[e] only for e < dim
        double xv[kPredBatch];
#pragma unroll
        for (int j = 0; j < kPredBatch; ++j) xv[j] = grow_at(xt, col + static_cast<unsigned>(j) * row_bytes);
#pragma unroll
        for (int j = 0; j < kPredBatch; ++j) {
            const bool have = e0 + j < dim;
            const int e = have ? e0 + j : dim - 1;
#pragma unroll
            for (int i = 0; i < T; ++i) {
                const double qv = qt[qoff[i] + e];
                eta[i] = __builtin_fma(xv[j], have ? qv : 0.0, eta[i]);
            }
        }
    }
}

// The link of a tile's eta, the functor's expressions: l[i] the pointwise log-likelihood at the lane's y = yn (constants
// dropped), mu[i] the mean response sigmoid(eta) | exp(eta) | eta. A caller that wants mu alone passes any yn and drops l.
template <int T>
__device__ __forceinline__ void glm_link_of_eta(int lik, double yn, double isig2, const double (&eta)[T], double (&l)[T],
                                                double (&mu)[T]) {
    if (lik == kGlmBernoulli) {
#pragma unroll
        for (int i = 0; i < T; ++i) {
            const double ex = exp_lane(-fabs(eta[i]));
            mu[i] = ((eta[i] >= 0.0) ? 1.0 : ex) / (1.0 + ex);
            l[i] = yn * eta[i] - (fmax(eta[i], 0.0) + log1p_unit(ex));
        }
    } else if (lik == kGlmPoisson) {
#pragma unroll
        for (int i = 0; i < T; ++i) {
            mu[i] = exp_lane(eta[i]);
            l[i] = yn * eta[i] - mu[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < T; ++i) {
            const double res = yn - eta[i];
            mu[i] = eta[i];
            l[i] = -0.5 * ((res * res) * isig2);
        }
    }
}

// mu alone (l is the caller's scratch), a NaN eta carried into it: exp_lane clamps through fmax / fmin, which would drop it.
template <int T>
__device__ __forceinline__ void glm_mu_of_eta(int lik, const double (&eta)[T], double (&l)[T], double (&mu)[T]) {
    glm_link_of_eta(lik, 0.0, 0.0, eta, l, mu);
#pragma unroll
    for (int i = 0; i < T; ++i) mu[i] = (eta[i] != eta[i]) ? eta[i] : mu[i];
}

// eta and the link of a tile: yn the lane's y. l[i], mu[i] for i >= k repeat draw k - 1.
__device__ __forceinline__ void glm_link_tile(const double* qt, int k, int dim, GRow xt, unsigned col0, unsigned row_bytes,
                                              int lik, double yn, double isig2, double (&l)[kPredT], double (&mu)[kPredT]) {
    double eta[kPredT];
    glm_eta_tile(qt, k, dim, xt, col0, row_bytes, eta);
    glm_link_of_eta(lik, yn, isig2, eta, l, mu);
}

}  // namespace lmc
