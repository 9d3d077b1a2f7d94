// Eighth translation unit of liblmc_hip.so: posterior predictions at new X for the GLM family, from the draws where they
// live (HBM). include/lmc_hip.h: lmc_glm_linpred; littlemcmc_amd/predictive.py: linear_predictor(), predict().
//
// Wanted is, per point to predict at (an "observation" of a GLM parameter row whose y section is not read) and per group,
// the linear predictor eta[s] = x' q_s of every draw s -- written out, so that the radix select (lmc_select.hip) takes its
// exact order statistics from the array as it takes them from a trace -- and the moments of eta and of the mean response
// mu = sigmoid(eta) | exp(eta) | eta over the draws, which merge over blocks of draws and are never looked for in the array.
//
// linpred_kernel: one wavefront per (chain, segment of kLinSeg draws, observation block), lane = observation. The wave walks
// its draws kPredT at a time through glm_eta_tile (lmc_predict_tile.hpp) -- the contraction of pointwise_kernel and
// pointwise_loglik_kernel and of the sampler's functor, bit for bit -- and
//   * stores every draw's 64 values as ONE coalesced 512-byte row of eta[chain][t][W] (the [chains, draws, dim] layout of a
//     trace with dim = W: the draw index is the slow one, so nothing is transposed on the way to the select);
//   * forms the tile's two-pass (mean, M2) of eta and of mu and merges them into the wave's running block (Chan).
// A segment is a fixed number of draws whatever the launch, so the blocks a group is merged from -- and their order, (chain,
// segment) ascending in linpred_reduce_kernel -- depend on the data's shape alone: two calls give the same bits, a call on a
// sub-range of observation blocks gives the bits of the full call, and so does a call without one of the two outputs. No LDS,
// no scratch, no atomics. Per (draw, observation) the kernel moves 8 bytes out (the eta store) and d / 8 L2-resident loads of
// X in (one per coefficient and kPredT draws); the trace row comes through the scalar unit, once per wave and tile.
// At d = 32 the store is the floor: the kernel is a write stream of chains x draws x W doubles.
// The entry point's checks of the trace view, the grouping and the GLM table are trace_span, glm_span and glm_check_headers
// (lmc_trace_pass.hpp), shared by every pass over the trace.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lmc_hip.h"
#include "lmc_predict_tile.hpp"
#include "lmc_targets.hpp"
#include "lmc_trace_pass.hpp"

namespace lmc {

constexpr int kLinPlanes = 5;     // n_g, mean eta, M2 eta, mean mu, M2 mu
constexpr int kLinSeg = 256;      // draws of one wavefront: a multiple of kPredT, fixed (the merge order must not depend on a launch)
static_assert(kLinSeg % kPredT == 0, "a segment is whole tiles");

struct LinStats {
    double mean_e, M2_e, mean_m, M2_m;
};

// a <- merge(a, b) (Chan); na, nb are the counts (as doubles; the caller adds them). A side of count 0 is skipped by its count.
__device__ __forceinline__ void lin_merge(double na, LinStats& a, double nb, const LinStats& b) {
    if (nb == 0.0) return;
    if (na == 0.0) {
        a = b;
        return;
    }
    const double n = na + nb;
    const double w = nb / n, cross = na * nb / n;
    chan_merge(w, cross, a.mean_e, a.M2_e, b.mean_e, b.M2_e);
    chan_merge(w, cross, a.mean_m, a.M2_m, b.mean_m, b.M2_m);
}

// eta_out[chain][t][W] and / or partial[chain][segment][obs block][5][64] (either may be NULL, not both)
__global__ __launch_bounds__(64) void linpred_kernel(const double* __restrict__ x, long long draws_stride, int dim, long long t0,
                                                     long long n, const double* __restrict__ rows, long long row_len, int npad,
                                                     int ob0, int nobr, long long segs, long long first_chain, long long per,
                                                     double* __restrict__ eta_out, double* __restrict__ partial) {
    const unsigned lane = threadIdx.x;
    const int obr = static_cast<int>(blockIdx.x % static_cast<unsigned>(nobr));
    const long long cs = blockIdx.x / static_cast<unsigned>(nobr);   // (chain, segment): the order of the partials
    const long long c = cs / segs, seg = cs % segs;
    const GlmRowView row = glm_row_view(rows, row_len, npad, (first_chain + c) / per);   // its y section is never read
    const unsigned col0 = (static_cast<unsigned>(ob0 + obr) * 64u + lane) * 8u;   // padding observations: X = 0 -> eta = 0
    const double* xc = x + (c * draws_stride + t0) * dim;
    const long long W = static_cast<long long>(nobr) * 64;
    double* o = eta_out ? eta_out + c * n * W + obr * 64 + lane : nullptr;

    LinStats acc = {0.0, 0.0, 0.0, 0.0};
    double cnt = 0.0;
    const DrawWindow win = draw_window(seg, kLinSeg, n);
    for (long long t = win.ta; t < win.tb; t += kPredT) {
        const int k = (win.tb - t < kPredT) ? static_cast<int>(win.tb - t) : kPredT;   // draws of this tile (wave-uniform)
        double eta[kPredT];
        glm_eta_tile(xc + t * dim, k, dim, row.xt, col0, row.row_bytes, eta);
        if (o) {
#pragma unroll
            for (int i = 0; i < kPredT; ++i)
                if (i < k) o[(t + i) * W] = eta[i];   // 64 lanes, 64 consecutive doubles: one 512-byte row
        }
        if (partial) {   // (wave-uniform)
            double l[kPredT], mu[kPredT];
            glm_mu_of_eta(row.lik, eta, l, mu);
            // ---- the tile's statistics: two passes; a tile's missing draws repeat its last one and are deselected
            double se = 0.0, sm = 0.0;
#pragma unroll
            for (int i = 0; i < kPredT; ++i) {
                const bool on = i < k;
                se += on ? eta[i] : 0.0;
                sm += on ? mu[i] : 0.0;
            }
            const double kd = static_cast<double>(k);
            LinStats tile = {se / kd, 0.0, sm / kd, 0.0};
#pragma unroll
            for (int i = 0; i < kPredT; ++i) {
                const bool on = i < k;
                const double dv = on ? eta[i] - tile.mean_e : 0.0;
                const double dw = on ? mu[i] - tile.mean_m : 0.0;
                tile.M2_e += dv * dv;
                tile.M2_m += dw * dw;
            }
            lin_merge(cnt, acc, kd, tile);
            cnt += kd;
        }
    }
    if (partial) {
        double* p = partial + (cs * nobr + obr) * kLinPlanes * 64 + lane;
        p[0] = cnt;
        p[64] = acc.mean_e;
        p[128] = acc.M2_e;
        p[192] = acc.mean_m;
        p[256] = acc.M2_m;
    }
}

// stats[group][plane][W] = the (chain, segment) blocks of the group's chains present, merged in that order (deterministic)
__global__ void linpred_reduce_kernel(const double* __restrict__ partial, int nobr, long long segs, long long chains,
                                      long long first_chain, long long per, long long g0, long long groups,
                                      double* __restrict__ stats) {
    const long long W = static_cast<long long>(nobr) * 64;
    const long long idx = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (idx >= groups * W) return;
    const long long gi = idx / W;
    const int j = static_cast<int>(idx % W);
    const int obr = j / 64, lane = j % 64;
    long long c_lo = (g0 + gi) * per - first_chain, c_hi = c_lo + per;   // this group's chains inside the trace block
    if (c_lo < 0) c_lo = 0;
    if (c_hi > chains) c_hi = chains;
    LinStats acc = {0.0, 0.0, 0.0, 0.0};
    double cnt = 0.0;
    for (long long cs = c_lo * segs; cs < c_hi * segs; ++cs) {
        const double* p = partial + (cs * nobr + obr) * kLinPlanes * 64 + lane;
        const double nb = p[0];
        const LinStats b = {p[64], p[128], p[192], p[256]};
        lin_merge(cnt, acc, nb, b);
        cnt += nb;
    }
    double* o = stats + gi * kLinPlanes * W + j;
    o[0] = cnt;
    o[W] = acc.mean_e;
    o[2 * W] = acc.M2_e;
    o[3 * W] = acc.mean_m;
    o[4 * W] = acc.M2_m;
}

}  // namespace lmc

// See include/lmc_hip.h. x, rows, eta and stats are DEVICE pointers on the current device; the work is enqueued on `stream`.
extern "C" int lmc_glm_linpred(const double* x, int64_t chains, int64_t draws_stride, int32_t dim, int64_t t0, int64_t n,
                               const double* rows, int64_t row_len, int64_t n_rows, int64_t first_chain, int64_t chains_per_group,
                               int64_t ob0, int64_t ob1, double* eta, double* stats, void* stream) {
    using namespace lmc;
    const int64_t lim = int64_t(1) << 31;
    TraceSpan span;
    GlmSpan glm;
    if ((!eta && !stats) || trace_span(x, chains, draws_stride, dim, t0, n, first_chain, chains_per_group, &span) != LMC_OK ||
        glm_span(rows, row_len, n_rows, dim, span, ob0, ob1, &glm) != LMC_OK)
        return LMC_ERR_INVALID;
    const int64_t per = span.per, g0 = span.g0, groups = span.groups, npad = glm.npad;
    const int64_t nobr = ob1 - ob0, W = nobr * 64;
    // eta[chains][n][W] of 2^40 elements or more is refused: chains < 2^31 and W < 2^29, so chains * W cannot overflow, and
    // the kernels index with 64 bits throughout (the launch limits below are the tighter ones)
    if (n > ((int64_t(1) << 40) - 1) / (chains * W)) return LMC_ERR_INVALID;
    const int64_t segs = (n + kLinSeg - 1) / kLinSeg;
    const int64_t blocks = chains * segs * nobr;   // < 2^40 / 64
    const int64_t total = groups * W;
    if (blocks >= lim || (total + 255) / 256 >= lim) return LMC_ERR_INVALID;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the headers of the touched rows: one strided copy, the call's only host look, before anything is launched
    const int hdr_rc = glm_check_headers(rows, row_len, span, npad, dim, s);
    if (hdr_rc != LMC_OK) return hdr_rc;
    double* partial = nullptr;
    if (stats) {
        const size_t bytes = static_cast<size_t>(blocks) * kLinPlanes * 64 * sizeof(double);
        if (hipMallocAsync(reinterpret_cast<void**>(&partial), bytes, s) != hipSuccess) return LMC_ERR_HIP;
    }
    (void)hipGetLastError();
    hipLaunchKernelGGL(linpred_kernel, dim3(static_cast<unsigned>(blocks)), dim3(64), 0, s, x, static_cast<long long>(draws_stride),
                       dim, static_cast<long long>(t0), static_cast<long long>(n), rows, static_cast<long long>(row_len),
                       static_cast<int>(npad), static_cast<int>(ob0), static_cast<int>(nobr), static_cast<long long>(segs),
                       static_cast<long long>(first_chain), static_cast<long long>(per), eta, partial);
    if (stats)
        hipLaunchKernelGGL(linpred_reduce_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, s, partial,
                           static_cast<int>(nobr), static_cast<long long>(segs), static_cast<long long>(chains),
                           static_cast<long long>(first_chain), static_cast<long long>(per), static_cast<long long>(g0),
                           static_cast<long long>(groups), stats);
    const hipError_t err = hipGetLastError();
    if (partial) (void)hipFreeAsync(partial, s);
    return err == hipSuccess ? LMC_OK : LMC_ERR_HIP;
}
