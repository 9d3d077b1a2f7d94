// Device log-densities: the plug-in `logp_dlogp_func(q) -> (logp, dlogp)` of the reference
// (/root/reference/littlemcmc/integration.py:40,62,115) as a __device__ functor that is inlined
// into the leapfrog of the transition kernel.
//
// Contract (the "thread-distributed" form of the plug-in). A chain is owned by a team of 64*W threads
// (lmc_team.hpp; W = 1 for d <= 128); thread t = tm.tid() owns elements e = t*NS + s, s < NS. Elements with
// e >= d are padding: they arrive as 0 and MUST be returned as 0 in g.
//   template <int NS> struct Target {
//       static constexpr bool kLanePartial = ...;
//       template <class Team> __device__ void init(Team& tm, const double* params, int d);   // once per kernel
//       // logp must be team-uniform: reduce with tm.sum(); neighbours with tm.neighbours(); thread 0's value
//       // with tm.bcast0()
//       template <class Team> __device__ double logp_grad(Team& tm, const double (&q)[NS], double (&g)[NS]) const;
//       // only if kLanePartial: the per-thread partial p_t with logp = sum_t p_t; lets the integrator fuse this
//       // reduction with the kinetic-energy one
//       template <class Team> __device__ double logp_grad_partial(Team& tm, const double (&q)[NS], double (&g)[NS]) const;
//   };
// The CPU statements of the same densities are in oracle/targets.py (same operation order).
//
// GLMTarget (below) is the one family that carries data -- y and both layouts of the design matrix X in its parameter row --
// and the one whose functor reads OTHER lanes' coordinates at will: eta = X q needs every q_e in every lane. It does so with
// v_readlane (wave-uniform SGPR operands of the FMAs), which is why it exists for one-wavefront chains only (d <= 512): the
// selectors (lmc_dispatch.hpp: has_shape) have no kernel of it for a team of several wavefronts. Its CPU statements are in
// tests/_glm_model.py.
#pragma once
#include "lmc_team.hpp"

namespace lmc {

// Per-group parameters: `params` of a job is a table with one row per group of chains (ChainArrays::tparam_*,
// lmc_engine_set_target_params_grouped). The row of the engine-wide chain index c -- blockIdx.x plus the launch's first
// chain, never the bare block index -- is chosen ONCE, where the kernel calls init(); the functor sees its row as `params`
// and nothing of the choice lives on into the iteration loop. stride == 0 is the job with one closure for every chain:
// the pointer goes through as it came, without the division. Rows start 16-byte aligned (the stride is even).
__device__ __forceinline__ const double* target_param_row(const double* tparams, int stride, int first, int group, int c) {
    if (stride == 0) return tparams;
    return tparams + static_cast<long long>(static_cast<unsigned>(first + c) / static_cast<unsigned>(group)) * stride;
}

// InlineTransition<T>::value is T::kInlineTransition if the functor declares it, else false: a functor whose body is beyond the inliner's budget asks the
// sampling kernel to inline its transition all the same (lmc_sampler.hpp: run_kernel)
template <class T, class = const bool>
struct InlineTransition { static constexpr bool value = false; };
template <class T>
struct InlineTransition<T, decltype(T::kInlineTransition)> { static constexpr bool value = T::kInlineTransition; };

enum TargetFamily : int {
    kStdNormal = 0,
    kDiagGaussian = 1,
    kAR1 = 2,
    kFunnel = 3,
    kNormal1D = 4,
    kUser = 5,
    kGLM = 8,
};

// logp = -1/2 sum q^2 ; g = -q
template <int NS>
struct StdNormalTarget {
    static constexpr bool kLanePartial = true;
    template <class Team>
    __device__ void init(Team&, const double*, int) {}
    template <class Team>
    __device__ double logp_grad_partial(Team&, const double (&q)[NS], double (&g)[NS]) const {
        double part = 0.0;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            part = __builtin_fma(q[s], q[s], part);
            g[s] = -q[s];
        }
        return -0.5 * part;   // exact scaling: sum(-q^2/2) == -(sum q^2)/2 bit for bit
    }
    template <class Team>
    __device__ double logp_grad(Team& tm, const double (&q)[NS], double (&g)[NS]) const {
        return tm.sum(logp_grad_partial(tm, q, g));
    }
};

// g = -(prec*q) ; logp = 1/2 q.g  (params = prec[d])
template <int NS>
struct DiagGaussianTarget {
    static constexpr bool kLanePartial = true;
    double prec[NS];
    template <class Team>
    __device__ void init(Team& tm, const double* params, int d) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int e = tm.tid() * NS + s;
            prec[s] = (e < d) ? params[e] : 0.0;
        }
    }
    template <class Team>
    __device__ double logp_grad_partial(Team&, const double (&q)[NS], double (&g)[NS]) const {
        double part = 0.0;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            g[s] = -(prec[s] * q[s]);
            part = __builtin_fma(q[s], g[s], part);
        }
        return 0.5 * part;
    }
    template <class Team>
    __device__ double logp_grad(Team& tm, const double (&q)[NS], double (&g)[NS]) const {
        return tm.sum(logp_grad_partial(tm, q, g));
    }
};

// AR(1): (Pq)_i = (diag_i q_i + off q_{i-1}) + off q_{i+1}; g = -Pq; logp = 1/2 q.g
// params = {c_end, c_mid, off}
template <int NS>
struct AR1Target {
    static constexpr bool kLanePartial = true;
    // per-thread coefficient slices, fixed for the whole kernel: diagonal and coupling. Padding elements carry 0
    // coefficients, so the hot loop has no selects; ONE coupling slice serves both neighbours: the element below
    // e = 0 and the one above e = d-1 are exact zeros (team edge / padding), so their products vanish by themselves.
    double diag[NS], cpl[NS];
    template <class Team>
    __device__ void init(Team& tm, const double* params, int d) {
        const double c_end = params[0], c_mid = params[1], off = params[2];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int e = tm.tid() * NS + s;
            diag[s] = (e >= d) ? 0.0 : ((e == 0 || e == d - 1) ? c_end : c_mid);
            cpl[s] = (e < d) ? off : 0.0;
        }
    }
    template <class Team>
    __device__ double logp_grad(Team& tm, const double (&q)[NS], double (&g)[NS]) const {
        return tm.sum(logp_grad_partial(tm, q, g));
    }
    template <class Team>
    __device__ double logp_grad_partial(Team& tm, const double (&q)[NS], double (&g)[NS]) const {
        double below, above;   // element e-1 of this thread's first slot, e+1 of its last slot
        tm.neighbours(q[NS - 1], q[0], below, above);
        double part = 0.0;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const double prev = (s == 0) ? below : q[s - 1];
            const double next = (s == NS - 1) ? above : q[s + 1];
            // (diag q + off q_{e-1}) + off q_{e+1}; a zero coefficient adds +0.0, which leaves the sum unchanged
            const double pq = (diag[s] * q[s] + cpl[s] * prev) + cpl[s] * next;
            g[s] = -pq;
            part = __builtin_fma(q[s], g[s], part);
        }
        return 0.5 * part;
    }
};

// Neal's funnel: v = q_0, x = q_{1..d-1}
// Everything that depends on v alone -- e^{-v}, -v^2/18, -v/9 -- is wave-uniform scalar work on the critical path of every
// leapfrog (a chain in the funnel's neck builds 4095-leapfrog trees alone on its SIMD, where each dependent instruction
// costs a full pipeline latency: DESIGN.md section 6, C5). It is therefore kept short: the exponential is the table-driven
// uniform form (lmc_wave.hpp: ~15 VALU, < 1 ulp, instead of ~40 for the generic exp) and is issued BEFORE the reduction of
// sum x^2 so that the two overlap; the divisions by the constants 18 and 9 are multiplications by their reciprocals
// (~2 VALU instead of ~12 each; the result differs from numpy's quotient by at most one ulp, like the exponential's).
template <int NS>
struct FunnelTarget {
    static constexpr bool kLanePartial = false;
    int d;
    template <class Team>
    __device__ void init(Team&, const double*, int d_) { d = d_; }
    template <class Team>
    __device__ double logp_grad(Team& tm, const double (&q)[NS], double (&g)[NS]) const {
        const int t = tm.tid();
        const double v = tm.bcast0(q[0]);
        const double ev = exp_uniform_fast(fmax(-v, -700.0));   // (q_0 beyond 700 has diverged long before)
        double part = 0.0;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int e = t * NS + s;
            if (e > 0) part = __builtin_fma(q[s], q[s], part);
        }
        const double dm1 = static_cast<double>(d - 1);
        const double lin = -(v * v) * (1.0 / 18.0) - 0.5 * dm1 * v;      // the part of logp that needs no reduction
        const double g0_lin = -v * (1.0 / 9.0) - 0.5 * dm1;
        const double ssum = tm.sum(part);
        const double hes = 0.5 * ev * ssum;
        const double logp = lin - hes;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int e = t * NS + s;
            g[s] = (e == 0) ? (g0_lin + hes) : ((e < d) ? -(ev * q[s]) : 0.0);
        }
        return logp;
    }
};

// The reference's own test target (/root/reference/tests/test_utils.py:19-28), d == 1:
// logp = -z^2/2 - log(scale sqrt(2 pi)), z = (x-loc)/scale ; dlogp = -(x-loc)/scale (sic).
// params = {loc, scale}
template <int NS>
struct Normal1DTarget {
    static constexpr bool kLanePartial = false;
    double loc, scale, lognorm;
    template <class Team>
    __device__ void init(Team&, const double* params, int) {
        loc = params[0];
        scale = params[1];
        lognorm = log(scale * sqrt(2.0 * 3.141592653589793));
    }
    template <class Team>
    __device__ double logp_grad(Team& tm, const double (&q)[NS], double (&g)[NS]) const {
        const double x = tm.bcast0(q[0]);
        const double z = (x - loc) / scale;
#pragma unroll
        for (int s = 0; s < NS; ++s) g[s] = (tm.tid() == 0 && s == 0) ? -(x - loc) / scale : 0.0;
        return -0.5 * z * z - lognorm;
    }
};

// exp and log1p for PER-LANE arguments with the polynomial constants in SGPRs (lmc_wave.hpp: exp_uniform is the wave-uniform
// form of the same). The OCML bodies keep ~25 VGPR pairs alive between them; inlined into a sampling kernel that already sits
// at its register cap, that is what spills. These keep the argument, the reduced argument and one accumulator.
// exp_lane: Cody-Waite reduction by ln2 (hi/lo), degree-13 Taylor polynomial on |r| <= ln2/2 (truncation 4e-18 relative),
// ldexp; |error| < 1.5 ulp. Arguments are clamped to [-800, 800]: beyond 709.78 the result is +inf as it must be.
__device__ __forceinline__ double exp_lane(double x) {
    const double xv = fmin(fmax(x, -800.0), 800.0);
    const double kf = rint(xv * LMC_SC(1.4426950408889634074));
    double r = __builtin_fma(-kf, LMC_SC(6.93147180369123816490e-01), xv);
    r = __builtin_fma(-kf, LMC_SC(1.90821492927058770002e-10), r);
    double p = fma_sgpr_addend(r, LMC_SC(1.0 / 6227020800.0), LMC_SC(1.0 / 479001600.0));
    p = fma_sgpr_addend(p, r, LMC_SC(1.0 / 39916800.0));
    p = fma_sgpr_addend(p, r, LMC_SC(1.0 / 3628800.0));
    p = fma_sgpr_addend(p, r, LMC_SC(1.0 / 362880.0));
    p = fma_sgpr_addend(p, r, LMC_SC(1.0 / 40320.0));
    p = fma_sgpr_addend(p, r, LMC_SC(1.0 / 5040.0));
    p = fma_sgpr_addend(p, r, LMC_SC(1.0 / 720.0));
    p = fma_sgpr_addend(p, r, LMC_SC(1.0 / 120.0));
    p = fma_sgpr_addend(p, r, LMC_SC(1.0 / 24.0));
    p = fma_sgpr_addend(p, r, LMC_SC(1.0 / 6.0));
    p = __builtin_fma(p, r, 0.5);
    p = __builtin_fma(p, r, 1.0);
    p = __builtin_fma(p, r, 1.0);
    return ldexp(p, static_cast<int>(kf));
}
// log1p_unit: log(1 + x) for x in [0, 1] (the softplus argument e^-|eta|) as 2 atanh(s), s = x / (2 + x) <= 1/3: no
// cancellation anywhere, so small x keep their relative accuracy (log1p(x) -> x). z = s^2 <= 1/9; the series
// 2 s (1 + z/3 + z^2/5 + ... + z^16/33) is cut where the next term is below 2e-18 relative. |error| < 2.5 ulp
// (0.5 for 2 + x, 0.5 for the quotient, the rest for the polynomial and the last product).
__device__ __forceinline__ double log1p_unit(double x) {
    const double s = x / (2.0 + x);
    const double z = s * s;
    double p = fma_sgpr_addend(z, LMC_SC(1.0 / 33.0), LMC_SC(1.0 / 31.0));
    p = fma_sgpr_addend(p, z, LMC_SC(1.0 / 29.0));
    p = fma_sgpr_addend(p, z, LMC_SC(1.0 / 27.0));
    p = fma_sgpr_addend(p, z, LMC_SC(1.0 / 25.0));
    p = fma_sgpr_addend(p, z, LMC_SC(1.0 / 23.0));
    p = fma_sgpr_addend(p, z, LMC_SC(1.0 / 21.0));
    p = fma_sgpr_addend(p, z, LMC_SC(1.0 / 19.0));
    p = fma_sgpr_addend(p, z, LMC_SC(1.0 / 17.0));
    p = fma_sgpr_addend(p, z, LMC_SC(1.0 / 15.0));
    p = fma_sgpr_addend(p, z, LMC_SC(1.0 / 13.0));
    p = fma_sgpr_addend(p, z, LMC_SC(1.0 / 11.0));
    p = fma_sgpr_addend(p, z, LMC_SC(1.0 / 9.0));
    p = fma_sgpr_addend(p, z, LMC_SC(1.0 / 7.0));
    p = fma_sgpr_addend(p, z, LMC_SC(1.0 / 5.0));
    p = fma_sgpr_addend(p, z, LMC_SC(1.0 / 3.0));
    const double s2 = s + s;
    return __builtin_fma(s2 * z, p, s2);
}

// (the values of include/lmc_hip.h: LMC_GLM_*, asserted equal in lmc_dispatch.hpp; this header is also compiled at run time)
constexpr int kGlmHeader = 8, kGlmBernoulli = 0, kGlmPoisson = 1, kGlmGaussian = 2, kGlmMaxDim = 512;

// Generalised linear model with its data in the parameter row (include/lmc_hip.h, LMC_TARGET_GLM: the layout):
//   eta = X q;  logp = sum_n l(y_n, eta_n) - 1/2 tau sum_e q_e^2;  g_e = sum_n X[n][e] r_n - tau q_e
// ONE wavefront per chain (the selectors have no GLM kernel for a team of several), no LDS: every value that crosses lanes
// goes through v_readlane into an SGPR pair and feeds the FMA as its scalar operand. Per block j of 64 observations:
//   eta pass   lane l owns observation n = 64 j + l: eta = fma(Xt[e][n], q_e, eta), e ascending. q_e lives in lane e / NS,
//              slot e % NS: the slot is a compile-time index, the lane a run-time one. One Xt row of a block is 512 coalesced
//              bytes. Eight rows are loaded before their eight FMAs (a chain has few wavefronts next to it to hide a load
//              behind); Xt has d rounded up to 8 rows, the added ones zero, and padding coefficients arrive as zero.
//   link       l_n, r_n per lane in the stable forms below; lanes with n >= N are SELECTED to exact zeros.
//   gradient   the lane that owns e = t NS + s: g[s] = fma(Xr[n][e], r_n, g[s]), n ascending; r_n from lane n - 64 j; a lane
//              reads its NS contiguous doubles of row n, 8 / NS rows before their FMAs (rows n >= N are zero, like r_n).
// then g_e = fma(-tau, q_e, g_e) (padding e >= d: 0), and the lane partial of logp is its observations' l_n (blocks ascending)
// plus -1/2 tau sum_s q_s^2. These orders are the definition; tests/_glm_model.py states them in numpy. A chain reads
// 2 N d doubles of design matrix per gradient, shared by every chain of its group (L1 / L2).
// State: three pointers and six scalars, all wave-uniform (SGPRs). An overflowing exp(eta) (poisson) gives a non-finite logp:
// the sampler's divergence, not clamped.
template <int NS>
struct GLMTarget {
    static constexpr bool kLanePartial = true;
    static constexpr bool kInlineTransition = true;   // the two passes and the link, at every leapfrog of the tree build
    // doubles a lane has in flight in either pass: eight, but two at one element per lane, where the sampling kernels' register
    // cap is lowest (128 VGPRs, four wavefronts per SIMD to hide a load behind) -- with four, three of the six run_kernel<1, 1>
    // variants spill more than their AR1Target counterparts ("Register budget"). Divides the 8 that Xt's rows are
    // padded to. -DLMC_GLM_BATCH_NS1=4 builds the other choice for an A/B run.
#ifndef LMC_GLM_BATCH_NS1
#define LMC_GLM_BATCH_NS1 2
#endif
    static constexpr int kBatch = NS == 1 ? LMC_GLM_BATCH_NS1 : 8;
    static_assert(8 % kBatch == 0, "the batch divides the 8 rows Xt is padded to");
    static constexpr int kRows = NS >= kBatch ? 1 : kBatch / NS;   // ... as rows of Xr
    static_assert(NS <= kBatch && kBatch % NS == 0, "GLMTarget: 1, 2, 4 or 8 elements per lane");
    // the row lives in global memory and its address is wave-uniform; said in the type and in uniform_row(), a load is
    // "scalar base + 32-bit lane offset" and no lane holds a 64-bit address
    typedef const __attribute__((address_space(1))) double* Row;
    Row y;    // y[npad]
    Row xt;   // Xt[d8][npad]
    Row xr;   // Xr[npad][64 NS]
    int lik, nobs, npad, d;
    double tau, isig2;
    // base[bytes / 8] with a 32-bit BYTE offset -- the form the load instruction takes next to a scalar base (a row is below
    // 4 GiB: the setters refuse longer ones)
    static __device__ __forceinline__ double at(Row base, unsigned bytes) {
        return *reinterpret_cast<Row>(reinterpret_cast<const __attribute__((address_space(1))) char*>(base) + bytes);
    }
    // two adjacent doubles at a 16-byte aligned offset (every section starts 16-byte aligned): one dwordx4 load
    typedef double Pair __attribute__((ext_vector_type(2)));
    static __device__ __forceinline__ Pair at2(Row base, unsigned bytes) {
        return *reinterpret_cast<const __attribute__((address_space(1))) Pair*>(
            reinterpret_cast<const __attribute__((address_space(1))) char*>(base) + bytes);
    }
    static __device__ __forceinline__ Row uniform_row(const double* p) {
        const unsigned long long v = reinterpret_cast<unsigned long long>(p);
        const unsigned lo = first_u32(static_cast<unsigned>(v)), hi = first_u32(static_cast<unsigned>(v >> 32));
        return reinterpret_cast<Row>((static_cast<unsigned long long>(hi) << 32) | lo);
    }
    // a header count (an integer in [0, 2^31) stored as a double) decoded with integer operations: they stay on the scalar
    // unit, where a float-to-int conversion would move the value, and every address made from it, into vector registers
    static __device__ __forceinline__ int header_int(double v) {
        const unsigned lo = first_u32(static_cast<unsigned>(__double2loint(v))), hi = first_u32(static_cast<unsigned>(__double2hiint(v)));
        const int e = static_cast<int>((hi >> 20) & 0x7ffu);
        const unsigned long long m = (static_cast<unsigned long long>((hi & 0xfffffu) | 0x100000u) << 32) | lo;
        return (e < 1023 || e > 1053) ? 0 : static_cast<int>(m >> (1075 - e));
    }
    template <class Team>
    __device__ void init(Team&, const double* params, int d_) {
        static_assert(Team::kWaves == 1, "GLMTarget: a chain is one wavefront");
        const Row row = uniform_row(params);
        lik = header_int(row[0]);
        nobs = header_int(row[1]);
        npad = header_int(row[2]);
        tau = first_f64(row[3]);
        isig2 = first_f64(row[4]);
        d = d_;
        y = row + kGlmHeader;
        xt = y + npad;
        xr = xt + static_cast<long long>((d + 7) / 8 * 8) * npad;   // Xt has d rounded up to 8 rows, whatever the batch
    }
    template <class Team>
    __device__ __forceinline__ double logp_grad(Team& tm, const double (&q)[NS], double (&g)[NS]) const {
        return tm.sum(logp_grad_partial(tm, q, g));
    }
    template <class Team>
    __device__ __forceinline__ double logp_grad_partial(Team& tm, const double (&q)[NS], double (&g)[NS]) const {
        const unsigned lane = static_cast<unsigned>(tm.tid());
        const unsigned row_bytes = static_cast<unsigned>(npad) * 8u;
        double lsum = 0.0;
#pragma unroll
        for (int s = 0; s < NS; ++s) g[s] = 0.0;
        for (int n0 = 0; n0 < nobs; n0 += 64) {
            // ---- eta pass: byte offset `col` walks down the rows of Xt, kBatch at a time
            unsigned col = (static_cast<unsigned>(n0) + lane) * 8u;
            double eta = 0.0;
            for (int e0 = 0; e0 < d; e0 += kBatch) {
                double x[kBatch];
#pragma unroll
                for (int k = 0; k < kBatch; ++k) x[k] = at(xt, col + static_cast<unsigned>(k) * row_bytes);
                const int owner = first_i32(e0 / NS);   // (wave-uniform already: this only tells the compiler so)
#pragma unroll
                for (int k = 0; k < kBatch; ++k) eta = __builtin_fma(x[k], readlane_f64(q[k % NS], owner + k / NS), eta);
                col += kBatch * row_bytes;
            }
            // ---- link
            const double yn = at(y, (static_cast<unsigned>(n0) + lane) * 8u);
            double l, r;
            if (lik == kGlmBernoulli) {
                const double ex = exp_lane(-fabs(eta));
                r = yn - ((eta >= 0.0) ? 1.0 : ex) / (1.0 + ex);   // (before l: one value fewer is alive across log1p_unit)
                l = yn * eta - (fmax(eta, 0.0) + log1p_unit(ex));
            } else if (lik == kGlmPoisson) {
                const double mu = exp_lane(eta);
                l = yn * eta - mu;
                r = yn - mu;
            } else {
                const double res = yn - eta;
                l = -0.5 * ((res * res) * isig2);
                r = res * isig2;
            }
            const bool live = n0 + static_cast<int>(lane) < nobs;
            l = live ? l : 0.0;
            r = live ? r : 0.0;
            lsum += l;
            // ---- gradient pass: byte offset `row` walks down the rows of Xr, kRows at a time
            const int cnt = (nobs - n0 < 64) ? nobs - n0 : 64;
            unsigned row = (static_cast<unsigned>(n0) * (64 * NS) + lane * NS) * 8u;
            for (int i0 = 0; i0 < cnt; i0 += kRows) {
                double x[kRows][NS];
#pragma unroll
                for (int k = 0; k < kRows; ++k)
                    if constexpr (NS == 1) {
                        x[k][0] = at(xr, row + k * 64 * 8u);
                    } else {
#pragma unroll
                        for (int s = 0; s < NS; s += 2) {
                            const Pair v = at2(xr, row + (k * 64 * NS + s) * 8u);
                            x[k][s] = v.x;
                            x[k][s + 1] = v.y;
                        }
                    }
                const int src = first_i32(i0);
#pragma unroll
                for (int k = 0; k < kRows; ++k) {
                    const double rn = readlane_f64(r, src + k);
#pragma unroll
                    for (int s = 0; s < NS; ++s) g[s] = __builtin_fma(x[k][s], rn, g[s]);
                }
                row += kRows * 64 * NS * 8u;
            }
        }
        double pp = 0.0;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            pp = __builtin_fma(q[s], q[s], pp);
            g[s] = (static_cast<int>(lane) * NS + s < d) ? __builtin_fma(-tau, q[s], g[s]) : 0.0;
        }
        return __builtin_fma(-0.5 * tau, pp, lsum);
    }
};

}  // namespace lmc
