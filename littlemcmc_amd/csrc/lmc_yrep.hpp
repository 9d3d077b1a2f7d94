// The replicated response y_rep ~ p(y | q_s) of one (draw, observation) of a GLM, stated ONCE: yrep_kernel writes it out,
// yrep_stats_kernel (both in lmc_yrep.hip) reduces it to test statistics -- one device function, yrep_value, so the bits of
// the written array are the bits the statistics were taken from. include/lmc_hip.h states the same definition;
// tests/_yrep_model.py restates it in Python.
//
// Every value is a pure function of (seed, job chain, draw row, observation): nothing lives in memory, and a value does not
// depend on the launch shape, the chunking, the observation-block range, the chain-block partition or the device.
//   w(b)  = philox4x32_10(c0 = r, c1 = i, c2 = b, c3 = 0x6c6d6379 "lmcy", k0 = seed, k1 = job chain)
//           r the draw's row index t0 + t in the view, i the observation index in the row (< 2^29), b = 0, 1, .. the block
//   u_j   = counter_uniform_of(w(j >> 1), j & 1): the 53-bit form of the decision stream (lmc_rng.hpp), in [0, 1); its
//           integer is m_j = (a >> 5) 2^26 + (b >> 6), u_j = m_j 2^-53
// c3 keeps the counter space disjoint from the momentum stream's ("lmcm") and the decision stream's ("lmcu").
//   bernoulli  y = (u_0 < mu) ? 1 : 0
//   gaussian   y = fma(sigma, z, eta), z = Phi^-1((m_0 + 1/2) 2^-53) by Wichura's AS 241 (PPND16): float64, no rejection;
//              p is never 0 or 1 and z is antisymmetric in m <-> 2^53 - 1 - m (yrep_normal)
//   poisson    lam = mu: 0 -> 0; lam < 10: multiplication method; lam >= 10: Hoermann's PTRS (1993) with numpy's constants
// eta NaN, mu NaN, mu = +inf, or (poisson) mu > 2^52 give y = NaN. Loops are bounded -- 64 PTRS attempts or 1024 uniforms of
// the multiplication method, then y = NaN (probability below 1e-30) -- so no input keeps a wavefront spinning.
// A count is returned as a double. Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lmc_rng.hpp"
#include "lmc_targets.hpp"

namespace lmc {

constexpr uint32_t kYrepC3 = 0x6c6d6379u;   // "lmcy"
constexpr int kYrepMaxAttempts = 64;        // PTRS attempts (two uniforms each)
constexpr int kYrepMaxUniforms = 1024;      // uniforms of the multiplication method
constexpr double kYrepPtrsLam = 10.0;       // lam >= this: PTRS
constexpr double kYrepMaxMu = 4503599627370496.0;   // 2^52: a larger poisson mean is refused (NaN)

// The uniforms of one (seed, job chain, draw row, observation) in order; one Philox block serves two.
struct YrepStream {
    uint32_t r, i, seed, chain;
    int j;
    Philox4 w;
};
__device__ __forceinline__ YrepStream yrep_stream(uint32_t seed, uint32_t chain, uint32_t r, uint32_t i) {
    YrepStream s;
    s.r = r; s.i = i; s.seed = seed; s.chain = chain; s.j = 0;
    s.w.c[0] = s.w.c[1] = s.w.c[2] = s.w.c[3] = 0u;
    return s;
}
__device__ __forceinline__ void yrep_advance(YrepStream& s) {
    if ((s.j & 1) == 0) s.w = philox4x32_10(s.r, s.i, static_cast<uint32_t>(s.j >> 1), kYrepC3, s.seed, s.chain);
}
__device__ __forceinline__ double yrep_uniform(YrepStream& s) {
    yrep_advance(s);
    const double u = counter_uniform_of(s.w, s.j & 1);
    s.j += 1;
    return u;
}
// m_j: the 53-bit integer behind u_j (as a double: exact)
__device__ __forceinline__ double yrep_integer(YrepStream& s) {
    yrep_advance(s);
    const int odd = s.j & 1;
    const uint32_t a = (odd ? s.w.c[2] : s.w.c[0]) >> 5;
    const uint32_t b = (odd ? s.w.c[3] : s.w.c[1]) >> 6;
    s.j += 1;
    return static_cast<double>(a) * 67108864.0 + static_cast<double>(b);
}

// z = Phi^-1((m + 1/2) 2^-53), m an integer in [0, 2^53): AS 241, PPND16 (Wichura 1988; relative accuracy about 1e-16).
// q = p - 1/2 = (m - 2^52 + 1/2) 2^-53 is exact (an odd integer below 2^53 over 2^54), and the tail argument
// min(p, 1 - p) = (m + 1/2) 2^-53 for q < 0, (2^53 - m - 1/2) 2^-53 for q > 0 is exact too, so m and 2^53 - 1 - m give the same
// r and opposite q: z is antisymmetric, and finite for every m (the smallest tail argument is 2^-54).
// Horner steps are fmas.
#define LMC_AS241_RATIO(r, n7, n6, n5, n4, n3, n2, n1, n0, d7, d6, d5, d4, d3, d2, d1)                                           \
    (__builtin_fma(__builtin_fma(__builtin_fma(__builtin_fma(__builtin_fma(__builtin_fma(__builtin_fma(n7, r, n6), r, n5), r, n4), r, n3), r, n2), r, n1), r, n0) /  \
     __builtin_fma(__builtin_fma(__builtin_fma(__builtin_fma(__builtin_fma(__builtin_fma(__builtin_fma(d7, r, d6), r, d5), r, d4), r, d3), r, d2), r, d1), r, 1.0))
__device__ __forceinline__ double yrep_normal(double m) {
    const double q = ((m - 4503599627370496.0) + 0.5) * 1.1102230246251565e-16;   // 2^-53
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        return q * LMC_AS241_RATIO(r, 2.5090809287301226727e+3, 3.3430575583588128105e+4, 6.7265770927008700853e+4,
                                   4.5921953931549871457e+4, 1.3731693765509461125e+4, 1.9715909503065514427e+3,
                                   1.3314166789178437745e+2, 3.3871328727963666080e+0, 5.2264952788528545610e+3,
                                   2.8729085735721942674e+4, 3.9307895800092710610e+4, 2.1213794301586595867e+4,
                                   5.3941960214247511077e+3, 6.8718700749205790830e+2, 4.2313330701600911252e+1);
    }
    const double tail = ((q < 0.0) ? m + 0.5 : 9007199254740992.0 - m - 0.5) * 1.1102230246251565e-16;
    double r = sqrt(-log(tail));
    double x;
    if (r <= 5.0) {
        r = r - 1.6;
        x = LMC_AS241_RATIO(r, 7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1,
                            1.27045825245236838258e+0, 3.64784832476320460504e+0, 5.76949722146069140550e+0,
                            4.63033784615654529590e+0, 1.42343711074968357734e+0, 1.05075007164441684324e-9,
                            5.47593808499534494600e-4, 1.51986665636164571966e-2, 1.48103976427480074590e-1,
                            6.89767334985100004550e-1, 1.67638483018380384940e+0, 2.05319162663775882187e+0);
    } else {
        r = r - 5.0;
        x = LMC_AS241_RATIO(r, 2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3,
                            2.65321895265761230930e-2, 2.96560571828504891230e-1, 1.78482653991729133580e+0,
                            5.46378491116411436990e+0, 6.65790464350110377720e+0, 2.04426310338993978564e-15,
                            1.42151175831644588870e-7, 1.84631831751005468180e-5, 7.86869131145613259100e-4,
                            1.48753612908506148525e-2, 1.36929880922735805310e-1, 5.99832206555887937690e-1);
    }
    return (q < 0.0) ? -x : x;
}

// poisson(lam), 0 < lam < 10: prod *= u_j until prod <= exp(-lam); the number of uniforms before that one
__device__ __forceinline__ double yrep_poisson_mult(YrepStream& s, double lam) {
    const double enlam = exp_lane(-lam);
    double prod = 1.0;
    for (int k = 0; k < kYrepMaxUniforms; ++k) {
        prod *= yrep_uniform(s);
        if (prod <= enlam) return static_cast<double>(k);
    }
    return __builtin_nan("");
}

// poisson(lam), lam >= 10: PTRS, the transformed rejection method with squeeze (Hoermann 1993), numpy's legacy statement
__device__ __forceinline__ double yrep_poisson_ptrs(YrepStream& s, double lam) {
    const double slam = sqrt(lam), loglam = log(lam);
    const double b = 0.931 + 2.53 * slam;
    const double a = -0.059 + 0.02483 * b;
    const double invalpha = 1.1239 + 1.1328 / (b - 3.4);
    const double vr = 0.9277 - 3.6224 / (b - 2.0);
    for (int t = 0; t < kYrepMaxAttempts; ++t) {
        const double U = yrep_uniform(s) - 0.5;
        const double V = yrep_uniform(s);
        const double us = 0.5 - fabs(U);
        const double k = floor((2.0 * a / us + b) * U + lam + 0.43);
        if (us >= 0.07 && V <= vr) return k;
        if (k < 0.0 || (us < 0.013 && V > us)) continue;
        if ((log(V) + log(invalpha) - log(a / (us * us) + b)) <= (-lam + k * loglam - lgamma(k + 1.0))) return k;
    }
    return __builtin_nan("");
}

// y_rep of observation i of the row under draw row r of job chain `chain`: eta the linear predictor (glm_eta_tile), mu its
// mean response (glm_link_of_eta), sigma = 1 / sqrt(isig2) (gaussian).
__device__ __forceinline__ double yrep_value(int lik, double eta, double mu, double sigma, uint32_t seed, uint32_t chain,
                                             uint32_t r, uint32_t i) {
    if (eta != eta || mu != mu || mu == HUGE_VAL) return __builtin_nan("");   // (exp_lane swallows a NaN: eta is asked too)
    YrepStream s = yrep_stream(seed, chain, r, i);
    if (lik == kGlmBernoulli) return (yrep_uniform(s) < mu) ? 1.0 : 0.0;
    if (lik == kGlmPoisson) {
        if (mu > kYrepMaxMu) return __builtin_nan("");
        if (mu == 0.0) return 0.0;
        return (mu < kYrepPtrsLam) ? yrep_poisson_mult(s, mu) : yrep_poisson_ptrs(s, mu);
    }
    return __builtin_fma(sigma, yrep_normal(yrep_integer(s)), eta);
}

}  // namespace lmc
