// Sixth translation unit of liblmc_hip.so: Pareto-smoothed importance sampling leave-one-out (PSIS-LOO; Vehtari, Gelman,
// Gabry 2017) of rows of log-likelihood values in HBM. include/lmc_hip.h states the row algorithm (lmc_psis_rows);
// littlemcmc_amd/predictive.py: psis(), loo(). It knows nothing of GLMs: the rows that loo() hands it are written by
// pointwise_loglik_kernel (lmc_predict.hip), and any other log-likelihood array will do.
//
// psis_rows_kernel: one workgroup of kPsisThreads per row, ten passes over the row (256 KB at S = 32 000: it stays in L2):
//   pass 1      min l (c = -min l) and whether every l is finite
//   pass 2..9   radix select of the (M + 1)-th largest lw = min l - l: eight passes of 8 bits, most significant first, over
//               order-preserving 64-bit keys of lw, an LDS histogram of 256 counters (integer LDS atomics) and a suffix
//               count; the key that remains is the cutoff, exactly
//   pass 10     the tail {lw > cutoff} (at most M values) goes to LDS -- its l, appended through an integer LDS counter -- and
//               the other draws are summed: sum w, sum w^2 with w = exp(lw)
//   then, in LDS and registers: a bitonic sort of the tail (descending l = ascending lw; the appended order does not
//   survive it), x_i = exp(lw_i) - exp(cutoff) kept in registers (thread t owns i = t, t + 256, ..: 16 at most), the
//   Zhang-Stephens fit (at most 94 candidates b_j, each one log1p per tail element), the smoothed tail and the sums.
// Every floating-point sum is taken in a fixed order -- a thread's elements ascending, the wavefront by a xor butterfly, the
// wavefronts ascending -- so two calls on the same data give the same bits. LDS: the tail (32 KiB), the histogram (2 KiB),
// the fit's partial sums and candidates (5 KiB) and a few scalars, 40 KiB in all.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lmc_hip.h"

namespace lmc {

constexpr int kPsisThreads = 256;
constexpr int kPsisWaves = kPsisThreads / 64;
constexpr int kPsisMaxTail = LMC_PSIS_MAX_TAIL;
constexpr int kPsisOwn = kPsisMaxTail / kPsisThreads;   // tail elements a thread owns
constexpr int kPsisMaxCand = 30 + 64;                     // m = 30 + floor(sqrt(n_tail)), n_tail <= 4096
constexpr double kLogDblMin = -708.39641853226410622;     // log(DBL_MIN), rounded to nearest
static_assert(kPsisMaxTail == 4096 && kPsisOwn * kPsisThreads == kPsisMaxTail && kPsisWaves == 4, "the tail plan");

// order-preserving key of a double: a < b  <=>  key(a) < key(b) (-0 below +0; no NaN reaches it)
__device__ __forceinline__ unsigned long long psis_key(double v) {
    const unsigned long long u = static_cast<unsigned long long>(__double_as_longlong(v));
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double psis_unkey(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double(static_cast<long long>(u));
}

// sum over the wavefront in a fixed order (every lane gets it)
__device__ __forceinline__ double psis_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// sum over the workgroup: wavefronts ascending; red is kPsisWaves doubles of LDS; every thread gets the same bits
__device__ __forceinline__ double psis_block_sum(double v, double* red) {
    v = psis_wave_sum(v);
    __syncthreads();   // red is free again
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < kPsisWaves; ++w) s += red[w];
    return s;
}

__global__ __launch_bounds__(kPsisThreads) void psis_rows_kernel(const double* __restrict__ lrows, long long S,
                                                                 long long row_stride, int tail_len, double* __restrict__ out) {
    __shared__ double tail[kPsisMaxTail];                      // the tail's l, then sorted descending
    __shared__ unsigned long long hist[256];
    __shared__ double part[kPsisMaxCand][kPsisWaves];         // the fit's per-wavefront partial sums
    __shared__ double cand_b[kPsisMaxCand], cand_L[kPsisMaxCand], cand_bw[kPsisMaxCand];
    __shared__ double red[kPsisWaves];
    __shared__ unsigned long long sel[2];                      // the selected bin, the rank that remains
    __shared__ int tail_n, flags;

    const int tid = static_cast<int>(threadIdx.x);
    const double* l = lrows + static_cast<long long>(blockIdx.x) * row_stride;
    double* o = out + static_cast<long long>(blockIdx.x) * 8;
    const double nan = __builtin_nan("");

    // ---- pass 1: min l, and whether every l is finite
    if (tid == 0) {
        flags = 0;
        tail_n = 0;
    }
    double lmin = HUGE_VAL;
    int bad = 0;   // 1: some +-inf, 2: some NaN
    for (long long s = tid; s < S; s += kPsisThreads) {
        const double v = l[s];
        lmin = fmin(lmin, v);   // (fmin skips a NaN: the flag carries it)
        bad |= (v != v) ? 2 : ((v == HUGE_VAL || v == -HUGE_VAL) ? 1 : 0);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) lmin = fmin(lmin, __shfl_xor(lmin, off, 64));
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = lmin;
    if (bad) atomicOr(&flags, bad);
    __syncthreads();
    lmin = fmin(fmin(red[0], red[1]), fmin(red[2], red[3]));
    const int row_bad = flags;
    if (row_bad) {   // (uniform over the workgroup)
        if (tid == 0) {
            o[0] = o[1] = o[3] = o[4] = o[5] = nan;
            o[2] = 0.0;
            o[6] = (row_bad & 2) ? nan : lmin;
            o[7] = 0.0;
        }
        return;
    }

    // ---- passes 2..9: the (M + 1)-th largest lw by radix select, most significant byte first
    const long long M = (tail_len < S - 1) ? tail_len : S - 1;
    unsigned long long rank = static_cast<unsigned long long>(M) + 1;   // 1-based from the top, <= S
    unsigned long long prefix = 0;
    for (int p = 7; p >= 0; --p) {
        const int shift = 8 * p;
        hist[tid] = 0;
        __syncthreads();
        for (long long s = tid; s < S; s += kPsisThreads) {
            const unsigned long long key = psis_key(lmin - l[s]);
            const bool match = (p == 7) || (((key ^ prefix) >> (shift + 8)) == 0);
            if (match) atomicAdd(&hist[(key >> shift) & 0xff], 1ull);
        }
        __syncthreads();
        unsigned long long above = 0;   // matching keys whose byte is larger than this thread's bin
        for (int b = tid + 1; b < 256; ++b) above += hist[b];
        const unsigned long long mine = hist[tid];
        if (above < rank && rank <= above + mine) {   // exactly one bin
            sel[0] = static_cast<unsigned long long>(tid);
            sel[1] = rank - above;
        }
        __syncthreads();
        prefix |= sel[0] << shift;
        rank = sel[1];
        __syncthreads();
    }
    const double cutoff = fmax(psis_unkey(prefix), kLogDblMin);
    const double expc = exp(cutoff);

    // ---- pass 10: the tail to LDS, the sums of the other draws
    double sw = 0.0, sw2 = 0.0;
    for (long long s = tid; s < S; s += kPsisThreads) {
        const double v = l[s];
        const double lw = lmin - v;
        if (lw > cutoff) {
            const int pos = atomicAdd(&tail_n, 1);
            if (pos < kPsisMaxTail) tail[pos] = v;   // (at most M <= kPsisMaxTail values lie above the (M + 1)-th largest)
        } else {
            const double w = exp(lw);
            sw += w;
            sw2 += w * w;
        }
    }
    __syncthreads();
    const int nt = tail_n < kPsisMaxTail ? tail_n : kPsisMaxTail;
    const double ntd = static_cast<double>(nt);

    // ---- sort the tail: descending l (ascending lw; equal lw in descending l), padding -inf last
    int P = 1;
    while (P < nt) P <<= 1;
    for (int i = nt + tid; i < P; i += kPsisThreads) tail[i] = -HUGE_VAL;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += kPsisThreads) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const double a = tail[i], b = tail[ixj];
                    const bool down = (i & k) == 0;   // this run descends
                    if (down ? (a < b) : (a > b)) {
                        tail[i] = b;
                        tail[ixj] = a;
                    }
                }
            }
            __syncthreads();
        }
    }

    // ---- the fit (n_tail > 4): x in registers, thread t owns i = t + 256 r
    double kk = HUGE_VAL, sigma = nan;
    double x[kPsisOwn];
#pragma unroll
    for (int r = 0; r < kPsisOwn; ++r) {
        const int i = tid + r * kPsisThreads;
        x[r] = (i < nt) ? exp(lmin - tail[i]) - expc : 0.0;
    }
    if (nt > 4) {
        const int m = 30 + static_cast<int>(floor(sqrt(ntd)));
        const int q = static_cast<int>(floor(ntd / 4.0 + 0.5));   // 1-based
        const double xq = exp(lmin - tail[q - 1]) - expc;
        const double xn = exp(lmin - tail[nt - 1]) - expc;
        for (int j = 0; j < m; ++j) {
            const double bj = (1.0 - sqrt(static_cast<double>(m) / (static_cast<double>(j + 1) - 0.5))) / (3.0 * xq) + 1.0 / xn;
            double acc = 0.0;
#pragma unroll
            for (int r = 0; r < kPsisOwn; ++r)
                if (tid + r * kPsisThreads < nt) acc += log1p(-bj * x[r]);
            acc = psis_wave_sum(acc);
            if ((tid & 63) == 0) part[j][tid >> 6] = acc;
            if (tid == 0) cand_b[j] = bj;
        }
        __syncthreads();
        if (tid < m) {
            const double kj = (((part[tid][0] + part[tid][1]) + part[tid][2]) + part[tid][3]) / ntd;
            cand_L[tid] = ntd * (log(-cand_b[tid] / kj) - kj - 1.0);
        }
        __syncthreads();
        if (tid < m) {
            double den = 0.0;
            for (int i = 0; i < m; ++i) den += exp(cand_L[i] - cand_L[tid]);
            cand_bw[tid] = cand_b[tid] * (1.0 / den);
        }
        __syncthreads();
        double b = 0.0;
        for (int j = 0; j < m; ++j) b += cand_bw[j];
        double acc = 0.0;
#pragma unroll
        for (int r = 0; r < kPsisOwn; ++r)
            if (tid + r * kPsisThreads < nt) acc += log1p(-b * x[r]);
        kk = psis_block_sum(acc, red) / ntd;
        sigma = -kk / b;
        kk = (ntd * kk + 5.0) / (ntd + 10.0);
    }

    // ---- the smoothed tail and the sums: A = sum exp(lw' + l - min l) (1 for every draw outside the tail), B = sum exp(lw')
    const bool smooth = nt > 4 && kk == kk && kk != HUGE_VAL && kk != -HUGE_VAL;
    double sa = 0.0;
#pragma unroll
    for (int r = 0; r < kPsisOwn; ++r) {
        const int i = tid + r * kPsisThreads;
        if (i < nt) {
            const double lw = lmin - tail[i];
            double lwn = lw;
            if (smooth) {
                const double pi = (static_cast<double>(i + 1) - 0.5) / ntd;
                lwn = log(expc + sigma * expm1(-kk * log1p(-pi)) / kk);
            }
            lwn = (lwn > 0.0) ? 0.0 : lwn;
            sa += exp(lwn - lw);
            const double w = exp(lwn);
            sw += w;
            sw2 += w * w;
        }
    }
    const double A = static_cast<double>(S - nt) + psis_block_sum(sa, red);
    const double B = psis_block_sum(sw, red);
    const double B2 = psis_block_sum(sw2, red);
    if (tid == 0) {
        o[0] = lmin + (log(A) - log(B));
        o[1] = kk;
        o[2] = ntd;
        o[3] = sigma;
        o[4] = (B * B) / B2;
        o[5] = cutoff;
        o[6] = lmin;
        o[7] = 0.0;
    }
}

}  // namespace lmc

// See include/lmc_hip.h. l and out are DEVICE pointers on the current device; the work is enqueued on `stream`.
extern "C" int lmc_psis_rows(const double* l, int64_t rows, int64_t S, int64_t row_stride, int32_t tail_len, double* out,
                             void* stream) {
    using namespace lmc;
    if (!l || !out || rows < 1 || S < 1 || row_stride < S) return LMC_ERR_INVALID;
    if (tail_len < 0 || tail_len > LMC_PSIS_MAX_TAIL || (S > 1 && tail_len >= S)) return LMC_ERR_INVALID;
    if (rows >= (int64_t(1) << 31)) return LMC_ERR_INVALID;
    (void)hipGetLastError();
    hipLaunchKernelGGL(psis_rows_kernel, dim3(static_cast<unsigned>(rows)), dim3(kPsisThreads), 0, static_cast<hipStream_t>(stream),
                       l, static_cast<long long>(S), static_cast<long long>(row_stride), static_cast<int>(tail_len), out);
    return hipGetLastError() == hipSuccess ? LMC_OK : LMC_ERR_HIP;
}
