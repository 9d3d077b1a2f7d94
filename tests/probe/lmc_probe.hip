// Test-only probe: the device primitives of csrc/ (lmc_wave.hpp, lmc_team.hpp, lmc_rng.hpp, lmc_targets.hpp) behind plain
// launchers, so that tests/test_gpu_primitives.py can hold each of them to an exact reference on its own instead of
// through whole trajectories. The product headers are included unchanged and compiled with the library's flags
// (tests/_probe.py); nothing here is part of liblmc_hip.so, and there is no engine: every launcher takes HOST pointers,
// allocates, copies, launches, synchronises and returns the hipError_t (0 = ok, kProbeBadArgument for a shape or size it
// does not have). Every kernel indexes buffers that its launcher sized from the same arguments.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lmc_rng.hpp"
#include "lmc_targets.hpp"
#include "lmc_dispatch.hpp"

namespace lmc {
namespace probe {

constexpr int kProbeBadArgument = -2;

template <class T>
struct DevBuf {
    T* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc(reinterpret_cast<void**>(&p), (n ? n : 1) * sizeof(T)); }
    hipError_t put(const T* host, size_t n) { return n ? hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice) : hipSuccess; }
    hipError_t get(T* host, size_t n) const { return n ? hipMemcpy(host, p, n * sizeof(T), hipMemcpyDeviceToHost) : hipSuccess; }
    hipError_t zero(size_t n) { return hipMemset(p, 0, (n ? n : 1) * sizeof(T)); }
};

#define PROBE_TRY(expr)                                         \
    do {                                                        \
        const hipError_t err_ = (expr);                         \
        if (err_ != hipSuccess) return static_cast<int>(err_);  \
    } while (0)

static int finish(int launch_rc) {
    if (launch_rc != 0) return launch_rc;
    return static_cast<int>(hipDeviceSynchronize());
}

// ---- exponentials: one wave-uniform argument per wave (block b = wave b) ---------------------------------------------------
template <int FAST>
__global__ __launch_bounds__(64) void exp_kernel(const double* x, double* out, int n) {
    const int b = blockIdx.x;
    if (b >= n) return;
    const double arg = x[b];
    const double y = FAST ? exp_uniform_fast(arg) : exp_uniform(arg);
    if (lane_id() == 0) out[b] = y;
    if (lane_id() == 63) out[n + b] = y;   // the value is wave-uniform: the last lane's copy must be the same bits
}

// ---- log_unit: per lane -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void log_unit_kernel(const double* x, double* out, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = log_unit(x[i]);
}

// ---- wave_sum6_totals: in [blocks][6][64], out [blocks][6] ------------------------------------------------------------------
__global__ __launch_bounds__(64) void sum6_kernel(const double* in, double* out) {
    const int b = blockIdx.x, lane = lane_id();
    double d[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) d[k] = in[(static_cast<long long>(b) * 6 + k) * 64 + lane];
    wave_sum6_totals(d);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) out[b * 6 + k] = d[k];
    }
}

// ---- Team<W>: `rounds` consecutive rounds of every team operation in ONE kernel (fresh data each round, so the parity
// double buffering of the LDS exchange is exercised back to back) ------------------------------------------------------------
// in   [blocks][rounds][kTeamIn][T]   T = 64 W threads; rows: sum x | sum2 a, b | nonpositive2 d0, d1 | nonpositive6 d0..d5 |
//                                     bcast0 x | neighbours lo_src, hi_src
// outu [blocks][rounds][W][kTeamUni]  per wave (every wave must hold the same team-uniform value): sum, sum2 a, sum2 b,
//                                     nonpositive2, nonpositive6 (0.0 / 1.0)
// outt [blocks][rounds][kTeamThr][T]  per thread: bcast0, below, above
constexpr int kTeamIn = 14, kTeamUni = 5, kTeamThr = 3;

template <int W>
__global__ __launch_bounds__(64 * W) void team_kernel(const double* in, double* outu, double* outt, int rounds) {
    __shared__ double xbuf[2 * W * kTeamSlots];
    constexpr int T = 64 * W;
    Team<W> tm{xbuf, 0};
    const int t = static_cast<int>(threadIdx.x), b = blockIdx.x;
    const int w = t >> 6;
    for (int r = 0; r < rounds; ++r) {
        const double* row = in + (static_cast<long long>(b) * rounds + r) * kTeamIn * T + t;
        double v[kTeamIn];
#pragma unroll
        for (int k = 0; k < kTeamIn; ++k) v[k] = row[k * T];
        const double s = tm.sum(v[0]);
        double a2 = v[1], b2 = v[2];
        tm.sum2(a2, b2);
        const bool n2 = tm.any_nonpositive2(v[3], v[4]);
        double d6[6] = {v[5], v[6], v[7], v[8], v[9], v[10]};
        const bool n6 = tm.any_nonpositive6(d6);
        const double b0 = tm.bcast0(v[11]);
        double below, above;
        tm.neighbours(v[12], v[13], below, above);
        double* u = outu + ((static_cast<long long>(b) * rounds + r) * W + w) * kTeamUni;
        if ((t & 63) == 0) {
            u[0] = s; u[1] = a2; u[2] = b2; u[3] = n2 ? 1.0 : 0.0; u[4] = n6 ? 1.0 : 0.0;
        }
        double* th = outt + (static_cast<long long>(b) * rounds + r) * kTeamThr * T + t;
        th[0] = b0; th[T] = below; th[2 * T] = above;
    }
}

// ---- densities: logp_grad of functor T<NS> on Team<W>; one chain per block ---------------------------------------------------
// q [chains][d]; logp [chains][W] (one copy per wave); g [chains][64 NS W] (padding slots included)
template <int NS, int W, template <int> class TargetT>
__global__ __launch_bounds__(64 * W) void logp_probe_kernel(int d, const double* tparams, const double* qin, double* logp_out,
                                                            double* g_out) {
    __shared__ double xbuf[2 * W * kTeamSlots];
    constexpr int DP = 64 * NS * W;
    Team<W> tm{xbuf, 0};
    const int c = blockIdx.x, t = static_cast<int>(threadIdx.x);
    TargetT<NS> tgt;
    tgt.init(tm, tparams, d);
    double q[NS], g[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int e = t * NS + s;
        q[s] = (e < d) ? qin[static_cast<long long>(c) * d + e] : 0.0;
    }
    const double logp = tgt.logp_grad(tm, q, g);
#pragma unroll
    for (int s = 0; s < NS; ++s) g_out[static_cast<long long>(c) * DP + t * NS + s] = g[s];
    if ((t & 63) == 0) logp_out[c * W + (t >> 6)] = logp;
}

typedef void (*LogpKernel)(int, const double*, const double*, double*, double*);

// every (NS, W) the product instantiates a density for: the unit kernels (W = 1, NS 1..16), the fused sampling teams
// <4,2> and <4,4> (LMC_PAIR_SHAPES) and the general kernels' 16-wave team (NS 1..16)
template <template <int> class T>
static LogpKernel logp_kernel_of(TargetTag<T>, int ns, int w) {
    if (w == 1) return with_int<1, 2, 4, 8, 16>(ns, [](auto NS) -> LogpKernel { return &logp_probe_kernel<NS, 1, T>; });
    if (w == 16) return with_int<1, 2, 4, 8, 16>(ns, [](auto NS) -> LogpKernel { return &logp_probe_kernel<NS, 16, T>; });
    if (w == 2 && ns == 4) return &logp_probe_kernel<4, 2, T>;
    if (w == 4 && ns == 4) return &logp_probe_kernel<4, 4, T>;
    return nullptr;
}

}  // namespace probe
}  // namespace lmc

using namespace lmc;
using namespace lmc::probe;

#ifndef LMC_PROBE_HASH
#define LMC_PROBE_HASH "unstamped"
#endif

extern "C" {

static const char kProbeStamp[] = "LMC_PROBE_HASH=" LMC_PROBE_HASH;
const char* lmc_probe_hash(void) { return kProbeStamp + 15; }

// which: 0 exp_uniform, 1 exp_uniform_fast. out[0..n) lane 0's value, out[n..2n) lane 63's.
int lmc_probe_exp(int which, const double* x, double* out, int n) {
    if (!x || !out || n < 1 || (which != 0 && which != 1)) return kProbeBadArgument;
    DevBuf<double> dx, dy;
    PROBE_TRY(dx.alloc(n)); PROBE_TRY(dy.alloc(2 * static_cast<size_t>(n)));
    PROBE_TRY(dx.put(x, n));
    const int rc = which ? launch(&exp_kernel<1>, dim3(n), dim3(64), 0, nullptr, dx.p, dy.p, n)
                         : launch(&exp_kernel<0>, dim3(n), dim3(64), 0, nullptr, dx.p, dy.p, n);
    const int done = finish(rc);
    if (done != 0) return done;
    return static_cast<int>(dy.get(out, 2 * static_cast<size_t>(n)));
}

int lmc_probe_log_unit(const double* x, double* out, int n) {
    if (!x || !out || n < 1) return kProbeBadArgument;
    DevBuf<double> dx, dy;
    PROBE_TRY(dx.alloc(n)); PROBE_TRY(dy.alloc(n));
    PROBE_TRY(dx.put(x, n));
    const int done = finish(launch(&log_unit_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, dx.p, dy.p, n));
    if (done != 0) return done;
    return static_cast<int>(dy.get(out, n));
}

int lmc_probe_sum6(const double* in, double* out, int blocks) {
    if (!in || !out || blocks < 1) return kProbeBadArgument;
    const size_t n_in = static_cast<size_t>(blocks) * 6 * 64, n_out = static_cast<size_t>(blocks) * 6;
    DevBuf<double> di, dout;
    PROBE_TRY(di.alloc(n_in)); PROBE_TRY(dout.alloc(n_out));
    PROBE_TRY(di.put(in, n_in));
    const int done = finish(launch(&sum6_kernel, dim3(blocks), dim3(64), 0, nullptr, di.p, dout.p));
    if (done != 0) return done;
    return static_cast<int>(dout.get(out, n_out));
}

int lmc_probe_team_rows(int* n_in, int* n_uniform, int* n_thread) {
    if (n_in) *n_in = kTeamIn;
    if (n_uniform) *n_uniform = kTeamUni;
    if (n_thread) *n_thread = kTeamThr;
    return 0;
}

int lmc_probe_team(int w, int blocks, int rounds, const double* in, double* outu, double* outt) {
    if (!in || !outu || !outt || blocks < 1 || rounds < 1) return kProbeBadArgument;
    if (w != 1 && w != 2 && w != 4 && w != 16) return kProbeBadArgument;
    const size_t T = 64 * static_cast<size_t>(w), br = static_cast<size_t>(blocks) * rounds;
    const size_t n_in = br * kTeamIn * T, n_u = br * w * kTeamUni, n_t = br * kTeamThr * T;
    DevBuf<double> di, du, dt;
    PROBE_TRY(di.alloc(n_in)); PROBE_TRY(du.alloc(n_u)); PROBE_TRY(dt.alloc(n_t));
    PROBE_TRY(di.put(in, n_in));
    const auto kernel = with_int<1, 2, 4, 16>(w, [](auto W) { return &team_kernel<W>; });
    const int done = finish(launch(kernel, dim3(blocks), dim3(64 * w), 0, nullptr, di.p, du.p, dt.p, rounds));
    if (done != 0) return done;
    PROBE_TRY(du.get(outu, n_u));
    return static_cast<int>(dt.get(outt, n_t));
}

// params: n_params doubles (DiagGaussian: d precisions; AR1: c_end, c_mid, off; Normal1D: loc, scale; others: none)
int lmc_probe_logp(int family, int ns, int w, int d, int chains, const double* params, int n_params, const double* q,
                   double* logp, double* g) {
    if (!q || !logp || !g || chains < 1 || d < 1 || ns < 1 || w < 1 || n_params < 0 || (n_params > 0 && !params)) return kProbeBadArgument;
    const auto kernel = with_builtin_target(family, [&](auto t) { return logp_kernel_of(t, ns, w); });
    if (!kernel) return kLaunchUnsupported;
    const int dpad = 64 * ns * w;
    if (d > dpad) return kProbeBadArgument;
    const int need = family == LMC_TARGET_DIAG_GAUSSIAN ? d : family == LMC_TARGET_AR1 ? 3 : family == LMC_TARGET_NORMAL1D ? 2 : 0;
    if (n_params < need) return kProbeBadArgument;
    const size_t n_q = static_cast<size_t>(chains) * d, n_l = static_cast<size_t>(chains) * w, n_g = static_cast<size_t>(chains) * dpad;
    DevBuf<double> dp, dq, dl, dg;
    PROBE_TRY(dp.alloc(n_params)); PROBE_TRY(dq.alloc(n_q)); PROBE_TRY(dl.alloc(n_l)); PROBE_TRY(dg.alloc(n_g));
    PROBE_TRY(dp.zero(n_params));
    PROBE_TRY(dp.put(params, n_params)); PROBE_TRY(dq.put(q, n_q));
    const int done = finish(launch(kernel, dim3(chains), dim3(64 * w), 0, nullptr, d, dp.p, dq.p, dl.p, dg.p));
    if (done != 0) return done;
    PROBE_TRY(dl.get(logp, n_l));
    return static_cast<int>(dg.get(g, n_g));
}

}  // extern "C"
