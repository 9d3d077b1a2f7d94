// Third translation unit of liblmc_hip.so: the general ("wide") kernels (lmc_wide.hpp) and their launchers -- model_ndim
// beyond 1024, dense mass matrices beyond 256 dimensions, float64 adaptive diagonals. Compiled in parallel with
// lmc_engine.hip and lmc_dense.hip.
#include <hip/hip_runtime.h>

#include "../../include/lmc_hip.h"
#include "lmc_wide.hpp"
#include "lmc_tick.hpp"
#include "lmc_wide_launch.hpp"
#include "lmc_dispatch.hpp"

namespace lmc {

static_assert(kWideBlock == kWideThreads, "launcher and kernel agree on the team size");

// (elements per thread, wavefronts per chain): one wavefront with up to 8 elements per lane (model_ndim <= 512), the
// 16-wavefront team beyond -- the measured crossover (tools/wide_team_ab.py). f(NS, W) for the shape,
// nullptr for any other.
template <class F>
static auto with_wide_shape(int ns, int w, F&& f) {
    return with_int<1, kWideWaves>(w, [&](auto W) {
        if constexpr (W == 1) return with_int<1, 2, 4, 8>(ns, [&](auto NS) { return f(NS, W); });
        else return with_int<1, 2, 4, 8, 16>(ns, [&](auto NS) { return f(NS, W); });
    });
}
template <template <int> class T>
static auto run_wide_for(TargetTag<T>, int ns, int w) {
    return with_wide_shape(ns, w, [](auto NS, auto W) -> decltype(&run_wide_kernel<1, 1, T>) {
        if constexpr (has_shape<T>(NS, W)) return &run_wide_kernel<NS, W, T>;
        else return nullptr;
    });
}
template <template <int> class T>
static auto logp_wide_for(TargetTag<T>, int ns, int w) {
    return with_wide_shape(ns, w, [](auto NS, auto W) -> decltype(&wide_logp_kernel<1, 1, T>) {
        if constexpr (has_shape<T>(NS, W)) return &wide_logp_kernel<NS, W, T>;
        else return nullptr;
    });
}
template <template <int> class T>
static auto trajectory_wide_for(TargetTag<T>, int ns, int w) {
    return with_wide_shape(ns, w, [](auto NS, auto W) -> decltype(&wide_trajectory_kernel<1, 1, T>) {
        if constexpr (has_shape<T>(NS, W)) return &wide_trajectory_kernel<NS, W, T>;
        else return nullptr;
    });
}

int wide_scratch_slots(int max_levels) { return wide_scratch_vectors(max_levels); }
int wide_lds_bytes(int dpad) { return wide_lds_doubles(dpad) * 8; }

int wide_launch_run(int family, int ns, int w, hipStream_t stream, const ChainArrays& A, const DenseArrays& D, const SamplerParams& P,
                    const double* tparams, int n_chains) {
    const auto kernel = with_target(family, [&](auto t) { return run_wide_for(t, ns, w); });
    return launch(kernel, dim3(n_chains > 0 ? n_chains : A.chains), dim3(64 * w), wide_lds_bytes(A.dpad), stream, A, D, P, tparams);
}

int wide_launch_logp(int family, int ns, int w, hipStream_t stream, const ChainArrays& A, const double* tparams, const double* q,
                     double* logp, double* grad) {
    const auto kernel = with_target(family, [&](auto t) { return logp_wide_for(t, ns, w); });
    return launch(kernel, dim3(A.chains), dim3(64 * w), 2 * kWideWaves * kTeamSlots * 8, stream, A, tparams, q, logp, grad);
}

int wide_launch_trajectory(int family, int ns, int w, hipStream_t stream, const ChainArrays& A, const DenseArrays& D,
                           const double* tparams, const double* q0, const double* p0, int p0_is_f32, int sdot_mode, double eps,
                           int n_fwd, int n_back, double* oq, double* op, double* ov, double* og, double* oe, double* ol) {
    const auto kernel = with_target(family, [&](auto t) { return trajectory_wide_for(t, ns, w); });
    return launch(kernel, dim3(A.chains), dim3(64 * w), wide_lds_bytes(A.dpad), stream, A, D, tparams, q0, p0, p0_is_f32, sdot_mode,
                  eps, n_fwd, n_back, oq, op, ov, og, oe, ol);
}

int wide_launch_momentum(int ns, int w, hipStream_t stream, const ChainArrays& A, const DenseArrays& D, int momentum_f32, double* out) {
    const auto kernel = with_wide_shape(ns, w, [](auto NS, auto W) { return &wide_momentum_kernel<NS, W>; });
    return launch(kernel, dim3(A.chains), dim3(64 * w), wide_lds_bytes(A.dpad), stream, A, D, momentum_f32, out);
}

// ---- the tick state machine (lmc_tick.hpp: tick_step) for the shapes of the general kernels: externally evaluated densities
// (a Python callable, a batched torch callable) beyond 1024 dimensions. One chain = a workgroup of 16 wavefronts, model_ndim
// up to 16 384, diagonal mass matrices. What differs from the one-wavefront shape: the team's reductions and barriers, the
// normals drawn 1024 at a time by wave 0 (numpy's stream is sequential), the uniform stream shared by the team.
struct TickWideShape {
    typedef WideTeam TeamT;
    static constexpr int kThreads = kWideThreads;
    TeamT tm;
    double* bcast;
    __device__ __forceinline__ TickWideShape(double* lds, int dpad) {
        tm.xbuf = lds + wide_stage_doubles(dpad);
        tm.parity = 0;
        bcast = tm.xbuf + 2 * kWideWaves * kTeamSlots;
    }
    template <int NS>
    __device__ __forceinline__ void normals(RngState& rng, int d, int, double* lds, double (&z)[NS]) {
        wide_normals_regs<NS>(tm, rng, d, lds, bcast, z);
    }
};

template <int NS>
__global__ __launch_bounds__(kWideThreads, 1) void tick_wide_kernel(ChainArrays A, TickArrays K, SamplerParams P, const double* logp_in,
                                                                     const double* grad_in) {
    extern __shared__ __attribute__((aligned(16))) double lds[];   // wide_stage_doubles(dpad): normals chunk + staging / sdot staging; team exchange; broadcast words
    TickWideShape shape(lds, A.dpad);
    TickDiagMass<NS> mass(A, static_cast<long long>(blockIdx.x) * A.dpad, static_cast<int>(threadIdx.x));
    tick_step<NS>(A, K, P, logp_in, grad_in, lds, shape, mass, nullptr);
}

int tick_wide_launch(int ns, hipStream_t stream, const ChainArrays& A, const TickArrays& K, const SamplerParams& P,
                     const double* logp, const double* grad) {
    const auto kernel = with_int<1, 2, 4, 8, 16>(ns, [](auto NS) { return &tick_wide_kernel<NS>; });
    return launch(kernel, dim3(A.chains), dim3(kWideThreads), wide_lds_bytes(A.dpad), stream, A, K, P, logp, grad);
}

int tick_wide_launch_begin(int ns, hipStream_t stream, const ChainArrays& A, const TickArrays& K, long long iter_begin) {
    const auto kernel = with_int<1, 2, 4, 8, 16>(ns, [](auto NS) { return &tick_begin_kernel<NS, kWideThreads>; });
    return launch(kernel, dim3(A.chains), dim3(kWideThreads), 0, stream, A, K, iter_begin);
}

int wide_launch_mass_update(int ns, int w, hipStream_t stream, const ChainArrays& A, const SamplerParams& P) {
    const auto kernel = with_wide_shape(ns, w, [](auto NS, auto W) { return &wide_mass_update_kernel<NS, W>; });
    return launch(kernel, dim3(A.chains), dim3(64 * w), 0, stream, A, P);
}

}  // namespace lmc
