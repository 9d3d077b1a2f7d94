// Third translation unit of liblmc_hip.so: the tick kernels (externally evaluated log-densities, lmc_tick.hpp).
#include <hip/hip_runtime.h>

#include "lmc_tick.hpp"
#include "lmc_dispatch.hpp"

namespace lmc {

// chains that still want evaluations (only launched when the host asks: one atomic per 256 chains, not per chain
// per tick -- 65 536 atomics on one address cost more than the rest of the tick)
__global__ __launch_bounds__(256) void tick_count_kernel(TickArrays K, int chains) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    const bool active = c < chains && K.phase[c] != kTickDone;
    const unsigned long long m = ballot64(active);
    __shared__ int part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int n = part[0] + part[1] + part[2] + part[3];
        if (n) atomicAdd(K.n_active, n);
    }
}

int tick_launch(int ns, hipStream_t stream, const ChainArrays& A, const TickArrays& K, const SamplerParams& P,
                const double* logp, const double* grad) {
    const auto kernel = with_int<1, 2, 4, 8, 16>(ns, [](auto NS) { return &tick_kernel<NS>; });
    return launch(kernel, dim3(A.chains), dim3(64), 2 * A.dpad * 8, stream, A, K, P, logp, grad);
}

int tick_launch_begin(int ns, hipStream_t stream, const ChainArrays& A, const TickArrays& K, long long iter_begin) {
    const auto kernel = with_int<1, 2, 4, 8, 16>(ns, [](auto NS) { return &tick_begin_kernel<NS>; });
    return launch(kernel, dim3(A.chains), dim3(64), 0, stream, A, K, iter_begin);
}

int tick_launch_count(hipStream_t stream, const TickArrays& K, int chains) {
    return launch(tick_count_kernel, dim3((chains + 255) / 256), dim3(256), 0, stream, K, chains);
}

}  // namespace lmc
