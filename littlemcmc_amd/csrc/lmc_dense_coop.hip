// Third translation unit of liblmc_hip.so: the dense-mass sampling kernel for a matrix shared by all chains
// (QuadPotentialFull, /root/reference/littlemcmc/quadpotential.py:428-464) on the matrix cores. Eight one-wavefront
// chains share a workgroup and meet once per leapfrog for one v_mfma_f64_16x16x4_f64 product (lmc_dense.hpp:
// coop_product / run_dense_coop_kernel). A block here holds eight chains side by side, so "the thread's index in its
// chain" is the lane -- the one definition the shared device code needs to know about.
#include <hip/hip_runtime.h>

#define LMC_CHAIN_THREAD (static_cast<int>(threadIdx.x) & 63)
#define LMC_DENSE_COOP 1
#include "../../include/lmc_hip.h"
#include "lmc_dense.hpp"
#include "lmc_dense_launch.hpp"
#include "lmc_dispatch.hpp"

namespace lmc {

int dense_coop_lds_slots(int d, int dpad, int max_slots) {   // tree slots per chain that fit next to the panels (one workgroup per CU)
    long slots = (160L * 1024 - coop_lds_bytes(d, dpad, 0)) / (static_cast<long>(kCoopWaves) * dpad * 8);
    if (slots > max_slots) slots = max_slots;
    return static_cast<int>(slots < 0 ? 0 : slots);
}

typedef void (*CoopKernel)(ChainArrays, DenseArrays, SamplerParams, const double*, int);
// the shared-matrix kernel of (family, ns), nullptr where there is none: the stock library's families but the 1-D one (whatever the
// build), one or two elements per lane (dpad <= 128: the float32 matrix fits one CU's LDS next to the panels)
template <template <int> class T>
static CoopKernel coop_kernel_for(TargetTag<T>, int ns) {
    return with_int<1, 2>(ns, [](auto NS) -> CoopKernel {
        if constexpr (std::is_same<TargetTag<T>, TargetTag<Normal1DTarget>>::value) return nullptr;
        else return &run_dense_coop_kernel<NS, T>;
    });
}
static CoopKernel coop_kernel(int family, int ns) {
    return with_stock_target(family, [&](auto t) { return coop_kernel_for(t, ns); });
}

int dense_coop_supported(int family, int ns, int d, int dpad) {
    return coop_kernel(family, ns) != nullptr && coop_lds_bytes(d, dpad, 0) <= 160 * 1024;
}

int dense_launch_run_coop(int family, int ns, hipStream_t stream, const ChainArrays& A, const DenseArrays& D,
                          const SamplerParams& P, const double* tparams, int n_chains) {
    const int n = n_chains > 0 ? n_chains : A.chains;
    return launch(coop_kernel(family, ns), dim3((n + kCoopWaves - 1) / kCoopWaves), dim3(64 * kCoopWaves),
                  coop_lds_bytes(A.d, A.dpad, D.lds_slots), stream, A, D, P, tparams, n);
}

}  // namespace lmc
