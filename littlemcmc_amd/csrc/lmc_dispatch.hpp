// Host side of every launcher: run-time values (target family, elements per lane, waves per chain, ...) -> the kernel
// template instantiation, and the one way a kernel is launched. Kernels are chosen as typed pointers: a selector maps the
// run-time values to &kernel<...> or to nullptr when this build has no such instantiation, and launch() turns nullptr into
// kLaunchUnsupported.
//
// Include this header after the kernel headers of the translation unit: it includes LMC_USER_TARGET_HEADER (the functor
// UserTarget of a private build around a user density), whose code may use their device helpers.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include "../../include/lmc_hip.h"
#include "lmc_targets.hpp"
#ifdef LMC_USER_TARGET_HEADER
#include LMC_USER_TARGET_HEADER
#endif

namespace lmc {

constexpr int kLaunchUnsupported = -1;   // a launcher's result when this build has no such kernel (otherwise 0 or a hipError_t)

#ifdef LMC_USER_TARGET_HEADER
constexpr bool kUserCompiledIn = true;    // a private library around a user density: UserTarget is a family like the others
#else
constexpr bool kUserCompiledIn = false;   // LMC_TARGET_USER runs kernels compiled at run time (hiprtc), loaded as a module
#endif

// a density functor template (StdNormalTarget, ..., UserTarget) as a value: selectors take it as `TargetTag<T>` and so
// name the template itself, which is what the kernels are instantiated over
template <template <int> class T>
struct TargetTag {};

static_assert(kGlmHeader == LMC_GLM_HEADER && kGlmBernoulli == LMC_GLM_BERNOULLI && kGlmPoisson == LMC_GLM_POISSON &&
              kGlmGaussian == LMC_GLM_GAUSSIAN && kGlmMaxDim == LMC_GLM_MAX_DIM && kGLM == LMC_TARGET_GLM, "lmc_targets.hpp and lmc_hip.h agree");

// A family whose functor gathers across the lanes of ONE wavefront (GLMTarget) has kernels only where a chain is one
// wavefront: a selector returns nullptr for it at any other shape (waves per chain > 1, more elements per lane than one wave
// of the general kernels takes) instead of instantiating a kernel that could not run.
template <template <int> class T>
constexpr bool kOneWaveOnly = std::is_same<TargetTag<T>, TargetTag<GLMTarget>>::value;
constexpr int kOneWaveMaxNs = 8;   // LMC_GLM_MAX_DIM / 64
template <template <int> class T>
constexpr bool has_shape(int ns, int w) { return !kOneWaveOnly<T> || (w == 1 && ns <= kOneWaveMaxNs); }

// f(TargetTag<T>{}) for the functor of a built-in family, whatever LMC_ONLY_USER says; R{} (nullptr, false) for any other
template <class F>
auto with_builtin_target(int family, F&& f) {
    typedef decltype(f(TargetTag<StdNormalTarget>{})) R;
    switch (family) {
        case LMC_TARGET_STD_NORMAL: return f(TargetTag<StdNormalTarget>{});
        case LMC_TARGET_DIAG_GAUSSIAN: return f(TargetTag<DiagGaussianTarget>{});
        case LMC_TARGET_AR1: return f(TargetTag<AR1Target>{});
        case LMC_TARGET_FUNNEL: return f(TargetTag<FunnelTarget>{});
        case LMC_TARGET_NORMAL1D: return f(TargetTag<Normal1DTarget>{});
        default: return R{};
    }
}

// ... and for the functor of any family of the stock library: the built-in ones and GLMTarget. GLMTarget is kept out of
// with_builtin_target because that list is also what the test probe instantiates its kernels over, at EVERY shape (teams of 16
// wavefronts, 16 elements per lane), and GLMTarget exists for one-wavefront chains only (has_shape).
template <class F>
auto with_stock_target(int family, F&& f) {
#ifndef LMC_ONLY_USER   // (a private library around a user density stays without it)
    if (family == LMC_TARGET_GLM) return f(TargetTag<GLMTarget>{});
#endif
    return with_builtin_target(family, f);
}

// f(TargetTag<T>{}) for every family whose kernels this build instantiates; R{} for a family it does not have. A JIT build
// around a user density (LMC_USER_TARGET_HEADER with LMC_ONLY_USER) has that family only: seconds to compile, not a minute.
template <class F>
auto with_target(int family, F&& f) {
#ifdef LMC_USER_TARGET_HEADER
    if (family == LMC_TARGET_USER) return f(TargetTag<UserTarget>{});
#ifdef LMC_ONLY_USER
    return decltype(f(TargetTag<UserTarget>{})){};
#else
    return with_stock_target(family, f);
#endif
#else
    return with_stock_target(family, f);
#endif
}

// f(std::integral_constant<int, V>{}) for the V of Vs equal to v (elements per lane, waves per chain); R{} if none is
template <int V, int... Vs, class F>
auto with_int(int v, F&& f) {
    if (v == V) return f(std::integral_constant<int, V>{});
    if constexpr (sizeof...(Vs) > 0) return with_int<Vs...>(v, f);
    else return decltype(f(std::integral_constant<int, V>{})){};
}

// A kernel that takes more than 64 KiB of dynamic LDS must be allowed to before it is launched (or its occupancy is asked for).
template <class... KernelArgs>
hipError_t allow_lds(void (*kernel)(KernelArgs...), int lds) {
    if (lds <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
}

// Launch `kernel` (nullptr: kLaunchUnsupported). hipMemcpy(..., hipMemcpyDefault) on pageable host pointers can leave a
// stale "last error" behind (pointer-attribute probing): it is cleared first, so that the result is THIS launch's.
template <class... KernelArgs, class... Args>
int launch(void (*kernel)(KernelArgs...), dim3 grid, dim3 block, int lds, hipStream_t stream, Args&&... args) {
    if (!kernel) return kLaunchUnsupported;
    (void)hipGetLastError();
    const hipError_t err = allow_lds(kernel, lds);
    if (err != hipSuccess) return static_cast<int>(err);
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, std::forward<Args>(args)...);
    return static_cast<int>(hipGetLastError());
}

}  // namespace lmc
