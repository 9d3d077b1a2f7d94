// The host-side prologue of a pass over the trace, stated ONCE for the nine entry points that make one (lmc_diag.hip,
// lmc_select.hip, the two of lmc_predict.hip, lmc_linpred.hip, lmc_cross.hip, the two of lmc_yrep.hip, and lmc_threshold.hip). Host code only: pure argument checks that return
// LMC_ERR_INVALID before any HIP call, and the one host look at the headers of a GLM table. What differs per pass -- its
// output pointers, its own limits, its launch geometry -- stays in the entry point.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/lmc_hip.h"

namespace lmc {

// The groups a block of a job's chains touches: chain c of the block is chain first_chain + c of the job and lies in group
// (first_chain + c) / per (lmc_target_param_row); the block touches the groups [g0, g0 + groups).
struct TraceSpan {
    int64_t per, g0, groups;
};

// The view x[chains][draws_stride][dim], its sub-series [t0, t0 + n) and the grouping: every index below 2^31. per is
// chains_per_group clamped below 2^31 (no job chain has an index >= 2^31: the same groups).
inline int trace_span(const double* x, int64_t chains, int64_t draws_stride, int32_t dim, int64_t t0, int64_t n,
                      int64_t first_chain, int64_t chains_per_group, TraceSpan* out) {
    const int64_t lim = int64_t(1) << 31;
    if (!x || chains < 1 || dim < 1 || n < 1 || t0 < 0 || n > draws_stride || t0 > draws_stride - n) return LMC_ERR_INVALID;
    if (first_chain < 0 || chains_per_group < 1 || chains >= lim || first_chain >= lim || first_chain + chains >= lim)
        return LMC_ERR_INVALID;
    const int64_t per = chains_per_group < lim ? chains_per_group : lim - 1;
    int64_t g0 = 0, g1 = 0;                             // the groups of the block's first and last chain
    if (lmc_target_param_row(0, first_chain, per, &g0) != LMC_OK || lmc_target_param_row(chains - 1, first_chain, per, &g1) != LMC_OK)
        return LMC_ERR_INVALID;
    *out = {per, g0, g1 - g0 + 1};
    return LMC_OK;
}

// npad of a GLM row of row_len doubles at dimension dim, or 0 if no N gives that length (pure arithmetic)
inline int64_t glm_npad_of_row(int64_t row_len, int32_t dim) {
    int64_t ns = 1;
    while (ns * 64 < dim) ns *= 2;
    const int64_t per_obs = 1 + (dim + 7) / 8 * 8 + 64 * ns;
    if (row_len <= LMC_GLM_HEADER || row_len >= LMC_GLM_MAX_ROW || (row_len - LMC_GLM_HEADER) % per_obs != 0) return 0;
    const int64_t npad = (row_len - LMC_GLM_HEADER) / per_obs;
    return (npad % 64 == 0) ? npad : 0;
}

// A table rows[n_rows][row_len] of GLM parameter rows under a span, and a half-open range [ob0, ob1) of its nob = npad / 64
// blocks of 64 observations: every touched group has a row, the row length is that of some N at this dim, the range is not
// empty and lies inside. Pure: an entry point checks its own launch limits next, and only then looks at the headers.
struct GlmSpan {
    int64_t npad, nob;
};

inline int glm_span(const double* rows, int64_t row_len, int64_t n_rows, int32_t dim, const TraceSpan& span, int64_t ob0,
                    int64_t ob1, GlmSpan* out) {
    if (!rows || dim > LMC_GLM_MAX_DIM || n_rows < 1 || span.g0 + span.groups > n_rows) return LMC_ERR_INVALID;
    const int64_t npad = glm_npad_of_row(row_len, dim);
    if (npad < 64 || ob0 < 0 || ob1 <= ob0 || ob1 > npad / 64) return LMC_ERR_INVALID;
    *out = {npad, npad / 64};
    return LMC_OK;
}

// The headers of the span's rows of a DEVICE table: one strided copy on s, the entry points' only host look, before anything
// is launched. LMC_ERR_INVALID for a header that disagrees with dim or row_len (npad) or carries an unknown likelihood code.
inline int glm_check_headers(const double* rows, int64_t row_len, const TraceSpan& span, int64_t npad, int32_t dim, hipStream_t s) {
    std::vector<double> hdr(static_cast<size_t>(span.groups) * LMC_GLM_HEADER);
    if (hipMemcpy2DAsync(hdr.data(), LMC_GLM_HEADER * sizeof(double), rows + span.g0 * row_len,
                         static_cast<size_t>(row_len) * sizeof(double), LMC_GLM_HEADER * sizeof(double),
                         static_cast<size_t>(span.groups), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        (void)hipGetLastError();
        return LMC_ERR_HIP;
    }
    int64_t ns = 1;
    while (ns * 64 < dim) ns *= 2;
    for (int64_t i = 0; i < span.groups; ++i) {
        const double* h = hdr.data() + i * LMC_GLM_HEADER;
        const bool lik_ok = h[0] == LMC_GLM_BERNOULLI || h[0] == LMC_GLM_POISSON || h[0] == LMC_GLM_GAUSSIAN;
        const bool n_ok = h[1] >= 1.0 && h[1] <= static_cast<double>(npad) && h[1] > static_cast<double>(npad - 64);
        if (!lik_ok || !n_ok || h[2] != static_cast<double>(npad) || h[5] != static_cast<double>(dim) ||
            h[6] != static_cast<double>(64 * ns))
            return LMC_ERR_INVALID;
    }
    return LMC_OK;
}

}  // namespace lmc
