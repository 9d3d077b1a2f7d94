// Translation unit of liblmc_hip.so: the second moment of the positions of ALL chains, the statistic a shared dense mass
// matrix is adapted from during tuning (QuadPotentialFullPooled; lmc_engine_pool_* in include/lmc_hip.h).
//
// One snapshot is the contraction  S += X^T X  with X = q - shift, [C x dpad]: chains are the K dimension. It is split over
// workgroups in contiguous chain ranges (pool_plan: two workgroups per compute unit where the registers allow, so that one
// stages while the other multiplies); a workgroup stages 32 chains at a time through LDS, centred, and its eight
// wavefronts deal the 16 x 16 tiles of the lower triangle among themselves -- tile (ti, tj) of a chunk is eight
// v_mfma_f64_16x16x4_f64 with A[i][k] = X[k][16 ti + i], B[k][j] = X[k][16 tj + j], accumulated in registers over the
// workgroup's whole range. Every workgroup writes its tiles (and its column sums) as partials; pool_reduce_kernel adds them
// in workgroup order. No floating-point atomics anywhere: the same positions give the same bits.
// Padding columns of q are zero and so is their shift: they contribute exact zeros. Rows past the last chain are staged as
// zeros (not as -shift).
// Bound from shapes: one read of C * dpad * 8 bytes and C * dpad^2 FMA (about half of it, for the triangle).
#include <hip/hip_runtime.h>

#include "lmc_pool.hpp"
#include "lmc_dispatch.hpp"

namespace lmc {

typedef double v4d __attribute__((ext_vector_type(4)));

// tile t of the lower triangle, row by row: t = ti (ti + 1) / 2 + tj, tj <= ti
__device__ __forceinline__ void pool_tile_of(int t, int& ti, int& tj) {
    int i = 0;
    while ((i + 1) * (i + 2) / 2 <= t) ++i;
    ti = i;
    tj = t - i * (i + 1) / 2;
}

// column sums of q over the workgroup's chain range: thread = column (dpad <= 256 threads per row, 256 / dpad rows per pass)
__global__ __launch_bounds__(256) void pool_colsum_kernel(const double* __restrict__ q, int chains, PoolArrays P) {
    __shared__ double cs[256];
    const int tid = static_cast<int>(threadIdx.x), dp = P.dpad;
    const int col = tid % dp, r0 = tid / dp, rstep = 256 / dp;
    const long long c0 = static_cast<long long>(blockIdx.x) * P.chunks_per_group * kPoolChunk;
    long long c1 = c0 + static_cast<long long>(P.chunks_per_group) * kPoolChunk;
    if (c1 > chains) c1 = chains;
    double sum = 0.0;
    for (long long c = c0 + r0; c < c1; c += rstep) sum += q[c * dp + col];
    cs[tid] = sum;
    __syncthreads();
    if (tid < dp) {
        double a = cs[tid];
        for (int k = 1; k < rstep; ++k) a += cs[tid + k * dp];
        P.spart[static_cast<size_t>(blockIdx.x) * dp + tid] = a;
    }
}

// sum over workgroups g in [g0, g1) of p[g * stride], in order; the loads of eight terms are in flight together (the terms
// are independent, the additions are not: one load per addition would cost a memory latency each)
__device__ __forceinline__ double pool_sum_groups(const double* __restrict__ p, size_t stride, int g0, int g1) {
    double a = 0.0;
    int g = g0;
    for (; g + 8 <= g1; g += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = p[static_cast<size_t>(g + u) * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) a += v[u];
    }
    for (; g < g1; ++g) a += p[static_cast<size_t>(g) * stride];
    return a;
}

__global__ __launch_bounds__(256) void pool_shift_kernel(int chains, PoolArrays P) {
    const int j = static_cast<int>(threadIdx.x);
    if (j >= P.dpad) return;
    P.shift[j] = pool_sum_groups(P.spart + j, P.dpad, 0, P.groups) / static_cast<double>(chains);
}

// NT = dpad / 16 tile rows. Dynamic LDS: the chunk [32][dpad + 16] (the 16 doubles of padding put the two k-rows a half-wave
// reads on disjoint banks) and 512 doubles for the column sums.
template <int NT>
__global__ __launch_bounds__(64 * kPoolWaves) void pool_accumulate_kernel(const double* __restrict__ q, int chains, PoolArrays P) {
    constexpr int DP = 16 * NT, XS = DP + 16, T = NT * (NT + 1) / 2, TPW = (T + kPoolWaves - 1) / kPoolWaves;
    constexpr int THREADS = 64 * kPoolWaves, RSTEP = THREADS / DP;
    extern __shared__ double pool_lds[];
    double* x = pool_lds;
    double* cs = pool_lds + kPoolChunk * XS;
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int col = tid % DP, r0 = tid / DP;
    const long long c0 = static_cast<long long>(blockIdx.x) * P.chunks_per_group * kPoolChunk;
    long long c1 = c0 + static_cast<long long>(P.chunks_per_group) * kPoolChunk;
    if (c1 > chains) c1 = chains;
    const double sh = P.shift[col];
    double colsum = 0.0;
    int ti[TPW], tj[TPW];
    v4d acc[TPW];
#pragma unroll
    for (int u = 0; u < TPW; ++u) {
        const int t = wave + kPoolWaves * u;
        pool_tile_of(t < T ? t : 0, ti[u], tj[u]);
        acc[u] = v4d{0.0, 0.0, 0.0, 0.0};
    }
    for (long long c = c0; c < c1; c += kPoolChunk) {
        __syncthreads();   // the previous chunk has been read by every wave
#pragma unroll
        for (int rr = 0; rr < kPoolChunk / RSTEP; ++rr) {
            const int r = r0 + rr * RSTEP;
            double v = 0.0;
            if (c + r < c1) {
                v = q[(c + r) * DP + col] - sh;
                colsum += v;
            }
            x[r * XS + col] = v;
        }
        __syncthreads();
        // operand layout of the instruction: A[i][k] on lane i + 16 k, B[k][j] on lane j + 16 k
        const double* xr = x + (lane >> 4) * XS + (lane & 15);
#pragma unroll
        for (int kb = 0; kb < kPoolChunk / 4; ++kb) {
#pragma unroll
            for (int u = 0; u < TPW; ++u) {
                if (wave + kPoolWaves * u < T) {   // (the same for every lane of a wave)
                    const double a = xr[4 * kb * XS + 16 * ti[u]];
                    const double b = xr[4 * kb * XS + 16 * tj[u]];
                    acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[u], 0, 0, 0);
                }
            }
        }
    }
    // result layout: D[row = (lane >> 4) + 4 r][col = lane & 15] in result register r
#pragma unroll
    for (int u = 0; u < TPW; ++u) {
        const int t = wave + kPoolWaves * u;
        if (t < T) {
            double* o = P.part + (static_cast<size_t>(blockIdx.x) * T + t) * 256 + (lane >> 4) * 16 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) o[64 * r] = acc[u][r];
        }
    }
    cs[tid] = colsum;
    __syncthreads();
    if (tid < DP) {
        double a = cs[tid];
#pragma unroll
        for (int k = 1; k < RSTEP; ++k) a += cs[tid + k * DP];
        P.spart[static_cast<size_t>(blockIdx.x) * DP + tid] = a;
    }
}

// S, s, n += the partials: block t < tiles adds tile t, the last block adds s and n. Thread = (entry, quarter of the workgroup
// range): the quarters are summed side by side, each in workgroup order, and added in the order of the quarters.
__global__ __launch_bounds__(256 * kPoolReduceSplit) void pool_reduce_kernel(int chains, PoolArrays P) {
    __shared__ double quarter[kPoolReduceSplit][256];
    const int tiles = pool_tiles(P.dpad), t = static_cast<int>(blockIdx.x);
    const int e = static_cast<int>(threadIdx.x) & 255, k = static_cast<int>(threadIdx.x) >> 8;
    const int per = (P.groups + kPoolReduceSplit - 1) / kPoolReduceSplit;
    const int g0 = k * per < P.groups ? k * per : P.groups, g1 = g0 + per < P.groups ? g0 + per : P.groups;
    if (t < tiles) quarter[k][e] = pool_sum_groups(P.part + static_cast<size_t>(t) * 256 + e, static_cast<size_t>(tiles) * 256, g0, g1);
    else quarter[k][e] = e < P.dpad ? pool_sum_groups(P.spart + e, P.dpad, g0, g1) : 0.0;
    __syncthreads();
    if (k != 0) return;
    double a = quarter[0][e];
#pragma unroll
    for (int u = 1; u < kPoolReduceSplit; ++u) a += quarter[u][e];
    if (t < tiles) {
        int ti, tj;
        pool_tile_of(t, ti, tj);
        P.S[static_cast<size_t>(16 * ti + (e >> 4)) * P.dpad + 16 * tj + (e & 15)] += a;
        return;
    }
    if (e < P.dpad) P.s[e] += a;
    if (e == 0) *P.n += chains;
}

__global__ void pool_restart_da_kernel(double* da, int* da_count, int chains) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= chains) return;
    da[c * 4 + 3] = log(10.0 * exp(da[c * 4 + 0]));
    da[c * 4 + 1] = 0.0;
    da[c * 4 + 2] = 0.0;
    da_count[c] = 1;
}

int pool_launch_shift(hipStream_t stream, const PoolArrays& P, const double* q, int chains) {
    const int rc = launch(pool_colsum_kernel, dim3(P.groups), dim3(256), 0, stream, q, chains, P);
    if (rc != 0) return rc;
    return launch(pool_shift_kernel, dim3(1), dim3(256), 0, stream, chains, P);
}

typedef void (*PoolKernel)(const double*, int, PoolArrays);

int pool_launch_accumulate(hipStream_t stream, const PoolArrays& P, const double* q, int chains) {
    const PoolKernel kernel = with_int<4, 8, 16>(P.dpad / 16, [](auto NT) -> PoolKernel { return &pool_accumulate_kernel<NT>; });
    const int lds = (kPoolChunk * (P.dpad + 16) + 64 * kPoolWaves) * static_cast<int>(sizeof(double));
    const int rc = launch(kernel, dim3(P.groups), dim3(64 * kPoolWaves), lds, stream, q, chains, P);
    if (rc != 0) return rc;
    return launch(pool_reduce_kernel, dim3(pool_tiles(P.dpad) + 1), dim3(256 * kPoolReduceSplit), 0, stream, chains, P);
}

int pool_launch_restart_da(hipStream_t stream, double* da, int* da_count, int chains) {
    return launch(pool_restart_da_kernel, dim3((chains + 255) / 256), dim3(256), 0, stream, da, da_count, chains);
}

}  // namespace lmc
