// Per-field error sums on the device (pinn_field_error_sums of include/pinn_hip.h): what stands between a predict call and the relative L2
// against FEM data a training run is judged by (pointsets.relative_l2), without downloading the fields.
//   sums    for each compared row j:  sum_i (pred[rows[j]][i] - ref[j][i])^2  and  sum_i ref[j][i]^2,  differences and squares in fp64
//   order   two launches, the scheme of pinn_refine_keys' mean (pinn_sample.hpp): per-workgroup fp64 partials over CONTIGUOUS index ranges in a
//           fixed order, then one workgroup adds the partials in a fixed order -- no floating-point atomics, so the sums are a function of the
//           arguments alone
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "pinn_sample.hpp"

namespace pinn {
namespace validate {

constexpr int THREADS = sample::THREADS;
constexpr int MAX_BLOCKS = 1024;                       // workgroups of the partial launch = index ranges
constexpr int MAX_ROWS = 16;

struct ErrArgs {
    const float* pred;         // [pred_rows][n]
    const float* ref;          // [n_rows][n]
    uint32_t n;                // < 2^31
    uint32_t chunk;            // indices per workgroup (a multiple of THREADS)
    int n_rows;
    int rows[MAX_ROWS];        // row of `pred` compared with row j of `ref`
    int nblocks;               // workgroups of the partial launch
    double* partials;          // [nblocks][2][n_rows]
    double* sums_out;          // [2][n_rows]
};

inline size_t ws_bytes(int n_rows) { return (size_t)MAX_BLOCKS * 2 * n_rows * sizeof(double); }

template <int UNUSED = 0>
__global__ __launch_bounds__(THREADS) void partial_kernel(const ErrArgs a) {
    __shared__ double wsum[4];
    uint32_t lo, hi;
    reduce::range_of(a.chunk, a.n, lo, hi);
    for (int j = 0; j < a.n_rows; ++j) {
        const float* p = a.pred + (size_t)a.rows[j] * a.n;
        const float* r = a.ref + (size_t)j * a.n;
        double d2 = 0.0, r2 = 0.0;
        for (uint32_t i = lo + threadIdx.x; i < hi; i += THREADS) {
            const double rv = (double)r[i], d = (double)p[i] - rv;
            d2 += d * d;
            r2 += rv * rv;
        }
        d2 = sample::block_sum(d2, wsum);
        r2 = sample::block_sum(r2, wsum);
        if (threadIdx.x == 0) {
            a.partials[((size_t)blockIdx.x * 2 + 0) * a.n_rows + j] = d2;
            a.partials[((size_t)blockIdx.x * 2 + 1) * a.n_rows + j] = r2;
        }
    }
}

// one workgroup: reduce::records_sum for each sum in turn
template <int UNUSED = 0>
__global__ __launch_bounds__(THREADS) void final_kernel(const ErrArgs a) {
    __shared__ double wsum[4];
    for (int k = 0; k < 2 * a.n_rows; ++k) {
        const double s = reduce::records_sum(a.partials, a.nblocks, (size_t)2 * a.n_rows, k, wsum);
        if (threadIdx.x == 0) a.sums_out[k] = s;
    }
}

// enqueue the two launches (arguments already checked, n > 0)
inline int launch(ErrArgs a, void* ws, hipStream_t st) {
    const reduce::Split s = reduce::split_ranges(a.n, THREADS, MAX_BLOCKS);
    const int blocks = s.blocks;
    a.chunk = (uint32_t)s.chunk;
    a.nblocks = blocks;
    a.partials = static_cast<double*>(ws);
    hipLaunchKernelGGL((partial_kernel<0>), dim3(blocks), dim3(THREADS), 0, st, a);
    hipLaunchKernelGGL((final_kernel<0>), dim3(1), dim3(THREADS), 0, st, a);
    return (int)hipGetLastError();
}

}  // namespace validate
}  // namespace pinn
