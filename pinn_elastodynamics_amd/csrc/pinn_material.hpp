// The second half of pinn_wave2d_material_sums, pinn_plate2d_material_sums and pinn_nc3d_material_sums (include/pinn_hip.h): the per-wave
// records of the material heads (pinn_device.hpp) added up.  The record length NSUMS is a compile-time parameter: 14 (wave), 12 (plate, and
// each half of a PINN_PREC_FP32 pass of the 3-D call) or 24 (3-D).
//   order   the scheme of pinn_field_error_sums (pinn_validate.hpp): fp64 partial records written in a fixed place each, then ONE workgroup adds
//           them in index order -- thread t the records t, t + 256, ..., then the fixed tree of block_sum.  No floating-point atomics, so the
//           sums are a function of the arguments alone.
//   fp32    PINN_PREC_FP32 walks the points in passes: fp32_chain_kernel leaves the per-point terms of a pass in its `fsq` rows,
//           fp32_partial_kernel adds each row over contiguous index ranges in fp64, and the pass's total is added into sums_out in pass order.
//           The 3-D call's 24 terms do not fit the 16 rows: each pass runs in two halves (the twelve squares, then the twelve moments), half h
//           of a pass adds rows 0..11 into sums_out[12 h ..]; sum k thus still gets its passes' totals in pass order.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "pinn_device.hpp"
#include "pinn_sample.hpp"

namespace pinn {
namespace material {

constexpr int THREADS = sample::THREADS;
constexpr int MAX_RECORDS = 2048 * 4;                 // waves of the largest chain grid (Host::MAX_BLOCKS workgroups of 4 waves)
constexpr int FP32_BLOCKS = 1024;                     // index ranges of a PINN_PREC_FP32 pass

inline size_t ws_bytes() { return (size_t)MAX_RECORDS * MATERIAL_SUMS_MAX * sizeof(double); }

// one workgroup: sums_out[k] = (accumulate ? sums_out[k] : 0) + sum_r partials[r][k], records in index order
template <int NSUMS>
__global__ __launch_bounds__(THREADS) void final_kernel(const double* partials, int nrecords, double* sums_out, int accumulate) {
    __shared__ double wsum[4];
    // (the sums of a record side by side: one walk over the records instead of NSUMS -- the walk's latency is most of this launch; which is why
    // this is not NSUMS calls of reduce::records_sum (pinn_reduce.hpp), whose order per sum it keeps)
    double s[NSUMS];
#pragma unroll
    for (int k = 0; k < NSUMS; ++k) s[k] = 0.0;
    for (int r = threadIdx.x; r < nrecords; r += THREADS) {
#pragma unroll
        for (int k = 0; k < NSUMS; ++k) s[k] += partials[(size_t)r * NSUMS + k];
    }
#pragma unroll
    for (int k = 0; k < NSUMS; ++k) {
        const double v = sample::block_sum(s[k], wsum);
        if (threadIdx.x == 0) sums_out[k] = accumulate ? sums_out[k] + v : v;
    }
}

// PINN_PREC_FP32: record b = the fp64 sums of rows 0..NSUMS-1 of `terms` [NSUMS][m] over the indices [b * chunk, (b + 1) * chunk)
template <int NSUMS>
__global__ __launch_bounds__(THREADS) void fp32_partial_kernel(const float* terms, long m, long chunk, double* partials) {
    __shared__ double wsum[4];
    long lo, hi;
    reduce::range_of((uint64_t)chunk, m, lo, hi);
    for (int k = 0; k < NSUMS; ++k) {
        const float* row = terms + (size_t)k * m;
        double s = 0.0;
        for (long i = lo + threadIdx.x; i < hi; i += THREADS) s += (double)row[i];
        s = sample::block_sum(s, wsum);
        if (threadIdx.x == 0) partials[(size_t)blockIdx.x * NSUMS + k] = s;
    }
}

// the records of a chain launch of `nrecords` waves -> sums_out
template <int NSUMS>
inline int launch_final(const double* partials, int nrecords, double* sums_out, int accumulate, hipStream_t st) {
    hipLaunchKernelGGL((final_kernel<NSUMS>), dim3(1), dim3(THREADS), 0, st, partials, nrecords, sums_out, accumulate);
    return (int)hipGetLastError();
}

// one PINN_PREC_FP32 pass of m points: its terms -> records -> added into sums_out (pass > 0) or written (pass 0)
template <int NSUMS>
inline int launch_fp32_pass(const float* terms, long m, double* partials, double* sums_out, int pass, hipStream_t st) {
    const reduce::Split s = reduce::split_ranges((uint64_t)m, THREADS, FP32_BLOCKS);
    hipLaunchKernelGGL((fp32_partial_kernel<NSUMS>), dim3(s.blocks), dim3(THREADS), 0, st, terms, m, (long)s.chunk, partials);
    return launch_final<NSUMS>(partials, s.blocks, sums_out, pass > 0 ? 1 : 0, st);
}

}  // namespace material
}  // namespace pinn
