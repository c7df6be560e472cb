// Causal collocation sampling on the device (pinn_binned_sums, pinn_causal_cdf, pinn_sample_box_cdf of include/pinn_hip.h): what stands between
// a residual-score call and a collocation set whose TIME coordinate is drawn with density ~ w(t) = exp(-eps * accumulated earlier residual)
// (Wang, Sankaran, Perdikaris: "Respecting causality is all you need"), without a host round trip.
//   sums     per time bin: sum of the scores and their count, fp64.  A workgroup owns a CONTIGUOUS index range and walks it in tiles of TILE
//            points staged in LDS as (value, bin) pairs; thread (bin b, quarter q) = (tid & 63, tid >> 6) walks quarter q of every tile in index
//            order and keeps what falls into bin b -- all lanes of a wave read the same LDS address (a broadcast) --, the four quarters are added
//            in the order 0..3, and a final launch adds the per-workgroup records of each output in a fixed order (pinn_validate.hpp's scheme).
//            No floating-point atomics: the sums are a function of the arguments alone
//   table    m_b = sum_b / count_b, c_b = m_0 + .. + m_(b-1), w_b = exp(-eps c_b), d_b = max(w_b, floor), cdf_b = (d_0 + .. + d_(b-1)) / total: fp64,
//            one small launch, the prefix sums serial in ascending order; the fp32 table never decreases
//   draw     pinn_sample_box with the last column drawn from the piecewise-constant density of the table: same Philox block, same words, the
//            space columns bit-identical; the table is read from LDS, the search is at most 6 steps
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "pinn_sample.hpp"

namespace pinn {
namespace causal {

constexpr int THREADS = sample::THREADS;
constexpr int MAX_BINS = 64;                           // PINN_MAX_TIME_BINS: one lane of a wave per bin
constexpr int MAX_BLOCKS = 512;                        // workgroups of the partial launch = index ranges
constexpr int TILE = 1024;                             // points staged per trip: 4 per thread, a quarter per wave
constexpr int QUARTER = TILE / 4;
static_assert(THREADS == 4 * MAX_BINS && TILE % THREADS == 0, "thread (bin, quarter) = (tid & 63, tid >> 6)");

// ---- pinn_binned_sums -----------------------------------------------------------------------------------------------------------------
struct BinArgs {
    const float* value;
    const float* coord;
    uint32_t n;                // < 2^31
    uint32_t chunk;            // indices per workgroup (a multiple of TILE)
    float lo, scale;           // (float)lo, (float)(n_bins / (hi - lo))
    int n_bins;
    int nblocks;               // workgroups of the partial launch
    double* partials;          // [nblocks][2][n_bins]
    double* sums_out;          // [2][n_bins]
};

inline size_t ws_bytes(int n_bins) { return (size_t)MAX_BLOCKS * 2 * n_bins * sizeof(double); }      // (a multiple of 256)

struct Pair {
    float v;
    int b;                     // -1: skipped
};

// the bin of a coordinate, all in fp32 (the clamp in front of the floor: the same integer, and no conversion of a value out of int's range)
__device__ __forceinline__ int bin_of(const BinArgs& a, float c) {
    const float d = c - a.lo;
    const float q = d * a.scale;
    return (int)floorf(fminf(fmaxf(q, 0.f), (float)(a.n_bins - 1)));
}

template <int UNUSED = 0>
__global__ __launch_bounds__(THREADS) void bin_partial_kernel(const BinArgs a) {
    __shared__ Pair tile[TILE];
    __shared__ double qsum[4][MAX_BINS];
    __shared__ uint32_t qcount[4][MAX_BINS];
    const int b = threadIdx.x & 63, q = threadIdx.x >> 6;
    uint32_t lo, hi;
    reduce::range_of(a.chunk, a.n, lo, hi);
    double sum = 0.0;
    uint32_t count = 0;
    for (uint32_t base = lo; base < hi; base += TILE) {                        // (workgroup-uniform trip count)
        __syncthreads();                                                       // the previous tile has been walked
#pragma unroll
        for (int j = 0; j < TILE / THREADS; ++j) {
            const uint32_t s = j * THREADS + threadIdx.x, i = base + s;        // (base + s < 2^31 + TILE: no wrap)
            Pair p{0.f, -1};
            if (i < hi) {
                const float v = a.value[i], c = a.coord[i];
                if (v >= 0.f && v <= 3.402823466e+38f && c == c) p = Pair{v, bin_of(a, c)};
            }
            tile[s] = p;
        }
        __syncthreads();
        const uint32_t left = hi - base;
        const int end = left < (uint32_t)((q + 1) * QUARTER) ? (int)left : (q + 1) * QUARTER;
#pragma unroll 4
        for (int s = q * QUARTER; s < end; ++s) {                              // wave q, every lane the same address
            const Pair p = tile[s];
            if (p.b == b) {
                sum += (double)p.v;
                ++count;
            }
        }
    }
    qsum[q][b] = sum;
    qcount[q][b] = count;
    __syncthreads();
    if (q == 0 && b < a.n_bins) {
        double* out = a.partials + (size_t)blockIdx.x * 2 * a.n_bins;
        out[b] = ((qsum[0][b] + qsum[1][b]) + qsum[2][b]) + qsum[3][b];
        out[a.n_bins + b] = (double)(((qcount[0][b] + qcount[1][b]) + qcount[2][b]) + qcount[3][b]);
    }
}

// one workgroup per output k (2 * n_bins of them): reduce::records_sum -- the final pass of pinn_field_error_sums, spread over the outputs so that
// no thread walks more than MAX_BLOCKS / 256 records
template <int UNUSED = 0>
__global__ __launch_bounds__(THREADS) void bin_final_kernel(const BinArgs a) {
    __shared__ double wsum[4];
    const int k = blockIdx.x, outs = 2 * a.n_bins;
    const double s = reduce::records_sum(a.partials, a.nblocks, outs, k, wsum);
    if (threadIdx.x == 0) a.sums_out[k] = s;
}

// enqueue the two launches (arguments already checked, n > 0)
inline int launch_bins(BinArgs a, void* ws, hipStream_t st) {
    const reduce::Split s = reduce::split_ranges(a.n, TILE, MAX_BLOCKS);
    const int blocks = s.blocks;
    a.chunk = (uint32_t)s.chunk;
    a.nblocks = blocks;
    a.partials = static_cast<double*>(ws);
    hipLaunchKernelGGL((bin_partial_kernel<0>), dim3(blocks), dim3(THREADS), 0, st, a);
    hipLaunchKernelGGL((bin_final_kernel<0>), dim3(2 * a.n_bins), dim3(THREADS), 0, st, a);
    return (int)hipGetLastError();
}

// ---- pinn_causal_cdf ------------------------------------------------------------------------------------------------------------------
struct CdfArgs {
    const double* binned;      // [2][n_bins]
    int n_bins;
    double eps, floor;
    double* w_out;             // [n_bins]
    float* cdf_out;            // [n_bins + 1]
};

template <int UNUSED = 0>
__global__ __launch_bounds__(MAX_BINS) void cdf_kernel(const CdfArgs a) {
    __shared__ double m[MAX_BINS], c[MAX_BINS], d[MAX_BINS];
    const int b = threadIdx.x, B = a.n_bins;
    if (b < B) {
        const double cnt = a.binned[B + b];
        m[b] = cnt > 0.0 ? a.binned[b] / cnt : 0.0;
    }
    __syncthreads();
    if (b == 0) {                                      // c_b = m_0 + .. + m_(b-1), ascending
        double acc = 0.0;
        for (int j = 0; j < B; ++j) {
            c[j] = acc;
            acc += m[j];
        }
    }
    __syncthreads();
    if (b < B) {
        const double w = exp(-a.eps * c[b]);           // (c_0 = 0: w_0 = exp(-0) = 1 exactly)
        a.w_out[b] = w;
        const double fl = a.floor < 1.0 ? a.floor : 1.0;   // w_b <= 1: a floor above 1 gives the equal densities floor = 1 gives, and
        d[b] = w > fl ? w : fl;                            // the sum of 64 densities <= 1 cannot overflow
    }
    __syncthreads();
    if (b == 0) {
        double total = 0.0;
        for (int j = 0; j < B; ++j) total += d[j];     // >= d_0 >= 1
        double acc = 0.0;
        float prev = 0.f;
        a.cdf_out[0] = 0.f;
        for (int j = 1; j < B; ++j) {
            acc += d[j - 1];
            const float v = (float)(acc / total);
            prev = !(v >= prev) ? prev : v;            // the table a sampler reads never decreases (and holds no NaN)
            a.cdf_out[j] = prev;
        }
        a.cdf_out[B] = 1.f;
    }
}

inline int launch_cdf(const CdfArgs& a, hipStream_t st) {
    hipLaunchKernelGGL((cdf_kernel<0>), dim3(1), dim3(MAX_BINS), 0, st, a);
    return (int)hipGetLastError();
}

// ---- pinn_sample_box_cdf --------------------------------------------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(THREADS) void box_cdf_kernel(const sample::BoxArgs a, const float* __restrict__ t_cdf, const int n_bins) {
    __shared__ float cdf[MAX_BINS + 1];
    if ((int)threadIdx.x <= n_bins) cdf[threadIdx.x] = t_cdf[threadIdx.x];
    __syncthreads();
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i < a.n) {
        const sample::Words r = sample::words_of(a.seed, a.stream_id, a.first + i, 0u);
#pragma unroll
        for (int k = 0; k < DIM - 1; ++k) {
            const float u = (float)(r.w[k] >> 8) * 0x1p-24f;
            a.out[k][i] = fminf(__fmaf_rn(u, a.span[k], a.lo[k]), a.hi[k]);
        }
        const float u = (float)(r.w[DIM - 1] >> 8) * 0x1p-24f;
        int b = 0, e = n_bins;                         // the largest b in 0 .. n_bins - 1 with cdf[b] <= u: cdf[b] <= u < cdf[e] throughout
        while (e - b > 1) {
            const int mid = (b + e) >> 1;
            if (cdf[mid] <= u) b = mid;
            else e = mid;
        }
        const float f = fminf((u - cdf[b]) / (cdf[b + 1] - cdf[b]), 1.f);
        const float s = ((float)b + f) / (float)n_bins;
        a.out[DIM - 1][i] = fminf(__fmaf_rn(s, a.span[DIM - 1], a.lo[DIM - 1]), a.hi[DIM - 1]);
    }
}

// enqueue the draw (arguments already checked, n > 0; `a` filled as for sample::box_kernel)
inline int launch_box_cdf(const sample::BoxArgs& a, const float* t_cdf, int n_bins, hipStream_t st) {
    const uint32_t blocks = (a.n + THREADS - 1) / THREADS;
    if (a.dim == 3) hipLaunchKernelGGL((box_cdf_kernel<3>), dim3(blocks), dim3(THREADS), 0, st, a, t_cdf, n_bins);
    else hipLaunchKernelGGL((box_cdf_kernel<4>), dim3(blocks), dim3(THREADS), 0, st, a, t_cdf, n_bins);
    return (int)hipGetLastError();
}

}  // namespace causal
}  // namespace pinn
