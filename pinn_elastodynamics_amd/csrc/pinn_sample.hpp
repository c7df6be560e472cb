// Candidate points and selection keys on the device (pinn_sample_box, pinn_refine_keys of include/pinn_hip.h): what residual-adaptive
// refinement needs in front of the score call and between it and pinn_select_k, without a host round trip.
//   generator  Philox4x32-10, counter-based: element idx = first + i reads the block  counter = (lo32 idx, hi32 idx, stream_id, purpose),
//              key = (lo32 seed, hi32 seed);  purpose 0: coordinates (word k -> coordinate k in the order x, y, (z), t), purpose 1: the
//              sampling noise (word 0).  No state: a value is a function of (seed, stream_id, idx) alone, whatever the grid or the call's window
//   box        u = (r >> 8) 2^-24 in [0, 1);  value = min(fma(u, hi - lo, lo), hi), ONE explicit fma, so the bits do not hang on contraction
//   keys       MASK: key = score, -inf inside an excluded ball.  SAMPLE: key = log p + Gumbel noise with p = q / mean(q) + c, q = score^power;
//              the k largest keys are then a weighted sample without replacement, P ~ p (Efraimidis-Spirakis / Gumbel top-k).  The mean
//              is two launches: per-workgroup fp64 partials over CONTIGUOUS index ranges in a fixed order, then every workgroup of the key
//              launch re-adds the partials in the same fixed order -- no floating-point atomics, so the keys are a function of the inputs alone
// Exclusion is a mask on the keys, not rejection sampling: no loop, no fallback case, and index i stays the same point under every ball list.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "pinn_reduce.hpp"

namespace pinn {
namespace sample {

using reduce::block_sum;                               // (pinn_reduce.hpp: the fixed-order sum over the workgroup)

constexpr int THREADS = 256;
constexpr int MAX_BLOCKS = 1024;                       // workgroups of the key launches; index ranges of the partial sums
constexpr int MAX_BALLS = 4;                           // PINN_MAX_BALLS

struct Partial {                                       // one per workgroup of the mean launch
    double sum;                                        // of q over the valid points of its range
    uint64_t count;                                    // of those points
};
constexpr size_t WS_BYTES = (size_t)MAX_BLOCKS * sizeof(Partial);
static_assert(sizeof(Partial) == 16 && offsetof(Partial, count) == 8, "sample_kernel walks the records as two interleaved 8-byte columns");
static_assert(THREADS == reduce::THREADS, "block_sum, records_sum: one workgroup size");

struct Words { uint32_t w[4]; };

__device__ __forceinline__ Words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;                             // (the bump behind the last round is dead code)
        k1 += 0xBB67AE85u;
    }
    return Words{{c0, c1, c2, c3}};
}

__device__ __forceinline__ Words words_of(uint64_t seed, uint32_t stream_id, uint64_t idx, uint32_t purpose) {
    return philox4x32_10((uint32_t)idx, (uint32_t)(idx >> 32), stream_id, purpose, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// ---- pinn_sample_box ------------------------------------------------------------------------------------------------------------------
struct BoxArgs {
    uint64_t seed, first;
    uint32_t stream_id;
    uint32_t n;                // < 2^31
    int dim;                   // 3 | 4
    float lo[4], span[4], hi[4];
    float* out[4];             // the dim columns in the order x, y, (z), t
};

template <int DIM>
__global__ __launch_bounds__(THREADS) void box_kernel(const BoxArgs a) {
    const uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= a.n) return;
    const Words r = words_of(a.seed, a.stream_id, a.first + i, 0u);
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
        const float u = (float)(r.w[k] >> 8) * 0x1p-24f;
        a.out[k][i] = fminf(__fmaf_rn(u, a.span[k], a.lo[k]), a.hi[k]);
    }
}

// the arguments of a box draw (pinn_causal.hpp draws with them too)
inline BoxArgs box_args(uint64_t seed, uint32_t stream_id, uint64_t first, uint32_t n, int dim, const double* lo, const double* hi,
                        float* const* cols) {
    BoxArgs a;
    a.seed = seed;
    a.first = first;
    a.stream_id = stream_id;
    a.n = n;
    a.dim = dim;
    for (int k = 0; k < 4; ++k) {
        const bool on = k < dim;
        a.lo[k] = on ? (float)lo[k] : 0.f;
        a.span[k] = on ? (float)(hi[k] - lo[k]) : 0.f;
        a.hi[k] = on ? (float)hi[k] : 0.f;
        a.out[k] = on ? cols[k] : nullptr;
    }
    return a;
}

inline int launch_box(uint64_t seed, uint32_t stream_id, uint64_t first, uint32_t n, int dim, const double* lo, const double* hi,
                      float* const* cols, hipStream_t st) {
    const BoxArgs a = box_args(seed, stream_id, first, n, dim, lo, hi, cols);
    const uint32_t blocks = (n + THREADS - 1) / THREADS;
    if (dim == 3) hipLaunchKernelGGL((box_kernel<3>), dim3(blocks), dim3(THREADS), 0, st, a);
    else hipLaunchKernelGGL((box_kernel<4>), dim3(blocks), dim3(THREADS), 0, st, a);
    return (int)hipGetLastError();
}

// ---- pinn_refine_keys -----------------------------------------------------------------------------------------------------------------
struct Ball {
    float c[3];
    float r2;
    int ndim;                  // 2: disc in (x, y), 3: ball in (x, y, z)
    int closed;                // 1: the boundary is excluded too (d2 <= r2), 0: d2 < r2
};

enum { POW_ONE = 0, POW_SQRT = 1, POW_GENERAL = 2 };

struct KeyArgs {
    const float* score;
    const float* x;
    const float* y;
    const float* z;            // may be null when no ball has ndim == 3
    uint32_t n;                // < 2^31
    uint32_t chunk;            // indices per workgroup (a multiple of THREADS)
    int n_balls;
    Ball balls[MAX_BALLS];
    int pow_kind;
    float power, c;
    uint64_t seed, first;
    uint32_t stream_id;
    Partial* partials;         // [gridDim.x]
    float* key_out;
};

__device__ __forceinline__ bool in_a_ball(const KeyArgs& a, uint32_t i) {
    if (a.n_balls == 0) return false;                  // (the columns may be null then)
    const float xi = a.x[i], yi = a.y[i], zi = a.z ? a.z[i] : 0.f;
    bool in = false;
    for (int b = 0; b < a.n_balls; ++b) {
        const Ball& B = a.balls[b];
        const float dx = xi - B.c[0], dy = yi - B.c[1];
        float d2 = __fmaf_rn(dy, dy, dx * dx);
        if (B.ndim == 3) {
            const float dz = zi - B.c[2];
            d2 = __fmaf_rn(dz, dz, d2);
        }
        in = in || (B.closed ? d2 <= B.r2 : d2 < B.r2);
    }
    return in;
}

// valid for sampling: outside every ball, score finite and not negative
__device__ __forceinline__ bool samplable(const KeyArgs& a, uint32_t i, float s) {
    return s >= 0.f && s <= 3.402823466e+38f && !in_a_ball(a, i);
}

__device__ __forceinline__ float q_of(const KeyArgs& a, float s) {
    return a.pow_kind == POW_ONE ? s : (a.pow_kind == POW_SQRT ? sqrtf(s) : powf(s, a.power));
}

template <int UNUSED = 0>
__global__ __launch_bounds__(THREADS) void mask_kernel(const KeyArgs a) {
    const uint32_t stride = gridDim.x * THREADS;
    for (uint32_t i = blockIdx.x * THREADS + threadIdx.x; i < a.n; i += stride)
        a.key_out[i] = in_a_ball(a, i) ? -__builtin_inff() : a.score[i];
}

template <int UNUSED = 0>
__global__ __launch_bounds__(THREADS) void mean_kernel(const KeyArgs a) {
    __shared__ double dsum[4];
    __shared__ uint32_t csum[4];
    uint32_t lo, hi;
    reduce::range_of(a.chunk, a.n, lo, hi);
    double sum = 0.0;
    uint32_t count = 0;
    for (uint32_t i = lo + threadIdx.x; i < hi; i += THREADS) {
        const float s = a.score[i];
        if (samplable(a, i, s)) {
            sum += (double)q_of(a, s);
            ++count;
        }
    }
    sum = block_sum(sum, dsum);
    count = block_sum(count, csum);
    if (threadIdx.x == 0) {
        a.partials[blockIdx.x].sum = sum;
        a.partials[blockIdx.x].count = count;
    }
}

template <int UNUSED = 0>
__global__ __launch_bounds__(THREADS) void sample_kernel(const KeyArgs a) {
    __shared__ double dsum[4];
    __shared__ uint64_t csum[4];
    // the mean, re-derived by every workgroup from the records (sum, count) of the mean launch: reduce::records_sum
    const double sum = reduce::records_sum(&a.partials[0].sum, (int)gridDim.x, 2, 0, dsum);
    const uint64_t count = reduce::records_sum(&a.partials[0].count, (int)gridDim.x, 2, 0, csum);
    const float m = count ? (float)(sum / (double)count) : 0.f;
    uint32_t lo, hi;
    reduce::range_of(a.chunk, a.n, lo, hi);
    for (uint32_t i = lo + threadIdx.x; i < hi; i += THREADS) {
        const float s = a.score[i];
        float key = -__builtin_inff();
        if (samplable(a, i, s)) {
            const float p = (m != 0.f ? q_of(a, s) / m : 0.f) + a.c;
            if (p > 0.f) {                             // (p == 0 -- and a NaN from an overflown power -- never wins)
                const uint32_t r0 = words_of(a.seed, a.stream_id, a.first + i, 1u).w[0];
                const float u = ((float)(r0 >> 9) + 0.5f) * 0x1p-23f;          // in (0, 1), exact
                key = logf(p) - logf(-logf(u));
            }
        }
        a.key_out[i] = key;
    }
}

// enqueue the key launches (arguments already checked; `a` filled but for the geometry and the workspace)
inline int launch_keys(KeyArgs a, bool sampling, void* ws, hipStream_t st) {
    const reduce::Split s = reduce::split_ranges(a.n, THREADS, MAX_BLOCKS);
    const int blocks = s.blocks;
    a.chunk = (uint32_t)s.chunk;
    a.partials = static_cast<Partial*>(ws);
    if (!sampling) {
        hipLaunchKernelGGL((mask_kernel<0>), dim3(blocks), dim3(THREADS), 0, st, a);
    } else {
        hipLaunchKernelGGL((mean_kernel<0>), dim3(blocks), dim3(THREADS), 0, st, a);
        hipLaunchKernelGGL((sample_kernel<0>), dim3(blocks), dim3(THREADS), 0, st, a);
    }
    return (int)hipGetLastError();
}

}  // namespace sample
}  // namespace pinn
