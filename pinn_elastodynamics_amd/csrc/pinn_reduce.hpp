// The summation schemes of the library, one definition each.  Every loss sum and gradient is a function of the arguments alone: fixed order, no
// floating-point atomics -- and "the same bits as the separate calls" for the step launch -- hold because every kernel that adds something up
// calls the code below.  The 16-lane trees of chain_kernel, fp32_sum_kernel, the L-BFGS kernels and material::final_kernel (NSUMS sums side by
// side) are written out where they stand.
//   epilogue    weights_poison, column_sum / column_total, loss_term_sum, adam_tf1: the bodies of pinn_device.hpp's reduce_* kernels
//   ranges      split_ranges (host) and range_of (device): [0, n) in contiguous per-workgroup ranges of whole tiles
//   workgroup   block_sum, records_sum: 256 threads, the final passes over per-workgroup records
// LDS a helper needs is declared by the kernel and passed in: a __shared__ inside a shared inline function would be ONE object for all kernels
// under the host emulator (tools/emu defines __shared__ as static).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace pinn {
namespace reduce {

constexpr int THREADS = 256;                           // the workgroup of every kernel that calls into this header

// ---- epilogue of the loss-and-gradient calls (256 threads) -------------------------------------------------------------------------------------
// Weights outside the fused format's range (repack_kernel's flags): the launch computed with infinities.  Its results are replaced by NaN as a
// whole -- gradient and sums -- so that the condition is unmistakable (include/pinn_hip.h, PINN_FLAG_TWO_KERNEL).  Returns 0.0f or NaN, the
// same in every thread; all of them call it.
struct Flags {
    const int* flags;          // one per repack block
    int n;                     // 0: nothing to scan (the formats without a range)
};
__device__ __forceinline__ float weights_poison(const int* wflags, int nflags, int* lds_flag) {
    if (threadIdx.x == 0) *lds_flag = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < nflags; i += THREADS)
        if (wflags[i]) *lds_flag = 1;
    __syncthreads();
    return *lds_flag ? __builtin_nanf("") : 0.0f;
}

// Gradient column sum: sum_c partial[c][p] for the workgroup's 64 parameters p = 64 blockIdx.x + (tid & 63).  Its 4 waves each sum every 4th
// partial with four independent accumulators (the loop is latency-bound otherwise) and leave (s0 + s1) + (s2 + s3) in sub[wave]; behind a
// __syncthreads() column_total combines the four sub-sums in a fixed order.
__device__ __forceinline__ void column_sum(const float* partial, int nchunks, int nparams, float (*sub)[64]) {
    const int pl = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const long p = (long)blockIdx.x * 64 + pl;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    if (p < nparams) {
        int cidx = sl;
        for (; cidx + 12 < nchunks; cidx += 16) {
            s0 += partial[(long)cidx * nparams + p];
            s1 += partial[(long)(cidx + 4) * nparams + p];
            s2 += partial[(long)(cidx + 8) * nparams + p];
            s3 += partial[(long)(cidx + 12) * nparams + p];
        }
        for (; cidx < nchunks; cidx += 4) s0 += partial[(long)cidx * nparams + p];
    }
    sub[sl][pl] = (s0 + s1) + (s2 + s3);
}
__device__ __forceinline__ float column_total(const float (*sub)[64]) {
    const int pl = threadIdx.x & 63;
    return (sub[0][pl] + sub[1][pl]) + (sub[2][pl] + sub[3][pl]);
}

// Loss-term sum: sum over the waves w of lp[(w * slots + slot) * width + term].  32 lanes per term (lane tid & 31 walks the waves lane, lane + 32,
// ... in fp64), one cast to float, five xor steps; every lane of the 32 returns the total (0 for term >= nterms).
__device__ __forceinline__ float loss_term_sum(const float* lp, long nwaves, int slots, int slot, int width, int term, int nterms) {
    double s = 0.0;
    if (term < nterms)
        for (long w = threadIdx.x & 31; w < nwaves; w += 32) s += (double)lp[(w * slots + slot) * width + term];
    float v = (float)s;
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 8);
    v += __shfl_xor(v, 16);
    return v;
}

// tf.train.AdamOptimizer (TF1 rule; INF:131-133) on parameter i with gradient g: epsilon added to the UNCORRECTED sqrt(v); the bias
// correction lives in lr_t = lr * sqrt(1-beta2^t)/(1-beta1^t), computed by the caller in double.
__device__ __forceinline__ void adam_tf1(float* theta, float* m, float* v, long i, float g, float lr_t, float beta1, float beta2, float eps) {
    const float mi = beta1 * m[i] + (1.0f - beta1) * g;
    const float vi = beta2 * v[i] + (1.0f - beta2) * g * g;
    m[i] = mi;
    v[i] = vi;
    theta[i] -= lr_t * mi / (__builtin_amdgcn_sqrtf(vi) + eps);
}

// ---- contiguous per-workgroup index ranges ---------------------------------------------------------------------------------------------------------
// [0, n) over `blocks` workgroups, each a contiguous range of `chunk` indices, a multiple of `tile`: as few tiles per workgroup as max_blocks
// allows (one, up to n = max_blocks * tile).  tests/_grid_cap_cases.py::ranges is the same rule.
struct Split {
    int blocks;
    uint64_t chunk;
};
inline Split split_ranges(uint64_t n, int tile, int max_blocks) {
    const uint64_t tiles = (n + tile - 1) / tile;
    const int blocks = (int)(tiles < (uint64_t)max_blocks ? (tiles ? tiles : 1) : max_blocks);
    const uint64_t per = (n + blocks - 1) / blocks;
    return Split{blocks, (per + tile - 1) / tile * tile};
}

// the range [lo, hi) of this workgroup, clamped to n
template <class T>
__device__ __forceinline__ void range_of(uint64_t chunk, T n, T& lo, T& hi) {
    const uint64_t l = (uint64_t)blockIdx.x * chunk, h = l + chunk;
    lo = l < (uint64_t)n ? (T)l : n;
    hi = h < (uint64_t)n ? (T)h : n;
}

// ---- sums over the workgroup ---------------------------------------------------------------------------------------------------------------------
// sum over the 256 threads of the workgroup in a fixed order (all of them call it, all get the total); `wsum` is 4 words of LDS
template <class T>
__device__ __forceinline__ T block_sum(T v, T* wsum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
    __syncthreads();           // (wsum may still be read from the previous use)
    if (lane == 0) wsum[wave] = v;
    __syncthreads();
    return ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// the final pass over per-workgroup records: sum_r partials[r * stride + k], thread t adds the records t, t + 256, ... in that order, then the fixed
// tree of block_sum (all threads call it, all get the total)
template <class T>
__device__ __forceinline__ T records_sum(const T* partials, int nrecords, size_t stride, int k, T* wsum) {
    T s = 0;
    for (int r = threadIdx.x; r < nrecords; r += THREADS) s += partials[(size_t)r * stride + k];
    return block_sum(s, wsum);
}

}  // namespace reduce
}  // namespace pinn
