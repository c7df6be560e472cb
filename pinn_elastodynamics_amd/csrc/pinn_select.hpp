// Deterministic top-k / bottom-k selection on the device (pinn_select_k of include/pinn_hip.h): which k of n scores are the largest (or the
// smallest), ties to the lowest index, the answer written as ascending indices.  What residual-adaptive refinement needs between a score
// call and the row update, without a host round trip.
//   keys       float -> uint32 by the sign-flip map (monotone in the float order; a positive NaN sorts above +inf); bottom-k complements the
//              key, so every kernel below selects the LARGEST keys
//   hist x 4   8-bit radix select from the top byte down: per-workgroup LDS histogram of the elements that match the digits found so far,
//              added into a global 256-bin histogram with integer atomics.  The pick of a digit (which bin holds the k-th key) is not a launch
//              of its own: every workgroup of the NEXT launch redoes it from the finished histograms (256 integers, one scan) -- nothing is
//              written, so nothing races, and the call is memset + 6 launches
//   count      per-workgroup numbers of keys above the threshold and equal to it; a workgroup owns a CONTIGUOUS index range
//   write      exclusive sums of those counts over the workgroups in front, then a stable compaction: an element above the threshold goes out
//              always, one equal to it while fewer than `need` equals precede it (need = k - #above); its slot is #above in front + min(#equal
//              in front, need), which is ascending in the index
// Integer atomics only: the result is a function of the inputs alone.  No host synchronisation, no assumption on n.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "pinn_reduce.hpp"

namespace pinn {
namespace select {

constexpr int THREADS = 256;
constexpr int MAX_BLOCKS = 1024;                       // workgroups of every pass; index ranges of the count / write passes
constexpr size_t HIST_BYTES = 4 * 256 * sizeof(uint32_t);
constexpr size_t COUNT_BYTES = (size_t)MAX_BLOCKS * 2 * sizeof(uint32_t);
constexpr size_t WS_BYTES = HIST_BYTES + COUNT_BYTES;

struct Args {
    const float* score;
    uint32_t n;                // < 2^31
    uint32_t k;                // 1 .. n
    uint32_t flip;             // 0: largest, 0xffffffff: smallest (the key is complemented)
    uint32_t chunk;            // indices per workgroup of the count / write passes (a multiple of THREADS)
    uint32_t* hist;            // [4][256], zero before the first pass
    uint32_t* counts;          // [gridDim.x][2]: keys above / equal to the threshold in the workgroup's range
    int32_t* idx_out;          // [k]
};

__device__ __forceinline__ uint32_t key_of(float v, uint32_t flip) {
    const uint32_t u = __builtin_bit_cast(uint32_t, v);
    const uint32_t key = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return key ^ flip;
}

// inclusive sum over the 256 threads of the workgroup (all of them call it); `wsum` is 4 words of LDS
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* wsum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl(v, (lane - d) & 63);
        if (lane >= d) v += t;
    }
    __syncthreads();           // (wsum may still be read from the previous use)
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    for (int w = 0; w < wave; ++w) v += wsum[w];
    return v;
}

// The digits fixed by the first `passes` histograms: returns the key prefix (passes * 8 bits, right-aligned) and leaves in `need` how many of
// the keys that carry this prefix are wanted (k minus the keys above it).  Every thread of the workgroup calls it and gets the same answer.
__device__ __forceinline__ uint32_t picked_prefix(const uint32_t* hist, int passes, uint32_t k, uint32_t& need) {
    __shared__ uint32_t wsum[4];
    __shared__ uint32_t sel[2];
    uint32_t prefix = 0;
    need = k;
    for (int p = 0; p < passes; ++p) {
        const uint32_t bin = 255u - threadIdx.x;                   // thread j looks at the j-th largest digit
        const uint32_t h = hist[p * 256 + bin];
        const uint32_t incl = block_scan(h, wsum);
        if (incl - h < need && need <= incl) {                     // exactly one thread: the bin that holds the need-th key
            sel[0] = bin;
            sel[1] = need - (incl - h);
        }
        __syncthreads();
        prefix = (prefix << 8) | sel[0];
        need = sel[1];
        __syncthreads();
    }
    return prefix;
}

// radix pass PASS (0: top byte): histogram of digit PASS over the keys whose higher digits equal the prefix picked so far
template <int PASS>
__global__ __launch_bounds__(THREADS) void hist_kernel(const Args a) {
    __shared__ uint32_t lh[256];
    uint32_t need;
    const uint32_t prefix = picked_prefix(a.hist, PASS, a.k, need);
    lh[threadIdx.x] = 0;
    __syncthreads();
    constexpr int SHIFT = 24 - 8 * PASS;
    const uint32_t stride = gridDim.x * THREADS;
    for (uint32_t i = blockIdx.x * THREADS + threadIdx.x; i < a.n; i += stride) {
        const uint32_t key = key_of(a.score[i], a.flip);
        if (PASS == 0 || (key >> (SHIFT + 8)) == prefix) atomicAdd(&lh[(key >> SHIFT) & 255u], 1u);
    }
    __syncthreads();
    const uint32_t c = lh[threadIdx.x];
    if (c) atomicAdd(&a.hist[PASS * 256 + threadIdx.x], c);
}

template <int UNUSED = 0>
__global__ __launch_bounds__(THREADS) void count_kernel(const Args a) {
    __shared__ uint32_t cnt[2];
    uint32_t need;
    const uint32_t thr = picked_prefix(a.hist, 4, a.k, need);
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
    __syncthreads();
    uint32_t lo, hi;
    reduce::range_of(a.chunk, a.n, lo, hi);
    uint32_t above = 0, equal = 0;
    for (uint64_t i = (uint64_t)lo + threadIdx.x; i < hi; i += THREADS) {
        const uint32_t key = key_of(a.score[i], a.flip);
        above += key > thr;
        equal += key == thr;
    }
    if (above) atomicAdd(&cnt[0], above);
    if (equal) atomicAdd(&cnt[1], equal);
    __syncthreads();
    if (threadIdx.x < 2) a.counts[2 * blockIdx.x + threadIdx.x] = cnt[threadIdx.x];
}

template <int UNUSED = 0>
__global__ __launch_bounds__(THREADS) void write_kernel(const Args a) {
    __shared__ uint32_t wsum[4];
    __shared__ uint32_t front[2];
    uint32_t need;
    const uint32_t thr = picked_prefix(a.hist, 4, a.k, need);
    // keys above / equal in the ranges of the workgroups in front of this one
    if (threadIdx.x < 2) front[threadIdx.x] = 0;
    __syncthreads();
    uint32_t fa = 0, fe = 0;
    for (uint32_t b = threadIdx.x; b < blockIdx.x; b += THREADS) {
        fa += a.counts[2 * b];
        fe += a.counts[2 * b + 1];
    }
    if (fa) atomicAdd(&front[0], fa);
    if (fe) atomicAdd(&front[1], fe);
    __syncthreads();
    uint32_t above0 = front[0], equal0 = front[1];
    uint32_t lo, hi;
    reduce::range_of(a.chunk, a.n, lo, hi);
    // tiles of 256 consecutive indices, in order; the flags travel through one scan: above in the low half-word, equal in the high one
    for (uint64_t base = lo; base < hi; base += THREADS) {
        const uint64_t i = base + threadIdx.x;
        uint32_t flag = 0;
        if (i < hi) {
            const uint32_t key = key_of(a.score[i], a.flip);
            flag = key > thr ? 1u : (key == thr ? 0x10000u : 0u);
        }
        const uint32_t incl = block_scan(flag, wsum);
        const uint32_t excl = incl - flag;
        const uint32_t a_before = above0 + (excl & 0xffffu), e_before = equal0 + (excl >> 16);
        if (flag == 1u || (flag != 0u && e_before < need)) {
            const uint32_t pos = a_before + (e_before < need ? e_before : need);
            if (pos < a.k) a.idx_out[pos] = (int32_t)i;
        }
        // the tile's totals: the last thread's inclusive sum, by way of the scan's own LDS words
        __syncthreads();
        if (threadIdx.x == THREADS - 1) wsum[0] = incl;
        __syncthreads();
        const uint32_t tot = wsum[0];
        above0 += tot & 0xffffu;
        equal0 += tot >> 16;
    }
}

// enqueue the selection (arguments already checked: 1 <= k <= n < 2^31, ws 256-byte aligned and >= WS_BYTES)
inline int launch(const float* score, uint32_t n, uint32_t k, bool largest, int32_t* idx_out, void* ws, hipStream_t st) {
    Args a;
    a.score = score;
    a.n = n;
    a.k = k;
    a.flip = largest ? 0u : 0xffffffffu;
    a.hist = static_cast<uint32_t*>(ws);
    a.counts = reinterpret_cast<uint32_t*>(static_cast<char*>(ws) + HIST_BYTES);
    a.idx_out = idx_out;
    const reduce::Split s = reduce::split_ranges(n, THREADS, MAX_BLOCKS);
    const int blocks = s.blocks;
    a.chunk = (uint32_t)s.chunk;
    int rc = (int)hipMemsetAsync(a.hist, 0, HIST_BYTES, st);
    if (rc) return rc;
    hipLaunchKernelGGL((hist_kernel<0>), dim3(blocks), dim3(THREADS), 0, st, a);
    hipLaunchKernelGGL((hist_kernel<1>), dim3(blocks), dim3(THREADS), 0, st, a);
    hipLaunchKernelGGL((hist_kernel<2>), dim3(blocks), dim3(THREADS), 0, st, a);
    hipLaunchKernelGGL((hist_kernel<3>), dim3(blocks), dim3(THREADS), 0, st, a);
    hipLaunchKernelGGL((count_kernel<0>), dim3(blocks), dim3(THREADS), 0, st, a);
    hipLaunchKernelGGL((write_kernel<0>), dim3(blocks), dim3(THREADS), 0, st, a);
    return (int)hipGetLastError();
}

}  // namespace select
}  // namespace pinn
