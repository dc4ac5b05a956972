// kr_sample_dev.h -- device helpers shared by the single-row sampler (kr_sampler.hip), the multi-sequence argmax (kr_multi.hip) and the batched
// sampler (kr_multi_sample.hip).  Device code only: included by .hip translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// the sampler's unique 64-bit sort key of token i with scaled logit v: monotone float -> uint in the high word (-0 == +0, as partial_cmp), ~i in
// the low word, so descending key order = value descending, equal values by ascending id
__device__ __forceinline__ uint64_t kr_sample_key(float v, int i) {
    const float o = v == 0.0f ? 0.0f : v;
    uint32_t u = __float_as_uint(o);
    u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;
    return ((uint64_t)u << 32) | (uint32_t)(0xFFFFFFFFu - (uint32_t)i);
}

// first-maximum argmax of row[0 .. V) by one workgroup of 1024 threads (kr_argmax_kernel's rule: (value desc, index asc) is a total order on
// the row's values, so the tree returns the first maximum).  The result is valid in thread 0.
__device__ __forceinline__ int kr_row_argmax_1024(const float* __restrict__ row, int V) {
    __shared__ float bv[16]; __shared__ int bi[16];
    float v = -__builtin_inff(); int idx = 0x7FFFFFFF;
    for (int i = threadIdx.x; i < V; i += 1024) { const float t = row[i]; if (t > v || (t == v && i < idx)) { v = t; idx = i; } }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(v, off); const int oi = __shfl_xor(idx, off);
        if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
    }
    if ((threadIdx.x & 63) == 0) { bv[threadIdx.x >> 6] = v; bi[threadIdx.x >> 6] = idx; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < 16; w++) if (bv[w] > v || (bv[w] == v && bi[w] < idx)) { v = bv[w]; idx = bi[w]; }
    return idx;
}
