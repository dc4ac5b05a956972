// kr_mla_dev.h -- device pieces of the exact MLA arithmetic shared by the decode step / prompt pass (kr_mla.hip) and the multi-sequence step
// (kr_multi.hip): cache element codecs, the two-accumulator dot product, and the three sections of the prep launch (w_kc absorption tile,
// rope of q_pe, latent RMSNorm + rope of k_pe + cache append).  One definition, so every caller carries the same operations in the same order.
#pragma once
#include "kr_device.h"
#include "kr_exact_dev.h"
#include <hip/hip_fp16.h>

__device__ __forceinline__ float kr_h2f(uint16_t h) { return __half2float(__ushort_as_half(h)); }
// cache element i of a row / of the whole cache: FP16 (reference CPU decode) or E4M3 (the GPU cache dtype, extended to the latent cache)
template <bool FP8> __device__ __forceinline__ float kr_mla_ld(const void* base, size_t i) {
    if (FP8) return kr_e4m3_to_f32(reinterpret_cast<const uint8_t*>(base)[i]);
    return kr_h2f(reinterpret_cast<const uint16_t*>(base)[i]);
}
template <bool FP8> __device__ __forceinline__ float kr_stage_val(const unsigned char* row, int i) {   // element i of a staged (LDS) row
    if (FP8) return kr_e4m3_to_f32(row[i]);
    _Float16 hv; __builtin_memcpy(&hv, row + 2 * i, 2);
    return (float)hv;
}
template <bool FP8> __device__ __forceinline__ void kr_mla_st(void* base, size_t i, float v) {
    if (FP8) reinterpret_cast<uint8_t*>(base)[i] = kr_f32_to_e4m3(v);
    else reinterpret_cast<uint16_t*>(base)[i] = __half_as_ushort(__float2half_rn(v));
}

// end of a two-accumulator dot product on 16 lanes: lane (a, l) holds AVX lane l of accumulator a; _mm256_add_ps(acc0, acc1) with acc0 as the left
// operand on both halves, then the hsum.  Every lane of the 16 returns the result.
__device__ __forceinline__ float kr_mla_pair_hsum(float acc, int a) {
    const float other = __shfl_xor(acc, 8);
    return kr_hsum8(a == 0 ? acc + other : other + acc);
}
// 16 cooperating lanes (c = lane & 15) evaluate mla_attn_dot_fp16_avx2 / the w_vc row dot: chain (a = c >> 3, l = c & 7) owns the
// 8-blocks i with i % 2 == a (an odd trailing block goes to accumulator 0), ascending.  Every lane of the 16 returns the result.
template <typename LoadB>
__device__ __forceinline__ float kr_dot2acc(const float* q, LoadB loadb, int dim, int c) {
    const int n8 = dim >> 3, a = c >> 3, l = c & 7, paired = (n8 >> 1) << 1;
    float acc = 0.0f;
    for (int i = a; i < paired; i += 2) acc = __builtin_fmaf(q[i * 8 + l], loadb(i * 8 + l), acc);
    if ((n8 & 1) && a == 0) acc = __builtin_fmaf(q[(n8 - 1) * 8 + l], loadb((n8 - 1) * 8 + l), acc);
    return kr_mla_pair_hsum(acc, a);
}

// ---- the sections of the prep launch, each for a workgroup of 64 threads (t = threadIdx.x) ---------------------------------------------
// w_kc absorption, one tile: q_abs_h[j] = fma(q_nope[i], w_kc_h[i][j], .) for i ascending (mla_absorb_wkc_avx2); thread t owns output j.
// sh: nd floats of LDS.
__device__ __forceinline__ void kr_mla_absorb_tile(const float* qh, const float* w_kc_h, float* q_abs_h, int j, int nd, int klr, float* sh) {
    const int t = threadIdx.x;
    for (int i = t; i < nd; i += 64) sh[i] = qh[i];
    __syncthreads();
    const float* w = w_kc_h + j;
    float o = 0.0f;
    int i = 0;
    for (; i + 16 <= nd; i += 16) {
        float wv[16];
#pragma unroll
        for (int u = 0; u < 16; u++) wv[u] = __builtin_nontemporal_load(w + (size_t)(i + u) * klr);
#pragma unroll
        for (int u = 0; u < 16; u++) o = __builtin_fmaf(sh[i + u], wv[u], o);
    }
    for (; i < nd; i++) o = __builtin_fmaf(sh[i], w[(size_t)i * klr], o);
    q_abs_h[j] = o;
}
// de-interleave + rope of one head's q_pe at `pos` (decode.rs:3113-3128); threads t < half work
__device__ __forceinline__ void kr_mla_rope_qpe(const float* qh, float* q_pe_h, const float* rope_cos, const float* rope_sin, int pos, int nd, int half) {
    const int t = threadIdx.x;
    if (t < half) {
        const float x1 = qh[nd + 2 * t], x2 = qh[nd + 2 * t + 1];
        const float c = rope_cos[(size_t)pos * half + t], s = rope_sin[(size_t)pos * half + t];
        q_pe_h[t] = x1 * c - x2 * s;
        q_pe_h[half + t] = x2 * c + x1 * s;
    }
}
// compressed KV of one token: RMSNorm (decode.rs:3025-3030: scalar sequential sum, mul and add separate, x * (rms * w)), k_pe de-interleave +
// rope (decode.rs:3098-3107, 3131-3140), both rows stored at `pos` of the caches.  sh: 640 floats of LDS (klr <= 576 values, sh[639] = rms).
template <bool FP8>
__device__ __forceinline__ void kr_mla_append_row(const float* kv_out, const float* kv_a_norm, const float* rope_cos, const float* rope_sin, void* ckv_cache,
                                                  void* kpe_cache, int pos, int klr, int rd, float eps, float* sh, int at = -1) {
    const int wr = at < 0 ? pos : at;      // the row of the caches it lands in: `pos`, or (paged slots) the position inside the page the caches point at
    const int t = threadIdx.x, half = rd / 2;
    float* x = sh;
    for (int i = t; i < klr; i += 64) x[i] = kv_out[i];
    __syncthreads();
    if (t == 0) {
        float ss = 0.0f; int i = 0;
        for (; i + 8 <= klr; i += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) { v[u] = x[i + u]; v[u] = v[u] * v[u]; }
#pragma unroll
            for (int u = 0; u < 8; u++) ss += v[u];
        }
        for (; i < klr; i++) ss += x[i] * x[i];
        sh[639] = kr_rms_inv(ss, klr, eps);
    }
    __syncthreads();
    const float rms = sh[639];
    for (int i = t; i < klr; i += 64) {
        const float v = x[i] * (rms * kv_a_norm[i]);                                     // x *= rms * w (decode.rs:3030)
        kr_mla_st<FP8>(ckv_cache, (size_t)wr * klr + i, v);
    }
    if (t < half) {
        const float x1 = kv_out[klr + 2 * t], x2 = kv_out[klr + 2 * t + 1];
        const float c = rope_cos[(size_t)pos * half + t], s = rope_sin[(size_t)pos * half + t];
        kr_mla_st<FP8>(kpe_cache, (size_t)wr * rd + t, x1 * c - x2 * s);
        kr_mla_st<FP8>(kpe_cache, (size_t)wr * rd + half + t, x2 * c + x1 * s);
    }
}
