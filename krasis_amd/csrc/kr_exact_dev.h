// kr_exact_dev.h -- the formulas of the exact f32 arithmetic, each stated once.  Every exact path (decode step, prompt pass, chunked linear attention,
// the per-slot kernels of the batched decode, verify and commit) carries the bits of the single-sequence decode step by performing the reference's
// operations in the reference's order; a kernel gets that order by calling these functions, never by restating them (docs/design/02-numerics.md).
// Each function names the src/decode.rs lines it restates.
#pragma once
#include "kr_device.h"
#include "kr_libm.h"

// hsum of 8 AVX lanes as 8 consecutive GPU lanes: lo + hi, movehdup, movehl (every hsum of decode.rs, e.g. :1240-1248).  Any aligned group of 8 lanes.
__device__ __forceinline__ float kr_hsum8(float v) {
    v = v + __shfl_xor(v, 4);
    v = v + __shfl_xor(v, 1);
    v = v + __shfl_xor(v, 2);
    return v;
}

// sum of squares of x[0..n) (n % 8 == 0): lane l of an aligned group of 8 owns elements 8 b + l and chains fma over ascending b, then kr_hsum8
// (fused_add_rmsnorm_avx2 decode.rs:1235-1248, l2_normalize_expand_avx2 :3924-3936, gated_rmsnorm_silu_avx2 :4014-4025).  U0, U1: loads (LDS values) in
// flight per lane in the first and second batched loop, 0 = no such loop; they schedule the loads and never change the chain.
template <int U0, int U1>
__device__ __forceinline__ float kr_sumsq8(const float* x, int n, int l) {
    float acc = 0.0f;
    const int nb = n / 8;
    int b = 0;
    if constexpr (U0 > 0) {
        for (; b + U0 <= nb; b += U0) {
            float v[U0];
#pragma unroll
            for (int u = 0; u < U0; u++) v[u] = x[(b + u) * 8 + l];
#pragma unroll
            for (int u = 0; u < U0; u++) acc = __builtin_fmaf(v[u], v[u], acc);
        }
    }
    if constexpr (U1 > 0) {
        for (; b + U1 <= nb; b += U1) {
            float v[U1];
#pragma unroll
            for (int u = 0; u < U1; u++) v[u] = x[(b + u) * 8 + l];
#pragma unroll
            for (int u = 0; u < U1; u++) acc = __builtin_fmaf(v[u], v[u], acc);
        }
    }
    for (; b < nb; b++) { const float v = x[b * 8 + l]; acc = __builtin_fmaf(v, v, acc); }
    return kr_hsum8(acc);
}

// linear-attention gates of one value head (decode.rs:3891-3901): beta = sigmoid(b) and g = -e^{A_log} softplus(a + dt_bias), both through libm's
// expf / logf.  The state decays by e^g (decode.rs:1293): the caller applies kr_expf(g) where it needs it.
__device__ __forceinline__ float kr_la_beta(float b_raw) { return 1.0f / (1.0f + kr_expf(-b_raw)); }
__device__ __forceinline__ float kr_la_g(float a_p, float dt_bias, float a_log) {
    const float ap_dt = a_p + dt_bias;
    const float softplus = ap_dt > 20.0f ? ap_dt : kr_logf(1.0f + kr_expf(ap_dt));
    return -(kr_expf(a_log)) * softplus;
}
// both, in the reference's order: beta is stored before g's operands are read
__device__ __forceinline__ void kr_la_gate(float b_raw, float a_p, float dt_bias, float a_log, float& beta, float& g) {
    beta = kr_la_beta(b_raw);
    g = kr_la_g(a_p, dt_bias, a_log);
}

// conv1d of kernel 4 over the three carried inputs and the new one, then SiLU (decode_la_conv decode.rs:3815-3879: mul and add separate, left to
// right; fast_silu_avx2 :1639)
__device__ __forceinline__ float kr_conv4_silu(float s1, float s2, float s3, float x, const float4& w) {
    const float co = s1 * w.x + s2 * w.y + s3 * w.z + x * w.w;
    return co * kr_sigmoid_poly5(co);
}

// inverse L2 norm of a head's q or k from its sum of squares (decode.rs:3944: zero for a zero row)
__device__ __forceinline__ float kr_l2_inv(float ss) { return ss > 0.0f ? 1.0f / sqrtf(ss) : 0.0f; }
// inverse RMS from a sum of squares over n values (decode.rs:1254, :4028)
__device__ __forceinline__ float kr_rms_inv(float ss, int n, float eps) { return 1.0f / sqrtf(ss / (float)n + eps); }
// output of the head's gated RMSNorm: silu(z) * ((o * rms) * w) (gated_rmsnorm_silu_avx2 decode.rs:4031)
__device__ __forceinline__ float kr_gated_norm_out(float o, float rms, float w, float z) {
    const float normed = (o * rms) * w;
    return (z * kr_sigmoid_poly5(z)) * normed;
}

// maximum over the 64 lanes of a wave, in every lane (a maximum does not depend on the order: shared for brevity)
__device__ __forceinline__ float kr_wave_max(float mx) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    return mx;
}
