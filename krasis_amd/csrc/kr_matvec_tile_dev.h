// kr_matvec_tile_dev.h -- the streaming dequant-matvec's prologues and its per-wave tile (reference order, bit-exact), shared by the decode kernels of
// kr_moe_decode.hip and the few-row kernels of kr_rows_matvec.hip (kr_rows_dev.h).  The includer defines KR_BLOCK, the threads of its workgroups: every
// prologue below is run by the whole workgroup.
#pragma once
#include "kr_device.h"
#include "kr_kernels.h"
#include "kr_matvec_dev.h"
#include "kr_libm.h"
#include "kr_exact_dev.h"

#ifndef KR_BLOCK
#error "define KR_BLOCK (threads per workgroup) before including kr_matvec_tile_dev.h"
#endif

// ------------------------------------------------------------------------------------------
// prologues: build the INT16 activation image in LDS (whole workgroup cooperates)
// ------------------------------------------------------------------------------------------

// The first chunk of every prologue below is REQUESTED by a *_load function and consumed by the prologue itself: the kernels call the load before they request their
// weight records.  A wave's memory counter is in-order -- an input chunk requested behind eight weight records is not back before all of them are, and the image
// build then starts one whole weight fetch late (round 5; the arithmetic and its order are untouched).  Every thread loads (clamped index): no lane-masked merges.
struct KrVecPre { float v[8]; };
template <typename T>
__device__ __forceinline__ void kr_vec_load(const T* x, int K, KrVecPre& P) {
    const int nch = K / 8;
    kr_load8(x, (int)threadIdx.x < nch ? (int)threadIdx.x : nch - 1, P.v);
}
// quantize_activation_int16 / _f32 (avx2.rs:234,274): per-128 scale, round half away from zero
template <typename T, bool I8>
__device__ __forceinline__ void kr_prologue_quant(const T* x, int K, const KrActLds& L, const KrVecPre& P) {
    const int nchunks = K / 8;
    for (int c = threadIdx.x; c < nchunks; c += KR_BLOCK) {
        float v[8];
        if (c == (int)threadIdx.x) {
#pragma unroll
            for (int i = 0; i < 8; i++) v[i] = P.v[i];
        } else kr_load8(x, c, v);
        float mx = 0.0f;
#pragma unroll
        for (int i = 0; i < 8; i++) mx = fmaxf(mx, fabsf(v[i]));
        float scale, inv;
        kr_group_scale(mx, scale, inv);
        int q[8];
        kr_quant8<false>(v, inv, q);
        kr_store_chunk<I8>(L, c, q);
        if ((c & 15) == 0) L.ascale[c >> 4] = scale;
    }
}

// decode graph: f32 hidden, optionally rounded to bf16 first (decode.rs:3307-3309 feeds bf16(hidden) to the routed experts)
template <bool I8>
__device__ __forceinline__ void kr_prologue_quant_f32(const float* x, int K, const KrActLds& L, bool round_bf16, const KrVecPre& P) {
    const int nchunks = K / 8;
    for (int c = threadIdx.x; c < nchunks; c += KR_BLOCK) {
        float v[8];
        if (c == (int)threadIdx.x) {
#pragma unroll
            for (int i = 0; i < 8; i++) v[i] = P.v[i];
        } else kr_load8(x, c, v);
        float mx = 0.0f;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            if (round_bf16) v[i] = kr_bf16_to_f32(kr_f32_to_bf16(v[i]));
            mx = fmaxf(mx, fabsf(v[i]));
        }
        float scale, inv;
        kr_group_scale(mx, scale, inv);
        int q[8];
        kr_quant8<false>(v, inv, q);
        kr_store_chunk<I8>(L, c, q);
        if ((c & 15) == 0) L.ascale[c >> 4] = scale;
    }
}

// hidden = act(gate, up) then per-128 INT16 quantization, from gu = [gate(n) | up(n)] in global memory
struct KrHidPre { float g[8], u[8]; };
__device__ __forceinline__ void kr_hidden_load(const float* gu, int n, KrHidPre& P) {
    const int nch = n / 8, c = (int)threadIdx.x < nch ? (int)threadIdx.x : nch - 1;
    kr_load8(gu, c, P.g);
    kr_load8(gu + n, c, P.u);
}
template <int ACT, bool I8>
__device__ __forceinline__ void kr_prologue_hidden(const float* gu, int n, float swiglu_limit, float alpha, const KrActLds& L, const KrHidPre& P) {
    const int nchunks = n / 8;
    for (int c = threadIdx.x; c < nchunks; c += KR_BLOCK) {
        float g[8], u[8], h[8];
        if (c == (int)threadIdx.x) {
#pragma unroll
            for (int i = 0; i < 8; i++) { g[i] = P.g[i]; u[i] = P.u[i]; }
        } else {
            kr_load8(gu, c, g);
            kr_load8(gu + n, c, u);
        }
        float mx = 0.0f;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            if (ACT == KR_ACT_GPTOSS) {  // moe.rs:272-280
                float gate = g[i], up = u[i];
                if (gate > swiglu_limit) gate = swiglu_limit;
                if (up > swiglu_limit) up = swiglu_limit;
                if (up < -swiglu_limit) up = -swiglu_limit;
                const float glu = gate * kr_sigmoid_poly5_scalar(gate * alpha);
                h[i] = (up + 1.0f) * glu;
            } else {                      // avx2.rs:2331-2333 / decode.rs:1731-1733
                const float silu = g[i] * kr_sigmoid_poly5(g[i]);
                h[i] = silu * u[i];
            }
            mx = fmaxf(mx, fabsf(h[i]));
        }
        float scale, inv;
        kr_group_scale(mx, scale, inv);
        int q[8];
        if (ACT == KR_ACT_SILU_FUSED) kr_quant8<true>(h, inv, q);   // _mm256_cvtps_epi32
        else kr_quant8<false>(h, inv, q);                            // f32::round
        kr_store_chunk<I8>(L, c, q);
        if ((c & 15) == 0) L.ascale[c >> 4] = scale;
    }
}

// ------------------------------------------------------------------------------------------
// the streaming matvec tile: 8 columns per wave, 8 lanes per column
// ------------------------------------------------------------------------------------------

__device__ __forceinline__ float kr_chain(float acc, int isum, uint32_t sbits, float a_scale, bool fused) {
    const float comb = __uint_as_float(sbits << 16) * a_scale;       // bf16(w_scale) * a_scale, avx2.rs:1171
    const float gf = (float)isum;
    return fused ? __builtin_fmaf(gf, comb, acc) : (acc + gf * comb); // avx2.rs:1175 / :1201
}

#define KR_PRE 8   // group pairs (INT4) / groups (INT8) whose weights are fetched BEFORE the activation prologue runs

// The first KR_PRE weight records of a tile are requested before the workgroup builds its activation image, so the HBM
// latency of the stream overlaps the prologue (K = 2048 is covered entirely: 8 x 16 B per lane in flight).
struct KrPre { u32x4 w[KR_PRE]; uint32_t sc[KR_PRE]; };

template <int BITS>
__device__ __forceinline__ void kr_preload(KrPre& p, const void* qbase, const uint32_t* sbase, const KrMatDev& m, int tile, int lane, int unit0) {
    const int units = BITS == 4 ? m.ngp : m.ng;
    const u32x4* q = reinterpret_cast<const u32x4*>(qbase) + (size_t)tile * units * 64 + lane;
    const uint32_t* s = sbase + (size_t)tile * m.ngp * 8 + (lane >> 3);
#pragma unroll
    for (int u = 0; u < KR_PRE; u++)
        if (unit0 + u < units) { p.w[u] = kr_ldg_nt(q + (size_t)(unit0 + u) * 64); p.sc[u] = kr_ldg_nt(s + (BITS == 4 ? (unit0 + u) : ((unit0 + u) >> 1)) * 8); }
}

template <int BITS>
__device__ __forceinline__ float kr_matvec_tile(KrPre& p, bool preloaded, const void* qbase, const uint32_t* sbase, const KrMatDev& m, int tile,
                                               const KrActLds& L, int lane) {
    const int l8 = lane & 7, col = lane >> 3;
    const bool fused = (tile * 8 + col) < m.n_fma;
    const int units = BITS == 4 ? m.ngp : m.ng;
    float acc = 0.0f;
    for (int u0 = 0; u0 < units; u0 += KR_PRE) {
        if (u0 > 0 || !preloaded) kr_preload<BITS>(p, qbase, sbase, m, tile, lane, u0);
#pragma unroll
        for (int u = 0; u < KR_PRE; u++) {
            const int un = u0 + u;
            if (un < units) {
                if (BITS == 4) {
                    const int g0 = 2 * un, g1 = g0 + 1;
                    const int i0 = kr_red8_add_i32(kr_group_i4(p.w[u].x, p.w[u].y, g0, l8, L));
                    acc = kr_chain(acc, i0, p.sc[u] & 0xFFFFu, L.ascale[g0], fused);
                    if (g1 < m.ng) {
                        const int i1 = kr_red8_add_i32(kr_group_i4(p.w[u].z, p.w[u].w, g1, l8, L));
                        acc = kr_chain(acc, i1, p.sc[u] >> 16, L.ascale[g1], fused);
                    }
                } else {
                    const int i0 = kr_red8_add_i32(kr_group_i8(p.w[u], un, l8, L));
                    acc = kr_chain(acc, i0, (un & 1) ? (p.sc[u] >> 16) : (p.sc[u] & 0xFFFFu), L.ascale[un], fused);
                }
            }
        }
    }
    return acc;
}
