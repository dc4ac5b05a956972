// kr_gguf_dev.h -- device side of the native GGUF block experts, shared by kr_gguf.hip (the exact kernels: moe_forward_gguf bit for bit) and
// kr_decode_fast.hip (KR_DECODE_FAST: the same products with the row's blocks split over two waves and the select / activation / combine folded in) and
// kr_gguf_group.hip (the exact grouped pass: an expert's blocks loaded once per group of rows, every row with the chains and the hsum tree below).
#pragma once
#include "kr_device.h"
#include "kr_libm.h"
#include "kr_exact_dev.h"
#include "kr_gguf.h"
#include <hip/hip_fp16.h>

#define GG_BLOCK 256

__device__ __forceinline__ float gg_f16(uint32_t bits16) { return __half2float(__ushort_as_half((uint16_t)bits16)); }

// ---- activation image: per 32-element sub-block s and AVX lane l an 8-byte record {AH4, AL4} of elements {2l,2l+1,16+2l,17+2l} ----
struct GgAct { uint32_t* rec; float* scale; int* sum; float* f32v; };   // rec [K/32][8][2], scale/sum [K/32], f32v [K] (scalar path)
__device__ __forceinline__ GgAct gg_carve(char* smem, int K) {
    GgAct a; a.rec = reinterpret_cast<uint32_t*>(smem); a.scale = reinterpret_cast<float*>(smem + (size_t)(K / 32) * 64);
    a.sum = reinterpret_cast<int*>(a.scale + K / 32); a.f32v = reinterpret_cast<float*>(a.sum + K / 32);
    return a;
}
__host__ __device__ static inline size_t gg_lds_bytes(int K, bool want_f32) { return (size_t)(K / 32) * 64 + (size_t)(K / 32) * 8 + (want_f32 ? (size_t)K * 4 : 0) + 16; }

// quantize_bf16_to_int16 / quantize_f32_to_int16 (gguf_kernels.rs:110,143): per 32, f32::round, clamp, i32 sums.
// One thread per 8 elements, 4 consecutive lanes per sub-block.
__device__ __forceinline__ void gg_quant_store(const float (&v)[8], int c, const GgAct& A) {
    float mx = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; i++) mx = fmaxf(mx, fabsf(v[i]));
    mx = kr_red4_max_f32(mx);
    const float scale = mx > 0.0f ? mx / 32767.0f : 1.0f, inv = mx > 0.0f ? 32767.0f / mx : 0.0f;
    int q[8]; int s = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        int t = (int)roundf(v[i] * inv); t = t > 32767 ? 32767 : (t < -32768 ? -32768 : t);
        q[i] = t; s += t;
    }
    s += KR_DPP(s, KR_DPP_XOR1); s += KR_DPP(s, KR_DPP_XOR2);
    const int sb = c >> 2, part = c & 3;            // chunk part: 0,1 -> first pair halves of lanes 0-3 / 4-7 ; 2,3 -> second pair halves
    uint16_t* rec16 = reinterpret_cast<uint16_t*>(A.rec + (size_t)sb * 16);
#pragma unroll
    for (int p = 0; p < 4; p++) {
        const int l = (part & 1) * 4 + p;           // AVX lane served by this pair
        const int half = part >> 1;                 // 0: elements (2l,2l+1), 1: elements (16+2l,17+2l)
        const int a0 = q[2 * p], a1 = q[2 * p + 1];
        rec16[l * 4 + half] = (uint16_t)(((a0 >> 8) & 0xFF) | (((a1 >> 8) & 0xFF) << 8));       // AH bytes
        rec16[l * 4 + 2 + half] = (uint16_t)((a0 & 0xFF) | ((a1 & 0xFF) << 8));                  // AL bytes
    }
    if (part == 0) { A.scale[sb] = scale; A.sum[sb] = s; }
}

__device__ __forceinline__ void gg_prologue_bf16(const uint16_t* x, int K, const GgAct& A, bool keep_f32) {
    for (int c = threadIdx.x; c < K / 8; c += GG_BLOCK) {
        const u32x4 r = *reinterpret_cast<const u32x4*>(x + (size_t)c * 8);
        float v[8];
        v[0] = __uint_as_float(r.x << 16); v[1] = __uint_as_float(r.x & 0xFFFF0000u); v[2] = __uint_as_float(r.y << 16); v[3] = __uint_as_float(r.y & 0xFFFF0000u);
        v[4] = __uint_as_float(r.z << 16); v[5] = __uint_as_float(r.z & 0xFFFF0000u); v[6] = __uint_as_float(r.w << 16); v[7] = __uint_as_float(r.w & 0xFFFF0000u);
        if (keep_f32) {
#pragma unroll
            for (int i = 0; i < 8; i++) A.f32v[c * 8 + i] = v[i];
        }
        gg_quant_store(v, c, A);
    }
}
// the decode graph's f32 hidden: the routed experts see bf16(hidden) (decode.rs:3307-3309: f32 -> bf16 RNE before moe_forward), then the bf16 path above
__device__ __forceinline__ void gg_prologue_f32_as_bf16(const float* x, int K, const GgAct& A, bool keep_f32) {
    for (int c = threadIdx.x; c < K / 8; c += GG_BLOCK) {
        float v[8];
        kr_load8(x, c, v);
#pragma unroll
        for (int i = 0; i < 8; i++) v[i] = kr_bf16_to_f32(kr_f32_to_bf16(v[i]));
        if (keep_f32) {
#pragma unroll
            for (int i = 0; i < 8; i++) A.f32v[c * 8 + i] = v[i];
        }
        gg_quant_store(v, c, A);
    }
}
// hidden = silu(gate) * up with libm exp (gguf_kernels.rs:733-737), then per-32 quantization
__device__ __forceinline__ void gg_prologue_hidden_split(const float* gate, const float* up, int n, const GgAct& A, bool keep_f32, bool do_quant) {
    for (int c = threadIdx.x; c < n / 8; c += GG_BLOCK) {
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const float g = gate[c * 8 + i];
            const float silu = g / (1.0f + kr_expf(-g));
            v[i] = silu * up[c * 8 + i];
            if (keep_f32) A.f32v[c * 8 + i] = v[i];
        }
        if (do_quant) gg_quant_store(v, c, A);
    }
    // tail when n % 8 != 0 (scalar path only)
    if (keep_f32) for (int i = (n / 8) * 8 + threadIdx.x; i < n; i += GG_BLOCK) { const float g = gate[i]; A.f32v[i] = (g / (1.0f + kr_expf(-g))) * up[i]; }
}

__device__ __forceinline__ void gg_scale_min_k4(int j, uint32_t s0, uint32_t s1, uint32_t s2, int& sc, int& mn) {   // gguf_kernels.rs:640
    const uint32_t w[3] = {s0, s1, s2};
    auto B = [&](int i) -> uint32_t { return (w[i >> 2] >> ((i & 3) * 8)) & 0xFFu; };
    if (j < 4) { sc = (int)(B(j) & 63u); mn = (int)(B(j + 4) & 63u); }
    else { sc = (int)((B(j + 4) & 0xFu) | ((B(j - 4) >> 6) << 4)); mn = (int)((B(j + 4) >> 4) | ((B(j) >> 6) << 4)); }
}

// ---- the per-sub-block bodies of the int path, shared by the streaming tiles below and the grouped kernels (kr_gguf_group.hip): one weight word of one AVX
//      lane against one activation image; `s` indexes the image's sub-blocks (the grouped kernels pass a stage-relative index into their LDS images) ----
// Q4_K: chunk j of a super-block = sub-blocks s_lo (low nibbles) and s_lo + 1 (high nibbles), in this order (matvec_q4_k_avx2, gguf_kernels.rs:271)
__device__ __forceinline__ void gg_pair_q4k(uint32_t w, float d, float dmin, int sc_lo, int mn_lo, int sc_hi, int mn_hi, const GgAct& A, int s_lo, int l, float& acc, float& corr) {
    const int s_hi = s_lo + 1;
    const u32x2 r_lo = *reinterpret_cast<const u32x2*>(A.rec + ((size_t)s_lo * 8 + l) * 2);
    const u32x2 r_hi = *reinterpret_cast<const u32x2*>(A.rec + ((size_t)s_hi * 8 + l) * 2);
    const uint32_t lo = w & 0x0F0F0F0Fu, hi = (w >> 4) & 0x0F0F0F0Fu;
    const int i_lo = (__builtin_amdgcn_sdot4((int)lo, (int)r_lo.x, 0, false) << 8) + (int)__builtin_amdgcn_udot4(lo, r_lo.y, 0u, false);
    const int i_hi = (__builtin_amdgcn_sdot4((int)hi, (int)r_hi.x, 0, false) << 8) + (int)__builtin_amdgcn_udot4(hi, r_hi.y, 0u, false);
    const float as_lo = A.scale[s_lo], as_hi = A.scale[s_hi];
    acc = __builtin_fmaf((float)i_lo, d * (float)sc_lo * as_lo, acc);
    corr += dmin * (float)mn_lo * as_lo * (float)A.sum[s_lo];
    acc = __builtin_fmaf((float)i_hi, d * (float)sc_hi * as_hi, acc);
    corr += dmin * (float)mn_hi * as_hi * (float)A.sum[s_hi];
}
// Q8_0: one 32-wide block (matvec_q8_0_avx2, gguf_kernels.rs:379)
__device__ __forceinline__ void gg_sub_q8_0(uint32_t w, float d, const GgAct& A, int s, int l, float& acc) {
    const u32x2 r = *reinterpret_cast<const u32x2*>(A.rec + ((size_t)s * 8 + l) * 2);
    const int iv = (__builtin_amdgcn_sdot4((int)w, (int)r.x, 0, false) << 8) + __builtin_amdgcn_sdot4((int)w, (int)(r.y ^ 0x80808080u), 0, false) +
                   (__builtin_amdgcn_sdot4((int)w, 0x01010101, 0, false) << 7);
    acc = __builtin_fmaf((float)iv, d * A.scale[s], acc);
}

// ---- one row tile (8 rows x 8 lanes), int path; returns the row result in every lane of the row's 8-lane group ----
// The block records of a tile are REQUESTED IN BATCHES of GG_PF before the first one is consumed (round 4): the loop used to issue one block's two loads,
// wait for them (one HBM / fabric round trip each), compute, and go on -- K / 256 dependent round trips per tile, the whole duration of the launch.  Indices
// past the last block are clamped (the load is unconditional, its value unused), the arithmetic and its order are unchanged: same bits.
#define GG_PF 8
// [part, parts): the slice of the row's blocks this call walks (tolerance decode: two waves share a row tile and add their results -- (0, 1) is the whole row,
// the reference's order)
__device__ __forceinline__ float gg_tile_q4k(const GgMat& m, int tile, const GgAct& A, int lane, int part = 0, int parts = 1) {
    const int l = lane & 7, row = lane >> 3;
    const int nb = m.K / 256, per = (nb + parts - 1) / parts, b_lo = part * per, b_hi = b_lo + per < nb ? b_lo + per : nb;
    const u32x4* q = reinterpret_cast<const u32x4*>(m.q) + (size_t)tile * nb * 64 + lane;
    const u32x4* h = reinterpret_cast<const u32x4*>(m.h) + (size_t)tile * nb * 8 + row;
    float acc = 0.0f, corr = 0.0f;
    for (int b0 = b_lo; b0 < b_hi; b0 += GG_PF) {
        u32x4 wv[GG_PF], hv[GG_PF];
#pragma unroll
        for (int u = 0; u < GG_PF; u++) { const int bb = b0 + u < b_hi ? b0 + u : (b_hi > 0 ? b_hi - 1 : 0); wv[u] = kr_ldg_nt(q + (size_t)bb * 64); hv[u] = kr_ldg_nt(h + (size_t)bb * 8); }
#pragma unroll
        for (int u = 0; u < GG_PF; u++) {
            const int b = b0 + u;
            if (b < b_hi) {
                const u32x4 w = wv[u], hd = hv[u];
                const float d = gg_f16(hd.x & 0xFFFFu), dmin = gg_f16(hd.x >> 16);
                const uint32_t wj[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    int sc_lo, mn_lo, sc_hi, mn_hi;
                    gg_scale_min_k4(2 * j, hd.y, hd.z, hd.w, sc_lo, mn_lo); gg_scale_min_k4(2 * j + 1, hd.y, hd.z, hd.w, sc_hi, mn_hi);
                    gg_pair_q4k(wj[j], d, dmin, sc_lo, mn_lo, sc_hi, mn_hi, A, b * 8 + 2 * j, l, acc, corr);
                }
            }
        }
    }
    return kr_hsum8(acc) - corr;
}

__device__ __forceinline__ float gg_tile_q8_0(const GgMat& m, int tile, const GgAct& A, int lane, int part = 0, int parts = 1) {
    const int l = lane & 7, row = lane >> 3;
    const int nb = m.K / 32, nbg = (nb + 3) / 4, per = (nbg + parts - 1) / parts, g_lo = part * per, g_hi = g_lo + per < nbg ? g_lo + per : nbg;
    const u32x4* q = reinterpret_cast<const u32x4*>(m.q) + (size_t)tile * nbg * 64 + lane;
    const u32x2* h = reinterpret_cast<const u32x2*>(m.h) + (size_t)tile * nbg * 8 + row;
    float acc = 0.0f;
    for (int g0 = g_lo; g0 < g_hi; g0 += GG_PF) {      // batched requests, as gg_tile_q4k
        u32x4 wv[GG_PF]; u32x2 hv[GG_PF];
#pragma unroll
        for (int v = 0; v < GG_PF; v++) { const int gg = g0 + v < g_hi ? g0 + v : (g_hi > 0 ? g_hi - 1 : 0); wv[v] = kr_ldg_nt(q + (size_t)gg * 64); hv[v] = h[(size_t)gg * 8]; }
#pragma unroll
        for (int v = 0; v < GG_PF; v++) {
            const int bg = g0 + v;
            if (bg < g_hi) {
                const u32x4 w = wv[v]; const u32x2 hd = hv[v];
                const uint32_t wb[4] = {w.x, w.y, w.z, w.w};
                const float dd[4] = {gg_f16(hd.x & 0xFFFFu), gg_f16(hd.x >> 16), gg_f16(hd.y & 0xFFFFu), gg_f16(hd.y >> 16)};
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int s = bg * 4 + u;
                    if (s < nb) {
                        gg_sub_q8_0(wb[u], dd[u], A, s, l, acc);
                    }
                }
            }
        }
    }
    return kr_hsum8(acc);
}

__device__ __forceinline__ float gg_tile_q4_0(const GgMat& m, int tile, const GgAct& A, int lane, int part = 0, int parts = 1) {
    const int l = lane & 7, row = lane >> 3;
    const int nb = m.K / 32, nbg = (nb + 7) / 8, per = (nbg + parts - 1) / parts, g_lo = part * per, g_hi = g_lo + per < nbg ? g_lo + per : nbg;
    const u32x4* q = reinterpret_cast<const u32x4*>(m.q) + (size_t)tile * nbg * 64 + lane;
    const u32x4* h = reinterpret_cast<const u32x4*>(m.h) + (size_t)tile * nbg * 8 + row;
    float acc = 0.0f, corr = 0.0f;
    for (int bg = g_lo; bg < g_hi; bg++) {
        const u32x4 w = kr_ldg_nt(q + (size_t)bg * 64);
        const u32x4 hd = kr_ldg_nt(h + (size_t)bg * 8);
        const uint32_t wb[4] = {w.x, w.y, w.z, w.w}, hb[4] = {hd.x, hd.y, hd.z, hd.w};
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int s = bg * 8 + u;
            if (s < nb) {
                const uint32_t two = (wb[u >> 1] >> ((u & 1) * 16)) & 0xFFFFu;        // bytes qs[2l], qs[2l+1]
                const uint32_t nib = (two & 0x0F0Fu) | (((two >> 4) & 0x0F0Fu) << 16);  // {lo(b0), lo(b1), hi(b0), hi(b1)} = elems 2l,2l+1,16+2l,17+2l
                const float d = gg_f16((hb[u >> 1] >> ((u & 1) * 16)) & 0xFFFFu);
                const u32x2 r = *reinterpret_cast<const u32x2*>(A.rec + ((size_t)s * 8 + l) * 2);
                const int iv = (__builtin_amdgcn_sdot4((int)nib, (int)r.x, 0, false) << 8) + (int)__builtin_amdgcn_udot4(nib, r.y, 0u, false);
                const float as = A.scale[s];
                acc = __builtin_fmaf((float)iv, d * as, acc);
                corr += d * 8.0f * as * (float)A.sum[s];
            }
        }
    }
    return kr_hsum8(acc) - corr;
}

// ---- Q5_0 / Q6_K: the reference has no integer form for them (scalar f32 rows, gguf_kernels.rs:572-635: nothing is quantised on this path), so the tiles below
//      form the reference's TERMS from the f32 activation vector A.f32v (16-byte aligned) and give up its serial row chain: lane l of a row owns the slice the
//      layout hands it (kr_gguf.hip header), keeps its terms in two f32 chains in block order (one packed accumulator: elements of even and of odd index),
//      then kr_hsum8.  Tolerance form only (KR_DECODE_FAST, kr_gguf_matvec parts 1 | 2); the exact chain is gg_row_scalar (kr_gguf.hip).  Records and
//      headers are requested in batches, as in gg_tile_q4k; [part, parts) slices the block groups (Q5_0) / super-blocks (Q6_K). ----
typedef float gg_f32x2 __attribute__((ext_vector_type(2)));
#define GG_PF5 2      // Q5_0: block groups (8 blocks each) requested ahead -- per lane 4 record + 12 header words a group
#define GG_PF6 4      // Q6_K: super-blocks requested ahead -- per lane 6 record + 5 header words a block (the down launch of the mode has 128 registers a lane)

// Q5_0 term d * (q - 16) * x (gguf_kernels.rs:585-592) on elements {2l, 2l+1} and {16+2l, 17+2l} of every block
__device__ __forceinline__ float gg_tile_q5_0(const GgMat& m, int tile, const GgAct& A, int lane, int part = 0, int parts = 1) {
    const int l = lane & 7, row = lane >> 3;
    const int nb = m.K / 32, nbg = (nb + 7) / 8, per = (nbg + parts - 1) / parts, g_lo = part * per, g_hi = g_lo + per < nbg ? g_lo + per : nbg;
    const u32x4* q = reinterpret_cast<const u32x4*>(m.q) + (size_t)tile * nbg * 64 + lane;
    const u32x4* h = reinterpret_cast<const u32x4*>(m.h) + ((size_t)tile * nbg * 8 + row) * 3;
    gg_f32x2 acc = {0.0f, 0.0f};
    for (int g0 = g_lo; g0 < g_hi; g0 += GG_PF5) {
        u32x4 wv[GG_PF5], hv[GG_PF5][3];
#pragma unroll
        for (int v = 0; v < GG_PF5; v++) {
            const int gg = g0 + v < g_hi ? g0 + v : (g_hi > 0 ? g_hi - 1 : 0);
            wv[v] = kr_ldg_nt(q + (size_t)gg * 64);
#pragma unroll
            for (int i = 0; i < 3; i++) hv[v][i] = kr_ldg_nt(h + (size_t)gg * 24 + i);
        }
#pragma unroll
        for (int v = 0; v < GG_PF5; v++) {
            const int bg = g0 + v;
            if (bg < g_hi) {
                const uint32_t wb[4] = {wv[v].x, wv[v].y, wv[v].z, wv[v].w}, db[4] = {hv[v][0].x, hv[v][0].y, hv[v][0].z, hv[v][0].w};
                const uint32_t hb[8] = {hv[v][1].x, hv[v][1].y, hv[v][1].z, hv[v][1].w, hv[v][2].x, hv[v][2].y, hv[v][2].z, hv[v][2].w};
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const int s = bg * 8 + u;
                    if (s < nb) {
                        const uint32_t two = (wb[u >> 1] >> ((u & 1) * 16)) & 0xFFFFu;      // bytes qs[2l], qs[2l+1]
                        const uint32_t hq = hb[u] >> (2 * l);                                  // bits 0, 1, 16, 17: the fifth bits of elements 2l, 2l+1, 16+2l, 17+2l
                        const float d = gg_f16((db[u >> 1] >> ((u & 1) * 16)) & 0xFFFFu);
                        const gg_f32x2 dd = {d, d};
                        const gg_f32x2 q_lo = {(float)(int)((two & 0xFu) | ((hq & 1u) << 4)) - 16.0f, (float)(int)(((two >> 8) & 0xFu) | ((hq & 2u) << 3)) - 16.0f};
                        const gg_f32x2 q_hi = {(float)(int)(((two >> 4) & 0xFu) | (((hq >> 16) & 1u) << 4)) - 16.0f, (float)(int)(((two >> 12) & 0xFu) | (((hq >> 17) & 1u) << 4)) - 16.0f};
                        const gg_f32x2 x_lo = *reinterpret_cast<const gg_f32x2*>(A.f32v + s * 32 + 2 * l), x_hi = *reinterpret_cast<const gg_f32x2*>(A.f32v + s * 32 + 16 + 2 * l);
                        acc += (dd * q_lo) * x_lo;
                        acc += (dd * q_hi) * x_hi;
                    }
                }
            }
        }
    }
    return kr_hsum8(acc.x + acc.y);
}

// four consecutive elements of one 32-wide run of a Q6_K half: 6-bit codes in the bytes of `codes`, one scale product s = d * sc (gguf_kernels.rs:612-630)
__device__ __forceinline__ void gg_q6k_four(gg_f32x2& acc, float s, uint32_t codes, const float* x) {
    const float4 xv = *reinterpret_cast<const float4*>(x);
    const gg_f32x2 ss = {s, s};
    const gg_f32x2 q01 = {(float)(codes & 0xFFu) - 32.0f, (float)((codes >> 8) & 0xFFu) - 32.0f}, q23 = {(float)((codes >> 16) & 0xFFu) - 32.0f, (float)(codes >> 24) - 32.0f};
    const gg_f32x2 x01 = {xv.x, xv.y}, x23 = {xv.z, xv.w};
    acc += (ss * q01) * x01;
    acc += (ss * q23) * x23;
}

// Q6_K term (d * sc) * (q - 32) * x: lane l owns, per half, l' in [4l, 4l + 4) of the reference's inner loop -- 16 elements, scale index is = l / 4 throughout.
// The 6-bit unpack runs on whole words: four codes at a time from one ql word and one qh word.
__device__ __forceinline__ float gg_tile_q6k(const GgMat& m, int tile, const GgAct& A, int lane, int part = 0, int parts = 1) {
    const int l = lane & 7, row = lane >> 3;
    const int nb = m.K / 256, per = (nb + parts - 1) / parts, b_lo = part * per, b_hi = b_lo + per < nb ? b_lo + per : nb;
    const uint32_t* q = reinterpret_cast<const uint32_t*>(m.q) + ((size_t)tile * nb * 128 + lane) * 3;      // [block][half][8 rows][8 lanes] x 12 B
    const uint32_t* h = reinterpret_cast<const uint32_t*>(m.h) + ((size_t)tile * nb * 8 + row) * 5;          // [block][8 rows] x 20 B
    const int sh = (l >> 2) * 8;
    gg_f32x2 acc = {0.0f, 0.0f};
    for (int b0 = b_lo; b0 < b_hi; b0 += GG_PF6) {
        uint32_t wv[GG_PF6][2][3], hv[GG_PF6][5];
#pragma unroll
        for (int u = 0; u < GG_PF6; u++) {
            const int bb = b0 + u < b_hi ? b0 + u : (b_hi > 0 ? b_hi - 1 : 0);
#pragma unroll
            for (int i = 0; i < 6; i++) wv[u][i / 3][i % 3] = kr_ldg_nt(q + ((size_t)bb * 128 + (i / 3) * 64) * 3 + i % 3);
#pragma unroll
            for (int i = 0; i < 5; i++) hv[u][i] = kr_ldg_nt(h + (size_t)bb * 40 + i);
        }
#pragma unroll
        for (int u = 0; u < GG_PF6; u++) {
            const int b = b0 + u;
            if (b < b_hi) {
                const float d = gg_f16(hv[u][4] & 0xFFFFu);
#pragma unroll
                for (int hf = 0; hf < 2; hf++) {
                    const uint32_t s01 = hv[u][2 * hf] >> sh, s23 = hv[u][2 * hf + 1] >> sh;      // scale bytes is + {0, 2} and is + {4, 6} of this half
                    const float s0 = d * (float)(int8_t)(s01 & 0xFFu), s1 = d * (float)(int8_t)((s01 >> 16) & 0xFFu);
                    const float s2 = d * (float)(int8_t)(s23 & 0xFFu), s3 = d * (float)(int8_t)((s23 >> 16) & 0xFFu);
                    const uint32_t a = wv[u][hf][0], bq = wv[u][hf][1], c = wv[u][hf][2];         // ql[4l..], ql[32 + 4l..], qh[4l..] of the half
                    const float* in = A.f32v + b * 256 + hf * 128 + 4 * l;
                    gg_q6k_four(acc, s0, (a & 0x0F0F0F0Fu) | ((c & 0x03030303u) << 4), in);
                    gg_q6k_four(acc, s1, (bq & 0x0F0F0F0Fu) | ((c & 0x0C0C0C0Cu) << 2), in + 32);
                    gg_q6k_four(acc, s2, ((a >> 4) & 0x0F0F0F0Fu) | (c & 0x30303030u), in + 64);
                    gg_q6k_four(acc, s3, ((bq >> 4) & 0x0F0F0F0Fu) | ((c >> 2) & 0x30303030u), in + 96);
                }
            }
        }
    }
    return kr_hsum8(acc.x + acc.y);
}

// ---- Q5_K (docs/design/45-gguf-q5k.md): the reference de-quantizes the type (gguf.rs:740-803) and has no matvec for it; the value is w = (d sc_j) (q4 + 16 q5) - (dmin mn_j) with
//      dequant_q5_k's roundings, the exact chain is the scalar Q4_K row over these values (gg_row_q5k, kr_gguf.hip).  The tile: lane l owns Q4_K's record -- per chunk j of 64
//      elements one word, bytes {qs[32j+2l], qs[32j+2l+1], qs[32j+16+2l], qs[32j+17+2l]}, low nibbles = elements 64j + p, high nibbles = elements 64j + 32 + p -- and ONE header
//      word whose byte i carries the fifth bits of byte i of every chunk (bit 2j: low nibble, bit 2j + 1: high nibble).  Four codes at a time on whole words: two nibble masks
//      per chunk word, the fifth bits shifted under 0x10101010.  Values against A.f32v in one packed accumulator in block order, then kr_hsum8; [part, parts) slices super-blocks. ----
#define GG_PF5K 4     // super-blocks requested ahead -- per lane 4 record + 5 header words a block
// four codes (the bytes of `codes`) of one sub-block against the pairs x[0..1] (elements 2l, 2l + 1) and x[16..17] (elements 16 + 2l, 17 + 2l)
__device__ __forceinline__ void gg_q5k_four(gg_f32x2& acc, float d1, float m1, uint32_t codes, const float* x) {
    const gg_f32x2 dd = {d1, d1}, mm = {m1, m1};
    const gg_f32x2 q01 = {(float)(codes & 0xFFu), (float)((codes >> 8) & 0xFFu)}, q23 = {(float)((codes >> 16) & 0xFFu), (float)(codes >> 24)};
    const gg_f32x2 x01 = *reinterpret_cast<const gg_f32x2*>(x), x23 = *reinterpret_cast<const gg_f32x2*>(x + 16);
    acc += (dd * q01 - mm) * x01;
    acc += (dd * q23 - mm) * x23;
}
__device__ __forceinline__ float gg_tile_q5k(const GgMat& m, int tile, const GgAct& A, int lane, int part = 0, int parts = 1) {
    const int l = lane & 7, row = lane >> 3;
    const int nb = m.K / 256, per = (nb + parts - 1) / parts, b_lo = part * per, b_hi = b_lo + per < nb ? b_lo + per : nb;
    const u32x4* q = reinterpret_cast<const u32x4*>(m.q) + (size_t)tile * nb * 64 + lane;
    const u32x4* h = reinterpret_cast<const u32x4*>(m.h) + ((size_t)tile * nb * 8 + row) * 3;               // [block][8 rows] x 48 B
    gg_f32x2 acc = {0.0f, 0.0f};
    for (int b0 = b_lo; b0 < b_hi; b0 += GG_PF5K) {
        u32x4 wv[GG_PF5K], hv[GG_PF5K]; uint32_t fv[GG_PF5K];
#pragma unroll
        for (int u = 0; u < GG_PF5K; u++) {
            const int bb = b0 + u < b_hi ? b0 + u : (b_hi > 0 ? b_hi - 1 : 0);
            wv[u] = kr_ldg_nt(q + (size_t)bb * 64); hv[u] = kr_ldg_nt(h + (size_t)bb * 24);
            fv[u] = kr_ldg_nt(reinterpret_cast<const uint32_t*>(h + (size_t)bb * 24 + 1) + l);
        }
#pragma unroll
        for (int u = 0; u < GG_PF5K; u++) {
            const int b = b0 + u;
            if (b < b_hi) {
                const u32x4 hd = hv[u];
                const float d = gg_f16(hd.x & 0xFFFFu), dmin = gg_f16(hd.x >> 16);
                const uint32_t wj[4] = {wv[u].x, wv[u].y, wv[u].z, wv[u].w}, f = fv[u];
                // fifth bits of chunk j under the mask 0x10101010: bit 2j (low nibbles), bit 2j + 1 (high nibbles) of every byte of f
                const uint32_t f_lo[4] = {(f << 4) & 0x10101010u, (f << 2) & 0x10101010u, f & 0x10101010u, (f >> 2) & 0x10101010u};
                const uint32_t f_hi[4] = {(f << 3) & 0x10101010u, (f << 1) & 0x10101010u, (f >> 1) & 0x10101010u, (f >> 3) & 0x10101010u};
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    int sc_lo, mn_lo, sc_hi, mn_hi;
                    gg_scale_min_k4(2 * j, hd.y, hd.z, hd.w, sc_lo, mn_lo); gg_scale_min_k4(2 * j + 1, hd.y, hd.z, hd.w, sc_hi, mn_hi);
                    const float* in = A.f32v + b * 256 + j * 64 + 2 * l;
                    gg_q5k_four(acc, d * (float)sc_lo, dmin * (float)mn_lo, (wj[j] & 0x0F0F0F0Fu) | f_lo[j], in);
                    gg_q5k_four(acc, d * (float)sc_hi, dmin * (float)mn_hi, ((wj[j] >> 4) & 0x0F0F0F0Fu) | f_hi[j], in + 32);
                }
            }
        }
    }
    return kr_hsum8(acc.x + acc.y);
}

// ---- Q3_K (docs/design/47-gguf-q3k.md): the reference has neither a de-quantizer nor a matvec for the type; from ggml's block {hmask[32], qs[64], scales[12], f16 d} the value
//      of element 128 n + 32 j + p is w = (d sc_s) q, q = ((qs[32n + p] >> 2j) & 3 | hmask[p] bit (4n + j) << 2) - 4, s = 8n + 2j + (p >> 4), sc_s the 6-bit scale minus 32, two
//      rounded f32 products; the exact chain is the scalar Q4_K row over these values (gg_row_q3k, kr_gguf.hip).  The tile: lane l owns a 12-byte record -- words n = 0, 1 =
//      qs[32n + {2l, 2l+1, 16+2l, 17+2l}], word 2 = hmask[{2l, 2l+1, 16+2l, 17+2l}] -- the elements {2l, 2l+1, 16+2l, 17+2l} of each of the block's eight 32-element chunks
//      c = 4n + j.  Four codes at a time on whole words: two bits of word n under 0x03030303, bit c of every hmask byte under 0x04040404; bytes 0, 1 belong to sub-block 2c,
//      bytes 2, 3 to sub-block 2c + 1.  Values against A.f32v in one packed accumulator in block order, then kr_hsum8; [part, parts) slices super-blocks. ----
#define GG_PF3K 4     // super-blocks requested ahead -- per lane 3 record + 4 header words a block
// the four 6-bit scales 4g .. 4g + 3 (g < 4) of a Q3_K block as the bytes of one word, 32 not yet subtracted; s0, s1, s2: the 12 scale bytes as words
__device__ __forceinline__ uint32_t gg_q3k_scales4(int g, uint32_t s0, uint32_t s1, uint32_t s2) {
    const uint32_t lo = ((g & 1 ? s1 : s0) >> (g & 2 ? 4 : 0)) & 0x0F0F0F0Fu;
    return lo | (((s2 >> (2 * g)) & 0x03030303u) << 4);
}
// scale s < 16 of a Q3_K block, in -32 .. 31
__device__ __forceinline__ int gg_q3k_scale(int s, uint32_t s0, uint32_t s1, uint32_t s2) { return (int)((gg_q3k_scales4(s >> 2, s0, s1, s2) >> ((s & 3) * 8)) & 0xFFu) - 32; }
// four codes (the bytes of `codes`, 0 .. 7) of one chunk: bytes 0, 1 (sub-block scale d_lo) against x[0..1], bytes 2, 3 (d_hi) against x[16..17]
__device__ __forceinline__ void gg_q3k_four(gg_f32x2& acc, float d_lo, float d_hi, uint32_t codes, const float* x) {
    const gg_f32x2 dl = {d_lo, d_lo}, dh = {d_hi, d_hi};
    const gg_f32x2 q01 = {(float)(codes & 0xFFu) - 4.0f, (float)((codes >> 8) & 0xFFu) - 4.0f}, q23 = {(float)((codes >> 16) & 0xFFu) - 4.0f, (float)(codes >> 24) - 4.0f};
    const gg_f32x2 x01 = *reinterpret_cast<const gg_f32x2*>(x), x23 = *reinterpret_cast<const gg_f32x2*>(x + 16);
    acc += (dl * q01) * x01;
    acc += (dh * q23) * x23;
}
__device__ __forceinline__ float gg_tile_q3k(const GgMat& m, int tile, const GgAct& A, int lane, int part = 0, int parts = 1) {
    const int l = lane & 7, row = lane >> 3;
    const int nb = m.K / 256, per = (nb + parts - 1) / parts, b_lo = part * per, b_hi = b_lo + per < nb ? b_lo + per : nb;
    const uint32_t* q = reinterpret_cast<const uint32_t*>(m.q) + ((size_t)tile * nb * 64 + lane) * 3;      // [block][8 rows][8 lanes] x 12 B
    const u32x4* h = reinterpret_cast<const u32x4*>(m.h) + (size_t)tile * nb * 8 + row;                     // [block][8 rows] x 16 B
    gg_f32x2 acc = {0.0f, 0.0f};
    for (int b0 = b_lo; b0 < b_hi; b0 += GG_PF3K) {
        uint32_t wv[GG_PF3K][3]; u32x4 hv[GG_PF3K];
#pragma unroll
        for (int u = 0; u < GG_PF3K; u++) {
            const int bb = b0 + u < b_hi ? b0 + u : (b_hi > 0 ? b_hi - 1 : 0);
#pragma unroll
            for (int i = 0; i < 3; i++) wv[u][i] = kr_ldg_nt(q + (size_t)bb * 192 + i);
            hv[u] = kr_ldg_nt(h + (size_t)bb * 8);
        }
#pragma unroll
        for (int u = 0; u < GG_PF3K; u++) {
            const int b = b0 + u;
            if (b < b_hi) {
                const u32x4 hd = hv[u];
                const float d = gg_f16(hd.w & 0xFFFFu);
                const uint32_t hm = wv[u][2];
#pragma unroll
                for (int c = 0; c < 8; c++) {      // chunk c = 4 n + j: sub-blocks 2c, 2c + 1 = bytes (2c & 3), (2c & 3) + 1 of scale word c >> 1
                    const uint32_t s4 = gg_q3k_scales4(c >> 1, hd.x, hd.y, hd.z) >> ((c & 1) * 16);
                    const float d_lo = d * (float)((int)(s4 & 0xFFu) - 32), d_hi = d * (float)((int)((s4 >> 8) & 0xFFu) - 32);
                    const uint32_t codes = ((wv[u][c >> 2] >> (2 * (c & 3))) & 0x03030303u) | (((hm >> c) & 0x01010101u) << 2);
                    gg_q3k_four(acc, d_lo, d_hi, codes, A.f32v + b * 256 + c * 32 + 2 * l);
                }
            }
        }
    }
    return kr_hsum8(acc.x + acc.y);
}

__host__ __device__ static inline bool gg_int_path(int t) { return t == GG_Q4_K || t == GG_Q8_0 || t == GG_Q4_0; }
__host__ __device__ static inline bool gg_scalar_type(int t) { return t == GG_Q5_0 || t == GG_Q3_K || t == GG_Q5_K || t == GG_Q6_K; }
// one 8-row tile of a scalar type in the tolerance form
__device__ __forceinline__ float gg_tile_scalar(const GgMat& m, int tile, const GgAct& A, int lane, int part = 0, int parts = 1) {
    return m.type == GG_Q6_K ? gg_tile_q6k(m, tile, A, lane, part, parts) : m.type == GG_Q5_K ? gg_tile_q5k(m, tile, A, lane, part, parts)
         : m.type == GG_Q3_K ? gg_tile_q3k(m, tile, A, lane, part, parts) : gg_tile_q5_0(m, tile, A, lane, part, parts);
}

__device__ __forceinline__ GgMat gg_expert_mat(const GgMat& base, int e) {
    GgMat m = base;
    m.q = reinterpret_cast<const char*>(base.q) + (size_t)e * base.q_stride;
    m.h = reinterpret_cast<const char*>(base.h) + (size_t)e * base.h_stride;
    return m;
}

