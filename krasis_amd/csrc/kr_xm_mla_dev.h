// kr_xm_mla_dev.h -- the body of the EXACT MLA scores pass on the f32 matrix cores for a run of tokens entering a device slot under
// "multi_extend_mla_exact_mfma" (kr_multi_mla_xm.hip, docs/design/29-multi-extend-mla-exact-mfma.md).  It is the text of kr_mla_scores_mfma_kernel
// (kr_attn_exact_mfma.hip, where the arithmetic is described: 16 fma chains per dot, the AVX2 fold tree, two launches -- rope dot, then latent dot + that, *
// sm_scale), changed in three places: the query-row tile is (run, t0) of a tile table and its rows go through a row map (Rows: token t of the run -> pass row),
// p_max comes from the run's first position and count, and a position's cache row goes through kr_xm_cache_row<PAGED>.  The single-sequence kernel stays text
// of its own: it sits at 256 VGPRs + 256 AGPRs with zero scratch, and a register moved there is a scratch segment (doc 29, "Kernels").
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include "kr_device.h"
#include "kr_libm.h"
#include "kr_xm_dev.h"

// One workgroup of 4 waves = 2 x 2 blocks of 32 query rows x 32 positions: the position tile at p_lo, the query-row tile at token t0 (64 / nh tokens) of a run of
// cnt tokens whose first token stands at position pos0.  Tile row r is (token t0 + r / nh, head r % nh); its pass row is rows(token) * nh + head -- the row of qb
// [.][K], of the score scratch and of tmax.  kb = row 0 of the slot's cache (flat) or the pool (PAGED: ptab = the slot's row of the page table, 1 << psh tokens a
// page), rows of K values.  ROPE: qb = q_pe, kb = the rope-key rows, K = rd: the dot goes to the scratch; !ROPE: qb = q_abs, kb = the latent rows, K = klr: v = (dot +
// scratch) * sm_scale goes to the scratch and its maxima per 32 positions to tmax.  As, Bs: 64 * XM_LDF floats of LDS each.  nh divides 32: a power of two
template <bool FP8, bool ROPE, bool PAGED, class Rows>
__device__ __forceinline__ void kr_xm_mla_scores_body(const float* __restrict__ qb, const char* __restrict__ kb, int nh, int K, int pos0, int cnt, int t0, int p_lo,
                                                      const Rows rows, const int* ptab, int psh, float sm_scale, float* __restrict__ sc, int sc_ld,
                                                      float* __restrict__ tmax, float* As, float* Bs) {
    const int lnh = __builtin_ctz(nh), hm = nh - 1, TT = 64 >> lnh;
    const int tn = min(TT, cnt - t0), R = tn << lnh;
    const int p_max = pos0 + t0 + tn - 1;                                     // last position any row of the tile may see
    if (p_lo > p_max) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), r31 = lane & 31, kh = lane >> 5;
    const int rb = (wave >> 1) * 32, pb = (wave & 1) * 32;                    // scalars: as lane values they were spilled across the 256-register epilogue (ROPE form)
    constexpr int ESZ = FP8 ? 1 : 2, KCH = FP8 ? 1 : 2;                       // 16-byte cache chunks per thread per 64-k stage
    // staging maps of a 64-k stage: q 64 rows x 64 floats (4 float4 per thread), cache 64 positions x 64 values (rows past p_max re-read p_max)
    int qrow[4], qc4[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int u = tid + 256 * i, row = u >> 4, rr = row < R ? row : R - 1;
        qc4[i] = (u & 15) * 4; qrow[i] = rows(t0 + (rr >> lnh)) * nh + (rr & hm);
    }
    int krow[KCH], koff[KCH];      // a thread's position is the same for every stage of the k loop: PAGED looks its page up once, here
#pragma unroll
    for (int i = 0; i < KCH; i++) {
        const int u = tid + 256 * i, prow = FP8 ? (u >> 2) : (u >> 3);
        koff[i] = FP8 ? (u & 3) * 16 : (u & 7) * 16; krow[i] = (int)kr_xm_cache_row<PAGED>(min(p_lo + prow, p_max), ptab, psh);
    }
    xm_f4 qreg[4]; u32x4 kreg[KCH];
    auto load_stage = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; i++) qreg[i] = *reinterpret_cast<const xm_f4*>(qb + (size_t)qrow[i] * K + k0 + qc4[i]);
#pragma unroll
        for (int i = 0; i < KCH; i++) kreg[i] = *reinterpret_cast<const u32x4*>(kb + ((size_t)krow[i] * K + k0) * ESZ + koff[i]);
    };
    auto commit_stage = [&]() {
#pragma unroll
        for (int i = 0; i < 4; i++) { const int u = tid + 256 * i, row = u >> 4; *reinterpret_cast<xm_f4*>(As + row * XM_LDF + qc4[i]) = qreg[i]; }
        if (FP8) {
            const uint32_t ww[4] = {kreg[0].x, kreg[0].y, kreg[0].z, kreg[0].w};
            float* dst = Bs + (tid >> 2) * XM_LDF + (tid & 3) * 16;
#pragma unroll
            for (int q4 = 0; q4 < 4; q4++)
                *reinterpret_cast<xm_f4*>(dst + 4 * q4) = xm_f4{kr_e4m3_to_f32((uint8_t)ww[q4]), kr_e4m3_to_f32((uint8_t)(ww[q4] >> 8)),
                                                              kr_e4m3_to_f32((uint8_t)(ww[q4] >> 16)), kr_e4m3_to_f32((uint8_t)(ww[q4] >> 24))};
        } else {
#pragma unroll
            for (int i = 0; i < KCH; i++) {
                const int u = tid + 256 * i, prow = u >> 3, c8 = (u & 7) * 8;
                const uint32_t ww[4] = {kreg[i].x, kreg[i].y, kreg[i].z, kreg[i].w};
                float f[8];
#pragma unroll
                for (int j = 0; j < 4; j++) { f[2 * j] = __half2float(__ushort_as_half((uint16_t)(ww[j] & 0xFFFFu))); f[2 * j + 1] = __half2float(__ushort_as_half((uint16_t)(ww[j] >> 16))); }
                *reinterpret_cast<xm_f4*>(Bs + prow * XM_LDF + c8) = xm_f4{f[0], f[1], f[2], f[3]};
                *reinterpret_cast<xm_f4*>(Bs + prow * XM_LDF + c8 + 4) = xm_f4{f[4], f[5], f[6], f[7]};
            }
        }
    };
    xm_v16f acc[16];
#pragma unroll
    for (int j = 0; j < 16; j++)
#pragma unroll
        for (int i = 0; i < 16; i++) acc[j][i] = 0.0f;
    // 16 chains, 64 k per stage, next stage requested under the MFMAs
    load_stage(0);
    for (int k0 = 0; k0 < K; k0 += 64) {
        __syncthreads();
        commit_stage();
        if (k0 + 64 < K) load_stage(k0 + 64);
        __syncthreads();
        const float* ap = As + (rb + r31) * XM_LDF + 16 * kh;
        const float* bp = Bs + (pb + r31) * XM_LDF + 16 * kh;
#pragma unroll
        for (int m = 0; m < 2; m++) {                                         // 32 consecutive k: the (s, s + 1) pair of every chain
            float av[16], bv[16];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const xm_f4 x = *reinterpret_cast<const xm_f4*>(ap + 32 * m + 4 * q), y = *reinterpret_cast<const xm_f4*>(bp + 32 * m + 4 * q);
                av[4 * q] = x.x; av[4 * q + 1] = x.y; av[4 * q + 2] = x.z; av[4 * q + 3] = x.w;
                bv[4 * q] = y.x; bv[4 * q + 1] = y.y; bv[4 * q + 2] = y.z; bv[4 * q + 3] = y.w;
            }
#pragma unroll
            for (int j = 0; j < 16; j++) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], bv[j], acc[j], 0, 0, 0);
        }
    }
    // the lane id is formed again here (v_mbcnt needs no live register): kept across the k loop, the lane half was the one value the 256-register tree spilled
    int lane_e;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane_e));
    const int r31e = lane_e & 31, khe = lane_e >> 5;
    const int pos = p_lo + pb + r31e;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int r = rb + (i & 3) + 8 * (i >> 2) + 4 * khe;
        const float c0 = (acc[0][i] + acc[8][i]) + (acc[4][i] + acc[12][i]);
        const float c1 = (acc[1][i] + acc[9][i]) + (acc[5][i] + acc[13][i]);
        const float c2 = (acc[2][i] + acc[10][i]) + (acc[6][i] + acc[14][i]);
        const float c3 = (acc[3][i] + acc[11][i]) + (acc[7][i] + acc[15][i]);
        const float d = (c0 + c1) + (c2 + c3);
        float mv = -__builtin_inff();
        const int rr = r < R ? r : 0, tt = rr >> lnh;
        const size_t rowi = (size_t)rows(t0 + tt) * nh + (rr & hm);
        if (r < R && pos <= pos0 + t0 + tt) {
            if (ROPE) sc[rowi * sc_ld + pos] = d;                             // the second addend, picked up by the latent launch
            else { mv = (d + sc[rowi * sc_ld + pos]) * sm_scale; sc[rowi * sc_ld + pos] = mv; }      // v = dot(latent) + dot(rope); v *= sm_scale
        }
        if (!ROPE && tmax) {
            mv = kr_red16_max_f32(mv);                            // 4 DPP steps inside each 16-lane row, then one exchange between the two rows of the lane half
            mv = fmaxf(mv, __shfl_xor(mv, 16));
            if (r31e == 0 && r < R) tmax[rowi * (size_t)(sc_ld >> 5) + ((p_lo + pb) >> 5)] = mv;
        }
    }
}
