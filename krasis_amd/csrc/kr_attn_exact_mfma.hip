// kr_attn_exact_mfma.hip -- passes A (scores) and C (P.V) of the EXACT prompt-pass attention (decode.rs:4194-4281 order) on the f32 matrix
// cores, BIT-IDENTICAL to the vector-ALU kernels kr_pfm_gqa_scores*_kernel / kr_pfm_gqa_pv_kernel of kr_prefill_ops.hip (which stay as the
// fallback for group sizes that do not divide 32, and are what these were checked against: every prompt-pass == decode test runs them).
//
// v_mfma_f32_32x32x2_f32 computes D = fma(A[.][1], B[1][.], fma(A[.][0], B[0][.], C)): two fused multiply-adds in k order, no intermediate
// rounding beyond the fma's own -- a sequential f32 fma chain IS an accumulator fed with consecutive pairs (the router logits and the MLA
// projections of this round use the same fact, kr_route_mfma.hip).
//   * scores: the reference keeps 8 fma lanes per (query, position): lane l walks q[8b + l] * k[8b + l] over b ascending, then
//     ((l0 + l4) + (l1 + l5)) + ((l2 + l6) + (l3 + l7)), then * sm_scale.  Lane l of a 32-query x 32-position block is accumulator l fed with
//     the pairs (b, b + 1): A[q][k] = q[8 (2m + k) + l], B[k][p] = K[p][8 (2m + k) + l] -- 8 accumulators per block, hd / 16 MFMAs each.
//   * P.V: out[q][d] = chain over positions ascending of fma(p[q][pos], V[pos][d]): ONE accumulator per 32 x 32 (query, dim) block with the
//     positions as k.  A position a query must not see enters with p = 0: fma(0, v, acc) = acc exactly (v is finite: cache rows past the
//     last position of the tile are never read).
// Both run at the f32-MFMA rate, which is the vector fma rate on CDNA4 -- the gain is structural: operands staged once in LDS for 32 x 32
// outputs, no per-lane broadcast traffic (the vector P.V pass was bound by the LDS return path, the scores pass by 4 LDS reads per 4 fma).
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include "kr_device.h"
#include "kr_lds_optin.h"
#include "kr_libm.h"
#include "kr_prefill_ops.h"
#include "kr_xm_dev.h"

// ------------------------------------------------------------------------------------------------------------------------------------
// pass A.  grid (position tiles of 64, row tiles of 64 queries, nkv), 4 waves = 2 x 2 blocks of 32 queries x 32 positions.
// A query row r of the tile is (token t0 + r / group, head kvh * group + r % group), t0 = tile * (64 / group).
// ------------------------------------------------------------------------------------------------------------------------------------
template <bool FP8>
__global__ void __launch_bounds__(256, 2) kr_pfm_gqa_scores_mfma_kernel(const KrPfmGqaArgs a, float* __restrict__ sc, int sc_ld, int C, float* __restrict__ tmax) {
    __shared__ __attribute__((aligned(16))) float Qs[64 * XM_LDF];
    __shared__ __attribute__((aligned(16))) float Ks[64 * XM_LDF];
    const KrXmSeq q{a.q_out, a.gate, a.attn_out, a.k_cache, a.v_cache, a.gated, a.nh, a.nkv, a.pos0, C, a.sm_scale};
    const int TT = 64 >> __builtin_ctz(a.nh / a.nkv);
    kr_xm_scores_body<FP8, false>(q, a.hd, blockIdx.y * TT, blockIdx.x * 64, blockIdx.z, KrXmRowsIdentity(), nullptr, 0, sc, sc_ld, tmax, Qs, Ks);      // the body: kr_xm_dev.h
}

// ------------------------------------------------------------------------------------------------------------------------------------
// pass C.  grid (row tiles of 32 queries, nkv), 4 waves; wave w owns the 32-dim blocks w * NB .. w * NB + NB - 1 of the head (NB = hd / 128,
// head_dim 64: waves 0 and 1 one block each).  64 positions per stage: probabilities (masked) as f32 and the raw V rows in LDS.
// ------------------------------------------------------------------------------------------------------------------------------------
template <bool FP8, int HD, int PS>      // PS = positions per stage (64; 32 for the 512-wide latent rows of MLA: the V tile must fit the static LDS window)
__global__ void __launch_bounds__(256) kr_pfm_gqa_pv_mfma_kernel(const KrPfmGqaArgs a, const float* __restrict__ sc, int sc_ld, int C, const float* __restrict__ inv) {
    __shared__ __attribute__((aligned(16))) float Ps[32 * (PS + 4)];
    __shared__ __attribute__((aligned(16))) char Vs[PS * (HD * (FP8 ? 1 : 2) + 64)];
    const KrXmSeq q{a.q_out, a.gate, a.attn_out, a.k_cache, a.v_cache, a.gated, a.nh, a.nkv, a.pos0, C, a.sm_scale};
    const int TT = 32 >> __builtin_ctz(a.nh / a.nkv);
    kr_xm_pv_body<FP8, HD, PS, false>(q, blockIdx.x * TT, blockIdx.y, KrXmRowsIdentity(), nullptr, 0, sc, sc_ld, inv, Ps, Vs);      // the body: kr_xm_dev.h
}

// ------------------------------------------------------------------------------------------------------------------------------------
// MLA prompt pass, exact scores (decode.rs mla_attn_dot_fp16_avx2 twice: kr_dot2acc of kr_mla.hip): per (token, head) row and position
//     v = dot16(q_abs[row], ckv[pos]) + dot16(q_pe[row], kpe[pos]);  v *= sm_scale
// where dot16 keeps 16 fma chains (chain j over elements 16 s + j, s ascending) and folds them with the AVX2 tree -- the router's structure
// (kr_route_mfma.hip): 16 accumulators of a 32 x 32 block fed with (s, s + 1) pairs, tree (c0 + c1) + (c2 + c3), c0 = (a0 + a8) + (a4 + a12) ...
// grid (position tiles of 64, row tiles of 64, 1); rows are (token, head) pairs in token-major order; 64 k per LDS stage.
// ------------------------------------------------------------------------------------------------------------------------------------
// Two launches, one dot each (holding the first dot's 16 folded values across a second 256-register accumulation made the register allocator spill
// accumulators to scratch, and a kernel with a scratch segment runs with a fraction of the waves: 7.8 ms instead of ~1): ROPE = true writes
// dot16(q_pe, kpe) of every visible (row, position) to the scratch; ROPE = false reads it back as the second addend: v = dot16(q_abs, ckv) + that; v *= sm_scale.
template <bool FP8, bool ROPE>
__global__ void __launch_bounds__(256) kr_mla_scores_mfma_kernel(const float* __restrict__ qb, const void* __restrict__ kbv, int nh, int K, int pos0, int rows, float sm_scale,
                                                                 float* __restrict__ sc, int sc_ld, float* __restrict__ tmax) {
    __shared__ __attribute__((aligned(16))) float As[64 * XM_LDF];
    __shared__ __attribute__((aligned(16))) float Bs[64 * XM_LDF];
    const int row0 = blockIdx.y * 64, R = min(64, rows - row0);
    const int lnh = __builtin_ctz(nh);                                        // nh divides 32: a power of two
    const int p_lo = blockIdx.x * 64, p_max = pos0 + ((row0 + R - 1) >> lnh);  // last position any row of the tile may see
    if (p_lo > p_max) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), r31 = lane & 31, kh = lane >> 5;
    const int rb = (wave >> 1) * 32, pb = (wave & 1) * 32;                    // scalars: as lane values they were spilled across the 256-register epilogue (ROPE form)
    constexpr int ESZ = FP8 ? 1 : 2, KCH = FP8 ? 1 : 2;                       // 16-byte cache chunks per thread per 64-k stage
    // staging maps of a 64-k stage: q 64 rows x 64 floats (4 float4 per thread), cache 64 positions x 64 values (rows past p_max re-read p_max)
    int qrow[4], qc4[4];
#pragma unroll
    for (int i = 0; i < 4; i++) { const int u = tid + 256 * i, row = u >> 4; qc4[i] = (u & 15) * 4; qrow[i] = row0 + (row < R ? row : R - 1); }
    int kpos[KCH], koff[KCH];
#pragma unroll
    for (int i = 0; i < KCH; i++) { const int u = tid + 256 * i, prow = FP8 ? (u >> 2) : (u >> 3); koff[i] = FP8 ? (u & 3) * 16 : (u & 7) * 16; kpos[i] = min(p_lo + prow, p_max); }
    xm_f4 qreg[4]; u32x4 kreg[KCH];
    auto load_stage = [&](const float* qb, const char* kb, int K, int k0) {
#pragma unroll
        for (int i = 0; i < 4; i++) qreg[i] = *reinterpret_cast<const xm_f4*>(qb + (size_t)qrow[i] * K + k0 + qc4[i]);
#pragma unroll
        for (int i = 0; i < KCH; i++) kreg[i] = *reinterpret_cast<const u32x4*>(kb + ((size_t)kpos[i] * K + k0) * ESZ + koff[i]);
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
    const char* kb = reinterpret_cast<const char*>(kbv);
    xm_v16f acc[16];
#pragma unroll
    for (int j = 0; j < 16; j++)
#pragma unroll
        for (int i = 0; i < 16; i++) acc[j][i] = 0.0f;
    // 16 chains, 64 k per stage, next stage requested under the MFMAs
    load_stage(qb, kb, K, 0);
    for (int k0 = 0; k0 < K; k0 += 64) {
        __syncthreads();
        commit_stage();
        if (k0 + 64 < K) load_stage(qb, kb, K, k0 + 64);
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
        const size_t rowi = (size_t)row0 + (r < R ? r : 0);
        if (r < R && pos <= pos0 + (int)(rowi >> lnh)) {
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

// scores + P.V of the exact prompt pass on the matrix cores; non-zero = geometry not covered (the caller keeps the vector kernels)
int kr_pfm_gqa_exact_mfma_ok(const KrPfmGqaArgs& a) {
    const int group = a.nkv > 0 ? a.nh / a.nkv : 0;
    return group >= 1 && group <= 32 && (32 % group) == 0 && a.nh % a.nkv == 0 && (a.hd == 64 || a.hd == 128 || a.hd == 256);
}
void kr_launch_pfm_gqa_scores_mfma(const KrPfmGqaArgs& a, int C, float* sc, int sc_ld, float* tmax, hipStream_t st) {
    const int group = a.nh / a.nkv, TT = 64 / group;
    const dim3 grid((a.pos0 + C + 63) / 64, (C + TT - 1) / TT, a.nkv);
    if (a.kv_fp8) hipLaunchKernelGGL(kr_pfm_gqa_scores_mfma_kernel<true>, grid, dim3(256), 0, st, a, sc, sc_ld, C, tmax);
    else hipLaunchKernelGGL(kr_pfm_gqa_scores_mfma_kernel<false>, grid, dim3(256), 0, st, a, sc, sc_ld, C, tmax);
}
void kr_launch_pfm_gqa_pv_mfma(const KrPfmGqaArgs& a, int C, const float* sc, int sc_ld, const float* inv, hipStream_t st) {
    const int group = a.nh / a.nkv, TT = 32 / group;
    const dim3 grid((C + TT - 1) / TT, a.nkv);
#define KR_XPV(F_, H_, P_) hipLaunchKernelGGL((kr_pfm_gqa_pv_mfma_kernel<F_, H_, P_>), grid, dim3(256), 0, st, a, sc, sc_ld, C, inv)
    if (a.hd == 512) { if (a.kv_fp8) KR_XPV(true, 512, 32); else KR_XPV(false, 512, 32); }      // MLA latent rows (kr_launch_mla_exact_mfma)
    else if (a.hd == 256) { if (a.kv_fp8) KR_XPV(true, 256, 64); else KR_XPV(false, 256, 64); }
    else if (a.hd == 128) { if (a.kv_fp8) KR_XPV(true, 128, 64); else KR_XPV(false, 128, 64); }
    else { if (a.kv_fp8) KR_XPV(true, 64, 64); else KR_XPV(false, 64, 64); }
#undef KR_XPV
}
// MLA prompt pass: scores of n_tok tokens x nh heads against the latent + rope caches -> score scratch sc[n_tok * nh][sc_ld] + row maxima per 32
// positions; non-zero = geometry not covered (klr % 128, rd != 64, nh does not divide 32)
int kr_mla_exact_mfma_ok(int nh, int klr, int rd) { return nh >= 1 && nh <= 32 && (32 % nh) == 0 && (klr == 512 || klr == 256) && rd == 64; }
int kr_launch_mla_scores_mfma(const float* q_abs, const float* q_pe, const void* ckv, const void* kpe, int kv_fp8, int nh, int klr, int rd, int pos0, int n_tok,
                              float sm_scale, float* sc, int sc_ld, float* tmax, hipStream_t st) {
    if (!kr_mla_exact_mfma_ok(nh, klr, rd)) return 1;
    const int rows = n_tok * nh;
    const dim3 grid((pos0 + n_tok + 63) / 64, (rows + 63) / 64);
    if (klr % 64 || rd % 64) return 1;
#define KR_MS(F_, R_, Q_, C_, K_) hipLaunchKernelGGL((kr_mla_scores_mfma_kernel<F_, R_>), grid, dim3(256), 0, st, Q_, C_, nh, K_, pos0, rows, sm_scale, sc, sc_ld, tmax)
    if (kv_fp8) { KR_MS(true, true, q_pe, kpe, rd); KR_MS(true, false, q_abs, ckv, klr); }
    else { KR_MS(false, true, q_pe, kpe, rd); KR_MS(false, false, q_abs, ckv, klr); }
#undef KR_MS
    return 0;
}
