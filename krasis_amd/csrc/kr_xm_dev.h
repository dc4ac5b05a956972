// kr_xm_dev.h -- the bodies of passes A (scores) and C (P.V) of the EXACT attention on the f32 matrix cores, shared by the single-sequence prompt pass
// (kr_attn_exact_mfma.hip: one chunk of one flat cache at one pos0) and by a run of tokens entering a device slot under "multi_extend_exact_mfma"
// (kr_multi_xm.hip, docs/design/28-multi-extend-exact-mfma.md: a run of a batched pass over its slot, flat or paged).  One text, so both carry the same bits:
// what differs between the callers is where a token's row lies (Rows: token t of the chunk / run -> row of q_out, gate, attn_out, the score scratch and tmax)
// and where a position's cache row lies (PAGED: through the slot's row of the page table).  The arithmetic is described at the head of kr_attn_exact_mfma.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>

#include "kr_device.h"
#include "kr_libm.h"

typedef float xm_v16f __attribute__((ext_vector_type(16)));
typedef float xm_f4 __attribute__((ext_vector_type(4)));

#define XM_LDF 68          // floats per 64-float LDS row (272 B: consecutive rows 4 banks apart)

// one sequence's share of a pass: C tokens at positions pos0 .., their rows through Rows; the caches are the sequence's row 0 (flat) or the pools (PAGED)
struct KrXmSeq {
    const float* q_out; const float* gate; float* attn_out; const void* k_cache; const void* v_cache;
    int gated, nh, nkv, pos0, C; float sm_scale;
};
// the prompt pass: token t of the chunk is row t
struct KrXmRowsIdentity { __device__ __forceinline__ int operator()(int t) const { return t; } };
// cache row of position p.  PAGED: ptab = the slot's row of the page table, 1 << psh tokens a page; every page of the positions a tile reads was mapped by the
// host before the pass (-1 is clamped to page 0 all the same: a read, never a fault)
template <bool PAGED>
__device__ __forceinline__ size_t kr_xm_cache_row(int p, const int* ptab, int psh) {
    if constexpr (PAGED) return ((size_t)max(ptab[p >> psh], 0) << psh) | (size_t)(p & ((1 << psh) - 1));
    else return (size_t)p;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// pass A, one workgroup of 4 waves = 2 x 2 blocks of 32 queries x 32 positions: the position tile at p_lo, the query tile at token t0 (64 / group tokens) of KV
// head kvh.  A query row r of the tile is (token t0 + r / group, head kvh * group + r % group).  Qs, Ks: 64 * XM_LDF floats of LDS each.
// ------------------------------------------------------------------------------------------------------------------------------------
template <bool FP8, bool PAGED, class Rows>
__device__ __forceinline__ void kr_xm_scores_body(const KrXmSeq& a, int hd, int t0, int p_lo, int kvh, const Rows rows, const int* ptab, int psh,
                                                  float* __restrict__ sc, int sc_ld, float* __restrict__ tmax, float* Qs, float* Ks) {
    // group divides 32: a power of two -- tokens and heads of a row by shift and mask (a run-time integer division is ~50 instructions, and a lone wave
    // issues one per ~8 cycles: 16 rows x 2 divisions per lane were a third of a workgroup's life)
    const int group = a.nh / a.nkv, lg = __builtin_ctz(group), gm = group - 1, TT = 64 >> lg, kvs = a.nkv * hd, C = a.C;
    const int tn = min(TT, C - t0), R = group * tn;
    const int p_max = a.pos0 + t0 + tn - 1;          // last position any query of the tile may see
    if (p_lo > p_max) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r31 = lane & 31, kh = lane >> 5;
    const int rb = (wave >> 1) * 32, pb = (wave & 1) * 32;                    // this wave's block inside the tile
    xm_v16f acc[8];
#pragma unroll
    for (int j = 0; j < 8; j++)
#pragma unroll
        for (int i = 0; i < 16; i++) acc[j][i] = 0.0f;
    // staging: q 64 rows x 64 floats per stage (16 float4 per row, 4 per thread), K 64 positions x 64 values (positions past p_max re-read p_max:
    // their scores are never stored).  The next stage's requests are in flight during the MFMAs of the current one.
    const float* qsrc[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int u = tid + 256 * i, row = u >> 4, c4 = (u & 15) * 4;
        const int rr = row < R ? row : R - 1, tt = rr >> lg, hh = kvh * group + (rr & gm);
        qsrc[i] = a.q_out + (size_t)rows(t0 + tt) * a.nh * hd + (size_t)hh * hd + c4;
    }
    constexpr int KCH = FP8 ? 1 : 2;
    const char* ksrc[KCH];
#pragma unroll
    for (int i = 0; i < KCH; i++) {      // a thread's position is the same for every stage of the k loop: PAGED looks its page up once, here
        const int u = tid + 256 * i, prow = FP8 ? (u >> 2) : (u >> 3), off = FP8 ? (u & 3) * 16 : (u & 7) * 16;       // bytes inside the 64-value segment
        ksrc[i] = reinterpret_cast<const char*>(a.k_cache) + (kr_xm_cache_row<PAGED>(min(p_lo + prow, p_max), ptab, psh) * kvs + (size_t)kvh * hd) * (FP8 ? 1 : 2) + off;
    }
    xm_f4 qreg[4]; u32x4 kreg[KCH];
    auto load_stage = [&](int d0) {
#pragma unroll
        for (int i = 0; i < 4; i++) qreg[i] = *reinterpret_cast<const xm_f4*>(qsrc[i] + d0);
#pragma unroll
        for (int i = 0; i < KCH; i++) kreg[i] = *reinterpret_cast<const u32x4*>(ksrc[i] + (size_t)d0 * (FP8 ? 1 : 2));
    };
    auto commit_stage = [&]() {
#pragma unroll
        for (int i = 0; i < 4; i++) { const int u = tid + 256 * i, row = u >> 4, c4 = (u & 15) * 4; *reinterpret_cast<xm_f4*>(Qs + row * XM_LDF + c4) = qreg[i]; }
        if (FP8) {
            const uint32_t ww[4] = {kreg[0].x, kreg[0].y, kreg[0].z, kreg[0].w};
            float* dst = Ks + (tid >> 2) * XM_LDF + (tid & 3) * 16;
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
                *reinterpret_cast<xm_f4*>(Ks + prow * XM_LDF + c8) = xm_f4{f[0], f[1], f[2], f[3]};
                *reinterpret_cast<xm_f4*>(Ks + prow * XM_LDF + c8 + 4) = xm_f4{f[4], f[5], f[6], f[7]};
            }
        }
    };
    load_stage(0);
    for (int d0 = 0; d0 < hd; d0 += 64) {
        __syncthreads();                                                      // the previous stage's readers are done
        commit_stage();
        if (d0 + 64 < hd) load_stage(d0 + 64);
        __syncthreads();
        const float* qp = Qs + (rb + r31) * XM_LDF + 8 * kh;
        const float* kp = Ks + (pb + r31) * XM_LDF + 8 * kh;
#pragma unroll
        for (int m = 0; m < 4; m++) {                                         // 16 consecutive d: the (b, b + 1) pair of every lane chain
            const xm_f4 q0 = *reinterpret_cast<const xm_f4*>(qp + 16 * m), q1 = *reinterpret_cast<const xm_f4*>(qp + 16 * m + 4);
            const xm_f4 k0 = *reinterpret_cast<const xm_f4*>(kp + 16 * m), k1 = *reinterpret_cast<const xm_f4*>(kp + 16 * m + 4);
            const float qa[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w}, ka[8] = {k0.x, k0.y, k0.z, k0.w, k1.x, k1.y, k1.z, k1.w};
#pragma unroll
            for (int j = 0; j < 8; j++) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[j], ka[j], acc[j], 0, 0, 0);
        }
    }
    // hsum8 of the reference (kr_hsum8: xor 4, xor 1, xor 2), * sm_scale, causal store; the maximum of every row over this block's 32
    // positions goes to tmax[row][32-position block] so that pass B finds the row maximum without another walk over the score scratch (the
    // scratch is the traffic of the exact attention: a 20 k-token context is 1.3 GB of scores per chunk and layer)
    const int pos = p_lo + pb + r31;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int r = rb + (i & 3) + 8 * (i >> 2) + 4 * kh;
        const float sv = ((acc[0][i] + acc[4][i]) + (acc[1][i] + acc[5][i])) + ((acc[2][i] + acc[6][i]) + (acc[3][i] + acc[7][i]));
        float mv = -__builtin_inff();
        size_t rowi = 0;
        if (r < R) {
            const int tt = r >> lg, hh = kvh * group + (r & gm);
            rowi = (size_t)rows(t0 + tt) * a.nh + hh;
            if (pos <= a.pos0 + t0 + tt) { mv = sv * a.sm_scale; sc[rowi * sc_ld + pos] = mv; }
        }
        if (tmax) {        // maximum over the 32 lanes of this lane half (the other half holds other rows)
            mv = kr_red16_max_f32(mv);                            // 4 DPP steps inside each 16-lane row, then one exchange between the two rows of the lane half
            mv = fmaxf(mv, __shfl_xor(mv, 16));
            if (r31 == 0 && r < R) tmax[rowi * (size_t)(sc_ld >> 5) + ((p_lo + pb) >> 5)] = mv;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// pass C, one workgroup of 4 waves: the query tile at token t0 (32 / group tokens) of KV head kvh; wave w owns the 32-dim blocks w * NB .. w * NB + NB - 1 of the
// head (NB = hd / 128, head_dim 64: waves 0 and 1 one block each).  PS positions per stage: probabilities (masked) as f32 and the raw V rows in LDS.
// Ps: 32 * (PS + 4) floats, Vs: PS * (HD * element size + 64) bytes of LDS.
// ------------------------------------------------------------------------------------------------------------------------------------
template <bool FP8, int HD, int PS, bool PAGED, class Rows>      // PS = positions per stage (64; 32 for the 512-wide latent rows of MLA: the V tile must fit the static LDS window)
__device__ __forceinline__ void kr_xm_pv_body(const KrXmSeq& a, int t0, int kvh, const Rows rows, const int* ptab, int psh, const float* __restrict__ sc, int sc_ld,
                                              const float* __restrict__ inv, float* Ps, char* Vs) {
    constexpr int ESZ = FP8 ? 1 : 2, VROW = HD * ESZ + 64;                    // bytes per V row in LDS (+ 64: the two k halves land 16 banks apart)
    constexpr int NB = HD >= 128 ? HD / 128 : 1, NW = HD >= 128 ? 4 : HD / 32;   // blocks per wave, waves that own blocks
    constexpr int VCH = PS * HD * ESZ / 16 / 256;                             // 16-byte V chunks per thread per stage
    constexpr int PLD = PS + 4, PPT = PS / 8;                                 // floats per P row in LDS; probabilities per thread (8 threads per row)
    static_assert(VCH >= 1 && (PPT == 4 || PPT == 8), "stage shape");
    const int group = a.nh / a.nkv, lg = __builtin_ctz(group), gm = group - 1, TT = 32 >> lg, kvs = a.nkv * HD, C = a.C;      // group: a power of two
    const int tn = min(TT, C - t0), R = group * tn, p_max = a.pos0 + t0 + tn - 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r31 = lane & 31, kh = lane >> 5;
    xm_v16f acc[NB];
#pragma unroll
    for (int b = 0; b < NB; b++)
#pragma unroll
        for (int i = 0; i < 16; i++) acc[b][i] = 0.0f;
    // staging maps: P row = tid >> 3 (32 rows), PPT positions per thread; V chunk u = tid + 256 i: row u / CPR, 16-byte chunk u % CPR
    const int prow = tid >> 3, pseg = (tid & 7) * PPT;
    const int ptt = (prow < R ? prow : 0) >> lg, pg = (prow < R ? prow : 0) & gm, qpos = a.pos0 + t0 + ptt;
    const float* prow_p = sc + ((size_t)rows(t0 + ptt) * a.nh + (size_t)kvh * group + pg) * sc_ld;
    // pass B left the exponentials unscaled (inv != nullptr): p = e * (1 / sum) is formed here, the multiply the reference does in place (decode.rs:4260)
    const float iv = inv ? inv[(size_t)rows(t0 + ptt) * a.nh + (size_t)kvh * group + pg] : 1.0f;
    constexpr int CPR = HD * ESZ / 16;                                        // chunks per V row
    xm_f4 pp[PPT / 4]; u32x4 pv[VCH];
    auto load_stage = [&](int p0) {
#pragma unroll
        for (int q = 0; q < PPT / 4; q++) pp[q] = *reinterpret_cast<const xm_f4*>(prow_p + p0 + pseg + 4 * q);
#pragma unroll
        for (int i = 0; i < VCH; i++) {      // PAGED: the page of every row of the stage is looked up with the stage's loads, one stage ahead of its use
            const int u = tid + 256 * i, vr = u / CPR, vc = u % CPR;
            const int pos = min(p0 + vr, p_max);
            pv[i] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(a.v_cache) + (kr_xm_cache_row<PAGED>(pos, ptab, psh) * kvs + (size_t)kvh * HD) * ESZ + vc * 16);
        }
    };
    auto commit_stage = [&](int p0) {
#pragma unroll
        for (int q = 0; q < PPT / 4; q++) {
            const float e[4] = {pp[q].x, pp[q].y, pp[q].z, pp[q].w};
            float m[4];
#pragma unroll
            for (int j = 0; j < 4; j++) m[j] = (prow < R && p0 + pseg + 4 * q + j <= qpos) ? (inv ? e[j] * iv : e[j]) : 0.0f;      // select first: the scratch past qpos is not initialised
            *reinterpret_cast<xm_f4*>(Ps + prow * PLD + pseg + 4 * q) = xm_f4{m[0], m[1], m[2], m[3]};
        }
#pragma unroll
        for (int i = 0; i < VCH; i++) { const int u = tid + 256 * i, vr = u / CPR, vc = u % CPR; *reinterpret_cast<u32x4*>(Vs + vr * VROW + vc * 16) = pv[i]; }
    };
    load_stage(0);
    for (int p0 = 0; p0 <= p_max; p0 += PS) {
        __syncthreads();                                                      // the previous stage's readers are done
        commit_stage(p0);
        if (p0 + PS <= p_max) load_stage(p0 + PS);                            // in flight during the MFMAs below
        __syncthreads();
        if (wave < NW) {
            const int np = min(PS, p_max + 1 - p0);                           // positions of this stage any query may see
            const float* pr = Ps + r31 * PLD + kh;
            const char* vb = Vs + kh * VROW + (size_t)(wave * NB * 32 + r31) * ESZ;
#pragma unroll 4
            for (int s2 = 0; s2 < PS / 2; s2++) {                             // k = positions 2 s2 (lane half 0) and 2 s2 + 1 (lane half 1), ascending
                if (2 * s2 >= np) break;
                const float pa = pr[2 * s2];
#pragma unroll
                for (int b = 0; b < NB; b++) {
                    float v;
                    if (FP8) v = kr_e4m3_to_f32(*reinterpret_cast<const uint8_t*>(vb + 2 * s2 * VROW + b * 32));
                    else v = __half2float(__ushort_as_half(*reinterpret_cast<const uint16_t*>(vb + 2 * s2 * VROW + b * 64)));
                    acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(pa, v, acc[b], 0, 0, 0);
                }
            }
        }
    }
    if (wave >= NW) return;
#pragma unroll
    for (int b = 0; b < NB; b++)
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int r = (i & 3) + 8 * (i >> 2) + 4 * kh;
            if (r < R) {
                const int tt = r >> lg, hh = kvh * group + (r & gm);
                float o = acc[b][i];
                const size_t oi = (size_t)rows(t0 + tt) * a.nh * HD + (size_t)hh * HD + (size_t)(wave * NB + b) * 32 + r31;
                if (a.gated) { const float gt = a.gate[oi]; o *= 1.0f / (1.0f + kr_expf(-gt)); }
                a.attn_out[oi] = o;
            }
        }
}
