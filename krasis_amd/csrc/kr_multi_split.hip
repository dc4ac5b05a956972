// kr_multi_split.hip -- "multi_attn_exact_split" (docs/design/30-multi-attn-exact-split.md): the attention of kr_multi_gqa_attn_kernel (kr_multi.hip) as three
// launches behind the unchanged prep launch, bit for bit that kernel's result for every row:
//   1  scores   grid (position tile, KV head, row): a score depends on its own position alone, so any split over positions keeps it -- per position the 8-lane
//               fma chains over elements e * 8 + l (ascending e), kr_hsum8, * sm_scale.  The K rows come through LDS in 16-byte loads
//   2  softmax  one wave per (row, query head): kr_m_wave_softmax as it stands
//   3  P.V      grid (KV head x head-dim slice, row): output (g, d) is one fma per position, ascending, from 0.0f; the split is over d and heads, never over
//               positions.  The V rows come through LDS in 16-byte loads
// They read and write the score scratch a.scores[row][nh][sc_ld] exactly as that kernel does.  E4M3 -> f32 and f16 -> f32 are exact, so where a cache element is
// widened (on the way out of LDS, or into it) changes nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kr_device.h"
#include "kr_libm.h"
#include "kr_exact_dev.h"
#include "kr_multi.h"
#include "kr_multi_softmax_dev.h"

#define KR_MS_TILE 256      // positions per scores workgroup (= kr_gqa_attn_kernel's PHASE 1 tile)
#define KR_MS_KROWS 32      // K rows per LDS stage: one position per 8-lane group of the 256 threads; never straddles a page (KR_PAGE_MIN_TOKENS)
#define KR_MS_PT 64         // positions per P.V stage
#define KR_MS_DS 32         // outputs d per P.V workgroup
#define KR_MS_VLD 68        // floats per staged V column: KR_MS_PT positions and four of padding (16-byte aligned columns, 16 lanes of a 16-byte read on 64 banks)
#define KR_MS_TPD 8         // threads per output column of the P.V workgroup (256 / KR_MS_DS)
#define KR_MS_ACC 4         // heads per thread and pass of the P.V loop (32 heads a pass)

// byte offset of (position s, KV head kvh) of the row's slot in a cache of ESZ-byte elements.  PAGED: through the slot's table slice, one entry per call -- a
// workgroup reads only the entries of the positions it loads (every page of [0, seq) was mapped by the host before the pass: max(., 0) as in the unsplit kernel)
template <int HD, int ESZ, bool PAGED>
__device__ __forceinline__ size_t kr_ms_row_off(const KrMultiGqaArgs& a, int slot, int kvh, int s) {
    const size_t kvs = (size_t)a.nkv * HD;
    if constexpr (PAGED) {
        const int pg = max(a.page_table[(size_t)slot * a.page_stride + (s >> a.page_shift)], 0);
        return ((((size_t)pg << a.page_shift) | (size_t)(s & ((1 << a.page_shift) - 1))) * kvs + (size_t)kvh * HD) * ESZ;
    } else return ((size_t)slot * a.slot_elems + (size_t)s * kvs + (size_t)kvh * HD) * ESZ;
}
template <bool FP8> __device__ __forceinline__ float kr_ms_elem(const unsigned char* row, int i) {
    if (FP8) return kr_e4m3_to_f32(row[i]);
    _Float16 hv; __builtin_memcpy(&hv, row + 2 * i, 2);
    return (float)hv;
}
// element j of a 16-byte chunk held in registers (j a constant after unrolling: shifts, no addressing)
template <bool FP8> __device__ __forceinline__ float kr_ms_chunk_elem(const u32x4& r, int j) {
    if (FP8) return kr_e4m3_to_f32((uint8_t)(r[j >> 2] >> (8 * (j & 3))));
    return (float)__builtin_bit_cast(_Float16, (uint16_t)(r[j >> 1] >> (16 * (j & 1))));
}

// ---- 1: scores.  grid (ceil(sc_ld / KR_MS_TILE), nkv, rows), 256 threads; dynamic LDS = the G query rows f32, [G][8][NB + 4], + one stage of KR_MS_KROWS raw K rows.
// A stage is fetched by all 256 threads, 16 bytes each (NLD loads per thread), the next stage's loads issued before the current one is consumed.  Bounds: a row
// s is loaded only for s < min(seq, tile end), seq = pos + 1 <= the slot's capacity; the 16-byte chunks c < CPR tile the head's HD * ESZ bytes of that row exactly;
// scores are written for those s only, s < seq <= sc_ld.  Workgroups past the row's position, and the rows of the run kernels, leave ahead of every barrier
template <int NB, bool FP8, bool PAGED>
__global__ void __launch_bounds__(256) kr_multi_split_scores_kernel(const KrMultiGqaArgs a) {
    constexpr int HD = NB * 8, ESZ = FP8 ? 1 : 2, RB = HD * ESZ, CPR = RB / 16, PITCH = RB + 16, NLD = (KR_MS_KROWS * CPR + 255) / 256, QLD = NB + 4;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int kvh = blockIdx.y, row = blockIdx.z, t = threadIdx.x;
    if (kr_m_row_in_run(a, row)) return;      // the run kernels' row (workgroup-uniform, ahead of every barrier)
    const int seq = a.positions[row] + 1, t0 = blockIdx.x * KR_MS_TILE;
    if (t0 >= seq) return;                    // (workgroup-uniform, ahead of every barrier)
    const int tend = min(seq, t0 + KR_MS_TILE), G = a.nh / a.nkv, slot = a.slots[row];
    float* qs = sm;                                                             // [G][8][QLD]: lane l's elements e * 8 + l of a head side by side, for 16-byte reads
    unsigned char* stage = reinterpret_cast<unsigned char*>(qs + (size_t)G * 8 * QLD);      // [KR_MS_KROWS][PITCH]
    const unsigned char* kc = reinterpret_cast<const unsigned char*>(a.k_cache);
    u32x4 rg[NLD];
    auto issue = [&](int s0) {
#pragma unroll
        for (int i = 0; i < NLD; i++) {
            const int u = t + 256 * i, r = u / CPR, c = u % CPR;
            if (u < KR_MS_KROWS * CPR && s0 + r < tend) rg[i] = *reinterpret_cast<const u32x4*>(kc + kr_ms_row_off<HD, ESZ, PAGED>(a, slot, kvh, s0 + r) + c * 16);
        }
    };
    auto commit = [&](int s0) {
#pragma unroll
        for (int i = 0; i < NLD; i++) {
            const int u = t + 256 * i, r = u / CPR, c = u % CPR;
            if (u < KR_MS_KROWS * CPR && s0 + r < tend) *reinterpret_cast<u32x4*>(stage + r * PITCH + c * 16) = rg[i];
        }
    };
    issue(t0);
    const float* q = a.q_out + (size_t)row * a.nh * HD + (size_t)kvh * G * HD;
    for (int i = t; i < G * HD; i += 256) qs[((i / HD) * 8 + (i & 7)) * QLD + ((i % HD) >> 3)] = q[i];
    float* sc = a.scores + ((size_t)row * a.nh + (size_t)kvh * G) * a.sc_ld;        // [G][sc_ld]
    const int l = t & 7, grp = t >> 3;
    for (int s0 = t0; s0 < tend; s0 += KR_MS_KROWS) {
        __syncthreads();      // the stage before this one is consumed
        commit(s0);
        if (s0 + KR_MS_KROWS < tend) issue(s0 + KR_MS_KROWS);
        __syncthreads();      // (first stage: also the query rows)
        const int s = s0 + grp;
        if (s < tend) {       // whole 8-lane groups
            const unsigned char* kr_row = stage + grp * PITCH;
            float kr[NB];
#pragma unroll
            for (int e = 0; e < NB; e++) kr[e] = kr_ms_elem<FP8>(kr_row, e * 8 + l);
            for (int g = 0; g < G; g++) {
                const float* qg = qs + (g * 8 + l) * QLD;
                float acc = 0.0f;
#pragma unroll
                for (int e = 0; e < NB; e += 4) {
                    const float4 q4 = *reinterpret_cast<const float4*>(qg + e);
                    acc = __builtin_fmaf(q4.x, kr[e], acc); acc = __builtin_fmaf(q4.y, kr[e + 1], acc);
                    acc = __builtin_fmaf(q4.z, kr[e + 2], acc); acc = __builtin_fmaf(q4.w, kr[e + 3], acc);
                }
                acc = kr_hsum8(acc);
                if (l == 0) sc[(size_t)g * a.sc_ld + s] = acc * a.sm_scale;
            }
        }
    }
}

// ---- 2: softmax.  grid (ceil(nh / 4), rows), 256 threads: wave w takes query head 4 x + w of the row.  kr_m_wave_softmax holds workgroup barriers, as many as
// seq has tiles: the four waves of a workgroup belong to one row, so they share seq and pass the same barriers; a wave past the last head calls it with on =
// false on the row of head 0 (a valid pointer it never dereferences).  The run kernels' rows leave ahead of the call, the whole workgroup at once
__global__ void __launch_bounds__(256) kr_multi_split_softmax_kernel(const KrMultiGqaArgs a) {
    __shared__ __attribute__((aligned(16))) float tile[4 * KR_MG_TILE];
    const int row = blockIdx.y, t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (kr_m_row_in_run(a, row)) return;
    const int seq = a.positions[row] + 1, h = blockIdx.x * 4 + w;
    const bool on = h < a.nh;
    kr_m_wave_softmax(a.scores + ((size_t)row * a.nh + (size_t)(on ? h : 0)) * a.sc_ld, seq, tile + w * KR_MG_TILE, on, lane);
}

// ---- 3: P.V.  grid (nkv * HD / KR_MS_DS, rows), 256 threads: thread t owns output d0 + t % 32 of heads t / 32 + 8 k; one fma per position, ascending, from 0.0f;
// positions past the row's are skipped, not multiplied by zero; a gated layer's sigmoid gate at the end -- the unsplit kernel's statements.  Dynamic LDS = the
// probabilities of a stage [G][KR_MS_PT]; static: the stage's V slice widened to f32 and transposed, [KR_MS_DS][KR_MS_VLD] -- a thread reads four positions of its
// column, and four probabilities of a head, per 16-byte LDS read.  A stage is fetched 16 bytes per thread (at most one load each) and its first 512 probabilities
// two per thread, the next stage's loads issued before the current one is consumed.  Bounds: a V row s is loaded only for s < seq; the chunks c < CPS tile the 32 d
// of this slice exactly; probabilities are read for s < seq <= sc_ld only
// one stage of the chains of K heads (p0: the first one's probabilities, the others KR_MS_TPD rows further each) over column vrow: n positions, ascending
template <int K>
__device__ __forceinline__ void kr_ms_pv_stage(float (&o)[KR_MS_ACC], const float* p0, const float* vrow, int n) {
    int s1 = 0;
    for (; s1 + 8 <= n; s1 += 8) {
        const float4 va = *reinterpret_cast<const float4*>(vrow + s1), vb = *reinterpret_cast<const float4*>(vrow + s1 + 4);
#pragma unroll
        for (int k = 0; k < K; k++) {
            const float4 pa = *reinterpret_cast<const float4*>(p0 + k * KR_MS_TPD * KR_MS_PT + s1), pb = *reinterpret_cast<const float4*>(p0 + k * KR_MS_TPD * KR_MS_PT + s1 + 4);
            float x = o[k];
            x = __builtin_fmaf(pa.x, va.x, x); x = __builtin_fmaf(pa.y, va.y, x); x = __builtin_fmaf(pa.z, va.z, x); x = __builtin_fmaf(pa.w, va.w, x);
            x = __builtin_fmaf(pb.x, vb.x, x); x = __builtin_fmaf(pb.y, vb.y, x); x = __builtin_fmaf(pb.z, vb.z, x); x = __builtin_fmaf(pb.w, vb.w, x);
            o[k] = x;
        }
    }
    for (; s1 < n; s1++) {      // the last, partial group of the row (once per launch)
        const float v = vrow[s1];
#pragma unroll
        for (int k = 0; k < K; k++) o[k] = __builtin_fmaf(p0[k * KR_MS_TPD * KR_MS_PT + s1], v, o[k]);
    }
}
template <int NB, bool FP8, bool PAGED>
__global__ void __launch_bounds__(256) kr_multi_split_pv_kernel(const KrMultiGqaArgs a) {
    constexpr int HD = NB * 8, ESZ = FP8 ? 1 : 2, NSL = HD / KR_MS_DS, CPS = KR_MS_DS * ESZ / 16, EPC = 16 / ESZ;      // chunks per row slice, elements per chunk
    extern __shared__ __attribute__((aligned(16))) float pt[];                  // [G][KR_MS_PT]
    __shared__ __attribute__((aligned(16))) float vs[KR_MS_DS * KR_MS_VLD];     // [d][position]
    const int kvh = blockIdx.x / NSL, d0 = (blockIdx.x % NSL) * KR_MS_DS, row = blockIdx.y, t = threadIdx.x;
    if (kr_m_row_in_run(a, row)) return;      // the run kernels' row (workgroup-uniform, ahead of every barrier)
    const int seq = a.positions[row] + 1, G = a.nh / a.nkv, slot = a.slots[row];
    const unsigned char* vc = reinterpret_cast<const unsigned char*>(a.v_cache);
    const float* sc = a.scores + ((size_t)row * a.nh + (size_t)kvh * G) * a.sc_ld;
    const int lr = t / CPS, lc = t % CPS;      // this thread's row and chunk of a stage
    const bool loader = t < KR_MS_PT * CPS;
    const int ps = t % KR_MS_PT, pg = t / KR_MS_PT;      // this thread's two probabilities of a stage: position ps of heads pg and pg + 4
    u32x4 rg = {0, 0, 0, 0};
    float pr0 = 0.0f, pr1 = 0.0f;
    auto issue = [&](int s0) {
        if (loader && s0 + lr < seq) rg = *reinterpret_cast<const u32x4*>(vc + kr_ms_row_off<HD, ESZ, PAGED>(a, slot, kvh, s0 + lr) + (size_t)d0 * ESZ + lc * 16);
        if (s0 + ps < seq) {
            if (pg < G) pr0 = sc[(size_t)pg * a.sc_ld + s0 + ps];
            if (pg + 4 < G) pr1 = sc[(size_t)(pg + 4) * a.sc_ld + s0 + ps];
        }
    };
    auto commit = [&](int s0, int n) {
        if (loader && s0 + lr < seq) {
            float* dst = vs + lc * EPC * KR_MS_VLD + lr;
#pragma unroll
            for (int j = 0; j < EPC; j++) dst[j * KR_MS_VLD] = kr_ms_chunk_elem<FP8>(rg, j);
        }
        if (pg < G) pt[pg * KR_MS_PT + ps] = ps < n ? pr0 : 0.0f;
        if (pg + 4 < G) pt[(pg + 4) * KR_MS_PT + ps] = ps < n ? pr1 : 0.0f;
        for (int i = t + 512; i < G * KR_MS_PT; i += 256) { const int g = i / KR_MS_PT, s = i % KR_MS_PT; pt[i] = s < n ? sc[(size_t)g * a.sc_ld + s0 + s] : 0.0f; }
    };
    const int dl = t % KR_MS_DS, hg = t / KR_MS_DS;      // heads are dealt round-robin over the KR_MS_TPD threads of an output column
    const float* vrow = vs + dl * KR_MS_VLD;
    const float* gate = a.gate + (size_t)row * a.nh * HD + (size_t)kvh * G * HD;
    float* out = a.attn_out + (size_t)row * a.nh * HD + (size_t)kvh * G * HD;
    for (int gp = 0; gp < G; gp += KR_MS_ACC * KR_MS_TPD) {      // heads gp + hg + k * KR_MS_TPD, k < KR_MS_ACC
        const int ka = min(KR_MS_ACC, max(0, (G - gp - hg + KR_MS_TPD - 1) / KR_MS_TPD));      // this thread's heads in this pass
        const float* p0 = pt + (gp + hg) * KR_MS_PT;
        float o[KR_MS_ACC];
#pragma unroll
        for (int k = 0; k < KR_MS_ACC; k++) o[k] = 0.0f;
        issue(0);
        for (int s0 = 0; s0 < seq; s0 += KR_MS_PT) {
            const int n = min(KR_MS_PT, seq - s0);
            __syncthreads();      // the stage before this one is consumed
            commit(s0, n);
            if (s0 + KR_MS_PT < seq) issue(s0 + KR_MS_PT);
            __syncthreads();
            if (ka == 1) kr_ms_pv_stage<1>(o, p0, vrow, n);
            else if (ka == 4) kr_ms_pv_stage<4>(o, p0, vrow, n);
            else if (ka == 2) kr_ms_pv_stage<2>(o, p0, vrow, n);
            else if (ka == 3) kr_ms_pv_stage<3>(o, p0, vrow, n);
        }
#pragma unroll
        for (int k = 0; k < KR_MS_ACC; k++) {
            const int g = gp + hg + k * KR_MS_TPD;
            if (g < G) {
                float ov = o[k];
                if (a.gated) { const float gt = gate[(size_t)g * HD + d0 + dl]; ov *= 1.0f / (1.0f + kr_expf(-gt)); }
                out[(size_t)g * HD + d0 + dl] = ov;
            }
        }
    }
}

size_t kr_multi_split_lds_bytes(int G, int hd, int kv_fp8) {      // the scores launch's dynamic LDS, the largest of the three
    return (size_t)G * (hd + 32) * 4 + (size_t)KR_MS_KROWS * (hd * (kv_fp8 ? 1 : 2) + 16);
}

// the three launches over `rows` rows of the pass (after the prep launch).  The caller has made kr_launch_multi_gqa's checks (hd 64 / 128 / 256, nh % nkv == 0,
// sc_ld % 32 == 0, the page fields, the unsplit kernel's LDS bound -- a call refused with the option off is refused the same way with it on).  Under that bound the
// LDS asked here fits the default window: G (hd + 32) 4 + 32 (hd esz + 16) <= G hd 4 + 128 G + 16896, against the unsplit kernel's G hd 4 + 16384 + 256 G (+ the
// table) for G >= 4, and 20352 bytes at most for G < 4; the P.V launch asks 256 G + 8704
int kr_launch_multi_gqa_split(const KrMultiGqaArgs& a, int rows, hipStream_t st) {
    if ((a.hd != 64 && a.hd != 128 && a.hd != 256) || a.nkv < 1 || a.nh % a.nkv || a.sc_ld < 32 || a.sc_ld % 32 || rows < 1) return 1;
    if (a.page_table && (a.page_stride < 1 || a.page_shift < 5)) return 1;
    const int G = a.nh / a.nkv;
    const size_t lds_s = kr_multi_split_lds_bytes(G, a.hd, a.kv_fp8), lds_p = (size_t)G * KR_MS_PT * 4;
    if (lds_s > 64 * 1024 || lds_p + sizeof(float) * KR_MS_DS * KR_MS_VLD > 64 * 1024) return 1;
    const dim3 gs((a.sc_ld + KR_MS_TILE - 1) / KR_MS_TILE, a.nkv, rows), gm((a.nh + 3) / 4, rows), gp(a.nkv * (a.hd / KR_MS_DS), rows);
#define KR_MSL(NB_, F_, P_) do { \
        hipLaunchKernelGGL((kr_multi_split_scores_kernel<NB_, F_, P_>), gs, dim3(256), lds_s, st, a); \
        hipLaunchKernelGGL(kr_multi_split_softmax_kernel, gm, dim3(256), 0, st, a); \
        hipLaunchKernelGGL((kr_multi_split_pv_kernel<NB_, F_, P_>), gp, dim3(256), lds_p, st, a); } while (0)
#define KR_MSL_HD(F_, P_) do { if (a.hd == 256) KR_MSL(32, F_, P_); else if (a.hd == 128) KR_MSL(16, F_, P_); else KR_MSL(8, F_, P_); } while (0)
    if (a.page_table) { if (a.kv_fp8) KR_MSL_HD(true, true); else KR_MSL_HD(false, true); }
    else { if (a.kv_fp8) KR_MSL_HD(true, false); else KR_MSL_HD(false, false); }
#undef KR_MSL_HD
#undef KR_MSL
    return 0;
}
