// kr_pfm_flash_dev.h -- causal flash attention of one query tile of a prompt run, shared by two callers: the store's own KR_ATTN_FAST prompt pass
// (kr_attn_flash.hip) and a run of tokens entering a device slot under "multi_extend_flash" (kr_multi_pf_flash.hip), so that a run of a batched pass carries the
// bits of the single-sequence fast prompt pass (docs/design/25-multi-extend-flash.md).  The four-wave form (head_dim 64) is one KERNEL template,
// kr_pfm_gqa_flash_kernel<HD, FP8, Tiles>, which both callers instantiate with their own tile source; the wave-specialised form (head_dim 128 / 256) is a device
// function, kr_pfm_flashw_body, called by kr_pfm_gqa_flashw_kernel and kr_multi_pf_flashw_kernel.  The callers differ only in where the tile, its query rows, the
// cache rows and the outputs come from.  The layout of the computation is described in kr_attn_flash.hip.
#pragma once
#include <type_traits>
#include "kr_device.h"
#include "kr_libm.h"
#include "kr_fd_flash_dev.h"

#define FA_ROWS 128
#ifdef KR_TIMING   // tools/probes/flash_timing.hip: wall-clock stamps (10 ns units) of wave 0 of workgroup (0, 0) at one tile; no-op in the product build
__device__ unsigned long long kr_fstamps[32];
#define FA_STAMP(i) do { if (threadIdx.x == 0 && blockIdx.x == gridDim.x - 1 && blockIdx.y == 0 && tile == 40) kr_fstamps[i] = wall_clock64(); } while (0)
#define FA_STAMP2(i) do { if (threadIdx.x == 256 && blockIdx.x == gridDim.x - 1 && blockIdx.y == 0 && tile == 40) kr_fstamps[i] = wall_clock64(); } while (0)
#else
#define FA_STAMP(i) do { } while (0)
#define FA_STAMP2(i) do { } while (0)
#endif

// One query tile: tokens t0 .. t0 + 128 / G - 1 of a run of C tokens whose first token stands at position a.pos0, against KV head kvh.  Token t of the run is row
// row_of(t) of a.q_out / a.gate / a.attn_out ([rows][nh * HD]); the keys and values are rows [0, pos0 + min(t0 + 128 / G, C)) of a.k_cache / a.v_cache
// ([position][nkv * HD], FP16 or E4M3), the run's own rows among them.  `a` of kr_pfm_flashw_body is any structure with these members: the prompt pass hands its
// kernel argument on as it is (KrPfmGqaArgs), a batched pass fills this one per workgroup
struct KrPfFlashTile {
    const float *q_out, *gate; float* attn_out;
    const void *k_cache, *v_cache;
    int gated, nh, nkv, pos0; float sm_scale;
};
// dynamic LDS of the two forms in bytes (the launchers of both callers ask here)
inline size_t kr_pfm_flash_lds(int hd) { return (size_t)FA_TK * (hd * 2 + 16) + (size_t)hd * (FA_TK * 2 + 16); }
inline size_t kr_pfm_flashw_lds(int hd) { return (size_t)FA_TK * (hd * 2 + 16) + 2 * (size_t)FA_TK * (hd * 2 + 64) + 2 * (size_t)FA_ROWS * (FA_TK * 2 + 16) + 3 * FA_ROWS * 4; }
// the single-sequence prompt pass: token t of the chunk is row t (the wave-specialised body's row map)
struct KrPfRowsIdentity { __device__ __forceinline__ int operator()(int t) const { return t; } };

// PAGED (as kr_fd_flash_body, docs/design/23-multi-attn-fast-paged.md): k_cache / v_cache are pools of pages of 1 << psh positions (psh >= 5) and position p of
// the sequence is row (ptab[p >> psh] << psh) | (p & mask) of them.  A tile of FA_TK positions starts at a multiple of FA_TK, so it lies in one page, or in two
// at 32 positions per page.  lo = the byte offset of the page of p0 .. p0 + 31, hi = that of the page of min(p0 + 32, kv_end - 1), which holds every position of
// rows 32 .. 63 that is loaded, clamped ones included.  Both positions lie in [0, kv_end): the host mapped their pages before the pass; -1 is never turned into
// an address all the same.  The ids are workgroup-uniform and stay in scalar registers
__device__ __forceinline__ void kr_pf_tile_pages(const int* ptab, int psh, int p0, int kv_end, size_t rowb, size_t& lo, size_t& hi) {
    const int i0 = __builtin_amdgcn_readfirstlane(max(ptab[p0 >> psh], 0)), i1 = __builtin_amdgcn_readfirstlane(max(ptab[min(p0 + 32, kv_end - 1) >> psh], 0));
    lo = ((size_t)i0 << psh) * rowb; hi = ((size_t)i1 << psh) * rowb;
}

// ---- the four-wave form (head_dim 64): 256 threads, grid (tiles, nkv), dynamic LDS FA_TK * (HD * 2 + 16) + HD * (FA_TK * 2 + 16) bytes.
// This form is ONE KERNEL TEMPLATE for both callers, not an inlined device function: compiled as a callee inlined into a one-line kernel the register
// allocator splits the same text differently (130 + 64 instead of 158 + 32 VGPRs + AGPRs, the E4M3 instantiation 2 instead of 3 waves per SIMD), as a kernel of
// its own it keeps the allocation it always had.  Tiles says where the workgroup's tile lies: its argument structure Tiles::Args (with the members q_out, gate,
// attn_out, k_cache, v_cache, gated, nh, nkv, sm_scale), constructed from (a, Ck, tokens per tile) with C, t0, pos0, row(t) = the row of token t, and, for
// Tiles::SLOTS, cache_off = bytes to the sequence's row 0, for Tiles::PAGED, ptab / psh.  KrPfChunkTiles (kr_attn_flash.hip): the prompt pass's chunk, every
// member a compile-time identity, Ck = the chunk's tokens; KrPfSlotTiles<FP8, PAGED> (kr_multi_pf_flash.hip): a run of a batched pass, from its tile table
template <int HD, bool FP8, class Tiles>
__global__ void __launch_bounds__(256) kr_pfm_gqa_flash_kernel(const typename Tiles::Args a, int Ck) {
    constexpr bool PAGED = Tiles::PAGED;
    constexpr int KSTEPS = HD / 16, DB = HD / 32, LDK = HD * 2 + 16, LDV = FA_TK * 2 + 16;
    constexpr int CPR = FP8 ? HD / 16 : HD / 8;                 // 16-byte global chunks per cache row
    constexpr int KCH = FA_TK * CPR / 256;                      // K chunks per thread per tile  (>= 1 for HD >= 64)
    constexpr int VUN = (FA_TK / 2) * CPR;                      // V units (position pair x chunk) per tile
    constexpr int VPT = (VUN + 255) / 256;
    extern __shared__ __attribute__((aligned(16))) char fa_smem[];
    char* Ks = fa_smem;                                         // [64 positions][LDK]   f16
    char* Vt = fa_smem + FA_TK * LDK;                           // [HD dims][LDV]        f16, positions contiguous
    const int G = a.nh / a.nkv, TQ = FA_ROWS / G;
    const Tiles tl(a, Ck, TQ);
    const int kvh = blockIdx.y, t0 = tl.t0, C = tl.C;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n31 = lane & 31, khalf = lane >> 5;
    const int r = wave * 32 + n31, hl = r / TQ, ti = r % TQ, tok = t0 + ti;
    const bool row_ok = tok < C;
    const int h = kvh * G + hl, p_q = tl.pos0 + tok;
    const int kvs = a.nkv * HD, esz = FP8 ? 1 : 2;
    const int kv_end = tl.pos0 + (t0 + TQ < C ? t0 + TQ : C);     // positions [0, kv_end) are visible to some row of the tile
    const int n_tiles = (kv_end + FA_TK - 1) / FA_TK;
    const int full_vis = tl.pos0 + t0;                            // positions <= full_vis are visible to EVERY row

    // ---- Q^T fragments (B operand): row = this lane's query, k = dims 16 ks + 8 khalf + i; scale and log2(e) folded in, rounded to f16
    v8h qf[KSTEPS];
    {
        const float* q = a.q_out + ((size_t)tl.row(row_ok ? tok : 0) * a.nh + h) * HD + 8 * khalf;
        const float sc = a.sm_scale * 1.4426950408889634f;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ks++) {
            const float4 x0 = *reinterpret_cast<const float4*>(q + 16 * ks), x1 = *reinterpret_cast<const float4*>(q + 16 * ks + 4);
            const float xv[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
            for (int i = 0; i < 8; i++) qf[ks][i] = (_Float16)(row_ok ? xv[i] * sc : 0.0f);
        }
    }
    v16f oacc[DB];
#pragma unroll
    for (int db = 0; db < DB; db++)
#pragma unroll
        for (int i = 0; i < 16; i++) oacc[db][i] = 0.0f;
    float m_run = -__builtin_inff(), l_run = 0.0f;

    // ---- tile staging: global -> registers (issued one tile ahead) -> LDS
    const unsigned char* kc = reinterpret_cast<const unsigned char*>(a.k_cache) + (size_t)kvh * HD * esz;
    const unsigned char* vc = reinterpret_cast<const unsigned char*>(a.v_cache) + (size_t)kvh * HD * esz;
    if constexpr (Tiles::SLOTS) { kc += tl.cache_off; vc += tl.cache_off; }
    [[maybe_unused]] const size_t rowb = (size_t)kvs * esz;
    [[maybe_unused]] int pmask = 0;
    if constexpr (PAGED) pmask = (1 << tl.psh) - 1;
    u32x4 pk[KCH], pva[VPT], pvb[VPT];
    auto load_k = [&](int p0) {
        [[maybe_unused]] size_t lo = 0, hi = 0;
        if constexpr (PAGED) kr_pf_tile_pages(tl.ptab, tl.psh, p0, kv_end, rowb, lo, hi);
#pragma unroll
        for (int j = 0; j < KCH; j++) {
            const int c = tid + j * 256, row = c / CPR, dc = c % CPR, p = p0 + row;
            if constexpr (PAGED) pk[j] = p < kv_end ? *reinterpret_cast<const u32x4*>(kc + (row >= 32 ? hi : lo) + (size_t)(p & pmask) * rowb + dc * 16) : u32x4{0, 0, 0, 0};
            else pk[j] = p < kv_end ? *reinterpret_cast<const u32x4*>(kc + (size_t)p * kvs * esz + dc * 16) : u32x4{0, 0, 0, 0};
        }
    };
    auto load_v = [&](int p0) {
        [[maybe_unused]] size_t lo = 0, hi = 0;
        if constexpr (PAGED) kr_pf_tile_pages(tl.ptab, tl.psh, p0, kv_end, rowb, lo, hi);
#pragma unroll
        for (int j = 0; j < VPT; j++) {
            const int u = tid + j * 256, pp = u & 31, dc = u >> 5, p = p0 + 2 * pp;      // lanes walk the position pairs: conflict-free transposed LDS writes
            pva[j] = u32x4{0, 0, 0, 0}; pvb[j] = u32x4{0, 0, 0, 0};
            if (u < VUN) {
                if constexpr (PAGED) {      // p is even: p and p + 1 share a page
                    const unsigned char* ra = vc + (pp >= 16 ? hi : lo) + (size_t)(p & pmask) * rowb + dc * 16;
                    if (p < kv_end) pva[j] = *reinterpret_cast<const u32x4*>(ra);
                    if (p + 1 < kv_end) pvb[j] = *reinterpret_cast<const u32x4*>(ra + rowb);
                } else {
                    if (p < kv_end) pva[j] = *reinterpret_cast<const u32x4*>(vc + (size_t)p * kvs * esz + dc * 16);
                    if (p + 1 < kv_end) pvb[j] = *reinterpret_cast<const u32x4*>(vc + (size_t)(p + 1) * kvs * esz + dc * 16);
                }
            }
        }
    };
    auto commit_k = [&]() {
#pragma unroll
        for (int j = 0; j < KCH; j++) {
            const int c = tid + j * 256, row = c / CPR, dc = c % CPR;
            if (FP8) {
                const u32x4 w = pk[j];
                u32x4 lo = {fa_fp8x2_to_h2(w.x, false), fa_fp8x2_to_h2(w.x, true), fa_fp8x2_to_h2(w.y, false), fa_fp8x2_to_h2(w.y, true)};
                u32x4 hi = {fa_fp8x2_to_h2(w.z, false), fa_fp8x2_to_h2(w.z, true), fa_fp8x2_to_h2(w.w, false), fa_fp8x2_to_h2(w.w, true)};
                *reinterpret_cast<u32x4*>(Ks + row * LDK + dc * 32) = lo; *reinterpret_cast<u32x4*>(Ks + row * LDK + dc * 32 + 16) = hi;
            } else *reinterpret_cast<u32x4*>(Ks + row * LDK + dc * 16) = pk[j];
        }
    };
    auto commit_v = [&]() {
#pragma unroll
        for (int j = 0; j < VPT; j++) {
            const int u = tid + j * 256, pp = u & 31, dc = u >> 5;
            if (u < VUN) {
                uint32_t ha[8], hb[8];                    // f16 pairs of the two rows (FP16: 4 dwords each, FP8: 8 dwords each)
                constexpr int NW = FP8 ? 8 : 4;
                if (FP8) {
                    const uint32_t wa[4] = {pva[j].x, pva[j].y, pva[j].z, pva[j].w}, wb[4] = {pvb[j].x, pvb[j].y, pvb[j].z, pvb[j].w};
#pragma unroll
                    for (int m = 0; m < 4; m++) { ha[2 * m] = fa_fp8x2_to_h2(wa[m], false); ha[2 * m + 1] = fa_fp8x2_to_h2(wa[m], true);
                                                  hb[2 * m] = fa_fp8x2_to_h2(wb[m], false); hb[2 * m + 1] = fa_fp8x2_to_h2(wb[m], true); }
                } else {
                    ha[0] = pva[j].x; ha[1] = pva[j].y; ha[2] = pva[j].z; ha[3] = pva[j].w; hb[0] = pvb[j].x; hb[1] = pvb[j].y; hb[2] = pvb[j].z; hb[3] = pvb[j].w;
                }
                char* base = Vt + (size_t)(dc * (FP8 ? 16 : 8)) * LDV + fa_vslot(pp) * 4;
#pragma unroll
                for (int m = 0; m < NW; m++) {            // dims 2m, 2m+1 of the chunk: {row a, row b} -> one dword each
                    *reinterpret_cast<uint32_t*>(base + (2 * m) * LDV) = __builtin_amdgcn_perm(hb[m], ha[m], 0x05040100u);
                    *reinterpret_cast<uint32_t*>(base + (2 * m + 1) * LDV) = __builtin_amdgcn_perm(hb[m], ha[m], 0x07060302u);
                }
            }
        }
    };

    // per tile: [K -> LDS] barrier [V loads in flight | S^T, softmax] [V -> LDS, next K loads in flight] barrier [O^T += V^T P^T]
    // (only one of the K / V register sets is live at a time: 512 registers hold Q^T, O^T, S^T and one prefetch set without spilling)
    // E4M3 caches (16 + 16 prefetch registers) keep BOTH sets in flight: K and V of tile t + 1 are requested as soon as tile t went to LDS, a
    // whole tile ahead of their use.  FP16 caches (32 + 32) would spill: there only one set is live (V of the current tile, then K of the next).
    load_k(0);
    if (FP8) load_v(0);
    for (int tile = 0; tile < n_tiles; tile++) {
        const int p0 = tile * FA_TK;
        FA_STAMP(0);
        commit_k();
        if (FP8 && tile + 1 < n_tiles) load_k(p0 + FA_TK);
        __syncthreads();
        if (!FP8) load_v(p0);
        FA_STAMP(1);
        // ---- S^T = K Q^T  (two 32-position blocks)
        v16f sacc[2];
#pragma unroll
        for (int pb = 0; pb < 2; pb++) {
#pragma unroll
            for (int i = 0; i < 16; i++) sacc[pb][i] = 0.0f;
#pragma unroll
            for (int ks = 0; ks < KSTEPS; ks++) {
                const v8h kf = *reinterpret_cast<const v8h*>(Ks + (32 * pb + n31) * LDK + (16 * ks + 8 * khalf) * 2);
                sacc[pb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[ks], sacc[pb], 0, 0, 0);
                if ((ks & 3) == 3) __builtin_amdgcn_sched_barrier(0);      // keep the LDS fragment loads a few MFMAs ahead, not a whole tile (registers)
            }
        }
        FA_STAMP(2);
        // ---- online softmax of this lane's row (32 of the tile's 64 positions live here, the rest in lane ^ 32)
        const bool need_mask = p0 + FA_TK - 1 > full_vis;
        float mloc = -__builtin_inff();
#pragma unroll
        for (int pb = 0; pb < 2; pb++)
#pragma unroll
            for (int i = 0; i < 16; i++) {
                if (need_mask) { const int p = p0 + 32 * pb + (i & 3) + 8 * (i >> 2) + 4 * khalf; if (p > p_q || !row_ok) sacc[pb][i] = -__builtin_inff(); }
                mloc = fmaxf(mloc, sacc[pb][i]);
            }
        mloc = fmaxf(mloc, __shfl_xor(mloc, 32));
        const float m_new = fmaxf(m_run, mloc);
        const float m_use = m_new == -__builtin_inff() ? 0.0f : m_new;                   // nothing visible yet: exp2(-inf - 0) = 0 everywhere
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);                        // m_run = -inf -> 0
        float lsum = 0.0f;
        v8h pf[2][2];
#pragma unroll
        for (int pb = 0; pb < 2; pb++)
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const float pv = __builtin_amdgcn_exp2f(sacc[pb][i] - m_use);
                lsum += pv;
                pf[pb][i >> 3][i & 7] = (_Float16)pv;
            }
        lsum += __shfl_xor(lsum, 32);
        l_run = l_run * alpha + lsum;
        m_run = m_new;
        if (__any(alpha != 1.0f)) {
#pragma unroll
            for (int db = 0; db < DB; db++)
#pragma unroll
                for (int i = 0; i < 16; i++) oacc[db][i] *= alpha;
        }
        FA_STAMP(3);
        commit_v();
        if (tile + 1 < n_tiles) { if (FP8) load_v(p0 + FA_TK); else load_k(p0 + FA_TK); }
        FA_STAMP(4);
        __syncthreads();
        FA_STAMP(5);
        // ---- O^T += V^T P^T
#pragma unroll
        for (int db = 0; db < DB; db++)
#pragma unroll
            for (int kt = 0; kt < 4; kt++) {
                const v8h vv = *reinterpret_cast<const v8h*>(Vt + (size_t)(32 * db + n31) * LDV + 32 * kt + 16 * khalf);
                oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vv, pf[kt >> 1][kt & 1], oacc[db], 0, 0, 0);
                if (kt == 3) __builtin_amdgcn_sched_barrier(0);
            }
        FA_STAMP(6);
    }
    // ---- normalise, gate (attention.py:664-666 / decode.rs:4272-4280), store: accumulator rows 4g .. 4g+3 are dims 32 db + 8 g + 4 khalf + 0..3
    if (row_ok) {
        const float inv = l_run > 0.0f ? 1.0f / l_run : 0.0f;
        const size_t ob = ((size_t)tl.row(tok) * a.nh + h) * HD;
#pragma unroll
        for (int db = 0; db < DB; db++)
#pragma unroll
            for (int g4 = 0; g4 < 4; g4++) {
                const int d = 32 * db + 8 * g4 + 4 * khalf;
                float4 o = make_float4(oacc[db][4 * g4] * inv, oacc[db][4 * g4 + 1] * inv, oacc[db][4 * g4 + 2] * inv, oacc[db][4 * g4 + 3] * inv);
                if (a.gated) {
                    const float4 gt = *reinterpret_cast<const float4*>(a.gate + ob + d);
                    o.x *= 1.0f / (1.0f + kr_expf(-gt.x)); o.y *= 1.0f / (1.0f + kr_expf(-gt.y)); o.z *= 1.0f / (1.0f + kr_expf(-gt.z)); o.w *= 1.0f / (1.0f + kr_expf(-gt.w));
                }
                *reinterpret_cast<float4*>(a.attn_out + ob + d) = o;
            }
    }
}

// ---- the wave-specialised form (S waves / PV waves, described in kr_attn_flash.hip): 512 threads, dynamic LDS
// FA_TK * (HD * 2 + 16) + 2 * FA_TK * (HD * 2 + 64) + 2 * FA_ROWS * (FA_TK * 2 + 16) + 3 * FA_ROWS * 4 bytes
// one v_max3_f32 (the compiler's fmaxf chain canonicalises MFMA results first: two instructions per value)
__device__ __forceinline__ float fa_max3(float a, float b, float c) { float r; asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c)); return r; }
// the value lane ^ 32 holds: one v_permlane32_swap (the ds_bpermute of __shfl_xor is an LDS round trip on the softmax's serial path)
__device__ __forceinline__ float fa_other_half(float x, int khalf) {
    const uint32_t u = __builtin_bit_cast(uint32_t, x);
    const auto sw = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return __builtin_bit_cast(float, khalf ? sw[0] : sw[1]);
}
template <int HD, bool FP8, bool PAGED = false, class Args, class RowMap>
__device__ __forceinline__ void kr_pfm_flashw_body(const Args& a, int C, int t0, int kvh, RowMap row_of, const int* ptab = nullptr, int psh = 0) {
    constexpr int KSTEPS = HD / 16, DBW = HD / 128, LDK = HD * 2 + 16, LDP = FA_TK * 2 + 16;
    constexpr int LDV = HD * 2 + 64;                            // V rows [position][dim]: 16 banks between rows, so the four rows x 64 bytes a 32-lane group of a transpose-read touches are disjoint
    constexpr int CPR = HD / 8;                                 // staging chunks per cache row: 8 values each (8 bytes of an E4M3 row, 16 of an FP16 row) -> 16 bytes of f16 in LDS,
    constexpr int NCH = FA_TK * CPR / 256;                      // consecutive lanes on consecutive 16-byte slots (conflict-free writes); chunks per thread and tile
    extern __shared__ __attribute__((aligned(16))) char fa_smem[];
    char* Ks = fa_smem;                                         // [64 positions][LDK]   f16
    char* Vs = Ks + FA_TK * LDK;                                // [2][64 positions][LDV] f16, ROW-major like K: the P.V fragments come out of ds_read_b64_tr_b16
    char* Ps = Vs + 2 * FA_TK * LDV;                                // [2][128 rows][LDP]    f16 probabilities of a tile, positions contiguous
    float* Al = reinterpret_cast<float*>(Ps + 2 * FA_ROWS * LDP);      // [2][128] rescale factor of the row for the tile
    float* Il = Al + 2 * FA_ROWS;                               // [128] 1 / l at the end
    const int G = a.nh / a.nkv, TQ = FA_ROWS / G;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n31 = lane & 31, khalf = lane >> 5;
    const int kvs = a.nkv * HD, esz = FP8 ? 1 : 2;
    const int kv_end = a.pos0 + (t0 + TQ < C ? t0 + TQ : C);
    const int n_tiles = (kv_end + FA_TK - 1) / FA_TK;
    const int full_vis = a.pos0 + t0;
    // ---- staging of a K (S waves) or V (PV waves) tile by the 256 threads of a side: global -> registers (a tile ahead) -> f16 rows in LDS
    typedef typename std::conditional<FP8, u32x2, u32x4>::type chunk_t;
    const int stid = tid & 255, srow = stid / CPR, sdc = stid % CPR;
    constexpr int RSTEP = 256 / CPR;
    chunk_t stg[NCH];
    const unsigned char* cache = reinterpret_cast<const unsigned char*>(wave < 4 ? a.k_cache : a.v_cache) + (size_t)kvh * HD * esz + sdc * (FP8 ? 8 : 16);
    const size_t rowb = (size_t)kvs * esz;                       // bytes between cache rows (wave-uniform)
    [[maybe_unused]] const int pmask = (1 << psh) - 1;
    auto stage_load = [&](int p0, bool zero_past_end) {
        // PAGED: thread row srow + RSTEP j of the tile lies in the tile's first half (page lo) for j < NCH / 2 and in its second (page hi) otherwise
        [[maybe_unused]] size_t lo = 0, hi = 0;
        if constexpr (PAGED) kr_pf_tile_pages(ptab, psh, p0, kv_end, rowb, lo, hi);
        if (p0 + FA_TK <= kv_end) {                             // whole tile inside the cache rows this workgroup may see: one 64-bit multiply per tile, then row steps
            if constexpr (PAGED) {                              // ... per half: each has its page's base
                const unsigned char* rl = cache + lo + (size_t)((p0 + srow) & pmask) * rowb;
                const unsigned char* rh = cache + hi + (size_t)((p0 + 32 + srow) & pmask) * rowb;
#pragma unroll
                for (int j = 0; j < NCH; j++) stg[j] = *reinterpret_cast<const chunk_t*>((j < NCH / 2 ? rl : rh) + (size_t)(RSTEP * (j < NCH / 2 ? j : j - NCH / 2)) * rowb);
            } else {
                const unsigned char* rp = cache + (size_t)(p0 + srow) * rowb;
#pragma unroll
                for (int j = 0; j < NCH; j++) stg[j] = *reinterpret_cast<const chunk_t*>(rp + (size_t)(RSTEP * j) * rowb);
            }
        } else {
#pragma unroll
            for (int j = 0; j < NCH; j++) {
                const int p = p0 + srow + RSTEP * j;
                chunk_t v;
                if constexpr (PAGED) v = *reinterpret_cast<const chunk_t*>(cache + (j < NCH / 2 ? lo : hi) + (size_t)(min(p, kv_end - 1) & pmask) * rowb);
                else v = *reinterpret_cast<const chunk_t*>(cache + (size_t)min(p, kv_end - 1) * rowb);
                stg[j] = (zero_past_end && p >= kv_end) ? chunk_t{} : v;      // K rows past the end are masked by the causal test; V rows meet P = 0 and must be finite
            }
        }
    };
    auto stage_commit = [&](char* dst, int ld) {
#pragma unroll
        for (int j = 0; j < NCH; j++) {
            u32x4 o;
            if constexpr (FP8) o = u32x4{fa_fp8x2_to_h2(stg[j].x, false), fa_fp8x2_to_h2(stg[j].x, true), fa_fp8x2_to_h2(stg[j].y, false), fa_fp8x2_to_h2(stg[j].y, true)};
            else o = stg[j];
            *reinterpret_cast<u32x4*>(dst + (srow + RSTEP * j) * ld + sdc * 16) = o;
        }
    };
    if (wave < 4) {
        // ================================================================ S waves
        const int r = wave * 32 + n31, hl = r / TQ, ti = r % TQ, tok = t0 + ti;
        const bool row_ok = tok < C;
        const int h = kvh * G + hl, p_q = a.pos0 + tok;
        v8h qf[KSTEPS];
        {
            const float* q = a.q_out + ((size_t)row_of(row_ok ? tok : 0) * a.nh + h) * HD + 8 * khalf;
            const float sc = a.sm_scale * 1.4426950408889634f;
#pragma unroll
            for (int ks = 0; ks < KSTEPS; ks++) {
                const float4 x0 = *reinterpret_cast<const float4*>(q + 16 * ks), x1 = *reinterpret_cast<const float4*>(q + 16 * ks + 4);
                const float xv[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
                for (int i = 0; i < 8; i++) qf[ks][i] = (_Float16)(row_ok ? xv[i] * sc : 0.0f);
            }
        }
        float m_run = 0.0f, l_run = 0.0f;                      // m_run: the origin the row's scores are measured from (its running maximum from the first tile on)
        const char* krow = Ks + n31 * LDK + 16 * khalf;
        stage_load(0, false);
        stage_commit(Ks, LDK);
        if (n_tiles > 1) stage_load(FA_TK, false);
        for (int tile = 0; tile <= n_tiles; tile++) {
            FA_STAMP(0);
            __syncthreads();                                  // X: K(tile) is in LDS (and, for the other side, V(tile - 1) and P(tile - 1))
            FA_STAMP(1);
            if (tile < n_tiles) {
                const int p0 = tile * FA_TK;
                v16f sacc[2];
#pragma unroll
                for (int pb = 0; pb < 2; pb++)
#pragma unroll
                    for (int i = 0; i < 16; i++) sacc[pb][i] = -m_run;
                // K fragments through a ring of FW_RING registers sets: with one wave of this kind per SIMD an LDS round trip (a few hundred cycles while the
                // other side writes its tile) has to be covered by this wave's own MFMAs -- the compiler's schedule kept ~2 in flight and S^T ran at 0.58 of the pipe
                constexpr int NF = 2 * KSTEPS, RING = 8;
                v8h kf[RING];
                auto kaddr = [&](int f) { return krow + 32 * (f & 1) * LDK + 32 * (f >> 1); };      // fragment f: position block f & 1, k-step f >> 1 (the two accumulators alternate)
#pragma unroll
                for (int f = 0; f < RING; f++) kf[f] = *reinterpret_cast<const v8h*>(kaddr(f));
#pragma unroll
                for (int f = 0; f < NF; f++) {
                    sacc[f & 1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[f % RING], qf[f >> 1], sacc[f & 1], 0, 0, 0);
                    if (f + RING < NF) kf[f % RING] = *reinterpret_cast<const v8h*>(kaddr(f + RING));
                    if ((f & 3) == 3) __builtin_amdgcn_sched_barrier(0);
                }
                FA_STAMP(2);
                // The accumulators were started at -m (the row's running maximum, 0 before the first tile), so sacc = s - m already.  Once the maximum has settled
                // -- almost every tile of a long prompt -- no element needs another subtraction and the rescale factor is 1.
                const bool need_mask = p0 + FA_TK - 1 > full_vis || p0 + FA_TK > kv_end;
                if (need_mask) {
#pragma unroll
                    for (int pb = 0; pb < 2; pb++)
#pragma unroll
                        for (int i = 0; i < 16; i++) { const int p = p0 + 32 * pb + (i & 3) + 8 * (i >> 2) + 4 * khalf; if (p > p_q || !row_ok) sacc[pb][i] = -__builtin_inff(); }
                }
                float mloc = fa_max3(sacc[0][0], sacc[1][0], sacc[0][1]);
#pragma unroll
                for (int i = 1; i < 16; i++) mloc = fa_max3(mloc, sacc[0][i], sacc[1][i]);      // (element [0][1] twice: harmless)
                mloc = fa_max3(mloc, fa_other_half(mloc, khalf), tile == 0 ? -__builtin_inff() : 0.0f);      // the first tile sets the maximum, later ones only raise it
                const float shift = mloc == -__builtin_inff() ? 0.0f : mloc;       // >= 0 after the first tile; a row that has seen nothing keeps its origin
                const float alpha = __builtin_amdgcn_exp2f(-shift);
                float lsum = 0.0f;
                char* prow = Ps + (size_t)(tile & 1) * FA_ROWS * LDP + (size_t)r * LDP + 8 * khalf;
                if (__any(shift != 0.0f)) {
#pragma unroll
                    for (int pb = 0; pb < 2; pb++)
#pragma unroll
                        for (int i = 0; i < 16; i++) sacc[pb][i] -= shift;
                }
#pragma unroll
                for (int pb = 0; pb < 2; pb++)
#pragma unroll
                    for (int g4 = 0; g4 < 4; g4++) {      // accumulator rows 4 g4 .. + 3 = positions 32 pb + 8 g4 + 4 khalf .. + 3: one 8-byte store
                        float pv[4];
#pragma unroll
                        for (int u = 0; u < 4; u++) { pv[u] = __builtin_amdgcn_exp2f(sacc[pb][4 * g4 + u]); lsum += pv[u]; }
                        const u32x2 w = {__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(pv[0], pv[1])), __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(pv[2], pv[3]))};
                        *reinterpret_cast<u32x2*>(prow + (32 * pb + 8 * g4) * 2) = w;
                    }
                lsum += fa_other_half(lsum, khalf);
                l_run = l_run * alpha + lsum;
                m_run += shift;
                if (khalf == 0) Al[(tile & 1) * FA_ROWS + r] = alpha;
                FA_STAMP(3);
            }
            __syncthreads();                                  // Y: every S wave is past its K reads
            FA_STAMP(4);
            if (tile + 1 < n_tiles) { stage_commit(Ks, LDK); if (tile + 2 < n_tiles) stage_load((tile + 2) * FA_TK, false); }
            FA_STAMP(5);
        }
        if (khalf == 0) Il[r] = l_run > 0.0f ? 1.0f / l_run : 0.0f;
        __syncthreads();
    } else {
        // ================================================================ PV waves
        const int pw = wave - 4;
        v16f oacc[4][DBW];
#pragma unroll
        for (int rb = 0; rb < 4; rb++)
#pragma unroll
            for (int db = 0; db < DBW; db++)
#pragma unroll
                for (int i = 0; i < 16; i++) oacc[rb][db][i] = 0.0f;
        // V is staged exactly like K (f16 rows in LDS).  The A operand of O^T += V^T P^T wants, per lane, 8 POSITIONS of one dim -- a column of this image;
        // gfx950's LDS transpose-read delivers it: within a 16-lane group, lane i receives element (i & 3) of the 8 bytes addressed by lanes (i >> 2) + 4 j,
        // j = 0..3.  So lane s = 4 j + c of a group points at row (position) j, dims 4 c .. 4 c + 3 of the group's 16 dims, and lane i ends up with dim i
        // of positions 0..3: two reads (positions +0..3, +4..7) make one MFMA fragment.  (The transposing register pass of the eight-wave kernel -- 16
        // conversions + 16 byte permutes + 16 four-byte LDS writes per thread and tile -- was the longest phase of a tile.)
        typedef __fp16 fa_h4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
        const int tr_off = (8 * khalf + ((lane & 15) >> 2)) * LDV + (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;      // this lane's source row / dim quad inside a (16-position, 32-dim) block
        // V is double-buffered: the PV waves bring V(tile) in FIRST (their matrix work would only queue up behind the S waves' S^T MFMAs on the same SIMD for the
        // first half microsecond of an iteration), then run P.V(tile - 1) on the other buffer while the S waves are in their softmax
        stage_load(0, true);
        for (int tile = 0; tile <= n_tiles; tile++) {
            FA_STAMP2(8);
            __syncthreads();                                  // X: P(tile - 1) is in LDS; V(tile - 1) was committed before the previous Y
            FA_STAMP2(9);
            const char* pb_ = Ps + (size_t)((tile - 1) & 1) * FA_ROWS * LDP;
            const char* vb_ = Vs + (size_t)((tile - 1) & 1) * FA_TK * LDV;
            v8h vf[2][DBW], pf[2][4];
            auto fetch = [&](int kt, int bsel) {
#pragma unroll
                for (int db = 0; db < DBW; db++) {
                    const char* va = vb_ + (size_t)(16 * kt) * LDV + 32 * (pw * DBW + db) * 2 + tr_off;
                    const fa_h4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fa_h4*)(va));
                    const fa_h4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fa_h4*)(va + 4 * LDV));
                    const u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
                    vf[bsel][db] = __builtin_bit_cast(v8h, u32x4{l2.x, l2.y, h2.x, h2.y});
                }
#pragma unroll
                for (int rb = 0; rb < 4; rb++) pf[bsel][rb] = *reinterpret_cast<const v8h*>(pb_ + (size_t)(32 * rb + n31) * LDP + (16 * kt + 8 * khalf) * 2);
            };
            float av[4] = {1.0f, 1.0f, 1.0f, 1.0f};
            if (tile >= 1) {                                   // the first two k-steps' fragments (and the rows' factors) travel while this wave stages V
                const float* al = Al + ((tile - 1) & 1) * FA_ROWS;
#pragma unroll
                for (int rb = 0; rb < 4; rb++) av[rb] = al[32 * rb + n31];
                fetch(0, 0); fetch(1, 1);
            }
            if (tile < n_tiles) { stage_commit(Vs + (size_t)(tile & 1) * FA_TK * LDV, LDV); if (tile + 1 < n_tiles) stage_load((tile + 1) * FA_TK, true); }
            FA_STAMP2(10);
            if (tile >= 1) {
                if (__any(av[0] != 1.0f || av[1] != 1.0f || av[2] != 1.0f || av[3] != 1.0f)) {
#pragma unroll
                    for (int rb = 0; rb < 4; rb++)
#pragma unroll
                        for (int db = 0; db < DBW; db++)
#pragma unroll
                            for (int i = 0; i < 16; i++) oacc[rb][db][i] *= av[rb];
                }
#pragma unroll
                for (int kt = 0; kt < 4; kt++) {
#pragma unroll
                    for (int rb = 0; rb < 4; rb++)
#pragma unroll
                        for (int db = 0; db < DBW; db++) oacc[rb][db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[kt & 1][db], pf[kt & 1][rb], oacc[rb][db], 0, 0, 0);
                    if (kt + 2 < 4) fetch(kt + 2, kt & 1);      // two steps ahead, into the set this step has just consumed
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            FA_STAMP2(11);
            __syncthreads();                                  // Y (the S waves' K buffer turns over)
            FA_STAMP2(12);
        }
        __syncthreads();                                      // 1 / l of every row is in LDS
        // ---- normalise, gate (attention.py:664-666 / decode.rs:4272-4280), store: accumulator rows 4 g .. 4 g + 3 are dims 32 (pw DBW + db) + 8 g + 4 khalf + 0..3
#pragma unroll
        for (int rb = 0; rb < 4; rb++) {
            const int r = 32 * rb + n31, hl = r / TQ, ti = r % TQ, tok = t0 + ti;
            if (tok >= C) continue;
            const float inv = Il[r];
            const size_t ob = ((size_t)row_of(tok) * a.nh + kvh * G + hl) * HD;
#pragma unroll
            for (int db = 0; db < DBW; db++)
#pragma unroll
                for (int g4 = 0; g4 < 4; g4++) {
                    const int d = 32 * (pw * DBW + db) + 8 * g4 + 4 * khalf;
                    float4 o = make_float4(oacc[rb][db][4 * g4] * inv, oacc[rb][db][4 * g4 + 1] * inv, oacc[rb][db][4 * g4 + 2] * inv, oacc[rb][db][4 * g4 + 3] * inv);
                    if (a.gated) {
                        const float4 gt = *reinterpret_cast<const float4*>(a.gate + ob + d);
                        o.x *= 1.0f / (1.0f + kr_expf(-gt.x)); o.y *= 1.0f / (1.0f + kr_expf(-gt.y)); o.z *= 1.0f / (1.0f + kr_expf(-gt.z)); o.w *= 1.0f / (1.0f + kr_expf(-gt.w));
                    }
                    *reinterpret_cast<float4*>(a.attn_out + ob + d) = o;
                }
        }
    }
}
