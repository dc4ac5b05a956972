// kr_fd_flash_dev.h -- the split-KV flash-decode of one sequence as device functions: the chunk pass and the log-sum-exp merge.  kr_fd_flash_kernel /
// kr_fd_merge2_kernel (kr_attn_flash.hip, the store's own KR_ATTN_FAST step) and kr_multi_fd_flash_kernel / kr_multi_fd_merge_kernel (kr_multi_flash.hip, the
// batched step under "multi_attn_fast") call the same bodies, so a row of a batched step carries the bits of the single-sequence fast step
// (docs/design/16-multi-attn-fast.md).  The callers differ only in where the sequence length, the cache rows, the query and the partials come from.
#pragma once
#include "kr_device.h"
#include "kr_libm.h"
#include "kr_exact_dev.h"

typedef _Float16 v8h __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef float v2f __attribute__((ext_vector_type(2)));

#define FA_TK 64

__device__ __forceinline__ uint32_t fa_fp8x2_to_h2(uint32_t w, bool hi) {      // two E4M3 bytes -> packed f16 pair (exact): ONE v_cvt_scalef32_pk_f16_fp8 (scale 1)
    typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
    const h2_t h = hi ? __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, true) : __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, false);
    return __builtin_bit_cast(uint32_t, h);
}

// V^T rows in LDS hold the 64 positions of a tile as 32 dwords (position pairs).  Inside every group of 16 positions the pairs are stored in the order
// (0-3, 8-11 | 4-7, 12-15) -- pair index bits 1 and 2 swapped -- so that the 8 positions lane half `khalf` multiplies with its P^T fragment (the S^T
// accumulator's own row order) are ONE 16-byte read; in natural order they were two 8-byte reads whose 144-byte row stride put lanes i and i + 16 on
// the same banks (the P.V phase ran at half the LDS rate).
__device__ __forceinline__ int fa_vslot(int pp) { return (pp & ~6) | ((pp & 2) << 1) | ((pp & 4) >> 1); }

// Chunk c of KV head kvh of a sequence of `seq` positions: positions [c * chunk, min(seq, (c + 1) * chunk)) of the cache rows at k_cache / v_cache
// ([position][nkv * HD], FP16 or E4M3) against the G = nh / nkv query heads of the group, q_heads [nh][HD] after QK-norm / RoPE.  256 threads, dynamic LDS
// FA_TK * (HD * 2 + 16) + HD * (FA_TK * 2 + 16) bytes.  Writes the chunk's un-normalised O to fd_o [nkv][n_chunks][G][HD] and (max in log2 units, sum) to
// fd_ml [nh][n_chunks][2]; leaves at once when the chunk starts past the sequence.
// PAGED (docs/design/23-multi-attn-fast-paged.md): k_cache / v_cache are pools of pages of 1 << psh positions (psh >= 5) and position p of the sequence is row
// (ptab[p >> psh] << psh) | (p & mask) of them.  A tile of FA_TK positions starts at a multiple of FA_TK, so it lies in one page, or in two at 32
// positions per page: the two page ids are workgroup-uniform and their byte offsets stay in scalar registers; a lane adds its row's offset inside the page.
// Only the three cache addresses differ from the flat instantiation: the order of every operation is the same.
template <int HD, bool FP8, bool PAGED = false>
__device__ __forceinline__ void kr_fd_flash_body(int seq, int c, int kvh, const float* q_heads, const void* k_cache, const void* v_cache, float* fd_o, float* fd_ml,
                                                 int nh, int nkv, float sm_scale, int n_chunks, int chunk, const int* ptab = nullptr, int psh = 0) {
    constexpr int KSTEPS = HD / 16, DB = HD / 32, DBW = DB >= 4 ? DB / 4 : 1, LDK = HD * 2 + 16, LDV = FA_TK * 2 + 16;
    constexpr int CPR = FP8 ? HD / 16 : HD / 8, KCH = FA_TK * CPR / 256, VUN = (FA_TK / 2) * CPR, VPT = (VUN + 255) / 256;
    extern __shared__ __attribute__((aligned(16))) char fa_smem[];
    char* Ks = fa_smem; char* Vt = fa_smem + FA_TK * LDK;
    const int G = nh / nkv;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n31 = lane & 31, khalf = lane >> 5;
    const int pbeg = c * chunk;
    if (pbeg >= seq) return;
    const int pend = min(seq, pbeg + chunk), n_tiles = (pend - pbeg + FA_TK - 1) / FA_TK;
    const bool row_ok = n31 < G;
    const int h = kvh * G + (row_ok ? n31 : 0);
    const int kvs = nkv * HD, esz = FP8 ? 1 : 2;
    v8h qf[KSTEPS];
    {
        const float* q = q_heads + (size_t)h * HD + 8 * khalf;
        const float sc = sm_scale * 1.4426950408889634f;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ks++) {
            const float4 x0 = *reinterpret_cast<const float4*>(q + 16 * ks), x1 = *reinterpret_cast<const float4*>(q + 16 * ks + 4);
            const float xv[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
            for (int i = 0; i < 8; i++) qf[ks][i] = (_Float16)(row_ok ? xv[i] * sc : 0.0f);
        }
    }
    v16f oacc[DBW];
#pragma unroll
    for (int db = 0; db < DBW; db++)
#pragma unroll
        for (int i = 0; i < 16; i++) oacc[db][i] = 0.0f;
    float m_run = -__builtin_inff(), l_run = 0.0f;
    const unsigned char* kc = reinterpret_cast<const unsigned char*>(k_cache) + (size_t)kvh * HD * esz;
    const unsigned char* vc = reinterpret_cast<const unsigned char*>(v_cache) + (size_t)kvh * HD * esz;
    u32x4 pk[KCH], pva[VPT], pvb[VPT];
    // PAGED: byte offsets in the pools of the pages that hold the two halves of the tile at p0: lo = the page of p0 .. p0 + 31, hi = the page of
    // min(p0 + 32, pend - 1), which holds every clamped position of rows 32 .. 63 (the last position itself where the tile ends before them).  Both positions
    // lie in [pbeg, pend), so both entries were mapped by the host before the pass; -1 is never turned into an address all the same
    const size_t rowb = (size_t)kvs * esz;
    const int pmask = (1 << psh) - 1;
    auto tile_pages = [&](int p0, size_t& lo, size_t& hi) {
        const int i0 = __builtin_amdgcn_readfirstlane(max(ptab[p0 >> psh], 0)), i1 = __builtin_amdgcn_readfirstlane(max(ptab[min(p0 + 32, pend - 1) >> psh], 0));
        lo = ((size_t)i0 << psh) * rowb; hi = ((size_t)i1 << psh) * rowb;
    };
    auto load_k = [&](int p0) {
        [[maybe_unused]] size_t lo = 0, hi = 0;
        if constexpr (PAGED) tile_pages(p0, lo, hi);
#pragma unroll
        for (int j = 0; j < KCH; j++) {
            const int cc = tid + j * 256, row = cc / CPR, dc = cc % CPR, p = min(p0 + row, pend - 1);     // clamped: rows past the end are masked below
            if constexpr (PAGED) pk[j] = *reinterpret_cast<const u32x4*>(kc + (row >= 32 ? hi : lo) + (size_t)(p & pmask) * rowb + dc * 16);
            else pk[j] = *reinterpret_cast<const u32x4*>(kc + (size_t)p * kvs * esz + dc * 16);
        }
    };
    auto load_v = [&](int p0) {
        [[maybe_unused]] size_t lo = 0, hi = 0;
        if constexpr (PAGED) tile_pages(p0, lo, hi);
#pragma unroll
        for (int j = 0; j < VPT; j++) {
            const int u = tid + j * 256, pp = u & 31, dc = u >> 5, p = p0 + 2 * pp;
            pva[j] = u32x4{0, 0, 0, 0}; pvb[j] = u32x4{0, 0, 0, 0};
            if (u < VUN) {
                u32x4 va, vb;
                if constexpr (PAGED) {      // p is even: p and p + 1 share a page, and so do their clamped forms
                    const int pa = min(p, pend - 1), pb = min(p + 1, pend - 1);
                    const unsigned char* ra = vc + (pp >= 16 ? hi : lo) + (size_t)(pa & pmask) * rowb + dc * 16;
                    va = *reinterpret_cast<const u32x4*>(ra); vb = *reinterpret_cast<const u32x4*>(ra + (size_t)(pb - pa) * rowb);
                } else {
                    va = *reinterpret_cast<const u32x4*>(vc + (size_t)min(p, pend - 1) * kvs * esz + dc * 16);
                    vb = *reinterpret_cast<const u32x4*>(vc + (size_t)min(p + 1, pend - 1) * kvs * esz + dc * 16);
                }
                if (p < pend) pva[j] = va;                 // a probability of exactly 0 meets a finite value: rows past the end must not be NaN patterns
                if (p + 1 < pend) pvb[j] = vb;
            }
        }
    };
    auto commit_k = [&]() {
#pragma unroll
        for (int j = 0; j < KCH; j++) {
            const int cc = tid + j * 256, row = cc / CPR, dc = cc % CPR;
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
                uint32_t ha[8], hb[8];
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
                for (int m = 0; m < NW; m++) {
                    *reinterpret_cast<uint32_t*>(base + (2 * m) * LDV) = __builtin_amdgcn_perm(hb[m], ha[m], 0x05040100u);
                    *reinterpret_cast<uint32_t*>(base + (2 * m + 1) * LDV) = __builtin_amdgcn_perm(hb[m], ha[m], 0x07060302u);
                }
            }
        }
    };
    // K and V of tile t + 1 are requested while tile t is consumed (each register set is free as soon as its tile went to LDS; a second
    // register set -- requests two tiles ahead -- was measured: 279 registers, one workgroup per CU, 18.4 -> 26.5 us per launch)
    load_k(pbeg); load_v(pbeg);
    for (int tile = 0; tile < n_tiles; tile++) {
        const int p0 = pbeg + tile * FA_TK;
        commit_k();
        if (tile + 1 < n_tiles) load_k(p0 + FA_TK);
        __syncthreads();
        v16f sacc[2];
#pragma unroll
        for (int pb = 0; pb < 2; pb++) {
#pragma unroll
            for (int i = 0; i < 16; i++) sacc[pb][i] = 0.0f;
#pragma unroll
            for (int ks = 0; ks < KSTEPS; ks++) {
                const v8h kf = *reinterpret_cast<const v8h*>(Ks + (32 * pb + n31) * LDK + (16 * ks + 8 * khalf) * 2);
                sacc[pb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[ks], sacc[pb], 0, 0, 0);
                if ((ks & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
        }
        const bool need_mask = p0 + FA_TK > pend;
        float mloc = -__builtin_inff();
#pragma unroll
        for (int pb = 0; pb < 2; pb++)
#pragma unroll
            for (int i = 0; i < 16; i++) {
                if (need_mask) { const int p = p0 + 32 * pb + (i & 3) + 8 * (i >> 2) + 4 * khalf; if (p >= pend) sacc[pb][i] = -__builtin_inff(); }
                mloc = fmaxf(mloc, sacc[pb][i]);
            }
        mloc = fmaxf(mloc, __shfl_xor(mloc, 32));
        const float m_new = fmaxf(m_run, mloc);                                           // finite: every tile holds at least one visible position
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        float lsum = 0.0f;
        v8h pf[2][2];
#pragma unroll
        for (int pb = 0; pb < 2; pb++)
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const float pv = __builtin_amdgcn_exp2f(sacc[pb][i] - m_new);
                lsum += pv;
                pf[pb][i >> 3][i & 7] = (_Float16)pv;
            }
        lsum += __shfl_xor(lsum, 32);
        l_run = l_run * alpha + lsum;
        m_run = m_new;
#pragma unroll
        for (int db = 0; db < DBW; db++)
#pragma unroll
            for (int i = 0; i < 16; i++) oacc[db][i] *= alpha;
        commit_v();
        if (tile + 1 < n_tiles) load_v(p0 + FA_TK);
        __syncthreads();
        if (wave * DBW < DB) {
#pragma unroll
            for (int db = 0; db < DBW; db++)
#pragma unroll
                for (int kt = 0; kt < 4; kt++) {
                    const v8h vv = *reinterpret_cast<const v8h*>(Vt + (size_t)(32 * (wave * DBW + db) + n31) * LDV + 32 * kt + 16 * khalf);
                    oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vv, pf[kt >> 1][kt & 1], oacc[db], 0, 0, 0);
                }
        }
    }
    // ---- partials: accumulator rows 4 g4 .. 4 g4 + 3 of block db are dims 32 (wave DBW + db) + 8 g4 + 4 khalf + 0..3, column = head n31
    if (row_ok) {
        float* po = fd_o + (((size_t)kvh * n_chunks + c) * G + n31) * HD;
        if (wave * DBW < DB) {
#pragma unroll
            for (int db = 0; db < DBW; db++)
#pragma unroll
                for (int g4 = 0; g4 < 4; g4++)
                    *reinterpret_cast<float4*>(po + 32 * (wave * DBW + db) + 8 * g4 + 4 * khalf) =
                        make_float4(oacc[db][4 * g4], oacc[db][4 * g4 + 1], oacc[db][4 * g4 + 2], oacc[db][4 * g4 + 3]);
        }
        if (wave == 0 && khalf == 0) { float* ml = fd_ml + ((size_t)(kvh * G + n31) * n_chunks + c) * 2; ml[0] = m_run; ml[1] = l_run; }
    }
}

// Head h of a sequence of `seq` positions: log-sum-exp merge of its ceil(seq / chunk) chunk partials (independent partial sums per chunk phase), the
// sigmoid gate (gate [nh][HD]) where the layer is gated, out [nh][HD]; img_out (optional): the INT16 image of out for the o-projection launch.  1024 threads.
template <int HD>
__device__ __forceinline__ void kr_fd_merge2_body(int seq, int h, const float* fd_o, const float* fd_ml, int nh, int nkv, const float* gate, int gated, float* out,
                                                  void* img_out, int n_chunks, int chunk) {
    __shared__ float wc[1024]; __shared__ float qs[1024]; __shared__ float red[32];
    const int t = threadIdx.x, G = nh / nkv, kvh = h / G, g = h % G;
    const int nc = min((seq + chunk - 1) / chunk, 1024);
    const float* ml = fd_ml + (size_t)h * n_chunks * 2;
    const float mv = t < nc ? ml[t * 2] : -__builtin_inff(), lv = t < nc ? ml[t * 2 + 1] : 0.0f;      // nc <= 1024 = one chunk per thread
    float mx = kr_wave_max(mv);
    if ((t & 63) == 0) red[t >> 6] = mx;
    __syncthreads();
    mx = red[0];
#pragma unroll
    for (int i = 1; i < 16; i++) mx = fmaxf(mx, red[i]);
    const float wv = t < nc ? __builtin_amdgcn_exp2f(mv - mx) : 0.0f;
    wc[t] = wv;
    float l = wv * lv;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) l += __shfl_xor(l, off);
    if ((t & 63) == 0) red[16 + (t >> 6)] = l;
    __syncthreads();
    float lt = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; i++) lt += red[16 + i];
    const float inv = 1.0f / lt;
    // thread = (dim d, chunk phase): 1024 / HD phases walk interleaved chunks with 4 independent sums each
    constexpr int NPH = 1024 / HD;
    const int d = t % HD, ph = t / HD;
    const float* ob = fd_o + ((size_t)kvh * n_chunks * G + g) * HD + d;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    int c = ph;
    for (; c + 3 * NPH < nc; c += 4 * NPH) {
        const float v0 = ob[(size_t)c * G * HD], v1 = ob[(size_t)(c + NPH) * G * HD], v2 = ob[(size_t)(c + 2 * NPH) * G * HD], v3 = ob[(size_t)(c + 3 * NPH) * G * HD];
        s0 = __builtin_fmaf(wc[c], v0, s0); s1 = __builtin_fmaf(wc[c + NPH], v1, s1); s2 = __builtin_fmaf(wc[c + 2 * NPH], v2, s2); s3 = __builtin_fmaf(wc[c + 3 * NPH], v3, s3);
    }
    for (; c < nc; c += NPH) s0 = __builtin_fmaf(wc[c], ob[(size_t)c * G * HD], s0);
    float o = (s0 + s1) + (s2 + s3);
    if (NPH > 1) {
        __syncthreads();
        qs[t] = o;                                   // HD * NPH == 1024
        __syncthreads();
        o = 0.0f;
        if (t < HD) for (int p = 0; p < NPH; p++) o += qs[p * HD + t];
        __syncthreads();
    }
    if (t < HD) {
        o *= inv;
        if (gated) { const float gt = gate[(size_t)h * HD + t]; o *= 1.0f / (1.0f + kr_expf(-gt)); }
        out[(size_t)h * HD + t] = o;
        if (img_out) qs[t] = o;
    }
    if (img_out) {
        __syncthreads();
        const KrActLds Lg = kr_carve_lds(reinterpret_cast<u32x4*>(img_out), nh * HD, false);
        constexpr int nch = HD / 8;
        if (t < nch) {
            float v8[8];
            kr_load8(qs, t, v8);
            float mx8 = 0.0f;
#pragma unroll
            for (int i = 0; i < 8; i++) mx8 = fmaxf(mx8, fabsf(v8[i]));
            float scale, qinv;
            kr_group_scale(mx8, scale, qinv);
            int q8[8];
            kr_quant8<false>(v8, qinv, q8);
            const int gc = h * nch + t;
            kr_store_chunk<false>(Lg, gc, q8);
            if ((gc & 15) == 0) Lg.ascale[gc >> 4] = scale;
        }
    }
}
