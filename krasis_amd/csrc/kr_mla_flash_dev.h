// kr_mla_flash_dev.h -- MLA flash attention on the f16 matrix cores as a device function.  kr_mla_flash_kernel (kr_mla_flash.hip: the prompt pass and, in its
// SPLIT form, the store's own KR_ATTN_FAST decode step) and kr_multi_mla_flash_kernel (kr_multi_mla_flash.hip, the batched step under "multi_mla_fast") call
// the same body, so a row of a batched step carries the bits of the single-sequence fast step (docs/design/24-multi-mla-fast.md); so does
// kr_multi_mla_pf_flash_kernel (kr_multi_mla_pf_flash.hip, a run of tokens entering a slot under "multi_extend_mla_flash"), whose runs carry the bits of the
// prompt pass (docs/design/27-multi-extend-mla-flash.md).  The callers differ only in where the position, the query rows, the cache rows and the partials come from.
//
// In the absorbed form (decode.rs:2993-3252; the reference's GPU side: flashinfer MLA, attention.py:300-349) ALL heads of ALL tokens of a tile
// attend over the SAME rows:   s[h][p] = (q_abs[h] . ckv[p] + q_pe[h] . kpe[p]) * sm_scale,   out[h] = sum_p softmax(s)[p] * ckv[p]
// = flash attention with K rows [ckv | kpe] (576 dims) and V = the first kv_lora_rank dims of the same rows.  One workgroup takes 64 query
// rows (token-major: row = token * nh + head) and streams the cache once for all of them:
//   * waves (wq, wd): wq picks 32 query rows, wd one half of the kv_lora_rank output dims (the S^T tile is computed by both d-waves: with
//     K = 576 and an f32 O^T of 512 dims per row the registers of one wave cannot hold a full-width accumulator);
//   * S^T = K Q^T with v_mfma_f32_32x32x16_f16: A = staged rows [position][576] (LDS), B = the query tile (LDS, scale and log2 e folded in),
//     accumulator column = query row = lane % 32 -> lane-local online softmax (kr_attn_flash.hip);
//   * O^T += V^T P^T: A = the same latent rows written TRANSPOSED ([dim][position], two positions per dword) while the tile is staged --
//     one global fetch feeds both operands --, B = P^T from the S^T accumulators.
// q, p rounded to f16; ckv / kpe exact in f16 (FP16 or E4M3 caches).  f32 accumulation and softmax.
#pragma once
#include "kr_device.h"
#include "kr_libm.h"

typedef _Float16 v8h __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef float v2f __attribute__((ext_vector_type(2)));

#define MF_TK 32
#define MF_ROWS 64

__device__ __forceinline__ uint32_t mf_fp8x2_to_h2(uint32_t w, bool hi) {      // two E4M3 bytes -> packed f16 pair (exact): ONE v_cvt_scalef32_pk_f16_fp8 (scale 1)
    typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
    const h2_t h = hi ? __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, true) : __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, false);
    return __builtin_bit_cast(uint32_t, h);
}
__device__ __forceinline__ uint32_t mf_f2h2(float a, float b) { return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(a, b)); }

// Row tile `tile_row` (64 query rows) of C tokens x nh heads at positions pos0 .. pos0 + C - 1: q_abs [C][nh][KLR], q_pe [C][nh][64] (f32), caches
// [position][KLR] / [position][64] (FP16 or E4M3).  256 threads, dynamic LDS (MF_ROWS + MF_TK) * ((KLR + 64) * 2 + 16) + KLR * (MF_TK * 2 + 16) bytes.
// Writes the normalised rows to attn_lat [C][nh][KLR].
// SPLIT (decode over a long cache): the workgroup is chunk `chunk` of the cache, walks `chunk_tiles` tiles of it and leaves the un-normalised O rows at
// fd_o [chunk][row][KLR] and (max in log2 units, sum) at fd_ml [row][n_chunks][2] for kr_fd_merge2_body (kr_fd_flash_dev.h); one that starts past the
// current length leaves at once.
// PAGED (docs/design/24-multi-mla-fast.md): ckv_cache / kpe_cache are pools of pages of 1 << psh positions (psh >= 5) and position p is row
// (ptab[p >> psh] << psh) | (p & mask) of both.  A tile of MF_TK positions starts at a multiple of MF_TK, so it lies in ONE page: the page id is
// workgroup-uniform and the page's byte offsets in the two pools stay in scalar registers; a lane adds its row's offset inside the page.  Only the cache
// addresses differ from the flat instantiation: the order of every operation is the same.
// RowMap (docs/design/27-multi-extend-mla-flash.md): the rows above are the caller's own count from 0; rmap(row) is where that row lies in q_abs / q_pe / attn_lat.
// The identity for a chunk of a prompt and for a decode row; a run of a batched pass maps its (token, head) rows to pass rows (kr_multi_mla_pf_flash.hip).  It
// is asked for rows below C * nh only, where the query tile is loaded and where the non-SPLIT form writes attn_lat; positions, masks and kv_end stay in the
// caller's rows
struct KrMfRowsIdentity {
    __device__ __forceinline__ int operator()(int row) const { return row; }
};
template <int KLR, bool FP8, bool SPLIT, bool PAGED = false, class RowMap = KrMfRowsIdentity>
__device__ __forceinline__ void kr_mla_flash_body(const float* q_abs, const float* q_pe, const void* ckv_cache, const void* kpe_cache, int pos0, int C, int nh, float sm_scale,
                                                  float* attn_lat, float* fd_o, float* fd_ml, int tile_row, int chunk, int n_chunks, int chunk_tiles,
                                                  const int* ptab = nullptr, int psh = 0, RowMap rmap = {}) {
    constexpr int RD = 64, DK = KLR + RD, KSTEPS = DK / 16, LDK = DK * 2 + 16, LDV = MF_TK * 2 + 16;
    constexpr int DBW = KLR / 64;                               // 32-dim output blocks per d-wave (two d-waves)
    constexpr int CB = FP8 ? 16 : 8;                            // dims per 16-byte global chunk
    constexpr int CPC = KLR / CB, CPRR = RD / CB, CPR = CPC + CPRR;      // chunks per row: latent part, rope part
    constexpr int NUN = (MF_TK / 2) * CPR, UPT = (NUN + 255) / 256;       // (position pair, chunk) units per tile / per thread
    extern __shared__ __attribute__((aligned(16))) char mf_smem[];
    char* Qs = mf_smem;                                         // [64 rows][LDK]        f16 (scaled)
    char* Ks = Qs + MF_ROWS * LDK;                              // [32 positions][LDK]   f16
    char* Vt = Ks + MF_TK * LDK;                                // [KLR dims][LDV]       f16, positions contiguous
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n31 = lane & 31, khalf = lane >> 5, wq = wave & 1, wd = wave >> 1;
    const int nrows = C * nh, row0 = tile_row * MF_ROWS;
    const int tok_first = row0 / nh, tok_last = min(C - 1, (row0 + MF_ROWS - 1) / nh);
    const int kv_end = pos0 + tok_last + 1, full_vis = pos0 + tok_first;
    const int n_tiles_all = (kv_end + MF_TK - 1) / MF_TK;
    const int tile_beg = SPLIT ? chunk * chunk_tiles : 0, n_tiles = SPLIT ? min(n_tiles_all, tile_beg + chunk_tiles) : n_tiles_all;
    if (SPLIT && tile_beg >= n_tiles_all) return;               // chunk past the current length (the grid is sized for the whole cache)
    const int myrow = row0 + wq * 32 + n31;
    const bool row_ok = myrow < nrows;
    const int p_q = pos0 + (row_ok ? myrow / nh : 0);

    // ---- query tile -> LDS (f16, sm_scale * log2 e folded in); rows past the end are zero
    {
        const float sc = sm_scale * 1.4426950408889634f;
        for (int i = tid; i < MF_ROWS * (DK / 8); i += 256) {
            const int r = i / (DK / 8), c8 = i % (DK / 8), gr = row0 + r;
            u32x4 o = {0, 0, 0, 0};
            if (gr < nrows) {
                const size_t qr = (size_t)rmap(gr);
                const float* src = c8 < KLR / 8 ? q_abs + qr * KLR + c8 * 8 : q_pe + qr * RD + (c8 - KLR / 8) * 8;
                const float4 x0 = *reinterpret_cast<const float4*>(src), x1 = *reinterpret_cast<const float4*>(src + 4);
                o = u32x4{mf_f2h2(x0.x * sc, x0.y * sc), mf_f2h2(x0.z * sc, x0.w * sc), mf_f2h2(x1.x * sc, x1.y * sc), mf_f2h2(x1.z * sc, x1.w * sc)};
            }
            *reinterpret_cast<u32x4*>(Qs + r * LDK + c8 * 16) = o;
        }
    }
    v16f oacc[DBW];
#pragma unroll
    for (int db = 0; db < DBW; db++)
#pragma unroll
        for (int i = 0; i < 16; i++) oacc[db][i] = 0.0f;
    float m_run = -__builtin_inff(), l_run = 0.0f;

    const unsigned char* cc = reinterpret_cast<const unsigned char*>(ckv_cache);
    const unsigned char* cr = reinterpret_cast<const unsigned char*>(kpe_cache);
    constexpr int esz = FP8 ? 1 : 2;
    [[maybe_unused]] const int pmask = (1 << psh) - 1;
    u32x4 pa[UPT], pb[UPT];
    auto load_tile = [&](int p0) {
        // PAGED: p0 < kv_end at every call, so the entry of its page was mapped by the host before the pass; -1 is never turned into an address all the same
        [[maybe_unused]] size_t pgc = 0, pgr = 0;               // byte offsets of the tile's page in the latent pool and in the rope-key pool
        if constexpr (PAGED) {
            const size_t r0 = (size_t)__builtin_amdgcn_readfirstlane(max(ptab[p0 >> psh], 0)) << psh;
            pgc = r0 * (size_t)(KLR * esz); pgr = r0 * (size_t)(RD * esz);
        }
#pragma unroll
        for (int j = 0; j < UPT; j++) {
            const int u = tid + j * 256, pp = u & 15, dc = u >> 4, p = p0 + 2 * pp;       // lanes walk the position pairs (transposed LDS writes)
            pa[j] = u32x4{0, 0, 0, 0}; pb[j] = u32x4{0, 0, 0, 0};
            if (u < NUN) {
                const size_t ld = (size_t)(dc < CPC ? KLR : RD) * esz;
                if constexpr (PAGED) {      // p is even: p and p + 1 share the page
                    const unsigned char* base = dc < CPC ? cc + pgc + (size_t)dc * 16 : cr + pgr + (size_t)(dc - CPC) * 16;
                    const size_t off = (size_t)(p & pmask) * ld;
                    if (p < kv_end) pa[j] = *reinterpret_cast<const u32x4*>(base + off);
                    if (p + 1 < kv_end) pb[j] = *reinterpret_cast<const u32x4*>(base + off + ld);
                } else {
                    const unsigned char* base = dc < CPC ? cc + (size_t)dc * 16 : cr + (size_t)(dc - CPC) * 16;
                    if (p < kv_end) pa[j] = *reinterpret_cast<const u32x4*>(base + (size_t)p * ld);
                    if (p + 1 < kv_end) pb[j] = *reinterpret_cast<const u32x4*>(base + (size_t)(p + 1) * ld);
                }
            }
        }
    };
    auto commit_tile = [&]() {
#pragma unroll
        for (int j = 0; j < UPT; j++) {
            const int u = tid + j * 256, pp = u & 15, dc = u >> 4;
            if (u < NUN) {
                constexpr int NW = FP8 ? 8 : 4;
                uint32_t ha[8], hb[8];
                if (FP8) {
                    const uint32_t wa[4] = {pa[j].x, pa[j].y, pa[j].z, pa[j].w}, wb[4] = {pb[j].x, pb[j].y, pb[j].z, pb[j].w};
#pragma unroll
                    for (int m = 0; m < 4; m++) { ha[2 * m] = mf_fp8x2_to_h2(wa[m], false); ha[2 * m + 1] = mf_fp8x2_to_h2(wa[m], true);
                                                  hb[2 * m] = mf_fp8x2_to_h2(wb[m], false); hb[2 * m + 1] = mf_fp8x2_to_h2(wb[m], true); }
                } else {
                    ha[0] = pa[j].x; ha[1] = pa[j].y; ha[2] = pa[j].z; ha[3] = pa[j].w; hb[0] = pb[j].x; hb[1] = pb[j].y; hb[2] = pb[j].z; hb[3] = pb[j].w;
                    ha[4] = ha[5] = ha[6] = ha[7] = 0; hb[4] = hb[5] = hb[6] = hb[7] = 0;
                }
                // row-major K rows (dims dc * CB ..)
                char* ka = Ks + (2 * pp) * LDK + dc * CB * 2; char* kb = ka + LDK;
                *reinterpret_cast<u32x4*>(ka) = u32x4{ha[0], ha[1], ha[2], ha[3]}; *reinterpret_cast<u32x4*>(kb) = u32x4{hb[0], hb[1], hb[2], hb[3]};
                if (FP8) { *reinterpret_cast<u32x4*>(ka + 16) = u32x4{ha[4], ha[5], ha[6], ha[7]}; *reinterpret_cast<u32x4*>(kb + 16) = u32x4{hb[4], hb[5], hb[6], hb[7]}; }
                // transposed value rows (latent part only): dims 2m, 2m+1 of the chunk, {row a, row b} in one dword
                if (dc < CPC) {
                    char* base = Vt + (size_t)(dc * CB) * LDV + pp * 4;
#pragma unroll
                    for (int m = 0; m < NW; m++) {
                        *reinterpret_cast<uint32_t*>(base + (2 * m) * LDV) = __builtin_amdgcn_perm(hb[m], ha[m], 0x05040100u);
                        *reinterpret_cast<uint32_t*>(base + (2 * m + 1) * LDV) = __builtin_amdgcn_perm(hb[m], ha[m], 0x07060302u);
                    }
                }
            }
        }
    };

    load_tile(tile_beg * MF_TK);
    for (int tile = tile_beg; tile < n_tiles; tile++) {
        const int p0 = tile * MF_TK;
        commit_tile();
        if (tile + 1 < n_tiles) load_tile(p0 + MF_TK);
        __syncthreads();
        // ---- S^T = K Q^T (32 positions x 32 query rows)
        v16f sacc;
#pragma unroll
        for (int i = 0; i < 16; i++) sacc[i] = 0.0f;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ks++) {
            const v8h kf = *reinterpret_cast<const v8h*>(Ks + n31 * LDK + (16 * ks + 8 * khalf) * 2);
            const v8h qf = *reinterpret_cast<const v8h*>(Qs + (wq * 32 + n31) * LDK + (16 * ks + 8 * khalf) * 2);
            sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf, sacc, 0, 0, 0);
            if ((ks & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
        // ---- online softmax of this lane's row (16 of the tile's 32 positions live here, the rest in lane ^ 32)
        const bool need_mask = p0 + MF_TK - 1 > full_vis;
        float mloc = -__builtin_inff();
#pragma unroll
        for (int i = 0; i < 16; i++) {
            if (need_mask) { const int p = p0 + (i & 3) + 8 * (i >> 2) + 4 * khalf; if (p > p_q || !row_ok) sacc[i] = -__builtin_inff(); }
            mloc = fmaxf(mloc, sacc[i]);
        }
        mloc = fmaxf(mloc, __shfl_xor(mloc, 32));
        const float m_new = fmaxf(m_run, mloc);
        const float m_use = m_new == -__builtin_inff() ? 0.0f : m_new;
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);
        float lsum = 0.0f;
        v8h pf[2];
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const float pv = __builtin_amdgcn_exp2f(sacc[i] - m_use);
            lsum += pv;
            pf[i >> 3][i & 7] = (_Float16)pv;
        }
        lsum += __shfl_xor(lsum, 32);
        l_run = l_run * alpha + lsum;
        m_run = m_new;
        if (__any(alpha != 1.0f)) {
#pragma unroll
            for (int db = 0; db < DBW; db++)
#pragma unroll
                for (int i = 0; i < 16; i++) oacc[db][i] *= alpha;
        }
        // ---- O^T += V^T P^T (this wave's half of the latent dims)
#pragma unroll
        for (int db = 0; db < DBW; db++)
#pragma unroll
            for (int kt = 0; kt < 2; kt++) {
                const char* vr = Vt + (size_t)(wd * (KLR / 2) + 32 * db + n31) * LDV + (16 * kt + 4 * khalf) * 2;
                const u32x2 v0 = *reinterpret_cast<const u32x2*>(vr), v1 = *reinterpret_cast<const u32x2*>(vr + 16);
                const u32x4 vv = {v0.x, v0.y, v1.x, v1.y};
                oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(v8h, vv), pf[kt], oacc[db], 0, 0, 0);
            }
        __syncthreads();
    }
    if (SPLIT) {
        if (row_ok) {
            float* out = fd_o + ((size_t)chunk * nh + myrow) * KLR + wd * (KLR / 2);          // [chunk][head][KLR]
#pragma unroll
            for (int db = 0; db < DBW; db++)
#pragma unroll
                for (int g4 = 0; g4 < 4; g4++)
                    *reinterpret_cast<float4*>(out + 32 * db + 8 * g4 + 4 * khalf) = make_float4(oacc[db][4 * g4], oacc[db][4 * g4 + 1], oacc[db][4 * g4 + 2], oacc[db][4 * g4 + 3]);
            if (wd == 0 && khalf == 0) { float* ml = fd_ml + ((size_t)myrow * n_chunks + chunk) * 2; ml[0] = m_run; ml[1] = l_run; }
        }
        return;
    }
    if (row_ok) {
        const float inv = l_run > 0.0f ? 1.0f / l_run : 0.0f;
        float* out = attn_lat + (size_t)rmap(myrow) * KLR + wd * (KLR / 2);
#pragma unroll
        for (int db = 0; db < DBW; db++)
#pragma unroll
            for (int g4 = 0; g4 < 4; g4++)
                *reinterpret_cast<float4*>(out + 32 * db + 8 * g4 + 4 * khalf) =
                    make_float4(oacc[db][4 * g4] * inv, oacc[db][4 * g4 + 1] * inv, oacc[db][4 * g4 + 2] * inv, oacc[db][4 * g4 + 3] * inv);
    }
}

// dynamic LDS of the body in bytes: query tile + K tile + transposed latent tile
template <int KLR> static size_t kr_mla_flash_lds() { return (size_t)(MF_ROWS + MF_TK) * ((KLR + 64) * 2 + 16) + (size_t)KLR * (MF_TK * 2 + 16); }
