// kr_gguf.hip -- native GGUF block experts on gfx950: Q4_K / Q8_0 / Q4_0 with INT16 activations (exact integer dots),
// Q5_0 / Q6_K through the reference's scalar f32 form, Q5_K through the same form over dequant_q5_k's values (gguf.rs:740), Q3_K over the values of ggml's block definition (docs/design/47-gguf-q3k.md).  Replaces src/gguf_kernels.rs (matvec_q4_k_avx2 :271, matvec_q8_0_avx2 :379,
// matvec_q4_0_avx2 :436, scalar fallbacks :495-635, quantize_*_to_int16 :110-172, expert_forward_gguf :690) and moe_forward_gguf
// (src/moe.rs:990) bit for bit: the 8 AVX lanes of a row are 8 GPU lanes that see exactly the bytes their AVX twin sees
// (bytes {2l, 2l+1, 16+2l, 16+2l+1} of every 32-byte chunk), run the same per-sub-block fma chain and the same hsum tree.
//
// HBM layout (built at upload from the raw row-major GGUF blocks, kr_engine.cpp::retile_gguf; one copy, nothing keeps the raw blocks):
//   Q4_K  q[rows/8][blocks][8 rows][8 lanes] x 16 B  : lane record = 4 chunks j x bytes {qs[32j+2l], qs[32j+2l+1], qs[32j+16+2l], qs[32j+17+2l]}
//         h[rows/8][blocks][8 rows] x 16 B           : {f16 d, f16 dmin, 12 scale bytes}
//   Q5_K  q as Q4_K, unchanged (low nibbles of chunk j = elements 64j + p, high nibbles = elements 64j + 32 + p, p = the byte's position in the 32-byte chunk)
//         h[rows/8][blocks][8 rows] x 48 B           : Q4_K's 16 B, then eight u32, one per lane l: {qh[2l], qh[2l+1], qh[16+2l], qh[17+2l]} -- byte i carries the fifth
//         bits of byte i of every chunk of lane l's record: bit 2j for the low nibble, bit 2j + 1 for the high nibble.  176 B per block, as in the file
//   Q3_K  q[rows/8][blocks][8 rows][8 lanes] x 12 B  : lane record = words n = 0, 1: bytes qs[32n + {2l, 2l+1, 16+2l, 17+2l}] (bits 2j of a byte = the low two bits of
//         element 128n + 32j + p, p = the byte's position in the 32 bytes), word 2: hmask[{2l, 2l+1, 16+2l, 17+2l}] (bit 4n + j = the high bit of the same element)
//         h[rows/8][blocks][8 rows] x 16 B           : {12 scale bytes, f16 d, 2 bytes of padding}.  112 B per block against 110 in the file; the one lane per row of the
//         exact kernel reads the row's 96 B of records in six 16-byte loads and the header in one, a lane of the tolerance tile its 12 B record and the header
//   Q8_0  q[rows/8][blocks/4][8][8] x 16 B (4 blocks x 4 bytes), h[rows/8][blocks/4][8] x 8 B (4 x f16 d)
//   Q4_0  q[rows/8][blocks/8][8][8] x 16 B (8 blocks x 2 bytes), h[rows/8][blocks/8][8] x 16 B (8 x f16 d)
//   Q5_0  q as Q4_0: lane l's record of a group of 8 blocks = 8 x bytes {qs[2l], qs[2l+1]}, the nibbles of elements {2l, 2l+1, 16+2l, 17+2l}
//         h[rows/8][blocks/8][8 rows] x 48 B         : {8 x f16 d, 8 x u32 qh}; bits 2l, 2l+1, 16+2l, 17+2l of a block's qh are lane l's fifth bits
//   Q6_K  q[rows/8][blocks][2 halves][8 rows][8 lanes] x 12 B : lane l's slice of a 128-element half = {ql[4l..4l+4), ql[32+4l..32+4l+4), qh[4l..4l+4)} (offsets inside the
//         half's 64 ql and 32 qh bytes): l' in [4l, 4l+4) of the reference's inner loop, 16 elements with one scale index is = l / 4
//         h[rows/8][blocks][8 rows] x 20 B           : {16 scale bytes, f16 d, 2 bytes of padding}
//   Who reads what (Q5_0 / Q6_K): a wave of the tolerance tiles (kr_gguf_dev.h: 8 rows x 8 lanes) reads 1024 B (Q5_0, per block group) / 768 B (Q6_K, per block and
//   half) of contiguous records; the one lane per row of the exact kernel below finds its row's eight lane records side by side -- 128 B per Q5_0 block group, and
//   for Q6_K the 96 B of half 0, then 768 B further the 96 B of half 1 -- and reads them with 16-byte loads.  Q5_K: a wave reads the 1024 B of a block's records and,
//   per lane, the 16 B head and one fifth-bit word of its row's header; the one lane reads 128 B of records and the 48 B header in three 16-byte loads.
#include "kr_gguf_dev.h"

// ---- scalar f32 rows (gguf_kernels.rs:572-635): one lane per row walks the reference's serial chain -- the same terms in the same order, mul, mul, add, no
//      contraction -- over the row's lane records; the records of GG_PFR5 block groups / GG_PFR6 super-blocks are requested before the first is consumed ----
#define GG_PFR5 2
#define GG_PFR6 2
__device__ __forceinline__ float gg_row_q5_0(const GgMat& m, int r, const float* x) {
    const int tile = r >> 3, row = r & 7, nb = m.K / 32, nbg = (nb + 7) / 8;
    const u32x4* q = reinterpret_cast<const u32x4*>(m.q) + ((size_t)tile * nbg * 8 + row) * 8;
    const u32x4* h = reinterpret_cast<const u32x4*>(m.h) + ((size_t)tile * nbg * 8 + row) * 3;
    float sum = 0.0f;
    for (int g0 = 0; g0 < nbg; g0 += GG_PFR5) {
        u32x4 wv[GG_PFR5][8], hv[GG_PFR5][3];
#pragma unroll
        for (int v = 0; v < GG_PFR5; v++) {
            const int gg = g0 + v < nbg ? g0 + v : nbg - 1;
#pragma unroll
            for (int l = 0; l < 8; l++) wv[v][l] = kr_ldg_nt(q + (size_t)gg * 64 + l);
#pragma unroll
            for (int i = 0; i < 3; i++) hv[v][i] = kr_ldg_nt(h + (size_t)gg * 24 + i);
        }
#pragma unroll
        for (int v = 0; v < GG_PFR5; v++) {
            const int bg = g0 + v;
            if (bg < nbg) {
                uint32_t w[8][4];
#pragma unroll
                for (int l = 0; l < 8; l++) { w[l][0] = wv[v][l].x; w[l][1] = wv[v][l].y; w[l][2] = wv[v][l].z; w[l][3] = wv[v][l].w; }
                const uint32_t db[4] = {hv[v][0].x, hv[v][0].y, hv[v][0].z, hv[v][0].w};
                const uint32_t hb[8] = {hv[v][1].x, hv[v][1].y, hv[v][1].z, hv[v][1].w, hv[v][2].x, hv[v][2].y, hv[v][2].z, hv[v][2].w};
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const int b = bg * 8 + u;
                    if (b < nb) {
                        const float d = gg_f16((db[u >> 1] >> ((u & 1) * 16)) & 0xFFFFu);
                        const uint32_t qh = hb[u];
                        const float* in = x + b * 32;
#pragma unroll
                        for (int j = 0; j < 32; j++) {
                            const uint32_t byte = (w[(j & 15) >> 1][u >> 1] >> ((u & 1) * 16 + (j & 1) * 8)) & 0xFFu;      // qs[j & 15]
                            const uint32_t q4 = j < 16 ? (byte & 0x0Fu) : ((byte >> 4) & 0x0Fu);
                            const int qv = (int)(q4 | (((qh >> j) & 1u) << 4)) - 16;
                            sum += d * (float)qv * in[j];
                        }
                    }
                }
            }
        }
    }
    return sum;
}
__device__ __forceinline__ float gg_row_q6k(const GgMat& m, int r, const float* x) {
    const int tile = r >> 3, row = r & 7, nb = m.K / 256;
    const u32x4* q = reinterpret_cast<const u32x4*>(m.q) + ((size_t)tile * nb * 16 + row) * 6;               // + (2 b + half) * 48: the row's eight slices of one half
    const uint32_t* h = reinterpret_cast<const uint32_t*>(m.h) + ((size_t)tile * nb * 8 + row) * 5;
    float sum = 0.0f;
    for (int b0 = 0; b0 < nb; b0 += GG_PFR6) {
        u32x4 wv[GG_PFR6][2][6]; uint32_t hv[GG_PFR6][5];
#pragma unroll
        for (int u = 0; u < GG_PFR6; u++) {
            const int bb = b0 + u < nb ? b0 + u : nb - 1;
#pragma unroll
            for (int i = 0; i < 12; i++) wv[u][i / 6][i % 6] = kr_ldg_nt(q + ((size_t)bb * 2 + i / 6) * 48 + i % 6);
#pragma unroll
            for (int i = 0; i < 5; i++) hv[u][i] = kr_ldg_nt(h + (size_t)bb * 40 + i);
        }
#pragma unroll
        for (int u = 0; u < GG_PFR6; u++) {
            const int b = b0 + u;
            if (b < nb) {
                const float d = gg_f16(hv[u][4] & 0xFFFFu); const float* in = x + b * 256;
#pragma unroll
                for (int hf = 0; hf < 2; hf++) {
                    uint32_t w[24];      // slice j of the half: words 3j (ql[4j..]), 3j + 1 (ql[32 + 4j..]), 3j + 2 (qh[4j..])
#pragma unroll
                    for (int i = 0; i < 6; i++) { w[4 * i] = wv[u][hf][i].x; w[4 * i + 1] = wv[u][hf][i].y; w[4 * i + 2] = wv[u][hf][i].z; w[4 * i + 3] = wv[u][hf][i].w; }
                    const int io = hf * 128;
#pragma unroll
                    for (int l = 0; l < 32; l++) {
                        const int is = l / 16, j = l >> 2, sft = (l & 3) * 8;
                        const uint32_t ql0 = (w[3 * j] >> sft) & 0xFFu, ql1 = (w[3 * j + 1] >> sft) & 0xFFu, qhb = (w[3 * j + 2] >> sft) & 0xFFu;
                        const int q0 = (int)(ql0 & 0xF) | ((int)((qhb >> 0) & 3) << 4);
                        const int q1 = (int)(ql1 & 0xF) | ((int)((qhb >> 2) & 3) << 4);
                        const int q2 = (int)((ql0 >> 4) & 0xF) | ((int)((qhb >> 4) & 3) << 4);
                        const int q3 = (int)((ql1 >> 4) & 0xF) | ((int)((qhb >> 6) & 3) << 4);
                        auto sc = [&](int k) { return (float)(int8_t)((hv[u][2 * hf + (k >> 2)] >> ((k & 3) * 8)) & 0xFFu); };      // scale byte k of this half
                        const float s0 = d * sc(is + 0), s1 = d * sc(is + 2), s2 = d * sc(is + 4), s3 = d * sc(is + 6);
                        sum += s0 * (float)(q0 - 32) * in[io + l];
                        sum += s1 * (float)(q1 - 32) * in[io + 32 + l];
                        sum += s2 * (float)(q2 - 32) * in[io + 64 + l];
                        sum += s3 * (float)(q3 - 32) * in[io + 96 + l];
                    }
                }
            }
        }
    }
    return sum;
}
// Q5_K: the reference's scalar Q4_K row (q4_k_block_dot_scalar / matvec_q4_k_scalar, gguf_kernels.rs:495-532) over dequant_q5_k's values (gguf.rs:740-803): per
// super-block s = 0, s += ((d sc_j) q - (dmin mn_j)) x_k for k = 0 .. 255 in element order, then sum += s.  Element 64j + 32 hi + p sits in record (p & 15) >> 1, word j,
// byte (p & 1) + 2 (p >> 4), nibble hi; its fifth bit is bit 2j + hi of the same byte of that record's header word.
#define GG_PFR5K 2
__device__ __forceinline__ float gg_row_q5k(const GgMat& m, int r, const float* x) {
    const int tile = r >> 3, row = r & 7, nb = m.K / 256;
    const u32x4* q = reinterpret_cast<const u32x4*>(m.q) + ((size_t)tile * nb * 8 + row) * 8;                // the row's eight lane records of a block side by side
    const u32x4* h = reinterpret_cast<const u32x4*>(m.h) + ((size_t)tile * nb * 8 + row) * 3;
    float sum = 0.0f;
    for (int b0 = 0; b0 < nb; b0 += GG_PFR5K) {
        u32x4 wv[GG_PFR5K][8], hv[GG_PFR5K][3];
#pragma unroll
        for (int u = 0; u < GG_PFR5K; u++) {
            const int bb = b0 + u < nb ? b0 + u : nb - 1;
#pragma unroll
            for (int l = 0; l < 8; l++) wv[u][l] = kr_ldg_nt(q + (size_t)bb * 64 + l);
#pragma unroll
            for (int i = 0; i < 3; i++) hv[u][i] = kr_ldg_nt(h + (size_t)bb * 24 + i);
        }
#pragma unroll
        for (int u = 0; u < GG_PFR5K; u++) {
            const int b = b0 + u;
            if (b < nb) {
                uint32_t w[8][4];
#pragma unroll
                for (int l = 0; l < 8; l++) { w[l][0] = wv[u][l].x; w[l][1] = wv[u][l].y; w[l][2] = wv[u][l].z; w[l][3] = wv[u][l].w; }
                const uint32_t f[8] = {hv[u][1].x, hv[u][1].y, hv[u][1].z, hv[u][1].w, hv[u][2].x, hv[u][2].y, hv[u][2].z, hv[u][2].w};
                const float d = gg_f16(hv[u][0].x & 0xFFFFu), dmin = gg_f16(hv[u][0].x >> 16);
                const float* in = x + b * 256;
                float s = 0.0f;
#pragma unroll
                for (int js = 0; js < 8; js++) {      // sub-block js = 2 j + hi
                    const int j = js >> 1, hi = js & 1;
                    int sc, mn;
                    gg_scale_min_k4(js, hv[u][0].y, hv[u][0].z, hv[u][0].w, sc, mn);
                    const float d1 = d * (float)sc, m1 = dmin * (float)mn;
#pragma unroll
                    for (int p = 0; p < 32; p++) {
                        const int l = (p & 15) >> 1, sft = ((p & 1) + 2 * (p >> 4)) * 8;
                        const uint32_t q4 = (w[l][j] >> (sft + 4 * hi)) & 0xFu, q5 = (f[l] >> (sft + js)) & 1u;
                        const float wk = d1 * (float)(q4 + 16u * q5) - m1;
                        s += wk * in[js * 32 + p];
                    }
                }
                sum += s;
            }
        }
    }
    return sum;
}
// Q3_K (docs/design/47-gguf-q3k.md): the same two-level chain over w = (d sc_s) q, the values kr_gguf_dev.h defines: per super-block s = 0, s += w_k x_k for k = 0 .. 255 in
// element order, then sum += s.  Element 128 n + 32 j + p sits in record (p & 15) >> 1, byte (p & 1) + 2 (p >> 4): its low two bits at bit 2j of word n, its high bit at bit
// 4n + j of word 2.  The row's eight 12-byte records are 96 B side by side: six 16-byte loads, and one for the header.
#define GG_PFR3K 2
__device__ __forceinline__ float gg_row_q3k(const GgMat& m, int r, const float* x) {
    const int tile = r >> 3, row = r & 7, nb = m.K / 256;
    const u32x4* q = reinterpret_cast<const u32x4*>(m.q) + ((size_t)tile * nb * 8 + row) * 6;
    const u32x4* h = reinterpret_cast<const u32x4*>(m.h) + (size_t)tile * nb * 8 + row;
    float sum = 0.0f;
    for (int b0 = 0; b0 < nb; b0 += GG_PFR3K) {
        u32x4 wv[GG_PFR3K][6], hv[GG_PFR3K];
#pragma unroll
        for (int u = 0; u < GG_PFR3K; u++) {
            const int bb = b0 + u < nb ? b0 + u : nb - 1;
#pragma unroll
            for (int i = 0; i < 6; i++) wv[u][i] = kr_ldg_nt(q + (size_t)bb * 48 + i);
            hv[u] = kr_ldg_nt(h + (size_t)bb * 8);
        }
#pragma unroll
        for (int u = 0; u < GG_PFR3K; u++) {
            const int b = b0 + u;
            if (b < nb) {
                uint32_t w[24];      // record l: words 3l (qs, n = 0), 3l + 1 (qs, n = 1), 3l + 2 (hmask)
#pragma unroll
                for (int i = 0; i < 6; i++) { w[4 * i] = wv[u][i].x; w[4 * i + 1] = wv[u][i].y; w[4 * i + 2] = wv[u][i].z; w[4 * i + 3] = wv[u][i].w; }
                const float d = gg_f16(hv[u].w & 0xFFFFu);
                const float* in = x + b * 256;
                float s = 0.0f;
#pragma unroll
                for (int c = 0; c < 8; c++) {      // chunk c = 4 n + j
                    const int n = c >> 2, j = c & 3;
                    const float d0 = d * (float)gg_q3k_scale(2 * c, hv[u].x, hv[u].y, hv[u].z), d1 = d * (float)gg_q3k_scale(2 * c + 1, hv[u].x, hv[u].y, hv[u].z);
#pragma unroll
                    for (int p = 0; p < 32; p++) {
                        const int l = (p & 15) >> 1, sft = ((p & 1) + 2 * (p >> 4)) * 8;
                        const int qv = (int)(((w[3 * l + n] >> (sft + 2 * j)) & 3u) | (((w[3 * l + 2] >> (sft + c)) & 1u) << 2)) - 4;
                        const float wk = (p < 16 ? d0 : d1) * (float)qv;
                        s += wk * in[c * 32 + p];
                    }
                }
                sum += s;
            }
        }
    }
    return sum;
}
__device__ __forceinline__ float gg_row_scalar(const GgMat& m, int r, const float* x) {
    return m.type == GG_Q6_K ? gg_row_q6k(m, r, x) : m.type == GG_Q5_K ? gg_row_q5k(m, r, x) : m.type == GG_Q3_K ? gg_row_q3k(m, r, x) : gg_row_q5_0(m, r, x);
}

// rows of one workgroup: the integer types take `tiles_per_wg` 8-row tiles on four waves, the scalar types one row per thread (GG_BLOCK rows)
__device__ __forceinline__ int gg_wg_tiles(int type, int tiles_per_wg) { return gg_int_path(type) ? tiles_per_wg : GG_BLOCK / 8; }

// SC: the launch holds a Q5_0 / Q3_K / Q5_K / Q6_K matrix.  The kernels without one carry no scalar-row code: the integer types keep their registers and their occupancy
template <bool SC>
__device__ __forceinline__ void gg_run_rows(const GgMat& m, const GgAct& A, float* out, int row_base_out, int tile0, int ntiles_wg) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (gg_int_path(m.type)) {
        const int ntiles = (m.N + 7) / 8;
        for (int t = wave; t < ntiles_wg; t += GG_BLOCK / 64) {
            const int tile = tile0 + t;
            if (tile >= ntiles) break;
            float r;
            if (m.type == GG_Q4_K) r = gg_tile_q4k(m, tile, A, lane);
            else if (m.type == GG_Q8_0) r = gg_tile_q8_0(m, tile, A, lane);
            else r = gg_tile_q4_0(m, tile, A, lane);
            const int row = tile * 8 + (lane >> 3);
            if ((lane & 7) == 0 && row < m.N) out[row_base_out + row] = r;
        }
    } else if constexpr (SC) {
        for (int r = tile0 * 8 + threadIdx.x; r < m.N && r < (tile0 + ntiles_wg) * 8; r += GG_BLOCK)
            out[row_base_out + r] = gg_row_scalar(m, r, A.f32v);
    }
}

extern __shared__ __attribute__((aligned(16))) char gg_smem[];

// stage 1: gu[b][slot] = [gate rows | up rows]      grid (row-tile groups of gate+up, n_slots, B)
template <bool SC>
__global__ void __launch_bounds__(GG_BLOCK) kr_gguf_w13_kernel(const GgMoeArgs a, int tiles_int) {
    const int slot = blockIdx.y, b = blockIdx.z;
    const bool shared = slot >= a.topk;
    const int e = shared ? 0 : a.ids[(size_t)b * a.topk + slot];
    if (e < 0 || (!shared && e >= a.E)) return;
    const GgMat gate = shared ? a.sgate : gg_expert_mat(a.gate, e), up = shared ? a.sup : gg_expert_mat(a.up, e);
    const int I = gate.N, nt = (I + 7) / 8, tiles_per_wg = gg_wg_tiles(gate.type, tiles_int);
    const int t0 = blockIdx.x * tiles_per_wg;
    if (t0 >= 2 * nt) return;
    const bool intp = gg_int_path(gate.type) && (a.H % 32 == 0);
    const GgAct A = gg_carve(gg_smem, a.H);
    // tiles [0, nt) are gate rows, [nt, 2nt) are up rows; a workgroup's span may straddle the boundary
    const int t1 = t0 + tiles_per_wg < 2 * nt ? t0 + tiles_per_wg : 2 * nt;
    const int ng = t0 < nt ? (t1 < nt ? t1 : nt) - t0 : 0;           // gate tiles of this workgroup, then its up tiles [us, us + nu)
    const int us = t0 > nt ? t0 - nt : 0, nu = t1 > nt ? (t1 - nt) - us : 0;
    if (a.act_f32) gg_prologue_f32_as_bf16(a.act_f32 + (size_t)b * a.H, a.H, A, !intp);
    else gg_prologue_bf16(a.act + (size_t)b * a.H, a.H, A, !intp);
    __syncthreads();
    float* gu = a.gu + ((size_t)b * a.n_slots + slot) * a.gu_ld;
    if (ng > 0) gg_run_rows<SC>(gate, A, gu, 0, t0, ng);
    if (nu > 0) gg_run_rows<SC>(up, A, gu, a.gu_ld / 2, us, nu);
}

// stage 2: eo[b][slot] = down . q(silu(gate)*up)
template <bool SC>
__global__ void __launch_bounds__(GG_BLOCK) kr_gguf_w2_kernel(const GgMoeArgs a, int tiles_int) {
    const int slot = blockIdx.y, b = blockIdx.z;
    const bool shared = slot >= a.topk;
    const int e = shared ? 0 : a.ids[(size_t)b * a.topk + slot];
    if (e < 0 || (!shared && e >= a.E)) return;
    const GgMat down = shared ? a.sdown : gg_expert_mat(a.down, e);
    const int I = down.K, nt = (down.N + 7) / 8, tiles_per_wg = gg_wg_tiles(down.type, tiles_int);
    const int t0 = blockIdx.x * tiles_per_wg;
    if (t0 >= nt) return;
    const bool intp = gg_int_path(down.type) && (I % 32 == 0);
    const GgAct A = gg_carve(gg_smem, I);
    const float* gu = a.gu + ((size_t)b * a.n_slots + slot) * a.gu_ld;
    // gu holds gate at [0,I) and up at [gu_ld/2, gu_ld/2+I): present them contiguously to the prologue
    gg_prologue_hidden_split(gu, gu + a.gu_ld / 2, I, A, !intp, intp);
    __syncthreads();
    gg_run_rows<SC>(down, A, a.eo + ((size_t)b * a.n_slots + slot) * a.H, 0, t0, tiles_per_wg);
}

// grid x of one stage: the workgroups of the slot kind (routed / shared) that needs most -- an integer type takes tiles_int tiles per workgroup, a scalar type 32
// (gg_wg_tiles); the workgroups a slot does not need leave at the top of the kernel
static int gg_grid_x(const GgMoeArgs& a, int ntiles, int tiles_int, int routed_type, int shared_type) {
    auto wgs = [&](int type) { const int tpw = gg_int_path(type) ? tiles_int : GG_BLOCK / 8; return (ntiles + tpw - 1) / tpw; };
    const int r = a.topk > 0 ? wgs(routed_type) : 0, s = a.n_slots > a.topk ? wgs(shared_type) : 0;
    return r > s ? r : (s > 0 ? s : 1);
}
void kr_launch_gguf_moe(const GgMoeArgs& a, hipStream_t st) {
    {
        const int nt2 = 2 * ((a.I_max + 7) / 8);
        int tpw = 8; while (tpw > 4 && (nt2 + tpw - 1) / tpw < 64) tpw >>= 1;
        dim3 grid(gg_grid_x(a, nt2, tpw, a.gate.type, a.sgate.type), a.n_slots, a.B);
        const bool sc = (a.topk > 0 && !gg_int_path(a.gate.type)) || (a.n_slots > a.topk && !gg_int_path(a.sgate.type));
        if (sc) hipLaunchKernelGGL(kr_gguf_w13_kernel<true>, grid, dim3(GG_BLOCK), gg_lds_bytes(a.H, true), st, a, tpw);
        else hipLaunchKernelGGL(kr_gguf_w13_kernel<false>, grid, dim3(GG_BLOCK), gg_lds_bytes(a.H, true), st, a, tpw);
    }
    {
        const int nt = (a.H + 7) / 8;
        int tpw = 8; while (tpw > 4 && (nt + tpw - 1) / tpw < 64) tpw >>= 1;
        dim3 grid(gg_grid_x(a, nt, tpw, a.down.type, a.sdown.type), a.n_slots, a.B);
        const bool sc = (a.topk > 0 && !gg_int_path(a.down.type)) || (a.n_slots > a.topk && !gg_int_path(a.sdown.type));
        if (sc) hipLaunchKernelGGL(kr_gguf_w2_kernel<true>, grid, dim3(GG_BLOCK), gg_lds_bytes(a.I_max, true), st, a, tpw);
        else hipLaunchKernelGGL(kr_gguf_w2_kernel<false>, grid, dim3(GG_BLOCK), gg_lds_bytes(a.I_max, true), st, a, tpw);
    }
}

// ---- kr_gguf_matvec: y = W x of one Q5_0 / Q3_K / Q5_K / Q6_K matrix with the device functions above as one launch.  parts 0: the exact chain, one lane per row, GG_BLOCK rows a
//      workgroup; parts 1 | 2: the tolerance tile, one 8-row tile per wave, the row's blocks walked whole or as two slices whose results are added (what the two
//      k-waves of the mode's gate|up launch do) ----
__global__ void __launch_bounds__(GG_BLOCK) kr_gguf_matvec_kernel(const GgMat m, const float* x, float* y, int parts) {
    float* xs = reinterpret_cast<float*>(gg_smem);
    for (int i = threadIdx.x; i < m.K; i += GG_BLOCK) xs[i] = x[i];
    __syncthreads();
    if (parts == 0) {
        const int r = blockIdx.x * GG_BLOCK + threadIdx.x;
        if (r < m.N) y[r] = gg_row_scalar(m, r, xs);
        return;
    }
    GgAct A{}; A.f32v = xs;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, tile = blockIdx.x * (GG_BLOCK / 64) + wave;
    if (tile >= (m.N + 7) / 8) return;
    float r = gg_tile_scalar(m, tile, A, lane, 0, parts);
    if (parts == 2) r = r + gg_tile_scalar(m, tile, A, lane, 1, 2);
    const int row = tile * 8 + (lane >> 3);
    if ((lane & 7) == 0 && row < m.N) y[row] = r;
}
int kr_launch_gguf_matvec(const GgMat& m, const float* x, float* y, int parts, hipStream_t st) {
    if (!gg_scalar_type(m.type) || parts < 0 || parts > 2 || m.N < 1 || m.K < 1 || m.K % (m.type == GG_Q5_0 ? 32 : 256) || (size_t)m.K * 4 > 60 * 1024) return 1;
    const int rows_wg = parts == 0 ? GG_BLOCK : 8 * (GG_BLOCK / 64);
    hipLaunchKernelGGL(kr_gguf_matvec_kernel, dim3((m.N + rows_wg - 1) / rows_wg), dim3(GG_BLOCK), (size_t)m.K * 4, st, m, x, y, parts);
    return 0;
}

size_t gg_q_bytes(int type, int K, int N) {
    const size_t nt = (size_t)(N + 7) / 8;
    switch (type) {
        case GG_Q4_K: case GG_Q5_K: return nt * (K / 256) * 64 * 16;
        case GG_Q8_0: return nt * (((K / 32) + 3) / 4) * 64 * 16;
        case GG_Q4_0: return nt * (((K / 32) + 7) / 8) * 64 * 16;
        case GG_Q5_0: return nt * (((K / 32) + 7) / 8) * 64 * 16;
        case GG_Q6_K: return nt * (K / 256) * 2 * 64 * 12;
        case GG_Q3_K: return nt * (K / 256) * 64 * 12;
        default: return 0;
    }
}
size_t gg_h_bytes(int type, int K, int N) {
    const size_t nt = (size_t)(N + 7) / 8;
    switch (type) {
        case GG_Q4_K: case GG_Q3_K: return nt * (K / 256) * 8 * 16;
        case GG_Q5_K: return nt * (K / 256) * 8 * 48;
        case GG_Q8_0: return nt * (((K / 32) + 3) / 4) * 8 * 8;
        case GG_Q4_0: return nt * (((K / 32) + 7) / 8) * 8 * 16;
        case GG_Q5_0: return nt * (((K / 32) + 7) / 8) * 8 * 48;
        case GG_Q6_K: return nt * (K / 256) * 8 * 20;
        default: return 16;
    }
}
