// kr_gguf_prefill_h.hip -- KR_GEMM_FAST (tolerance) prompt-pass GEMM for Q6_K and Q5_0 experts: f16 activation rows x block weights de-quantized in
// registers on v_mfma_f32_32x32x16_f16, f32 accumulation over the WHOLE k range.  The sibling of kr_pfh_gemm_kernel (kr_prefill_h.hip) for the two block
// types the reference walks with one serial f32 chain per row (gguf_kernels.rs:572-635): there is no integer form of them to reproduce, so their matrix-core
// form lives in the stated-tolerance mode only; the default pass and "gguf_exact_pass" keep the streaming kernels and their bits.
//
// No derived copy.  The Q4_K / Q8_0 tolerance forms re-tile into a second copy (gg_ensure_fast); this kernel reads the lane records retile_gguf wrote
// and the decode step reads (kr_gguf.hip header):
//   Q6_K  q[rows/8][blocks][2 halves][8 rows][8 lanes] x 12 B, h[rows/8][blocks][8 rows] x 20 B   -- one stage = one super-block (256 k)
//   Q5_0  q[rows/8][blocks/8][8 rows][8 lanes] x 16 B,         h[rows/8][blocks/8][8 rows] x 48 B -- one stage = one group of 8 blocks (256 k)
//
// k order.  A lane record is not a run of consecutive k: lane l of a Q6_K half holds elements {4l + i, 32 + 4l + i, 64 + 4l + i, 96 + 4l + i}, i < 4; lane l
// of a Q5_0 block group holds elements {2l, 2l + 1, 16 + 2l, 17 + 2l} of each of its 8 blocks.  An MFMA sums over k in any order as long as both operands
// agree, so the B side is left as stored and the permutation lives in HOW A IS LAID INTO LDS: the commit pass of a stage writes a row's 256 values as
// [record l][the record's elements in the order the unpack emits them] -- Q6_K [half][l][g = 0..3][i = 0..3], Q5_0 [l][block u = 0..7][e = 0..3].  A
// fragment of 8 values (one operand of one MFMA) is then 16 contiguous bytes in both cases and is read with one ds_read_b128, exactly as in the sibling
// kernel: LDS READ width is unchanged.  The cost is on the WRITE side: a 16-byte chunk of a row (8 consecutive k) scatters to two 8-byte pieces (Q6_K:
// records 2c and 2c + 1) or four 4-byte pieces (Q5_0: four records), 2x / 4x the ds_write instructions of a verbatim copy -- 16 / 32 per lane per stage,
// against the 8 x 4 waves x (4 | 2) fragment reads the same stage issues.  (The permutation on the read side would turn every fragment read of every wave
// into two b64 / four b32 reads.)
//
// LDS map (bytes; one stage):                                        Q6_K            Q5_0
//   As   [64 rows][528]         f16, permuted as above               33 792          33 792
//   Bs   raw records            Q6_K [16 tiles][1552]: the 2 x 768 B of a tile's super-block verbatim, 16 B of padding a tile (tile stride = 4 banks mod 64)
//                               Q5_0 [128 cols][144]: the 8 records of a column side by side, 16 B of padding a column
//                                                                    24 832          18 432
//   rmul[64] row_src[64] row_dst[64]                                    768             768
//                                                                    59 392          52 992      -> two workgroups per CU
//   Headers (Q6_K: 16 scale bytes + f16 d; Q5_0: 8 x f16 d + 8 x u32 qh of the lane's column) go global -> registers, one stage ahead, as the sibling
//   kernel holds its group scales: every lane needs every header word of its column, LDS would only add a round trip.
//
// Tile: 64 sorted rows of one expert x 128 weight rows per workgroup of 4 waves, each wave 64 x 32 = two 32 x 32 accumulators.  Every global load of stage
// st + 1 (8 A chunks, 6 | 4 record chunks, 5 | 12 header words per lane) is issued before the MFMA loop of stage st.  A lane (column n, k half kh) walks the
// records l = 2 t + kh, t < 4: a 12-byte Q6_K record of each half gives two fragments (g = 0, 1 | g = 2, 3), a 16-byte Q5_0 record four (blocks 2f, 2f + 1).
//
// Numerics.  A operand: the f16 rows of kr_prefill_h.hip (row scaled by a power of two, RNE to 11 bits; the multiplier 2^e / 16 comes back in the final
// store, or in the combine pass for f16 output rows).  Weights: the code minus its centre is formed EXACTLY in f16 on whole words -- Q6_K: four 6-bit codes
// from one ql and one qh word with three masks (the unpack of gg_tile_q6k); Q5_0: four 5-bit codes of two blocks from one record word, the fifth bits spread
// from the two qh words by one shift, one mask and one byte permute -- each code byte placed under the exponent of 1024.0 (0x6400 | q = 1024 + q) and
// 1056 | 1040 subtracted: q - 32 | q - 16, exact.  The scale is folded into the fragment with one f16 multiplication (one rounding to 11 bits of a
// 6 + 11 bit product): Q6_K 16 d sc, the exact product of the f16 d and the 8-bit sc rounded ONCE to f16 (v_pk_mul_f16 of 16 d -- exact -- and sc -- exact --
// is that rounding); Q5_0 16 d, exact.  The factor 16 keeps small scales out of the f16 subnormals (Q6_K's d is ~1e-5 for weights of ~0.05).  Products are
// accumulated by the MFMA in f32.  Neither type has an offset term once the code is centred: no per-32 sums of A, no extra k columns.
//
// Q5_K and Q3_K (docs/design/45-gguf-q5k.md, 47-gguf-q3k.md) came later and share Q5_0's A image.  Q3_K: 12-byte records, q[rows/8][blocks][8 rows][8 lanes], and 16-byte
// headers; lane l of a super-block holds elements {2l, 2l + 1, 16 + 2l, 17 + 2l} of each 32-element chunk c < 8, so a row's 256 values are laid [record l][chunk c][4 values] --
// Q5_0's image with "block u" read as "chunk c", the same four 4-byte pieces per 16-byte chunk of A.  Bs holds a tile's 768 B verbatim, [16 tiles][784], as Q6_K's does.  The
// 3-bit code (two bits of a qs word, one bit of the hmask word) goes under the exponent of 1024.0 and 1028 is subtracted: q - 4, exact; the scale 16 d sc (sc the 6-bit scale
// minus 32, formed the same way with 1056) is rounded once to f16.  33 792 + 12 544 + 768 = 47 104 B of LDS.
//
// Limits: Q6_K, Q5_K, Q3_K K % 256 == 0, Q5_0 K % 32 == 0 (the last block group may be ragged: its missing blocks get scale 0, its A chunks re-read the head of the
// stage), N % 8 == 0, K % 8 == 0 rows of at most 4 GiB in all (32-bit row offsets, as the sibling).  Loads are never masked: a row past the tile reads row 0,
// a column tile past the last re-reads the last; the stores are guarded.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "kr_lds_optin.h"
#include "kr_device.h"
#include "kr_kernels.h"
#include "kr_prefill.h"
#include "kr_gguf.h"
#include "kr_pfh_dev.h"
#include "kr_gguf_dev.h"               // gg_q3k_scales4

#define GFH_BM 64
#define GFH_BN 128
#define GFH_KS 256
#define GFH_LDA (GFH_KS * 2 + 16)      // bytes per A row of a stage
#define GFH_T6 1552                    // Q6_K: bytes per 8-column tile of a stage (2 halves x 768 B + 16)
#define GFH_LDB5 144                   // Q5_0: bytes per column of a stage (8 records x 16 B + 16)
#define GFH_T3 784                     // Q3_K: bytes per 8-column tile of a stage (768 B + 16: tile stride = 4 banks mod 64, as GFH_T6)

struct KrGfhArgs {
    GgMat m;
    const uint16_t* a; const float* a_mul;      // f16 rows [rows_or_tokens][K] (image order of kr_pfh_dev.h), row multipliers
    const int* row_pair; int topk; int gather_tokens;
    const int* tile_expert; const int* tile_row0; const int* tile_rows; const int* n_tiles;
    void* out; int out_ld; int out_f16;         // out_f16: f16 rows of RAW accumulators (kr_pf_combine_kernel<2> applies the row multiplier), else f32 rows
    int single_expert; int total_rows; int run;
};

// 4 code bytes (one word) -> 4 f16 (code - centre) * scale: lo pair scaled by s_lo, hi pair by s_hi
__device__ __forceinline__ void gfh_bytes4(uint32_t codes, v2h off, v2h s01, v2h s23, v2h& r01, v2h& r23) {
    const uint32_t Kc = 0x64646464u;
    const uint32_t t0 = __builtin_amdgcn_perm(Kc, codes, 0x04010400u), t1 = __builtin_amdgcn_perm(Kc, codes, 0x04030402u);
    r01 = (__builtin_bit_cast(v2h, t0) + off) * s01;
    r23 = (__builtin_bit_cast(v2h, t1) + off) * s23;
}

// Q5_K: 4 code bytes of one sub-block -> 4 f16 values code * s + nm, s = 16 d sc, nm = -16 dmin mn, one rounding each (v_pk_fma_f16)
__device__ __forceinline__ void gfh_q5k4(uint32_t codes, v2h off, v2h s, v2h nm, v2h& r01, v2h& r23) {
    const uint32_t Kc = 0x64646464u;
    const uint32_t t0 = __builtin_amdgcn_perm(Kc, codes, 0x04010400u), t1 = __builtin_amdgcn_perm(Kc, codes, 0x04030402u);
    r01 = __builtin_elementwise_fma(__builtin_bit_cast(v2h, t0) + off, s, nm);
    r23 = __builtin_elementwise_fma(__builtin_bit_cast(v2h, t1) + off, s, nm);
}

template <int TYPE>
__global__ void __launch_bounds__(256, 2) kr_gfh_gemm_kernel(const KrGfhArgs a) {
    static_assert(TYPE == GG_Q6_K || TYPE == GG_Q5_0 || TYPE == GG_Q5_K || TYPE == GG_Q3_K, "lane-record form of Q6_K, Q5_0, Q5_K and Q3_K");
    constexpr bool Q6 = TYPE == GG_Q6_K, Q5K = TYPE == GG_Q5_K;      // Q5_K shares Q5_0's stage geometry: 16-byte records, 48-byte headers, the same As / Bs maps
    constexpr bool Q3K = TYPE == GG_Q3_K;                            // Q3_K: Q5_0's As map (its "block u" = the 32-element chunk c), tile-wise Bs of 12-byte records as Q6_K
    constexpr int LDA = GFH_LDA, BS_BYTES = Q6 ? 16 * GFH_T6 : Q3K ? 16 * GFH_T3 : GFH_BN * GFH_LDB5;
    constexpr int NBC = Q6 ? 6 : Q3K ? 3 : 4;     // 16-byte record chunks per thread per stage
    constexpr int NHW = Q6 ? 5 : Q5K ? 8 : Q3K ? 4 : 12;    // header words per lane per stage (Q5_K: the 16-byte head and the fifth-bit words of the lane's four records; Q3_K: the 16-byte header)
    constexpr int TB = Q6 ? 1536 : Q3K ? 768 : 1024;        // record bytes of an 8-column tile per stage
    constexpr int HB = Q6 ? 20 : Q3K ? 16 : 48;             // header bytes of a column per stage
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* As = smem;
    char* Bs = As + GFH_BM * LDA;
    float* rmul = reinterpret_cast<float*>(Bs + BS_BYTES);
    int* row_src = reinterpret_cast<int*>(rmul + GFH_BM);
    int* row_dst = row_src + GFH_BM;

    const GgMat m = a.m;
    const int K = m.K, N = m.N;
    const int ncb = (N + GFH_BN - 1) / GFH_BN;
    int mt, cb;
    if (a.single_expert) { cb = blockIdx.x % ncb; mt = blockIdx.x / ncb; }
    else {      // `run` consecutive row tiles (mostly one expert's) on one XCD, as the sibling kernel orders them
        const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, per = ncb * a.run, grp = slot / per, local = slot - grp * per;
        mt = (grp * 8 + xcd) * a.run + local / ncb; cb = local % ncb;
    }
    int expert, row0, rows;
    if (a.single_expert) { expert = 0; row0 = mt * GFH_BM; rows = a.total_rows - row0 < GFH_BM ? a.total_rows - row0 : GFH_BM; if (rows <= 0) return; }
    else { if (mt >= a.n_tiles[0]) return; expert = a.tile_expert[mt]; row0 = a.tile_row0[mt]; rows = a.tile_rows[mt]; }
    const int n0 = cb * GFH_BN;
    const bool two = rows > 32;                    // uniform: a tile of at most 32 rows skips the second row block
    const char* wq = reinterpret_cast<const char*>(m.q) + (size_t)expert * m.q_stride;
    const char* wh = reinterpret_cast<const char*>(m.h) + (size_t)expert * m.h_stride;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, n31 = lane & 31, khalf = lane >> 5;
    const int nblk = Q6 ? K / 256 : K / 32;        // blocks of the type along k
    const int nst = Q6 ? nblk : (nblk + 7) / 8;    // stages = super-blocks | block groups
    const int last_tile = (N - 1) >> 3;

    v16f acc[2][1];
#pragma unroll
    for (int s = 0; s < 2; s++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[s][0][r] = 0.0f;

    int col[1] = {n0 + wave * 32 + n31};
    const int lc = wave * 32 + n31, cc = col[0] < N ? col[0] : N - 1;
    // this lane's column: header base (bytes, without the stage term) and record base inside Bs
    const uint32_t hbase = (uint32_t)(((cc >> 3) * nst * 8 + (cc & 7)) * HB);
    const int bcol = Q6 ? (lc >> 3) * GFH_T6 + (lc & 7) * 96 : Q3K ? (lc >> 3) * GFH_T3 + (lc & 7) * 96 : lc * GFH_LDB5;

    // record chunks of a stage: Q6_K 16 tiles x 96 chunks (a tile's super-block is 1536 contiguous bytes), Q5_0 16 tiles x 64 chunks (1024 bytes), Q3_K 16 tiles x 48 chunks (768 bytes)
    uint32_t bsrc[NBC], bdst[NBC];
#pragma unroll
    for (int j = 0; j < NBC; j++) {
        const int idx = tid + j * 256, t8 = Q6 ? idx / 96 : Q3K ? idx / 48 : idx >> 6, c = Q6 ? idx - t8 * 96 : Q3K ? idx - t8 * 48 : idx & 63;
        int tile = (n0 >> 3) + t8; tile = tile < last_tile ? tile : last_tile;
        bsrc[j] = (uint32_t)tile * (uint32_t)nst * (uint32_t)TB + (uint32_t)c * 16u;
        bdst[j] = Q6 ? (uint32_t)(t8 * GFH_T6 + c * 16) : Q3K ? (uint32_t)(t8 * GFH_T3 + c * 16) : (uint32_t)((t8 * 8 + (c >> 3)) * GFH_LDB5 + (c & 7) * 16);
    }
    // A chunks: load j of a thread = row 8 j + (tid >> 5), chunk ck = tid & 31 of the stage's 32 (whole 128-byte lines per 8 lanes, as the sibling)
    const int arow = tid >> 5, ck = tid & 31;
    // where the chunk's 8 values go inside the row's stage image (see "k order" above)
    const int adst = Q6 ? (ck >> 4) * 256 + (ck & 3) * 64 + ((ck & 15) >> 2) * 8 : ((ck & 3) & 1) * 256 + (ck >> 2) * 8 + ((ck & 3) >> 1) * 4;
    const uint32_t* rofs = reinterpret_cast<const uint32_t*>(row_src);

    u32x4 pa[8], pb[NBC];
    uint32_t ph[NHW], hw[NHW];
    auto load_B = [&](int st) {
#pragma unroll
        for (int j = 0; j < NBC; j++) pb[j] = kr_ldg_nt(reinterpret_cast<const u32x4*>(wq + bsrc[j] + (size_t)st * TB));
        if constexpr (Q6) {
            const uint32_t* hp = reinterpret_cast<const uint32_t*>(wh + hbase + (size_t)st * 160);
#pragma unroll
            for (int i = 0; i < 5; i++) ph[i] = kr_ldg_nt(hp + i);
        } else if constexpr (Q3K) {
            const u32x4 v = kr_ldg_nt(reinterpret_cast<const u32x4*>(wh + hbase + (size_t)st * 128));
            ph[0] = v.x; ph[1] = v.y; ph[2] = v.z; ph[3] = v.w;
        } else if constexpr (Q5K) {
            const char* hp = wh + hbase + (size_t)st * 384;
            const u32x4 v = kr_ldg_nt(reinterpret_cast<const u32x4*>(hp));
            ph[0] = v.x; ph[1] = v.y; ph[2] = v.z; ph[3] = v.w;
#pragma unroll
            for (int t = 0; t < 4; t++) ph[4 + t] = kr_ldg_nt(reinterpret_cast<const uint32_t*>(hp + 16) + 2 * t + khalf);      // record l = 2 t + khalf
        } else {
            const u32x4* hp = reinterpret_cast<const u32x4*>(wh + hbase + (size_t)st * 384);
#pragma unroll
            for (int i = 0; i < 3; i++) { const u32x4 v = kr_ldg_nt(hp + i); ph[4 * i] = v.x; ph[4 * i + 1] = v.y; ph[4 * i + 2] = v.z; ph[4 * i + 3] = v.w; }
        }
    };
    auto load_A = [&](int st) {
        const int ckv = st * GFH_KS + ck * 8 < K ? ck : 0;       // a chunk past K (ragged Q5_0 stage) re-reads the head of the stage; its blocks get scale 0
        const char* ab = reinterpret_cast<const char*>(a.a) + (size_t)st * (GFH_KS * 2) + ckv * 16;
#pragma unroll
        for (int j = 0; j < 8; j++) pa[j] = *reinterpret_cast<const u32x4*>(ab + rofs[arow + 8 * j]);
    };

    if (wave != 0) load_B(0);      // the weight stream does not wait for the row table (wave 0 builds it first: in-order load counter)
    float mulv = 0.0f;
    if (tid < GFH_BM) {
        int src = -1;
        if (tid < rows) {
            if (a.single_expert) src = row0 + tid;
            else { const int pair = a.row_pair[row0 + tid]; src = a.gather_tokens ? pair / a.topk : row0 + tid; }
        }
        row_src[tid] = (int)((uint32_t)(src < 0 ? 0 : src) * (uint32_t)(K * 2));
        row_dst[tid] = row0 + tid;
        if (src >= 0) mulv = a.a_mul[src];
    }
    __syncthreads();
    if (wave == 0) load_B(0);
    load_A(0);

    auto commit_stage = [&]() {
#pragma unroll
        for (int i = 0; i < NHW; i++) hw[i] = ph[i];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            // the row image holds (a0,a4 | a1,a5 | a2,a6 | a3,a7) (kr_pfh_dev.h) -> natural pairs
            const u32x4 v = pa[j];
            const uint32_t n01 = __builtin_amdgcn_perm(v.y, v.x, 0x05040100u), n23 = __builtin_amdgcn_perm(v.w, v.z, 0x05040100u);
            const uint32_t n45 = __builtin_amdgcn_perm(v.y, v.x, 0x07060302u), n67 = __builtin_amdgcn_perm(v.w, v.z, 0x07060302u);
            char* d = As + (arow + 8 * j) * LDA + adst;
            if constexpr (Q6) {
                *reinterpret_cast<u32x2*>(d) = u32x2{n01, n23};            // record 2c:     i = 0..3 of run g
                *reinterpret_cast<u32x2*>(d + 32) = u32x2{n45, n67};       // record 2c + 1
            } else {
                *reinterpret_cast<uint32_t*>(d) = n01; *reinterpret_cast<uint32_t*>(d + 64) = n23;         // records 4 (c & 1) + 0..3: the pair (2l, 2l + 1) or (16 + 2l, 17 + 2l)
                *reinterpret_cast<uint32_t*>(d + 128) = n45; *reinterpret_cast<uint32_t*>(d + 192) = n67;
            }
        }
#pragma unroll
        for (int j = 0; j < NBC; j++) *reinterpret_cast<u32x4*>(Bs + bdst[j]) = pb[j];
    };

    // the MFMA loop of one stage: 8 half-records per lane, each 2 fragments = 2 k-steps of 16 for NSA row blocks
    auto stage_mfma = [&](int st, auto nsa) {
        constexpr int NSA = decltype(nsa)::value;
        const v2h c16 = {(_Float16)16.0f, (_Float16)16.0f};
        v2h sc[8];              // Q6_K, Q3_K: the 16 scales 16 d sc_j as f16 pairs (j = 2 p, 2 p + 1); Q5_0: sc[f] = 16 (d_2f, d_2f+1), f < 4
        if constexpr (Q6) {
            const uint32_t dw = hw[4] & 0xFFFFu;
            const v2h d16 = __builtin_bit_cast(v2h, dw | (dw << 16)) * c16;
            const v2h o8 = {(_Float16)-1152.0f, (_Float16)-1152.0f};
#pragma unroll
            for (int w = 0; w < 4; w++) {
                const uint32_t x = hw[w] ^ 0x80808080u;      // (1024 + (b ^ 0x80)) - 1152 = the signed byte
                sc[2 * w] = (__builtin_bit_cast(v2h, __builtin_amdgcn_perm(0x64646464u, x, 0x04010400u)) + o8) * d16;
                sc[2 * w + 1] = (__builtin_bit_cast(v2h, __builtin_amdgcn_perm(0x64646464u, x, 0x04030402u)) + o8) * d16;
            }
        } else if constexpr (Q3K) {      // sc[2 g], sc[2 g + 1] = 16 d (sc_4g .. sc_4g+3): the four 6-bit scales of group g as one word, each byte under the exponent of 1024.0, minus 1056
            const uint32_t dw = hw[3] & 0xFFFFu;
            const v2h d16 = __builtin_bit_cast(v2h, dw | (dw << 16)) * c16;
            const v2h o32 = {(_Float16)-1056.0f, (_Float16)-1056.0f};
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const uint32_t x = gg_q3k_scales4(g, hw[0], hw[1], hw[2]);
                sc[2 * g] = (__builtin_bit_cast(v2h, __builtin_amdgcn_perm(0x64646464u, x, 0x04010400u)) + o32) * d16;
                sc[2 * g + 1] = (__builtin_bit_cast(v2h, __builtin_amdgcn_perm(0x64646464u, x, 0x04030402u)) + o32) * d16;
            }
        } else if constexpr (Q5K) {      // sc[js] = (16 d sc_js, -16 dmin mn_js), js < 8: each the exact product of two f16 values rounded once
            const v2h dm16 = __builtin_bit_cast(v2h, hw[0]) * c16;
#pragma unroll
            for (int js = 0; js < 8; js++) {
                const uint32_t b_lo = (hw[1] >> ((js & 3) * 8)) & 0xFFu, b_mid = (hw[2] >> ((js & 3) * 8)) & 0xFFu, b_hi = (hw[3] >> ((js & 3) * 8)) & 0xFFu;
                // get_scale_min_k4: bytes j, j + 4 (j < 4) | bytes j + 4, j - 4, j (j >= 4) of the 12 scale bytes hw[1..3]
                const uint32_t scq = js < 4 ? (b_lo & 63u) : ((b_hi & 0xFu) | ((b_lo >> 6) << 4)), mnq = js < 4 ? (b_mid & 63u) : ((b_hi >> 4) | ((b_mid >> 6) << 4));
                const v2h q = {(_Float16)(float)scq, (_Float16)-(float)mnq};
                sc[js] = q * dm16;
            }
        } else {
#pragma unroll
            for (int f = 0; f < 4; f++) {
                uint32_t dd = hw[f];
                if (st * 8 + 2 * f >= nblk) dd = 0; else if (st * 8 + 2 * f + 1 >= nblk) dd &= 0xFFFFu;      // blocks past K: scale 0
                sc[f] = __builtin_bit_cast(v2h, dd) * c16;
            }
        }
        v8h af[2][NSA][2];
        uint32_t br[2][3];
        auto rd = [&](int hr, int buf) {
            // Q6_K: hr = 4 half + t; Q5_0, Q5_K, Q3_K: hr = 2 t + (record half); record l = 2 t + khalf
            const int t = Q6 ? (hr & 3) : (hr >> 1), l = 2 * t + khalf;
            const int aoff = Q6 ? (hr >> 2) * 256 + l * 32 : l * 64 + (hr & 1) * 32;
#pragma unroll
            for (int s2 = 0; s2 < NSA; s2++) {
                af[buf][s2][0] = *reinterpret_cast<const v8h*>(As + (s2 * 32 + n31) * LDA + aoff);
                af[buf][s2][1] = *reinterpret_cast<const v8h*>(As + (s2 * 32 + n31) * LDA + aoff + 16);
            }
            if constexpr (Q6) {
                const uint32_t* p = reinterpret_cast<const uint32_t*>(Bs + bcol + (hr >> 2) * 768 + l * 12);
                br[buf][0] = p[0]; br[buf][1] = p[1]; br[buf][2] = p[2];
            } else if constexpr (Q3K) {      // half n = hr & 1 of the record: its qs word and the hmask word
                const uint32_t* p = reinterpret_cast<const uint32_t*>(Bs + bcol + l * 12);
                br[buf][0] = p[hr & 1]; br[buf][1] = p[2];
            } else {
                const u32x2 p = *reinterpret_cast<const u32x2*>(Bs + bcol + l * 16 + (hr & 1) * 8);
                br[buf][0] = p.x; br[buf][1] = p.y;
            }
        };
        auto dq = [&](int hr, int buf, v8h (&bf)[2]) {
            v2h r0, r1, r2, r3;
            if constexpr (Q6) {
                const int hf = hr >> 2, is = (hr & 3) >> 1;      // scale index of the record: l / 4 = t / 2
                const v2h o = {(_Float16)-1056.0f, (_Float16)-1056.0f};
                const uint32_t ql = br[buf][0], qm = br[buf][1], qh = br[buf][2];      // ql[4l..], ql[32 + 4l..], qh[4l..] of the half
                // scale of run g: byte 8 hf + is + 2 g = word 2 hf + (g >> 1), byte is + 2 (g & 1) -> pair sc[4 hf + 2 (g >> 1) + (g & 1)], component is
                auto S = [&](int g) { const v2h p = sc[4 * hf + g]; const _Float16 s = is ? p.y : p.x; return v2h{s, s}; };
                gfh_bytes4((ql & 0x0F0F0F0Fu) | ((qh & 0x03030303u) << 4), o, S(0), S(0), r0, r1);
                gfh_bytes4((qm & 0x0F0F0F0Fu) | ((qh & 0x0C0C0C0Cu) << 2), o, S(1), S(1), r2, r3);
                bf[0] = v8h{r0.x, r0.y, r1.x, r1.y, r2.x, r2.y, r3.x, r3.y};
                gfh_bytes4(((ql >> 4) & 0x0F0F0F0Fu) | (qh & 0x30303030u), o, S(2), S(2), r0, r1);
                gfh_bytes4(((qm >> 4) & 0x0F0F0F0Fu) | ((qh >> 2) & 0x30303030u), o, S(3), S(3), r2, r3);
                bf[1] = v8h{r0.x, r0.y, r1.x, r1.y, r2.x, r2.y, r3.x, r3.y};
            } else if constexpr (Q3K) {
                // word n = hr & 1 of the record holds the chunks c = 4 n + j: bits 2j of its bytes and bit c of the hmask bytes are the four codes of chunk c in the order As
                // holds them; bytes 0, 1 belong to sub-block 2 c, bytes 2, 3 to sub-block 2 c + 1 = the pair sc[c].  Fragment ff = chunks 4 n + 2 ff, 4 n + 2 ff + 1
                const int n = hr & 1;
                const uint32_t w = br[buf][0], hm = br[buf][1];
                const v2h o = {(_Float16)-1028.0f, (_Float16)-1028.0f};
#pragma unroll
                for (int ff = 0; ff < 2; ff++) {
                    const int c0 = 4 * n + 2 * ff, c1 = c0 + 1;
                    gfh_bytes4(((w >> (4 * ff)) & 0x03030303u) | (((hm >> c0) & 0x01010101u) << 2), o, v2h{sc[c0].x, sc[c0].x}, v2h{sc[c0].y, sc[c0].y}, r0, r1);
                    gfh_bytes4(((w >> (4 * ff + 2)) & 0x03030303u) | (((hm >> c1) & 0x01010101u) << 2), o, v2h{sc[c1].x, sc[c1].x}, v2h{sc[c1].y, sc[c1].y}, r2, r3);
                    bf[ff] = v8h{r0.x, r0.y, r1.x, r1.y, r2.x, r2.y, r3.x, r3.y};
                }
            } else if constexpr (Q5K) {
                // word j of the record = chunk j: low nibbles the four values of sub-block 2 j, high nibbles those of sub-block 2 j + 1, in the order As holds them;
                // the fifth bits come from the record's header word under one mask per (chunk, nibble), as in gg_tile_q5k
                const uint32_t fb = hw[4 + (hr >> 1)];
                const v2h o = {(_Float16)-1024.0f, (_Float16)-1024.0f};
#pragma unroll
                for (int ff = 0; ff < 2; ff++) {
                    const int j = 2 * (hr & 1) + ff;
                    const uint32_t w = br[buf][ff];
                    const uint32_t f_lo = (j < 2 ? fb << (4 - 2 * j) : fb >> (2 * j - 4)) & 0x10101010u, f_hi = (j < 2 ? fb << (3 - 2 * j) : fb >> (2 * j - 3)) & 0x10101010u;
                    const uint32_t lo = (w & 0x0F0F0F0Fu) | f_lo, hi = ((w >> 4) & 0x0F0F0F0Fu) | f_hi;
                    const v2h s_lo = {sc[2 * j].x, sc[2 * j].x}, m_lo = {sc[2 * j].y, sc[2 * j].y}, s_hi = {sc[2 * j + 1].x, sc[2 * j + 1].x}, m_hi = {sc[2 * j + 1].y, sc[2 * j + 1].y};
                    gfh_q5k4(lo, o, s_lo, m_lo, r0, r1);
                    gfh_q5k4(hi, o, s_hi, m_hi, r2, r3);
                    bf[ff] = v8h{r0.x, r0.y, r1.x, r1.y, r2.x, r2.y, r3.x, r3.y};
                }
            } else {
                const int t = hr >> 1, sh = 4 * t + 2 * khalf;      // 2 l
                const v2h o = {(_Float16)-1040.0f, (_Float16)-1040.0f};
#pragma unroll
                for (int ff = 0; ff < 2; ff++) {
                    const int f = 2 * (hr & 1) + ff;                 // blocks 2 f (low half of the word) and 2 f + 1
                    const uint32_t w = br[buf][ff];
                    // fifth bits 2l, 2l + 1, 16 + 2l, 17 + 2l of a block's qh -> bit 0 of bytes 0..3
                    const uint32_t pa5 = (hw[4 + 2 * f] >> sh) & 0x00030003u, pb5 = (hw[5 + 2 * f] >> sh) & 0x00030003u;
                    const uint32_t ta = (pa5 | (pa5 << 7)) & 0x01010101u, tb = (pb5 | (pb5 << 7)) & 0x01010101u;
                    const uint32_t fl = __builtin_amdgcn_perm(tb, ta, 0x05040100u), fh = __builtin_amdgcn_perm(tb, ta, 0x07060302u);
                    const uint32_t lo = (w & 0x0F0F0F0Fu) | (fl << 4), hi = ((w >> 4) & 0x0F0F0F0Fu) | (fh << 4);      // (e0A, e1A, e0B, e1B), (e2A, e3A, e2B, e3B)
                    const v2h sa = {sc[f].x, sc[f].x}, sb = {sc[f].y, sc[f].y};
                    gfh_bytes4(lo, o, sa, sb, r0, r2);
                    gfh_bytes4(hi, o, sa, sb, r1, r3);
                    bf[ff] = v8h{r0.x, r0.y, r1.x, r1.y, r2.x, r2.y, r3.x, r3.y};
                }
            }
        };
        rd(0, 0);
#pragma unroll
        for (int hr = 0; hr < 8; hr++) {
            const int cur = hr & 1;
            if (hr + 1 < 8) rd(hr + 1, cur ^ 1);
            v8h bf[2];
            dq(hr, cur, bf);
#pragma unroll
            for (int h = 0; h < 2; h++)
#pragma unroll
                for (int s2 = 0; s2 < NSA; s2++) acc[s2][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[cur][s2][h], bf[h], acc[s2][0], 0, 0, 0);
        }
    };
    auto main_loop = [&](auto nsa) {
        for (int st = 0; st < nst; st++) {
            commit_stage();
            if (st + 1 < nst) { load_A(st + 1); load_B(st + 1); }
            __syncthreads();
            stage_mfma(st, nsa);
            __syncthreads();
        }
    };
    if (two) main_loop(std::integral_constant<int, 2>{}); else main_loop(std::integral_constant<int, 1>{});

    if (tid < GFH_BM) rmul[tid] = a.out_f16 ? 1.0f : mulv;
    __syncthreads();
    {
        const bool full = rows == (two ? 64 : 32) && n0 + GFH_BN <= N;      // uniform
        const int nsb = two ? 2 : 1;
#define GFH_ST(F_, OT_) pfh_store_tile<2, 1, F_, OT_, false>(acc, nsb, rows, row0, rmul, row_dst, a.out, a.out_ld, col, N, lane)
        if (a.out_f16) { if (full) GFH_ST(true, 2); else GFH_ST(false, 2); }
        else { if (full) GFH_ST(true, 0); else GFH_ST(false, 0); }
#undef GFH_ST
    }
}

bool kr_gfh_type_supported(int type, int K, int N) {
    return (((type == GG_Q6_K || type == GG_Q5_K || type == GG_Q3_K) && K % 256 == 0) || (type == GG_Q5_0 && K % 32 == 0)) && K > 0 && N > 0 && N % 8 == 0;
}

template <int TYPE>
static void gfh_launch(const KrGfhArgs& a, int mt, hipStream_t st) {
    const size_t lds = (size_t)GFH_BM * GFH_LDA + (TYPE == GG_Q6_K ? (size_t)16 * GFH_T6 : TYPE == GG_Q3_K ? (size_t)16 * GFH_T3 : (size_t)GFH_BN * GFH_LDB5) + 3 * GFH_BM * 4;
    (void)kr_lds_optin((const void*)kr_gfh_gemm_kernel<TYPE>, 64 * 1024);      // per (kernel, device)
    const int ncb = (a.m.N + GFH_BN - 1) / GFH_BN;
    dim3 grid;
    if (a.single_expert) grid = dim3(mt * ncb);
    else { const int span = 8 * a.run; grid = dim3(((mt + span - 1) / span) * span * ncb); }
    hipLaunchKernelGGL(kr_gfh_gemm_kernel<TYPE>, grid, dim3(256), lds, st, a);
}

void kr_launch_gfh_gemm(const GgMat& m, const uint16_t* a_h, const float* a_mul, const KrPfSort* sort, int topk, int gather_tokens, int max_tiles,
                        int single_expert_rows, void* out, int out_ld, int col_off, int out_f16, int run, hipStream_t st) {
    KrGfhArgs a{};
    a.m = m; a.a = a_h; a.a_mul = a_mul; a.topk = topk; a.gather_tokens = gather_tokens;
    if (sort) { a.row_pair = sort->row_pair; a.tile_expert = sort->tile_expert; a.tile_row0 = sort->tile_row0; a.tile_rows = sort->tile_rows; a.n_tiles = sort->n_tiles; }
    a.out = out_f16 ? (void*)((uint16_t*)out + col_off) : (void*)((float*)out + col_off);
    a.out_ld = out_ld; a.out_f16 = out_f16;
    a.single_expert = single_expert_rows > 0; a.total_rows = single_expert_rows;
    a.run = (single_expert_rows > 0 || run < 1) ? 1 : run;
    const int mt = single_expert_rows > 0 ? (single_expert_rows + GFH_BM - 1) / GFH_BM : max_tiles;
    if (mt <= 0) return;
    if (m.type == GG_Q6_K) gfh_launch<GG_Q6_K>(a, mt, st); else if (m.type == GG_Q5_K) gfh_launch<GG_Q5_K>(a, mt, st); else if (m.type == GG_Q3_K) gfh_launch<GG_Q3_K>(a, mt, st); else gfh_launch<GG_Q5_0>(a, mt, st);
}
