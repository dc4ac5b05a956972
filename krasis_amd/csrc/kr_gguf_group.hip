// kr_gguf_group.hip -- the EXACT grouped pass over native GGUF block experts (kr_decode_set_option "gguf_exact_pass", docs/design/20-gguf-exact-pass.md).
//
// The streaming kernels of kr_gguf.hip are bit-exact but take a grid of (row tiles, slots, B): every (token, slot) pair re-reads its expert's blocks and
// re-quantizes its activation row in every workgroup.  The int8-MFMA form of kr_gguf_prefill.hip reads an expert once per 64 rows but sums in another
// order (tolerance).  Here: rows sorted by expert (kr_launch_pf_sort with a tile of GGG_R rows), the activation row quantized ONCE per row into a global
// image (the GgAct records of kr_gguf_dev.h), and a workgroup that owns one group of at most GGG_R rows of one expert and a span of 8-row output tiles.
// A wave's lanes are 8 output rows x 8 AVX lanes as in gg_tile_*; a lane loads a block's record and header once and runs gg_pair_q4k / gg_sub_q8_0 (the
// streaming tiles' own bodies) against each row's image staged in LDS: GGG_R independent (acc, corr) chains per lane, each with the order of blocks,
// sub-blocks and lo / hi halves, the kr_hsum8 tree and the `- corr` of the decode step.  Rows never meet: a row's bits do not depend on its group.
// Q6_K / Q5_0 / Q5_K projections have a grouped form of their own further down (kr_ggs_kernel, docs/design/43-gguf-exact-grouped-scalar.md, 46-gguf-q5k-grouped.md):
// no image, one lane per output row, the serial f32 chains of gg_row_q6k / gg_row_q5_0 / gg_row_q5k over the group's f32 rows staged in LDS, behind the same sort.
//
// Image of one row (global, stride ggg_image_stride(K)): rec [K/32][8 lanes]{AH4, AL4}, then scale f32 [K/32], then sum i32 [K/32] -- gg_carve's layout.
// LDS stage: GGG_STAGE sub-blocks (= GG_PF Q4_K super-blocks, one request batch of the streaming tile) of GGG_R rows, 72 B per sub-block: 36 864 B.
// The 8-byte record reads of a wave touch 8 distinct addresses (one per AVX lane, 64 contiguous bytes; the 8 output rows read the same ones: broadcast),
// so neither 32-lane half of a ds_read_b64 meets a bank twice.
#include "kr_gguf_dev.h"
#include "kr_prefill.h"

#define GGG_R 8            // rows per group: 16 accumulators per lane beside the 64 registers of a request batch
#define GGG_STAGE 64       // sub-blocks per LDS stage (2048 k)
#define GGG_ROW_BYTES (GGG_STAGE * 72)

static_assert(GGG_STAGE == GG_PF * 8, "a stage is one request batch of Q4_K super-blocks");

__host__ __device__ static inline size_t ggg_stride(int K) { return (((size_t)(K / 32) * 72) + 15) & ~(size_t)15; }
size_t kr_ggg_image_stride(int K) { return ggg_stride(K); }
bool kr_ggg_type_supported(int type, int K) { return (type == GG_Q4_K && K > 0 && K % 256 == 0) || (type == GG_Q8_0 && K > 0 && K % 32 == 0); }
int kr_ggg_group_rows() { return GGG_R; }

extern __shared__ __attribute__((aligned(16))) char ggg_smem[];

// LDS image -> global image of one row: nsub * 72 contiguous bytes (nsub * 18 words)
__device__ __forceinline__ void ggg_store_image(const char* smem, char* dst, int nsub) {
    const u32x2* s = reinterpret_cast<const u32x2*>(smem); u32x2* d = reinterpret_cast<u32x2*>(dst);
    for (int i = threadIdx.x; i < nsub * 9; i += GG_BLOCK) d[i] = s[i];
}

// image of every token row: gg_quant_store's arithmetic on the bf16 row (the prompt pass's bf16 copy of the normalised hidden = bf16_rne(normed), what
// gg_prologue_f32_as_bf16 forms from the decode step's f32 hidden).  grid (rows)
__global__ void __launch_bounds__(GG_BLOCK) kr_ggg_image_x_kernel(const uint16_t* __restrict__ x, int K, char* __restrict__ img, size_t stride) {
    const GgAct A = gg_carve(ggg_smem, K);
    gg_prologue_bf16(x + (size_t)blockIdx.x * K, K, A, false);
    __syncthreads();
    ggg_store_image(ggg_smem, img + (size_t)blockIdx.x * stride, K / 32);
}
// image of silu(gate) * up of every sorted (token, slot) row, libm exp as gg_prologue_hidden_split.  grid (pairs); rows past the sort's count hold nothing
__global__ void __launch_bounds__(GG_BLOCK) kr_ggg_image_h_kernel(const float* __restrict__ gu, int I, int gu_ld, const int* __restrict__ n_tiles, char* __restrict__ img, size_t stride) {
    const int r = blockIdx.x;
    if (r >= n_tiles[1]) return;
    const GgAct A = gg_carve(ggg_smem, I);
    const float* g = gu + (size_t)r * gu_ld;
    gg_prologue_hidden_split(g, g + I, I, A, false, true);
    __syncthreads();
    ggg_store_image(ggg_smem, img + (size_t)r * stride, I / 32);
}

struct GggArgs {
    GgMat m0, m1;               // one or two projections of N rows each that share the activation (gate, up); m1.N == 0: one
    const char* img; size_t stride;
    const int* tile_expert; const int* tile_row0; const int* tile_rows; const int* n_tiles; const int* row_pair;
    int topk, gather_tokens;    // gather_tokens: image of sorted row r is the one of token row_pair[r] / topk
    float* out; int out_ld;     // out[r][c]: m0's rows at columns [0, N), m1's at [N, 2N)
    int tiles_per_wave;
};

// stage `s0` (sub-blocks [s0, s0 + GGG_STAGE) of nsub) of the group's rows into LDS: per row rec [GGG_STAGE][16] | scale [GGG_STAGE] | sum [GGG_STAGE]
__device__ __forceinline__ void ggg_stage_load(const GggArgs& a, int row0, int nr, int s0, int nsub) {
    const int ns = nsub - s0 < GGG_STAGE ? nsub - s0 : GGG_STAGE;
    for (int i = 0; i < nr; i++) {
        const int r = row0 + i;
        const size_t src = a.gather_tokens ? (size_t)(a.row_pair[r] / a.topk) : (size_t)r;
        const char* g = a.img + src * a.stride;
        char* d = ggg_smem + (size_t)i * GGG_ROW_BYTES;
        const u32x4* grec = reinterpret_cast<const u32x4*>(g) + (size_t)s0 * 4;
        for (int t = threadIdx.x; t < ns * 4; t += GG_BLOCK) reinterpret_cast<u32x4*>(d)[t] = grec[t];
        const uint32_t* gsc = reinterpret_cast<const uint32_t*>(g + (size_t)nsub * 64) + s0;
        const uint32_t* gsm = reinterpret_cast<const uint32_t*>(g + (size_t)nsub * 68) + s0;
        uint32_t* dsc = reinterpret_cast<uint32_t*>(d + GGG_STAGE * 64);
        for (int t = threadIdx.x; t < 2 * GGG_STAGE; t += GG_BLOCK) {
            const int q = t & (GGG_STAGE - 1);
            if (q < ns) dsc[t] = t < GGG_STAGE ? gsc[q] : gsm[q];
        }
    }
}
__device__ __forceinline__ GgAct ggg_lds_act(int i) {
    char* d = ggg_smem + (size_t)i * GGG_ROW_BYTES;
    GgAct A; A.rec = reinterpret_cast<uint32_t*>(d); A.scale = reinterpret_cast<float*>(d + GGG_STAGE * 64); A.sum = reinterpret_cast<int*>(d + GGG_STAGE * 68); A.f32v = nullptr;
    return A;
}

// one stage of one 8-row output tile against the group's rows: gg_tile_q4k's walk over super-blocks [s0 / 8, s0 / 8 + GG_PF)
__device__ __forceinline__ void ggg_stage_q4k(const GgMat& m, int tile, int s0, int nr, int lane, float (&acc)[GGG_R], float (&corr)[GGG_R]) {
    const int l = lane & 7, row = lane >> 3;
    const int nb = m.K / 256, b0 = s0 / 8;
    const u32x4* q = reinterpret_cast<const u32x4*>(m.q) + (size_t)tile * nb * 64 + lane;
    const u32x4* h = reinterpret_cast<const u32x4*>(m.h) + (size_t)tile * nb * 8 + row;
    u32x4 wv[GG_PF], hv[GG_PF];
#pragma unroll
    for (int u = 0; u < GG_PF; u++) { const int bb = b0 + u < nb ? b0 + u : nb - 1; wv[u] = kr_ldg_nt(q + (size_t)bb * 64); hv[u] = kr_ldg_nt(h + (size_t)bb * 8); }
#pragma unroll
    for (int u = 0; u < GG_PF; u++) {
        if (b0 + u < nb) {
            const u32x4 w = wv[u], hd = hv[u];
            const float d = gg_f16(hd.x & 0xFFFFu), dmin = gg_f16(hd.x >> 16);
            const uint32_t wj[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                int sc_lo, mn_lo, sc_hi, mn_hi;
                gg_scale_min_k4(2 * j, hd.y, hd.z, hd.w, sc_lo, mn_lo); gg_scale_min_k4(2 * j + 1, hd.y, hd.z, hd.w, sc_hi, mn_hi);
#pragma unroll
                for (int i = 0; i < GGG_R; i++)
                    if (i < nr) gg_pair_q4k(wj[j], d, dmin, sc_lo, mn_lo, sc_hi, mn_hi, ggg_lds_act(i), u * 8 + 2 * j, l, acc[i], corr[i]);
            }
        }
    }
}
// ... gg_tile_q8_0's walk over block groups [s0 / 4, s0 / 4 + GGG_STAGE / 4), two request batches; the last group may be ragged (s < nb)
__device__ __forceinline__ void ggg_stage_q8_0(const GgMat& m, int tile, int s0, int nr, int lane, float (&acc)[GGG_R]) {
    const int l = lane & 7, row = lane >> 3;
    const int nb = m.K / 32, nbg = (nb + 3) / 4;
    const u32x4* q = reinterpret_cast<const u32x4*>(m.q) + (size_t)tile * nbg * 64 + lane;
    const u32x2* h = reinterpret_cast<const u32x2*>(m.h) + (size_t)tile * nbg * 8 + row;
    const int g_hi = s0 / 4 + GGG_STAGE / 4 < nbg ? s0 / 4 + GGG_STAGE / 4 : nbg;
    for (int g0 = s0 / 4; g0 < g_hi; g0 += GG_PF) {
        u32x4 wv[GG_PF]; u32x2 hv[GG_PF];
#pragma unroll
        for (int v = 0; v < GG_PF; v++) { const int gg = g0 + v < g_hi ? g0 + v : g_hi - 1; wv[v] = kr_ldg_nt(q + (size_t)gg * 64); hv[v] = h[(size_t)gg * 8]; }
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
#pragma unroll
                        for (int i = 0; i < GGG_R; i++)
                            if (i < nr) gg_sub_q8_0(wb[u], dd[u], ggg_lds_act(i), s - s0, l, acc[i]);
                    }
                }
            }
        }
    }
}

// grid (output-tile spans, groups of the sort's tile table); a workgroup's 4 waves share the staged images, wave w takes tiles t0 + w, t0 + w + 4, ...
template <int TYPE>
__global__ void __launch_bounds__(GG_BLOCK) kr_ggg_kernel(const GggArgs a) {
    const int g = blockIdx.y;
    if (g >= a.n_tiles[0]) return;
    const int e = a.tile_expert[g], row0 = a.tile_row0[g];
    int nr = a.tile_rows[g]; nr = nr < GGG_R ? nr : GGG_R;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nt = (a.m0.N + 7) / 8, total = a.m1.N ? 2 * nt : nt;
    const int t0 = blockIdx.x * (GG_BLOCK / 64) * a.tiles_per_wave;
    if (t0 >= total) return;
    const int nsub = a.m0.K / 32, nstages = (nsub + GGG_STAGE - 1) / GGG_STAGE;
    for (int round = 0; round < a.tiles_per_wave; round++) {
        const int t = t0 + round * (GG_BLOCK / 64) + wave;
        const bool live = t < total;
        const bool second = live && t >= nt;
        const GgMat m = gg_expert_mat(second ? a.m1 : a.m0, e);
        const int tile = second ? t - nt : t;
        float acc[GGG_R], corr[GGG_R];
#pragma unroll
        for (int i = 0; i < GGG_R; i++) { acc[i] = 0.0f; corr[i] = 0.0f; }
        for (int st = 0; st < nstages; st++) {
            if (nstages > 1 || round == 0) {       // uniform over the workgroup: a single stage stays in LDS for every round
                __syncthreads();
                ggg_stage_load(a, row0, nr, st * GGG_STAGE, nsub);
                __syncthreads();
            }
            if (live) {
                if (TYPE == GG_Q4_K) ggg_stage_q4k(m, tile, st * GGG_STAGE, nr, lane, acc, corr);
                else ggg_stage_q8_0(m, tile, st * GGG_STAGE, nr, lane, acc);
            }
        }
        if (live) {
            const int orow = tile * 8 + (lane >> 3);
#pragma unroll
            for (int i = 0; i < GGG_R; i++) {
                if (i < nr) {
                    const float r = TYPE == GG_Q4_K ? kr_hsum8(acc[i]) - corr[i] : kr_hsum8(acc[i]);
                    if ((lane & 7) == 0 && orow < m.N) a.out[(size_t)(row0 + i) * a.out_ld + (second ? a.m0.N : 0) + orow] = r;
                }
            }
        }
    }
}

// ---- Q6_K / Q5_0 / Q5_K in the grouped form (docs/design/43-gguf-exact-grouped-scalar.md; Q5_K further down).  The contract is gg_row_q6k / gg_row_q5_0 of kr_gguf.hip: per
// (activation row, output row) ONE serial f32 chain over k, each term (s * (float)(q - c)) * x then sum += term -- mul, mul, add, nothing contracted.  The first
// product does not depend on the activation row, nor do the record loads and the 5- / 6-bit unpack: a lane owns one output row, loads and unpacks its records once
// and feeds GGG_R chains, one per row of the group, each in the reference's k order.  The group's activation rows sit in LDS as f32, [k][GGG_R rows], a stage of
// GGS_STAGE k at a time (32 KiB): every lane of a wave reads the same address (a broadcast), one 16-byte read gives four rows' values of one k, paired for
// v_pk_mul_f32 / v_pk_add_f32 (component-wise the same IEEE operations).  A unit is 256 k -- a Q6_K super-block (12 + 5 loads, the addresses of gg_row_q6k) or a
// Q5_0 block group (8 + 3, the last one ragged) -- requested one unit ahead of its use; the sums stay in registers across stages.  NR = 2 / 4 / 8 chains are
// compiled: a workgroup takes the smallest that holds its group's rows (a decode step's groups mostly hold one row).
// Q5_K (docs/design/46-gguf-q5k-grouped.md): the contract is gg_row_q5k -- w = (d sc_j) (float)(q4 + 16 q5) - (dmin mn_j), per super-block s = 0, s += w_k x_k over
// its 256 k in element order, then sum += s: a chain of two levels, so a lane carries NR partial sums s beside its NR sums and folds them at the end of every unit
// (a unit is one super-block: the row's eight lane records and its 48-byte header, 8 + 3 loads, the addresses of gg_row_q5k; K % 256 == 0, no ragged unit).  The
// weights do not depend on the activation row and only the order of a chain's adds is fixed, so a sub-block's 32 values are formed word-wise -- a record word and
// its fifth-bit word give four finished 5-bit codes under one mask-or, one byte-to-float conversion each -- and then walked in element order into the chains.
#define GGS_STAGE 1024     // k per LDS stage: GGG_R rows x 4 KiB
#define GGS_UNIT 256       // k per request: a Q6_K / Q5_K super-block, a Q5_0 group of 8 blocks
typedef float ggs_f32x4 __attribute__((ext_vector_type(4)));

bool kr_ggs_type_supported(int type, int K) { return ((type == GG_Q6_K || type == GG_Q5_K) && K > 0 && K % 256 == 0) || (type == GG_Q5_0 && K > 0 && K % 32 == 0); }

struct GgsArgs {
    GgMat m0, m1;               // gate and up side by side (m1.N == 0: one projection), N rows each
    const void* x; int x_bf16; size_t x_ld;      // activation rows, bf16 (the pass's token rows) or f32, x_ld elements apart
    const int* tile_expert; const int* tile_row0; const int* tile_rows; const int* n_tiles; const int* row_pair;
    int topk, gather_tokens;    // gather_tokens: sorted row r reads activation row row_pair[r] / topk, else row r
    int out_pairs;              // sorted row r writes out row row_pair[r] (the stand-alone operator), else row r
    float* out; int out_ld;     // m0's rows at columns [0, N), m1's at [N, 2N)
};

// f32 silu(gate) * up of every sorted row, the expression of gg_prologue_hidden_split (libm exp).  grid (pairs); rows past the sort's count hold nothing
__global__ void __launch_bounds__(GG_BLOCK) kr_ggs_hidden_kernel(const float* __restrict__ gu, int I, int gu_ld, const int* __restrict__ n_tiles, float* __restrict__ hid) {
    const int r = blockIdx.x;
    if (r >= n_tiles[1]) return;
    const float* g = gu + (size_t)r * gu_ld;
    for (int i = threadIdx.x; i < I; i += GG_BLOCK) { const float gv = g[i]; hid[(size_t)r * I + i] = (gv / (1.0f + kr_expf(-gv))) * g[I + i]; }
}

// k [k0, k0 + ns) of the group's rows into LDS as [k][GGG_R] f32; a thread takes two k of every row.  Rows past nr hold zeros (their chains are computed when NR > nr
// and never stored).  bf16 -> f32 is the shift of gg_prologue_bf16
__device__ __forceinline__ void ggs_stage_load(const GgsArgs& a, const size_t (&src)[GGG_R], int nr, int k0, int ns) {
    ggs_f32x4* lds = reinterpret_cast<ggs_f32x4*>(ggg_smem);
    for (int p = threadIdx.x; p < ns / 2; p += blockDim.x) {
        float v0[GGG_R], v1[GGG_R];
#pragma unroll
        for (int i = 0; i < GGG_R; i++) {
            v0[i] = 0.0f; v1[i] = 0.0f;
            if (i < nr) {
                if (a.x_bf16) {
                    const uint32_t w = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint16_t*>(a.x) + src[i] + k0)[p];
                    v0[i] = __uint_as_float(w << 16); v1[i] = __uint_as_float(w & 0xFFFF0000u);
                } else {
                    const u32x2 w = reinterpret_cast<const u32x2*>(reinterpret_cast<const float*>(a.x) + src[i] + k0)[p];
                    v0[i] = __uint_as_float(w.x); v1[i] = __uint_as_float(w.y);
                }
            }
        }
        lds[4 * p + 0] = ggs_f32x4{v0[0], v0[1], v0[2], v0[3]}; lds[4 * p + 1] = ggs_f32x4{v0[4], v0[5], v0[6], v0[7]};
        lds[4 * p + 2] = ggs_f32x4{v1[0], v1[1], v1[2], v1[3]}; lds[4 * p + 3] = ggs_f32x4{v1[4], v1[5], v1[6], v1[7]};
    }
}

// sum[i] += w * x_i[k] for the NR chains of a lane: a product, then an add
template <int NR>
__device__ __forceinline__ void ggs_term(float w, int k, gg_f32x2 (&sum)[NR / 2]) {
    const gg_f32x2 w2 = {w, w};
    if (NR == 2) {
        const gg_f32x2 x = reinterpret_cast<const gg_f32x2*>(ggg_smem)[k * 4];
        sum[0] = sum[0] + w2 * x;
    } else {
#pragma unroll
        for (int h = 0; h < NR / 4; h++) {
            const ggs_f32x4 x = reinterpret_cast<const ggs_f32x4*>(ggg_smem)[k * 2 + h];
            sum[2 * h] = sum[2 * h] + w2 * gg_f32x2{x.x, x.y};
            sum[2 * h + 1] = sum[2 * h + 1] + w2 * gg_f32x2{x.z, x.w};
        }
    }
}

// The NR chains of a lane pass one empty statement together: no instruction, but no chain's next add may be placed before every chain's previous one.  Q5_K's weights
// are formed apart from the terms, and without this the compiler walks a whole unit chain pair by chain pair with the 256 weights kept beside it (8 KB of scratch)
// `k` (the stage offset that the group after next reads through) passes it too: the LDS reads run at most one group of terms ahead of the adds, not a whole unit
template <int NR>
__device__ __forceinline__ void ggs_tie(gg_f32x2 (&sum)[NR / 2], int& k) {
    if (NR == 2) asm("" : "+v"(sum[0]), "+v"(k));
    if (NR == 4) asm("" : "+v"(sum[0]), "+v"(sum[1]), "+v"(k));
    if (NR == 8) asm("" : "+v"(sum[0]), "+v"(sum[1]), "+v"(sum[2]), "+v"(sum[3]), "+v"(k));
}
// ... and the block scales that the next sub-block's weights are formed from pass one with a chain, half a sub-block ahead: 48 weights in registers, not 256
__device__ __forceinline__ void ggs_tie_scales(gg_f32x2& sum0, float& d, float& dmin) { asm("" : "+v"(sum0), "+v"(d), "+v"(dmin)); }

// the records of one unit of a lane's output row: Q6_K wv[0 .. 12) = two halves x six 16-byte words, hv = {16 scale bytes, f16 d}; Q5_0 wv[0 .. 8) = the eight
// lane records of a block group, hv[0 .. 3) as words = {8 x f16 d, 8 x u32 qh}; Q5_K wv[0 .. 8) = the eight lane records of a super-block, hv[0 .. 3) as words =
// {f16 d | f16 dmin, 12 scale bytes, 8 x u32 fifth bits (one word per lane record)}.  Q5_0 and Q5_K units have one shape and, with K % 256 == 0, the same addresses
template <int TYPE> struct GgsUnit { u32x4 wv[TYPE == GG_Q6_K ? 12 : 8]; uint32_t hv[TYPE == GG_Q6_K ? 5 : 12]; };

template <int TYPE>
__device__ __forceinline__ void ggs_request(const GgMat& m, int r, int unit, GgsUnit<TYPE>& R) {
    const int tile = r >> 3, row = r & 7;
    if (TYPE == GG_Q6_K) {
        const int nb = m.K / 256;
        const u32x4* q = reinterpret_cast<const u32x4*>(m.q) + ((size_t)tile * nb * 16 + row) * 6;
        const uint32_t* h = reinterpret_cast<const uint32_t*>(m.h) + ((size_t)tile * nb * 8 + row) * 5;
#pragma unroll
        for (int i = 0; i < 12; i++) R.wv[i] = kr_ldg_nt(q + ((size_t)unit * 2 + i / 6) * 48 + i % 6);
#pragma unroll
        for (int i = 0; i < 5; i++) R.hv[i] = kr_ldg_nt(h + (size_t)unit * 40 + i);
    } else {      // Q5_0 block groups and Q5_K super-blocks: 8 records of 16 B and a 48-byte header per 256 k
        const int nbg = (m.K / 32 + 7) / 8;
        const u32x4* q = reinterpret_cast<const u32x4*>(m.q) + ((size_t)tile * nbg * 8 + row) * 8;
        const u32x4* h = reinterpret_cast<const u32x4*>(m.h) + ((size_t)tile * nbg * 8 + row) * 3;
#pragma unroll
        for (int l = 0; l < 8; l++) R.wv[l] = kr_ldg_nt(q + (size_t)unit * 64 + l);
#pragma unroll
        for (int i = 0; i < 3; i++) { const u32x4 v = kr_ldg_nt(h + (size_t)unit * 24 + i); R.hv[4 * i] = v.x; R.hv[4 * i + 1] = v.y; R.hv[4 * i + 2] = v.z; R.hv[4 * i + 3] = v.w; }
    }
}

// one unit against the staged rows; ks: the unit's first k inside the stage.  The walk, the unpack and the term order are gg_row_q6k's / gg_row_q5_0's
template <int TYPE, int NR>
__device__ __forceinline__ void ggs_consume(const GgsUnit<TYPE>& R, int unit, int nb32, int ks, gg_f32x2 (&sum)[NR / 2]) {
    if (TYPE == GG_Q6_K) {
        const float d = gg_f16(R.hv[4] & 0xFFFFu);
#pragma unroll
        for (int hf = 0; hf < 2; hf++) {
            uint32_t w[24];      // slice j of the half: words 3j (ql[4j..]), 3j + 1 (ql[32 + 4j..]), 3j + 2 (qh[4j..])
#pragma unroll
            for (int i = 0; i < 6; i++) { w[4 * i] = R.wv[hf * 6 + i].x; w[4 * i + 1] = R.wv[hf * 6 + i].y; w[4 * i + 2] = R.wv[hf * 6 + i].z; w[4 * i + 3] = R.wv[hf * 6 + i].w; }
            const int io = ks + hf * 128;
#pragma unroll
            for (int l = 0; l < 32; l++) {
                const int is = l / 16, j = l >> 2, sft = (l & 3) * 8;
                const uint32_t ql0 = (w[3 * j] >> sft) & 0xFFu, ql1 = (w[3 * j + 1] >> sft) & 0xFFu, qhb = (w[3 * j + 2] >> sft) & 0xFFu;
                const int q0 = (int)(ql0 & 0xF) | ((int)((qhb >> 0) & 3) << 4);
                const int q1 = (int)(ql1 & 0xF) | ((int)((qhb >> 2) & 3) << 4);
                const int q2 = (int)((ql0 >> 4) & 0xF) | ((int)((qhb >> 4) & 3) << 4);
                const int q3 = (int)((ql1 >> 4) & 0xF) | ((int)((qhb >> 6) & 3) << 4);
                auto sc = [&](int k) { return (float)(int8_t)((R.hv[2 * hf + (k >> 2)] >> ((k & 3) * 8)) & 0xFFu); };      // scale byte k of this half
                const float s0 = d * sc(is + 0), s1 = d * sc(is + 2), s2 = d * sc(is + 4), s3 = d * sc(is + 6);
                ggs_term<NR>(s0 * (float)(q0 - 32), io + l, sum);
                ggs_term<NR>(s1 * (float)(q1 - 32), io + 32 + l, sum);
                ggs_term<NR>(s2 * (float)(q2 - 32), io + 64 + l, sum);
                ggs_term<NR>(s3 * (float)(q3 - 32), io + 96 + l, sum);
            }
        }
    } else if (TYPE == GG_Q5_K) {
        float d[2], dmin[2];     // d and dmin, for the even and the odd sub-blocks (ggs_tie_scales)
        d[0] = d[1] = gg_f16(R.hv[0] & 0xFFFFu); dmin[0] = dmin[1] = gg_f16(R.hv[0] >> 16);
        gg_f32x2 s[NR / 2];      // the super-block's partial sums, the inner level of gg_row_q5k's chain
#pragma unroll
        for (int i = 0; i < NR / 2; i++) s[i] = gg_f32x2{0.0f, 0.0f};
        int kb[2] = {ks, ks};    // ks, for the even and the odd groups of eight terms (ggs_tie)
#pragma unroll
        for (int js = 0; js < 8; js++) {      // sub-block js = 2 j + hi: nibble hi of word j of every record, fifth bit 2 j + hi of every byte of the record's header word
            const int j = js >> 1, hi = js & 1;
            int sc, mn;
            gg_scale_min_k4(js, R.hv[1], R.hv[2], R.hv[3], sc, mn);
            const float d1 = d[hi] * (float)sc, m1 = dmin[hi] * (float)mn;
            uint32_t c[8];       // four finished codes per word: byte b of c[l] is element p = 2 l + (b & 1) + 16 (b >> 1)
#pragma unroll
            for (int l = 0; l < 8; l++) {
                const uint32_t wj = j == 0 ? R.wv[l].x : j == 1 ? R.wv[l].y : j == 2 ? R.wv[l].z : R.wv[l].w;
                c[l] = ((wj >> (4 * hi)) & 0x0F0F0F0Fu) | (((R.hv[4 + l] >> js) & 0x01010101u) << 4);
            }
#pragma unroll
            for (int p = 0; p < 32; p++) {
                const float q = (float)((c[(p & 15) >> 1] >> (8 * ((p & 1) + 2 * (p >> 4)))) & 0xFFu);
                ggs_term<NR>(d1 * q - m1, kb[(p >> 3) & 1] + js * 32 + p, s);
                if ((p & 7) == 7) ggs_tie<NR>(s, kb[(p >> 3) & 1]);
                if (p == 15) ggs_tie_scales(s[0], d[hi ^ 1], dmin[hi ^ 1]);
            }
        }
#pragma unroll
        for (int i = 0; i < NR / 2; i++) sum[i] = sum[i] + s[i];
    } else {
        uint32_t w[8][4];
#pragma unroll
        for (int l = 0; l < 8; l++) { w[l][0] = R.wv[l].x; w[l][1] = R.wv[l].y; w[l][2] = R.wv[l].z; w[l][3] = R.wv[l].w; }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            if (unit * 8 + u < nb32) {      // the last group may be ragged
                const float d = gg_f16((R.hv[u >> 1] >> ((u & 1) * 16)) & 0xFFFFu);
                const uint32_t qh = R.hv[4 + u];
#pragma unroll
                for (int j = 0; j < 32; j++) {
                    const uint32_t byte = (w[(j & 15) >> 1][u >> 1] >> ((u & 1) * 16 + (j & 1) * 8)) & 0xFFu;      // qs[j & 15]
                    const uint32_t q4 = j < 16 ? (byte & 0x0Fu) : ((byte >> 4) & 0x0Fu);
                    const int qv = (int)(q4 | (((qh >> j) & 1u) << 4)) - 16;
                    ggs_term<NR>(d * (float)qv, ks + u * 32 + j, sum);
                }
            }
        }
    }
}

// grid (spans of blockDim.x output rows, groups of the sort's tile table); thread t owns padded row p = blockIdx.x * blockDim.x + t of [m0's tiles | m1's tiles]
template <int TYPE, int NR>
__device__ __forceinline__ void ggs_run(const GgsArgs& a, int e, int row0, int nr) {
    const int np = ((a.m0.N + 7) / 8) * 8, total = a.m1.N ? 2 * np : np;
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    const bool in_grid = p < total;
    p = in_grid ? p : 0;                           // a lane past the last tile walks row 0 and stores nothing: every lane meets every barrier
    const bool second = p >= np;
    const int r = second ? p - np : p;             // rows [N, np) are the last tile's padding: their records exist
    const GgMat m = gg_expert_mat(second ? a.m1 : a.m0, e);
    const int K = m.K, nunits = (K + GGS_UNIT - 1) / GGS_UNIT;
    size_t src[GGG_R];
#pragma unroll
    for (int i = 0; i < GGG_R; i++) src[i] = (i < nr ? (a.gather_tokens ? (size_t)(a.row_pair[row0 + i] / a.topk) : (size_t)(row0 + i)) : 0) * a.x_ld;
    gg_f32x2 sum[NR / 2];
#pragma unroll
    for (int i = 0; i < NR / 2; i++) sum[i] = gg_f32x2{0.0f, 0.0f};
    GgsUnit<TYPE> cur, nxt;
    ggs_request<TYPE>(m, r, 0, cur);
    for (int u0 = 0; u0 < nunits; u0 += GGS_STAGE / GGS_UNIT) {
        const int k0 = u0 * GGS_UNIT, ns = K - k0 < GGS_STAGE ? K - k0 : GGS_STAGE;
        __syncthreads();                           // the stage before this one has been consumed
        ggs_stage_load(a, src, nr, k0, ns);
        __syncthreads();
        const int u1 = u0 + GGS_STAGE / GGS_UNIT < nunits ? u0 + GGS_STAGE / GGS_UNIT : nunits;
        for (int u = u0; u < u1; u++) {
            ggs_request<TYPE>(m, r, u + 1 < nunits ? u + 1 : nunits - 1, nxt);      // requested before this unit is consumed; the last one asks for itself again
            ggs_consume<TYPE, NR>(cur, u, K / 32, (u - u0) * GGS_UNIT, sum);
            cur = nxt;
        }
    }
    if (in_grid && r < m.N) {
#pragma unroll
        for (int i = 0; i < NR; i++) {
            if (i < nr) {
                const size_t orow = a.out_pairs ? (size_t)a.row_pair[row0 + i] : (size_t)(row0 + i);
                a.out[orow * a.out_ld + (second ? a.m0.N : 0) + r] = (i & 1) ? sum[i >> 1].y : sum[i >> 1].x;
            }
        }
    }
}
template <int TYPE>
__global__ void __launch_bounds__(GG_BLOCK) kr_ggs_kernel(const GgsArgs a) {
    const int g = blockIdx.y;
    if (g >= a.n_tiles[0]) return;
    const int e = a.tile_expert[g], row0 = a.tile_row0[g];
    int nr = a.tile_rows[g]; nr = nr < GGG_R ? nr : GGG_R;
    if (nr <= 2) ggs_run<TYPE, 2>(a, e, row0, nr);
    else if (nr <= 4) ggs_run<TYPE, 4>(a, e, row0, nr);
    else ggs_run<TYPE, 8>(a, e, row0, nr);
}

void kr_launch_ggg_image_x(const uint16_t* x_bf16, int M, int K, void* img, hipStream_t st) {
    hipLaunchKernelGGL(kr_ggg_image_x_kernel, dim3(M), dim3(GG_BLOCK), gg_lds_bytes(K, false), st, x_bf16, K, (char*)img, ggg_stride(K));
}
void kr_launch_ggg_image_h(const float* gu, int pairs, int I, int gu_ld, const KrPfSort* sort, void* img, hipStream_t st) {
    hipLaunchKernelGGL(kr_ggg_image_h_kernel, dim3(pairs), dim3(GG_BLOCK), gg_lds_bytes(I, false), st, gu, I, gu_ld, sort->n_tiles, (char*)img, ggg_stride(I));
}
// m1: second projection on the same rows (up beside gate), or null.  The sort's tile table must have been built with kr_ggg_group_rows() rows per tile.
void kr_launch_ggg_gemm(const GgMat& m0, const GgMat* m1, const void* img, const KrPfSort* sort, int topk, int gather_tokens, int pairs, int n_experts, float* out, int out_ld, hipStream_t st) {
    GggArgs a{};
    a.m0 = m0; if (m1) a.m1 = *m1;
    a.img = (const char*)img; a.stride = ggg_stride(m0.K);
    a.tile_expert = sort->tile_expert; a.tile_row0 = sort->tile_row0; a.tile_rows = sort->tile_rows; a.n_tiles = sort->n_tiles; a.row_pair = sort->row_pair;
    a.topk = topk; a.gather_tokens = gather_tokens; a.out = out; a.out_ld = out_ld;
    const int total = (m1 ? 2 : 1) * ((m0.N + 7) / 8), waves = GG_BLOCK / 64;
    // groups are counted on the device; the host knows their bound (the tile table's size) and that a small pass has at most one group per pair.  A span
    // takes up to 4 tiles per wave (the staged images serve them all) while the grid still fills the machine: 256 CUs x 4 workgroups of this size x 4
    const int max_groups = pairs / GGG_R + n_experts + 1, est_groups = pairs < max_groups ? pairs : max_groups;
    int tpw = 4; while (tpw > 1 && (long)((total + waves * tpw - 1) / (waves * tpw)) * est_groups < 4096) tpw >>= 1;
    a.tiles_per_wave = tpw;
    const dim3 grid((total + waves * tpw - 1) / (waves * tpw), max_groups);
    const size_t lds = (size_t)GGG_R * GGG_ROW_BYTES;
    if (m0.type == GG_Q4_K) hipLaunchKernelGGL(kr_ggg_kernel<GG_Q4_K>, grid, dim3(GG_BLOCK), lds, st, a);
    else hipLaunchKernelGGL(kr_ggg_kernel<GG_Q8_0>, grid, dim3(GG_BLOCK), lds, st, a);
}
void kr_launch_ggs_hidden(const float* gu, int pairs, int I, int gu_ld, const KrPfSort* sort, float* hid, hipStream_t st) {
    hipLaunchKernelGGL(kr_ggs_hidden_kernel, dim3(pairs), dim3(GG_BLOCK), 0, st, gu, I, gu_ld, sort->n_tiles, hid);
}
// Q6_K / Q5_0 / Q5_K (kr_ggs_type_supported), the same sort.  x: activation rows x_ld elements apart, bf16 or f32; gather_tokens / out_pairs as in GgsArgs
void kr_launch_ggs_gemm(const GgMat& m0, const GgMat* m1, const void* x, int x_bf16, size_t x_ld, const KrPfSort* sort, int topk, int gather_tokens, int out_pairs, int pairs,
                        int n_experts, float* out, int out_ld, hipStream_t st) {
    GgsArgs a{};
    a.m0 = m0; if (m1) a.m1 = *m1;
    a.x = x; a.x_bf16 = x_bf16; a.x_ld = x_ld;
    a.tile_expert = sort->tile_expert; a.tile_row0 = sort->tile_row0; a.tile_rows = sort->tile_rows; a.n_tiles = sort->n_tiles; a.row_pair = sort->row_pair;
    a.topk = topk; a.gather_tokens = gather_tokens; a.out_pairs = out_pairs; a.out = out; a.out_ld = out_ld;
    const int total = (m1 ? 2 : 1) * ((m0.N + 7) / 8) * 8;
    // rows (threads) per workgroup: 256, fewer while spans x groups would leave CUs without two workgroups (the reasoning of kr_launch_ggg_gemm's tiles_per_wave)
    const int max_groups = pairs / GGG_R + n_experts + 1, est_groups = pairs < max_groups ? pairs : max_groups;
    int rows_wg = GG_BLOCK; while (rows_wg > 64 && (long)((total + rows_wg - 1) / rows_wg) * est_groups < 512) rows_wg >>= 1;
    const dim3 grid((total + rows_wg - 1) / rows_wg, max_groups);
    const size_t lds = (size_t)GGS_STAGE * GGG_R * 4;
    if (m0.type == GG_Q6_K) hipLaunchKernelGGL(kr_ggs_kernel<GG_Q6_K>, grid, dim3(rows_wg), lds, st, a);
    else if (m0.type == GG_Q5_K) hipLaunchKernelGGL(kr_ggs_kernel<GG_Q5_K>, grid, dim3(rows_wg), lds, st, a);
    else hipLaunchKernelGGL(kr_ggs_kernel<GG_Q5_0>, grid, dim3(rows_wg), lds, st, a);
}
