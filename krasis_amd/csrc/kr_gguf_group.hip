// kr_gguf_group.hip -- the EXACT grouped pass over native GGUF block experts (kr_decode_set_option "gguf_exact_pass", docs/design/20-gguf-exact-pass.md).
//
// The streaming kernels of kr_gguf.hip are bit-exact but take a grid of (row tiles, slots, B): every (token, slot) pair re-reads its expert's blocks and
// re-quantizes its activation row in every workgroup.  The int8-MFMA form of kr_gguf_prefill.hip reads an expert once per 64 rows but sums in another
// order (tolerance).  Here: rows sorted by expert (kr_launch_pf_sort with a tile of GGG_R rows), the activation row quantized ONCE per row into a global
// image (the GgAct records of kr_gguf_dev.h), and a workgroup that owns one group of at most GGG_R rows of one expert and a span of 8-row output tiles.
// A wave's lanes are 8 output rows x 8 AVX lanes as in gg_tile_*; a lane loads a block's record and header once and runs gg_pair_q4k / gg_sub_q8_0 (the
// streaming tiles' own bodies) against each row's image staged in LDS: GGG_R independent (acc, corr) chains per lane, each with the order of blocks,
// sub-blocks and lo / hi halves, the kr_hsum8 tree and the `- corr` of the decode step.  Rows never meet: a row's bits do not depend on its group.
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
