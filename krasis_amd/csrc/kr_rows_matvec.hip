// kr_rows_matvec.hip -- the exact streaming matvec over a few rows (1 .. 16) for gfx950: y[r][N] = W . quant(x[r][K]).
//
// The multi-row passes of at most 16 token rows ("pass_few_rows", docs/design/34-pass-few-rows.md) and kr_decode_matmul_rows run their projections here instead
// of the 64-row matrix-core tile of kr_prefill.hip.  The geometry is the decode step's (kr_moe_decode.hip): a wave owns 8 columns, 8 lanes per column, one
// 16-byte weight record per lane and group pair -- but a workgroup builds the INT16 activation image of EVERY row of its row group in LDS (one image after the
// other: kr_prologue_quant / kr_prologue_hidden per row) and a lane applies the weight record it holds to all of them (kr_rows_tile, kr_rows_dev.h).  Row r's
// sum is kr_matvec_tile's operation for operation, so every row carries the bits of kr_launch_multi_matvec on that row.
//   grid = (column workgroups, row groups); the launcher splits the rows so that a group's images fit the LDS window (kr_rows_plan.h), above 64 KiB by opt-in.
#include "kr_lds_optin.h"
#include "kr_device.h"
#include "kr_kernels.h"
#include "kr_rows_plan.h"

#define KR_BLOCK 256
#define KR_WAVES (KR_BLOCK / 64)
#include "kr_rows_dev.h"

extern __shared__ __attribute__((aligned(16))) u32x4 kr_rows_smem[];

struct KrRowsMat { KrMultiMat mm; int ld[KR_MAX_MULTI]; };

template <int BITS, int RG>
__global__ void __launch_bounds__(KR_BLOCK) kr_rows_matvec_kernel(const float* x, int ld_x, int R, int group, int img16, int act_mode, int tiles_per_wave, const KrRowsMat a) {
    const KrMultiMat& mm = a.mm;
    const int total = mm.tile_end[mm.n - 1];
    const int tile0 = (blockIdx.x * KR_WAVES) * tiles_per_wave;
    const int r0 = blockIdx.y * group;
    if (tile0 >= total || r0 >= R) return;
    const int nr = R - r0 < group ? R - r0 : group;      // <= RG (launcher)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int first = tile0 + wave * tiles_per_wave;
    int mi = 0;
    while (mi + 1 < mm.n && first >= mm.tile_end[mi]) mi++;
    const int K = mm.m[0].ng * 128;
    const float* xr = x + (size_t)r0 * ld_x;
    // row 0's first chunk, then the tile's first weight records, then the images row by row; row r + 1's first chunk is requested before row r is quantised
    KrHidPre HP; KrVecPre VP;
    if (act_mode == KR_ACT_SILU_MUL) kr_hidden_load(xr, K, HP); else kr_vec_load(xr, K, VP);
    KrRowsPre pre;
    if (first < total) kr_rows_preload<BITS>(pre, mm.m[mi].q, mm.m[mi].s, mm.m[mi], first - (mi ? mm.tile_end[mi - 1] : 0), lane, 0);
    for (int r = 0; r < nr; r++) {
        const KrActLds L = kr_carve_lds(kr_rows_smem + (size_t)r * img16, K, BITS == 8);
        const float* xc = xr + (size_t)r * ld_x;
        const float* xn = xr + (size_t)(r + 1 < nr ? r + 1 : r) * ld_x;
        if (act_mode == KR_ACT_SILU_MUL) {
            KrHidPre HN; kr_hidden_load(xn, K, HN);
            kr_prologue_hidden<KR_ACT_SILU_MUL, BITS == 8>(xc, K, 0.0f, 0.0f, L, HP);
            HP = HN;
        } else {
            KrVecPre VN; kr_vec_load(xn, K, VN);
            kr_prologue_quant<float, BITS == 8>(xc, K, L, VP);
            VP = VN;
        }
    }
    __syncthreads();
    for (int t = 0; t < tiles_per_wave; t++) {
        const int gt = first + t;
        if (gt >= total) break;
        while (mi + 1 < mm.n && gt >= mm.tile_end[mi]) mi++;
        const KrMatDev& m = mm.m[mi];
        const int tile = gt - (mi ? mm.tile_end[mi - 1] : 0);
        float acc[RG];
        kr_rows_tile<BITS, RG>(pre, t == 0, m.q, m.s, m, tile, kr_rows_smem, img16, K, nr, lane, acc);
        const int col = tile * 8 + (lane >> 3);
        if ((lane & 7) == 0 && col < m.N) {
            float* y = mm.y[mi] + (size_t)r0 * a.ld[mi] + col;
#pragma unroll
            for (int r = 0; r < RG; r++) if (r < nr) y[(size_t)r * a.ld[mi]] = acc[r];
        }
    }
}

// ------------------------------------------------------------------------------------------
// host launcher
// ------------------------------------------------------------------------------------------

template <int BITS, int RG>
static int kr_rows_launch(const KrRowsMat& a, const float* x, int ld_x, int R, const KrRowsPlan& p, int img16, int act_mode, int tpw, int col_wgs, hipStream_t st) {
    if (p.lds > KR_ROWS_LDS_DEFAULT && kr_lds_optin((const void*)kr_rows_matvec_kernel<BITS, RG>, KR_ROWS_LDS_LIMIT)) return 1;
    hipLaunchKernelGGL((kr_rows_matvec_kernel<BITS, RG>), dim3(col_wgs, p.n_groups), dim3(KR_BLOCK), p.lds, st, x, ld_x, R, p.group, img16, act_mode, tpw, a);
    return 0;
}

static int kr_rows_launch_same(const KrMatDev* mats, float* const* ys, const int* lds, int n, const float* x, int ld_x, int R, int act_mode, int group, hipStream_t st) {
    KrRowsMat a{};
    a.mm.n = n;
    int total = 0;
    for (int i = 0; i < n; i++) { a.mm.m[i] = mats[i]; a.mm.y[i] = ys[i]; a.ld[i] = lds[i]; total += (mats[i].N + 7) / 8; a.mm.tile_end[i] = total; }
    const int bits = mats[0].bits, K = mats[0].ng * 128;
    // the decode matvec's columns per wave: >= ~1 KiB streams, short-K matrices more columns per wave, while the grid keeps 32 workgroups
    int tpw = K >= 2048 ? 1 : (K >= 1024 ? 2 : 4);
    while (tpw > 1 && (total + KR_WAVES * tpw - 1) / (KR_WAVES * tpw) < 32) tpw >>= 1;
    const int col_wgs = (total + KR_WAVES * tpw - 1) / (KR_WAVES * tpw);
    const KrRowsPlan p = kr_rows_plan(R, K, bits, col_wgs, group);
    if (!p.group || total < 1 || kr_rows_image_bytes(K, bits) != kr_lds_bytes(K, bits == 8)) return 1;
    const int img16 = (int)(kr_rows_image_bytes(K, bits) / 16);
#define KR_ROWS_GO(B_, G_) return kr_rows_launch<B_, G_>(a, x, ld_x, R, p, img16, act_mode, tpw, col_wgs, st)
    if (bits == 4) { if (p.cap == 4) KR_ROWS_GO(4, 4); if (p.cap == 8) KR_ROWS_GO(4, 8); KR_ROWS_GO(4, 16); }
    if (p.cap == 4) KR_ROWS_GO(8, 4);
    if (p.cap == 8) KR_ROWS_GO(8, 8);
    KR_ROWS_GO(8, 16);
#undef KR_ROWS_GO
}

int kr_launch_rows_matvec(const KrMatDev* mats, float* const* ys, const int* lds, int n, const float* x, int ld_x, int R, int act_mode, int group, hipStream_t st) {
    if (n < 1 || R < 1 || R > KR_ROWS_MAX) return 1;
    bool same = n <= KR_MAX_MULTI;
    for (int i = 1; i < n && same; i++) same = mats[i].bits == mats[0].bits && mats[i].ng == mats[0].ng;
    if (same) return kr_rows_launch_same(mats, ys, lds, n, x, ld_x, R, act_mode, group, st);
    for (int i = 0; i < n; i++)      // mixed 4 / 8-bit (or unlike K): one launch per matrix
        if (kr_rows_launch_same(mats + i, ys + i, lds + i, 1, x, ld_x, R, act_mode, group, st)) return 1;
    return 0;
}
