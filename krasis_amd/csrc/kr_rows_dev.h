// kr_rows_dev.h -- the streaming matvec tile applied to a few rows at once (kr_rows_matvec.hip, docs/design/34-pass-few-rows.md): one wave, 8 columns, the
// lane's weight words and scales of a group held in registers and applied to every row's INT16 activation image in LDS.  Row r's sum is kr_matvec_tile's,
// operation for operation: kr_group_i4 / kr_group_i8 against row r's image, the 8-lane reduction, kr_chain in group order -- so a row carries the decode
// step's bits whatever the number of rows beside it.
#pragma once
#include "kr_matvec_tile_dev.h"

#define KR_ROWS_PRE 4   // group pairs (INT4) / groups (INT8) of a tile in flight: the unrolled body is KR_ROWS_PRE x RG rows long, a quarter of KR_PRE x RG

struct KrRowsPre { u32x4 w[KR_ROWS_PRE]; uint32_t sc[KR_ROWS_PRE]; };

// the records kr_preload would request, KR_ROWS_PRE at a time (same addresses, same non-temporal loads)
template <int BITS>
__device__ __forceinline__ void kr_rows_preload(KrRowsPre& p, const void* qbase, const uint32_t* sbase, const KrMatDev& m, int tile, int lane, int unit0) {
    const int units = BITS == 4 ? m.ngp : m.ng;
    const u32x4* q = reinterpret_cast<const u32x4*>(qbase) + (size_t)tile * units * 64 + lane;
    const uint32_t* s = sbase + (size_t)tile * m.ngp * 8 + (lane >> 3);
#pragma unroll
    for (int u = 0; u < KR_ROWS_PRE; u++)
        if (unit0 + u < units) { p.w[u] = kr_ldg_nt(q + (size_t)(unit0 + u) * 64); p.sc[u] = kr_ldg_nt(s + (BITS == 4 ? (unit0 + u) : ((unit0 + u) >> 1)) * 8); }
}

// acc[r] = column sum of row r < nr (nr <= RG, uniform); row r's image starts img16 records behind row r - 1's
template <int BITS, int RG>
__device__ __forceinline__ void kr_rows_tile(KrRowsPre& p, bool preloaded, const void* qbase, const uint32_t* sbase, const KrMatDev& m, int tile, u32x4* smem, int img16, int K,
                                             int nr, int lane, float (&acc)[RG]) {
    const int l8 = lane & 7, col = lane >> 3;
    const bool fused = (tile * 8 + col) < m.n_fma;
    const int units = BITS == 4 ? m.ngp : m.ng;
#pragma unroll
    for (int r = 0; r < RG; r++) acc[r] = 0.0f;
    for (int u0 = 0; u0 < units; u0 += KR_ROWS_PRE) {
        if (u0 > 0 || !preloaded) kr_rows_preload<BITS>(p, qbase, sbase, m, tile, lane, u0);
#pragma unroll
        for (int u = 0; u < KR_ROWS_PRE; u++) {
            const int un = u0 + u;
            if (un < units) {
#pragma unroll
                for (int r = 0; r < RG; r++) {
                    if (r < nr) {
                        const KrActLds L = kr_carve_lds(smem + (size_t)r * img16, K, BITS == 8);
                        if (BITS == 4) {
                            const int g0 = 2 * un, g1 = g0 + 1;
                            const int i0 = kr_red8_add_i32(kr_group_i4(p.w[u].x, p.w[u].y, g0, l8, L));
                            acc[r] = kr_chain(acc[r], i0, p.sc[u] & 0xFFFFu, L.ascale[g0], fused);
                            if (g1 < m.ng) {
                                const int i1 = kr_red8_add_i32(kr_group_i4(p.w[u].z, p.w[u].w, g1, l8, L));
                                acc[r] = kr_chain(acc[r], i1, p.sc[u] >> 16, L.ascale[g1], fused);
                            }
                        } else {
                            const int i0 = kr_red8_add_i32(kr_group_i8(p.w[u], un, l8, L));
                            acc[r] = kr_chain(acc[r], i0, (un & 1) ? (p.sc[u] >> 16) : (p.sc[u] & 0xFFFFu), L.ascale[un], fused);
                        }
                    }
                }
            }
        }
    }
}
