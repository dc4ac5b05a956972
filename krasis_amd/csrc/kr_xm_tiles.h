// kr_xm_tiles.h -- the query tiles of a batched pass under "multi_extend_exact_mfma" (docs/design/28-multi-extend-exact-mfma.md), on the host.  No HIP in here:
// the pass (kr_decode_prefill.cpp) and a stand-alone test program include it alike.
// The tables are kr_pf_tiles.h's -- [run, t0] for every run of >= 2 tokens in call order, rows through the same flatten -- at this option's two tile widths: the
// scores pass takes 64 query rows a workgroup, the P.V pass 32, a query row being (token, head of one KV head's group of G = nh / nkv).  G divides 32
// (kr_pfm_gqa_exact_mfma_ok), so the widths are powers of two from 2 to 64 and from 1 to 32 tokens.
#pragma once
#include "kr_pf_tiles.h"

#define KR_XM_ROWS_A 64      // query rows of a scores tile (kr_xm_scores_body, kr_xm_dev.h)
#define KR_XM_ROWS_C 32      // query rows of a P.V tile (kr_xm_pv_body)

inline int kr_xm_tile_tokens_a(int nh, int nkv) { return KR_XM_ROWS_A / (nh / nkv); }
inline int kr_xm_tile_tokens_c(int nh, int nkv) { return KR_XM_ROWS_C / (nh / nkv); }
// one past the largest position any run of >= 2 tokens reads: the scores pass's grid covers the position tiles below it.  0: every run has one token
inline int kr_xm_kv_end_max(int n, const int32_t* counts, const int32_t* positions) {
    int end = 0;
    for (int i = 0; i < n; i++)
        if (counts && counts[i] >= 2 && positions[i] + counts[i] > end) end = positions[i] + counts[i];
    return end;
}
