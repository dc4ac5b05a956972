// kr_pf_tiles.h -- the query tiles of a batched pass under "multi_extend_flash" (docs/design/25-multi-extend-flash.md), on the host.  No HIP in here: the pass
// (kr_decode_prefill.cpp) and a stand-alone test program include it alike.
// A pass has n runs; run i is counts[i] consecutive tokens of one slot.  Its rows are flattened as kr_decode_multi.cpp's lay_rows does (docs/design/17-multi-extend.md):
// the last token of run i is pass row i, the others follow from row n on in call order, so run i's first cnt - 1 tokens are rows off .. off + cnt - 2 with
// off = n + the sum of (counts[j] - 1) over j < i.  A run of one token is a unit row and keeps the per-row attention kernels; a run of >= 2 tokens is cut into
// query tiles of tq = 128 / (nh / nkv) tokens, one workgroup each per KV head (kr_multi_pf_flash.hip).
#pragma once
#include <stdint.h>

#include <vector>

#define KR_PF_TILE_ROWS 128      // query rows of a workgroup: tokens x the heads of one KV head's group (FA_ROWS, kr_pfm_flash_dev.h)

// tokens per query tile of a layer
inline int kr_pf_tile_tokens(int nh, int nkv) { return KR_PF_TILE_ROWS / (nh / nkv); }
// the pass row of token t < cnt of run i (the device side: kr_m_run_row, kr_multi.h)
inline int kr_pf_run_row(int i, int off, int cnt, int t) { return t == cnt - 1 ? i : off + t; }
// one past the last position the tile at t0 of a run of cnt tokens standing at pos0 .. reads: its last token's own position is the last one any row of it sees
inline int kr_pf_tile_kv_end(int pos0, int cnt, int t0, int tq) { return pos0 + (t0 + tq < cnt ? t0 + tq : cnt); }

struct KrPfTileStats { int n_tiles, n_unit, n_long, long_tokens; };      // tiles; runs of one token; runs of >= 2 and their tokens

// out = n_tiles x [run, t0]: every run of >= 2 tokens in call order, t0 = 0, tq, 2 tq, .. < counts[run].  counts null: every run has one token (a step)
inline KrPfTileStats kr_pf_build_tiles(int n, const int32_t* counts, int tq, std::vector<int32_t>& out) {
    KrPfTileStats st{0, 0, 0, 0};
    out.clear();
    for (int i = 0; i < n; i++) {
        const int c = counts ? counts[i] : 1;
        if (c < 2) { st.n_unit++; continue; }
        st.n_long++; st.long_tokens += c;
        for (int t0 = 0; t0 < c; t0 += tq) { out.push_back(i); out.push_back(t0); st.n_tiles++; }
    }
    return st;
}
