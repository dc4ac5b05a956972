// kr_mf_tiles.h -- the query-row tiles of a batched pass under "multi_extend_mla_flash" (docs/design/27-multi-extend-mla-flash.md), on the host.  No HIP in here:
// the pass (kr_decode_prefill.cpp) and a stand-alone test program include it alike.
// A pass has n runs; run i is counts[i] consecutive tokens of one slot, flattened as kr_pf_tiles.h says (docs/design/17-multi-extend.md): the last token of run i
// is pass row i, the others are rows off .. off + cnt - 2 with off = n + the sum of (counts[j] - 1) over j < i.  A run of one token is a unit row and keeps the
// per-row MLA attention kernels; a run of >= 2 tokens has cnt * nh (token, head) query rows, row = token * nh + head counted from the run's first token, cut into
// tiles of 64 rows, one workgroup each (kr_multi_mla_pf_flash.hip) -- what kr_launch_mla_flash does for a chunk of a prompt.
#pragma once
#include <stdint.h>

#include <vector>

#define KR_MF_TILE_ROWS 64      // query rows of a workgroup (MF_ROWS, kr_mla_flash_dev.h)

// tiles of a run of cnt tokens with nh heads
inline int kr_mf_run_tiles(int cnt, int nh) { return (int)(((int64_t)cnt * nh + KR_MF_TILE_ROWS - 1) / KR_MF_TILE_ROWS); }
// the pass row of token t < cnt of run i (the device side: kr_m_run_row, kr_multi.h)
inline int kr_mf_run_row(int i, int off, int cnt, int t) { return t == cnt - 1 ? i : off + t; }
// first and last token of tile tile_row of a run of cnt tokens (the body's tok_first / tok_last): the tile reads positions below pos0 + last + 1
inline int kr_mf_tile_first(int tile_row, int nh) { return tile_row * KR_MF_TILE_ROWS / nh; }
inline int kr_mf_tile_last(int cnt, int tile_row, int nh) { const int t = (tile_row * KR_MF_TILE_ROWS + KR_MF_TILE_ROWS - 1) / nh; return t < cnt - 1 ? t : cnt - 1; }

struct KrMfTileStats { int n_tiles, n_unit, n_long, long_tokens; };      // tiles; runs of one token; runs of >= 2 and their tokens

// out = n_tiles x [run, tile_row]: every run of >= 2 tokens in call order, tile_row = 0, 1, .. < ceil(counts[run] * nh / 64).  counts null: every run has one
// token (a step)
inline KrMfTileStats kr_mf_build_tiles(int n, const int32_t* counts, int nh, std::vector<int32_t>& out) {
    KrMfTileStats st{0, 0, 0, 0};
    out.clear();
    for (int i = 0; i < n; i++) {
        const int c = counts ? counts[i] : 1;
        if (c < 2) { st.n_unit++; continue; }
        st.n_long++; st.long_tokens += c;
        const int nt = kr_mf_run_tiles(c, nh);
        for (int r = 0; r < nt; r++) { out.push_back(i); out.push_back(r); st.n_tiles++; }
    }
    return st;
}
