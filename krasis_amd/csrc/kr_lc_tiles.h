// kr_lc_tiles.h -- the chunked runs of a batched pass under "multi_extend_la_chunk" (docs/design/26-multi-extend-la-chunk.md), on the host.  No HIP in here: the
// pass (kr_decode_prefill.cpp) and a stand-alone test program include it alike.
// A pass has n runs; run i is counts[i] consecutive tokens of one slot, flattened as kr_pf_tiles.h says.  A run of >= KR_LC_TOKENS tokens takes the chunked
// delta rule of the prompt pass (kr_lac_dev.h): it is cut into sub-chunks of KR_LC_TOKENS tokens, the last one partial; the prep launch takes one workgroup per
// (sub-chunk, value head), the scan one per (run, head, column slice) walking the run's sub-chunks in order.  Each sub-chunk owns one tile of the pass's scratch;
// the tiles follow the table's order, so a run's sub-chunk `sub` is scratch tile first + sub.  A shorter run keeps the exact run kernels.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#define KR_LC_TOKENS 64      // tokens per sub-chunk, and the shortest run that is chunked (LC_T, kr_lac_dev.h; kr_pfm_la_chunk_ok's rule)

struct KrLcStats { int n_runs, n_tiles, n_short, tokens; };      // chunked runs; their sub-chunks; the other runs; tokens of the chunked runs

// sub-chunks of a run of c tokens
inline int kr_lc_subs(int c) { return (c + KR_LC_TOKENS - 1) / KR_LC_TOKENS; }
// tokens of sub-chunk `sub` of a run of c tokens
inline int kr_lc_sub_tokens(int c, int sub) { const int r = c - sub * KR_LC_TOKENS; return r < KR_LC_TOKENS ? r : KR_LC_TOKENS; }
// runs = n_runs x [run, first scratch tile], every run of >= KR_LC_TOKENS tokens in call order; tiles = n_tiles x [run, sub], sub = 0 .. kr_lc_subs - 1 of each
// of them, in the same order: tile x of the table is scratch tile x.  counts null: every run has one token (a step)
inline KrLcStats kr_lc_build(int n, const int32_t* counts, std::vector<int32_t>& runs, std::vector<int32_t>& tiles) {
    KrLcStats st{0, 0, 0, 0};
    runs.clear(); tiles.clear();
    for (int i = 0; i < n; i++) {
        const int c = counts ? counts[i] : 1;
        if (c < KR_LC_TOKENS) { st.n_short++; continue; }
        runs.push_back(i); runs.push_back(st.n_tiles);
        st.n_runs++; st.tokens += c;
        for (int sub = 0; sub < kr_lc_subs(c); sub++) { tiles.push_back(i); tiles.push_back(sub); st.n_tiles++; }
    }
    return st;
}
// floats of scratch of one layer of nv value heads: per padded token and head the Y row, three pairs of bf16 planes and one G (kr_pfm_la_chunk_scratch_floats
// of 64 n_tiles tokens), plus alignment
inline size_t kr_lc_scratch_floats(int n_tiles, int nv) { return (size_t)n_tiles * KR_LC_TOKENS * nv * (4 * 128 + 1) + 4; }

// ---- "multi_extend_la_exact" (docs/design/36-multi-extend-la-exact.md): the staged runs of a pass ------------------------------------------------------------
// A run of >= min_tokens tokens (at least 2: a unit row is never staged) takes the exact staged form of the prompt pass (kr_pfm_la_dev.h): the conv launch takes a
// workgroup per (key head, tile of KR_LX_CONV_TOKENS tokens), the conv-state and delta-rule launches one per (., staged run), the gated norm one per (value head,
// tile of KR_LX_NORM_TOKENS tokens).  A shorter run keeps the run kernels.
#define KR_LX_CONV_TOKENS 16      // PFC_WT, kr_pfm_la_dev.h
#define KR_LX_NORM_TOKENS 8       // PFG_TT

struct KrLxStats { int n_runs, n_short, n16, n8, tokens; };      // staged runs; the other runs; tiles of 16 and of 8 tokens; tokens of the staged runs

// runs = n_runs x [run, first 16-token tile], every run of >= min_tokens tokens in call order; t16 / t8 = [run, t0], t0 = 0, 16, .. / 0, 8, .. < counts[run], of
// each of them in the same order.  counts null: every run has one token (a step)
inline KrLxStats kr_lx_build(int n, const int32_t* counts, int min_tokens, std::vector<int32_t>& runs, std::vector<int32_t>& t16, std::vector<int32_t>& t8) {
    KrLxStats st{0, 0, 0, 0, 0};
    runs.clear(); t16.clear(); t8.clear();
    if (min_tokens < 2) min_tokens = 2;
    for (int i = 0; i < n; i++) {
        const int c = counts ? counts[i] : 1;
        if (c < min_tokens) { st.n_short++; continue; }
        runs.push_back(i); runs.push_back(st.n16);
        st.n_runs++; st.tokens += c;
        for (int t0 = 0; t0 < c; t0 += KR_LX_CONV_TOKENS) { t16.push_back(i); t16.push_back(t0); st.n16++; }
        for (int t0 = 0; t0 < c; t0 += KR_LX_NORM_TOKENS) { t8.push_back(i); t8.push_back(t0); st.n8++; }
    }
    return st;
}
