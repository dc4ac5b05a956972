// kr_multi_plan.h -- everything the batched pass over device slots decides before it allocates, uploads or launches (docs/design/32-multi-pass-plan.md), on
// the host.  No HIP in here: the pass (kr_multi_pass, kr_decode_prefill.cpp) and a stand-alone test program (tests/multi_plan_check.cpp) include it alike.
// Inputs are plain values: the store's options and thresholds, per layer the numbers the plan reads, and the pass's rows.  The output is one KrMultiPlan: which
// rows the per-row kernels see, chunk counts and byte sizes, the score rows, the split flags, what the runs of >= 2 tokens take, and every tile table of the pass
// in ONE vector with an (offset, tiles) span per table.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "kr_lc_tiles.h"
#include "kr_mf_tiles.h"
#include "kr_multi_opts.h"
#include "kr_pf_tiles.h"
#include "kr_xm_tiles.h"

enum { KR_MP_OTHER = 0, KR_MP_LA = 1, KR_MP_GQA = 2, KR_MP_MLA = 3 };      // a layer's attention kind
enum { KR_MP_RUNS_ROWS = 0, KR_MP_RUNS_FLASH = 1, KR_MP_RUNS_XM = 2 };      // what the runs of >= 2 tokens take: per-row kernels, flash run kernels, exact matrix-core passes
enum { KR_MP_OK = 0, KR_MP_GQA_CHUNKS = 1, KR_MP_MLA_CHUNKS = 2 };          // result: a unit row needs more than KR_MP_MAX_CHUNKS flash-decode chunks
#define KR_MP_MAX_CHUNKS 1024      // the merge kernels have one thread per chunk

struct KrMultiPlanOpts {
    KrMultiOpts opt;     // the store's options as they stand, in one assignment (kr_multi_opts.h); the rest is what the pass derives
    bool attn_fast;      // "multi_attn_fast" || "multi_attn_fast_paged"
    int gqa_split_min, mla_split_min;
    int max_seq, fd_chunk, mla_chunk;      // the slots' capacity; kr_fd_flash_chunk(max_seq) and kr_mla_flash_decode_chunk(max_seq): the rules stay beside their kernels
};
struct KrMultiPlanLayer { int kind, nh, nkv, hd, klr, nv; };
struct KrMultiPlanRows { int n, n_final, max_pos; bool verify; const int32_t* counts; const int32_t* positions; };      // counts / positions: host, may be null (a plain step)

struct KrMpSpan { int off = -1, n = 0; };      // a table of n tiles of two ints at tables[off]; off < 0: the pass has no such table
struct KrMultiPlan {
    int rc = KR_MP_OK;      // KR_MP_GQA_CHUNKS: attn_pos needs fd_chunks of fd_chunk positions; KR_MP_MLA_CHUNKS: mla_pos, mla_chunks, mla_chunk; nothing behind them is planned
    int attn_rows = 0, attn_pos = 0, mla_rows = 0, mla_pos = 0;      // the rows and the longest position the per-row GQA / MLA kernels see
    bool row_attn = true, mla_row_attn = true;                       // some row takes them
    int fd_chunk = 0, fd_chunks = 0, mla_chunk = 0, mla_chunks = 0; size_t fd_o_bytes = 0, fd_ml_bytes = 0;      // split-KV flash-decode of the unit rows (0 chunks: the exact kernel)
    bool need_scores = false; int sc_ld = 0; size_t score_bytes = 0; int n_logits = 0;
    bool xs_split = false, mla_xs_split = false;
    int gqa_runs = KR_MP_RUNS_ROWS, mla_runs = KR_MP_RUNS_ROWS;
    int n_unit = 0;                                                  // runs of one token
    bool any_run = false;                                            // a non-verify pass with counts and positions holds a run of >= 2 tokens: what the run options apply to
    int kv_end = 0; size_t xm_inv_bytes = 0, xm_tmax_bytes = 0;      // matrix-core passes: one past the largest position a run reads; 1 / sum and row maxima per 32 positions
    int lc_nruns = 0, lc_ntiles = 0, lc_short = 0; size_t lc_scratch_floats = 0;      // chunked delta rule: runs of >= 64 tokens, their sub-chunks, the other runs
    int lx_nruns = 0, lx_short = 0;                                  // exact staged linear attention: runs of >= la_exact_min tokens, the runs left to the run kernels
    std::vector<int32_t> tables;                                     // every table of the pass, each at a multiple of four ints
    KrMpSpan pf[8], xa[8], xc[8];                                    // per tile width 1 << w tokens: flash query tiles; matrix-core scores and P.V tiles (GQA and MLA layers alike)
    struct Mf { int nh; KrMpSpan t; };
    std::vector<Mf> mf;                                              // per head count among the MLA layers: flash query-row tiles
    KrMpSpan lc_runs, lc_tiles;                                      // chunked runs [run, first tile] and their sub-chunks [run, sub]
    KrMpSpan lx_runs, lx_t16, lx_t8;                                 // staged runs [run, first 16-token tile], their tiles of 16 and of 8 tokens [run, t0]
};

inline int kr_mp_log2(int t) { int w = 0; while ((1 << w) < t) w++; return w; }      // tile widths are powers of two up to 128
// a layer's tables
inline KrMpSpan kr_mp_pf(const KrMultiPlan& p, int nh, int nkv) { return p.pf[kr_mp_log2(kr_pf_tile_tokens(nh, nkv))]; }
inline KrMpSpan kr_mp_xa(const KrMultiPlan& p, int nh, int nkv) { return p.xa[kr_mp_log2(kr_xm_tile_tokens_a(nh, nkv))]; }      // MLA: nkv = 1, one latent row serves every head
inline KrMpSpan kr_mp_xc(const KrMultiPlan& p, int nh, int nkv) { return p.xc[kr_mp_log2(kr_xm_tile_tokens_c(nh, nkv))]; }
inline KrMpSpan kr_mp_mf(const KrMultiPlan& p, int nh) { for (const KrMultiPlan::Mf& t : p.mf) if (t.nh == nh) return t.t; return KrMpSpan{}; }

// one table behind the others, at the next multiple of four ints
inline KrMpSpan kr_mp_append(std::vector<int32_t>& all, const std::vector<int32_t>& one) {
    all.resize((all.size() + 3) & ~(size_t)3, 0);
    KrMpSpan sp; sp.off = (int)all.size(); sp.n = (int)(one.size() / 2);
    all.insert(all.end(), one.begin(), one.end());
    return sp;
}
// the [run, t0] table at one tile width into its place among spans[log2 width]; a width that is there already is built once
inline void kr_mp_width_table(KrMultiPlan& p, const KrMultiPlanRows& r, int width, KrMpSpan* spans) {
    KrMpSpan& sp = spans[kr_mp_log2(width)];
    if (sp.off >= 0) return;
    std::vector<int32_t> one;
    kr_pf_build_tiles(r.n_final, r.counts, width, one);
    sp = kr_mp_append(p.tables, one);
}

inline int kr_multi_plan(const KrMultiPlanOpts& o, const KrMultiPlanLayer* layers, int n_layers, const KrMultiPlanRows& r, KrMultiPlan& p) {
    p = KrMultiPlan{};
    int nh_max = 1, nv_max = 0; size_t gqa_row = 0, mla_row = 0; bool has_gqa = false, has_mla = false;
    for (int l = 0; l < n_layers; l++) {
        const KrMultiPlanLayer& L = layers[l];
        if ((L.kind == KR_MP_GQA || L.kind == KR_MP_MLA) && L.nh > nh_max) nh_max = L.nh;      // a score row per query head of either kind
        if (L.kind == KR_MP_GQA) { has_gqa = true; if ((size_t)L.nh * L.hd > gqa_row) gqa_row = (size_t)L.nh * L.hd; }
        if (L.kind == KR_MP_MLA) { has_mla = true; if ((size_t)L.nh * L.klr > mla_row) mla_row = (size_t)L.nh * L.klr; }
        if (L.kind == KR_MP_LA && L.nv > nv_max) nv_max = L.nv;
    }
    // the one scan of the runs: is there a run of >= 2 tokens, how many have one, and the longest position among those.  A verify pass, or a caller that gave
    // no counts / positions (a plain step): no run option applies
    bool& any_run = p.any_run; int unit_pos = -1;
    p.n_unit = r.n_final;
    if (!r.verify && r.counts && r.positions) {
        p.n_unit = 0;
        for (int i = 0; i < r.n_final; i++) {
            if (r.counts[i] >= 2) any_run = true;
            else { p.n_unit++; if (r.positions[i] > unit_pos) unit_pos = r.positions[i]; }
        }
    }
    // split-KV flash-decode of the unit rows over slots longer than the store's capacity rule ("multi_attn_fast" 16 / 23, "multi_mla_fast" 24)
    const bool flash = o.attn_fast && has_gqa && o.max_seq > o.gqa_split_min, mla_flash = o.opt.mla_fast && has_mla && o.max_seq > o.mla_split_min;
    // what the runs of >= 2 tokens take.  Flash run kernels (25, 27): the per-row kernels then see the unit rows only, which lie among the first n_final rows, so
    // their score rows and partials are sized by n_final rows at the unit rows' longest position.  Exact matrix-core passes (28, 29): the runs keep their score
    // rows -- n rows at the pass's longest position.  Flash and matrix-core passes of one kind never meet, nor do "multi_extend_flash"
    // and an MLA layer (the rule list of kr_option_rules, kr_decode_prefill.cpp)
    if (any_run && has_gqa) p.gqa_runs = o.opt.extend_flash ? KR_MP_RUNS_FLASH : o.opt.extend_exact_mfma ? KR_MP_RUNS_XM : KR_MP_RUNS_ROWS;
    if (any_run && has_mla) p.mla_runs = o.opt.extend_mla_flash ? KR_MP_RUNS_FLASH : o.opt.extend_mla_exact_mfma ? KR_MP_RUNS_XM : KR_MP_RUNS_ROWS;
    const bool pf = p.gqa_runs == KR_MP_RUNS_FLASH, mf = p.mla_runs == KR_MP_RUNS_FLASH, xm = p.gqa_runs == KR_MP_RUNS_XM, xl = p.mla_runs == KR_MP_RUNS_XM;
    p.attn_rows = p.mla_rows = r.n; p.attn_pos = p.mla_pos = r.max_pos;
    if (pf) { p.attn_rows = r.n_final; p.attn_pos = unit_pos; }
    if (mf) { p.mla_rows = r.n_final; p.mla_pos = unit_pos; }
    if (mf && !has_gqa) { p.attn_rows = r.n_final; p.attn_pos = unit_pos; }      // an MLA-only store shrinks the score rows; one with GQA layers keeps theirs, which hold the MLA unit rows too
    p.row_attn = !pf || p.n_unit > 0; p.mla_row_attn = !mf || p.n_unit > 0;
    if (flash && p.row_attn) {
        p.fd_chunk = o.fd_chunk; p.fd_chunks = (p.attn_pos + p.fd_chunk) / p.fd_chunk;
        if (p.fd_chunks > KR_MP_MAX_CHUNKS) return p.rc = KR_MP_GQA_CHUNKS;
        p.fd_o_bytes = (size_t)p.attn_rows * p.fd_chunks * gqa_row * 4; p.fd_ml_bytes = (size_t)p.attn_rows * nh_max * p.fd_chunks * 8;
    }
    if (mla_flash && p.mla_row_attn) {      // its chunks are 64 / 128 positions against the GQA kernels' 128 / 256; the partials of both kinds share two buffers, sized for the larger need
        p.mla_chunk = o.mla_chunk; p.mla_chunks = (p.mla_pos + p.mla_chunk) / p.mla_chunk;
        if (p.mla_chunks > KR_MP_MAX_CHUNKS) return p.rc = KR_MP_MLA_CHUNKS;
        const size_t ob = (size_t)p.mla_rows * p.mla_chunks * mla_row * 4, mb = (size_t)p.mla_rows * nh_max * p.mla_chunks * 8;
        if (ob > p.fd_o_bytes) p.fd_o_bytes = ob;
        if (mb > p.fd_ml_bytes) p.fd_ml_bytes = mb;
    }
    // score rows: for every per-row kernel that is not a flash-decode, and for the matrix-core passes even then.  The row stride is a multiple of 64 under those
    // (the P.V pass reads stages of 64 columns, the row maxima are per 32): no bit depends on it
    p.need_scores = (has_gqa && !flash && p.row_attn) || (has_mla && !mla_flash && p.mla_row_attn) || xm || xl;
    p.sc_ld = xm || xl ? (p.attn_pos + 1 + 63) & ~63 : (p.attn_pos + 1 + 31) & ~31;
    p.score_bytes = (size_t)p.attn_rows * nh_max * p.sc_ld * 4;
    p.n_logits = r.verify ? r.n : r.n_final;      // a verify pass: the lm_head over every token row
    // the exact per-slot attention as three launches (30, 31): a pass-level choice by the longest attention of the per-row kernels; -1: no unit row, nothing launched
    p.xs_split = o.opt.attn_exact_split && has_gqa && p.attn_pos + 1 >= o.opt.attn_exact_split_min;
    p.mla_xs_split = o.opt.mla_exact_split && has_mla && p.mla_pos + 1 >= o.opt.mla_exact_split_min;
    std::vector<int32_t> one;
    for (int l = 0; l < n_layers; l++) {
        const KrMultiPlanLayer& L = layers[l];
        if (L.kind == KR_MP_GQA && pf) kr_mp_width_table(p, r, kr_pf_tile_tokens(L.nh, L.nkv), p.pf);
        if ((L.kind == KR_MP_GQA && xm) || (L.kind == KR_MP_MLA && xl)) {
            const int nkv = L.kind == KR_MP_MLA ? 1 : L.nkv;
            kr_mp_width_table(p, r, kr_xm_tile_tokens_a(L.nh, nkv), p.xa); kr_mp_width_table(p, r, kr_xm_tile_tokens_c(L.nh, nkv), p.xc);
        }
        if (L.kind == KR_MP_MLA && mf && kr_mp_mf(p, L.nh).off < 0) {
            kr_mf_build_tiles(r.n_final, r.counts, L.nh, one);
            p.mf.push_back(KrMultiPlan::Mf{L.nh, kr_mp_append(p.tables, one)});
        }
    }
    if (xm || xl) {
        const size_t sc_rows = (size_t)r.n * nh_max;
        p.kv_end = kr_xm_kv_end_max(r.n_final, r.counts, r.positions);
        p.xm_inv_bytes = (sc_rows * 4 + 255) & ~(size_t)255; p.xm_tmax_bytes = sc_rows * (size_t)(p.sc_ld / 32) * 4;
    }
    // chunked delta rule (26): one table for every linear-attention layer -- the chunked runs, then their sub-chunks -- and one scratch, sized by the widest layer
    if (o.opt.extend_la_chunk && !r.verify && r.counts && nv_max) {
        std::vector<int32_t> lr, lt;
        const KrLcStats ls = kr_lc_build(r.n_final, r.counts, lr, lt);
        if (ls.n_runs) {
            p.lc_runs = kr_mp_append(p.tables, lr); p.lc_tiles = kr_mp_append(p.tables, lt);
            p.lc_nruns = ls.n_runs; p.lc_ntiles = ls.n_tiles; p.lc_short = ls.n_short; p.lc_scratch_floats = kr_lc_scratch_floats(ls.n_tiles, nv_max);
        }
    }
    // exact staged linear attention (36): one set of tables for every linear-attention layer -- the staged runs, their conv tiles, their gated-norm tiles
    if (o.opt.extend_la_exact && !r.verify && r.counts && nv_max) {
        std::vector<int32_t> xr, x16, x8;
        const KrLxStats xs = kr_lx_build(r.n_final, r.counts, o.opt.extend_la_exact_min, xr, x16, x8);
        if (xs.n_runs) {
            p.lx_runs = kr_mp_append(p.tables, xr); p.lx_t16 = kr_mp_append(p.tables, x16); p.lx_t8 = kr_mp_append(p.tables, x8);
            p.lx_nruns = xs.n_runs; p.lx_short = xs.n_short;
        }
    }
    return p.rc;
}
