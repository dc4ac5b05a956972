// multi_plan_check.cpp -- stand-alone check of kr_multi_plan.h, everything the batched pass over device slots decides before it allocates, uploads or launches
// (docs/design/32-multi-pass-plan.md).  Host only, its own main: tests/test_multi_pass_plan.py compiles it with -fsanitize=address,undefined and runs it.
// The expected values of cases A .. J are written out by hand from the rules of the design notes; none comes from calling the planner.  The chunk sizes are
// what the kernels' rules give for each max_seq (128 / 256 positions for GQA below / from 131 072, 64 / 128 for MLA up to / above 16 384): the caller passes them.
// Each case prints its marker; the test files of the options assert the markers they rely on.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kr_multi_plan.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "multi_plan_check: line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

static const KrMultiPlanLayer GQA_8_2_64{KR_MP_GQA, 8, 2, 64, 0, 0}, MLA_16_512{KR_MP_MLA, 16, 0, 0, 512, 0}, LA_NV16{KR_MP_LA, 0, 0, 0, 0, 16};

static KrMultiPlanOpts opts(int max_seq, int fd_chunk, int mla_chunk) {
    KrMultiPlanOpts o{};
    o.opt.attn_exact_split_min = 512; o.opt.mla_exact_split_min = 512; o.gqa_split_min = 1024; o.mla_split_min = 512;      // the defaults
    o.max_seq = max_seq; o.fd_chunk = fd_chunk; o.mla_chunk = mla_chunk;
    return o;
}
struct Pass {
    std::vector<int32_t> counts, positions; bool verify = false;
    KrMultiPlanRows rows() const {
        int n = 0, max_pos = 0;
        for (size_t i = 0; i < counts.size(); i++) { n += counts[i]; if (positions[i] + counts[i] - 1 > max_pos) max_pos = positions[i] + counts[i] - 1; }
        return KrMultiPlanRows{n, (int)counts.size(), max_pos, verify, counts.data(), positions.data()};
    }
};
static KrMultiPlan plan(const KrMultiPlanOpts& o, const std::vector<KrMultiPlanLayer>& layers, const KrMultiPlanRows& r, int want_rc = KR_MP_OK) {
    KrMultiPlan p;
    CHECK(kr_multi_plan(o, layers.data(), (int)layers.size(), r, p) == want_rc && p.rc == want_rc);
    return p;
}
static int n_tables(const KrMultiPlan& p) {
    int n = (int)p.mf.size() + (p.lc_runs.off >= 0) + (p.lc_tiles.off >= 0);
    for (int w = 0; w < 8; w++) n += (p.pf[w].off >= 0) + (p.xa[w].off >= 0) + (p.xc[w].off >= 0);
    return n;
}
static bool no_run_option(const KrMultiPlan& p, const KrMultiPlanRows& r) {      // what a pass without a run of >= 2 tokens decides
    return p.gqa_runs == KR_MP_RUNS_ROWS && p.mla_runs == KR_MP_RUNS_ROWS && p.attn_rows == r.n && p.attn_pos == r.max_pos && p.mla_rows == r.n && p.mla_pos == r.max_pos &&
           p.row_attn && p.mla_row_attn && p.tables.empty() && n_tables(p) == 0 && p.kv_end == 0 && p.xm_inv_bytes == 0 && p.lc_nruns == 0;
}

static void case_a_f() {
    // case A: flash run kernels with unit rows
    KrMultiPlanOpts o = opts(2048, 128, 64);
    o.attn_fast = true; o.opt.extend_flash = true;
    Pass a; a.counts = {1, 3, 1}; a.positions = {700, 10, 5};
    const KrMultiPlanRows ra = a.rows();
    CHECK(ra.n == 5 && ra.n_final == 3 && ra.max_pos == 700);
    KrMultiPlan p = plan(o, {GQA_8_2_64}, ra);
    CHECK(p.gqa_runs == KR_MP_RUNS_FLASH && p.n_unit == 2 && p.attn_rows == 3 && p.attn_pos == 700 && p.row_attn);
    CHECK(p.fd_chunk == 128 && p.fd_chunks == 6 && p.fd_o_bytes == 36864 && p.fd_ml_bytes == 1152 && !p.need_scores && p.n_logits == 3);
    CHECK(n_tables(p) == 1 && p.pf[5].off == 0 && p.pf[5].n == 1 && p.tables == (std::vector<int32_t>{1, 0}));      // width 32 = 128 / (8 / 2): the tile [run 1, t0 0]
    std::puts("case A ok");
    // case B: no unit row
    Pass b; b.counts = {2, 3}; b.positions = {0, 10};
    o.opt.attn_exact_split = true;
    for (int mn : {1, 2, 512}) {
        o.opt.attn_exact_split_min = mn;
        p = plan(o, {GQA_8_2_64}, b.rows());
        CHECK(p.n_unit == 0 && p.attn_pos == -1 && p.attn_rows == 2 && !p.row_attn && p.fd_chunks == 0 && p.fd_o_bytes == 0 && p.fd_ml_bytes == 0 && !p.need_scores && !p.xs_split);
    }
    std::puts("case B ok");
    // case F: a verify pass takes no run option -- first A ...
    o.opt.attn_exact_split = false; a.verify = true;
    const KrMultiPlanRows rf = a.rows();
    p = plan(o, {GQA_8_2_64}, rf);
    CHECK(no_run_option(p, rf) && p.n_logits == 5 && p.fd_chunks == 6 && p.fd_o_bytes == (size_t)5 * 6 * 512 * 4);
}

static void case_c_d() {
    // case C: a mixed store keeps the score rows
    KrMultiPlanOpts o = opts(256, 128, 64);
    o.opt.extend_mla_flash = true;
    Pass c; c.counts = {1, 4}; c.positions = {40, 100};
    const KrMultiPlanRows r = c.rows();
    CHECK(r.n == 5 && r.max_pos == 103);
    KrMultiPlan p = plan(o, {GQA_8_2_64, MLA_16_512}, r);
    CHECK(p.mla_runs == KR_MP_RUNS_FLASH && p.gqa_runs == KR_MP_RUNS_ROWS && p.mla_rows == 2 && p.mla_pos == 40 && p.attn_rows == 5 && p.attn_pos == 103);
    CHECK(p.need_scores && p.sc_ld == 128 && p.score_bytes == 40960 && p.fd_chunks == 0 && p.mla_chunks == 0);
    CHECK(n_tables(p) == 1 && p.mf.size() == 1 && p.mf[0].nh == 16 && p.mf[0].t.n == 1 && kr_mp_mf(p, 16).off == 0 && kr_mp_mf(p, 8).off < 0);
    CHECK(p.tables == (std::vector<int32_t>{1, 0}));      // 4 tokens x 16 heads = one tile of 64 query rows: [run 1, tile_row 0]
    std::puts("case C ok");
    // case D: an MLA-only store shrinks them
    p = plan(o, {MLA_16_512}, r);
    CHECK(p.mla_rows == 2 && p.mla_pos == 40 && p.attn_rows == 2 && p.attn_pos == 40 && p.need_scores && p.sc_ld == 64 && p.score_bytes == 8192);
    std::puts("case D ok");
}

static void case_e_f() {
    // case E: matrix-core passes under flash
    KrMultiPlanOpts o = opts(2048, 128, 64);
    o.attn_fast = true; o.opt.extend_exact_mfma = true;
    Pass e; e.counts = {1, 3}; e.positions = {700, 10};
    const KrMultiPlanRows r = e.rows();
    KrMultiPlan p = plan(o, {GQA_8_2_64}, r);
    CHECK(p.gqa_runs == KR_MP_RUNS_XM && p.n_unit == 1 && p.attn_rows == 4 && p.attn_pos == 700 && p.fd_chunks == 6 && p.fd_o_bytes == 49152 && p.fd_ml_bytes == 1536);
    CHECK(p.need_scores && p.sc_ld == 704 && p.sc_ld % 64 == 0 && p.score_bytes == 90112 && p.kv_end == 13 && p.xm_inv_bytes == 256 && p.xm_tmax_bytes == 2816);
    CHECK(n_tables(p) == 2 && p.xa[4].n == 1 && p.xc[3].n == 1 && p.xa[4].off == 0 && p.xc[3].off == 4);      // scores at 64 / 4 = 16 tokens, P.V at 32 / 4 = 8
    CHECK(p.tables == (std::vector<int32_t>{1, 0, 0, 0, 1, 0}));
    std::puts("case E ok");
    // ... case F, second half: E as a verify pass
    e.verify = true;
    const KrMultiPlanRows rf = e.rows();
    p = plan(o, {GQA_8_2_64}, rf);
    CHECK(no_run_option(p, rf) && p.n_logits == 4 && !p.need_scores && p.sc_ld == 704);      // under flash no per-row kernel reads score rows; 701 rounds to 704 at 32 too
    // ... and the MLA run options and the chunked delta rule likewise
    KrMultiPlanOpts om = opts(2048, 128, 64);
    om.opt.extend_mla_exact_mfma = true;
    p = plan(om, {MLA_16_512}, rf);
    CHECK(no_run_option(p, rf) && p.need_scores && p.sc_ld == 704 && p.n_logits == 4);
    om.opt.extend_mla_exact_mfma = false; om.opt.extend_mla_flash = true; om.opt.extend_la_chunk = true;
    Pass lc; lc.counts = {70, 1}; lc.positions = {0, 9}; lc.verify = true;
    const KrMultiPlanRows rl = lc.rows();
    p = plan(om, {LA_NV16, MLA_16_512}, rl);      // (a store the refusals do not allow; the plan's rule holds whatever the store)
    CHECK(no_run_option(p, rl) && p.n_logits == 71);
    lc.verify = false;
    p = plan(om, {LA_NV16, MLA_16_512}, lc.rows());
    CHECK(p.mla_runs == KR_MP_RUNS_FLASH && p.lc_nruns == 1 && p.lc_ntiles == 2 && p.lc_short == 1 && p.lc_scratch_floats == (size_t)2 * 64 * 16 * 513 + 4);
    std::puts("case F ok");
}

static void case_g_h() {
    // case G: a plain step gives no counts
    KrMultiPlanOpts o = opts(2048, 128, 64);
    o.attn_fast = true; o.opt.extend_flash = true; o.opt.extend_la_chunk = true;
    KrMultiPlanRows r{3, 3, 700, false, nullptr, nullptr};
    KrMultiPlan p = plan(o, {LA_NV16, GQA_8_2_64}, r);
    CHECK(no_run_option(p, r) && p.n_unit == 3 && p.n_logits == 3 && p.fd_chunks == 6);
    Pass units; units.counts = {1, 1, 1}; units.positions = {700, 10, 5};      // the same as every run of one token
    const KrMultiPlanRows ru = units.rows();
    const KrMultiPlan q = plan(o, {LA_NV16, GQA_8_2_64}, ru);
    CHECK(no_run_option(q, ru) && q.n_unit == 3 && q.fd_chunks == p.fd_chunks && q.fd_o_bytes == p.fd_o_bytes && q.sc_ld == p.sc_ld && q.need_scores == p.need_scores);
    std::puts("case G ok");
    // case H: the split thresholds
    o = opts(2048, 128, 64);
    o.opt.attn_exact_split = true; o.opt.mla_exact_split = true;
    r = KrMultiPlanRows{1, 1, 510, false, nullptr, nullptr};
    CHECK(!plan(o, {GQA_8_2_64}, r).xs_split && !plan(o, {MLA_16_512}, r).mla_xs_split);
    r.max_pos = 511;
    CHECK(plan(o, {GQA_8_2_64}, r).xs_split && plan(o, {MLA_16_512}, r).mla_xs_split);
    CHECK(!plan(o, {GQA_8_2_64}, r).mla_xs_split && !plan(o, {MLA_16_512}, r).xs_split);      // no layer of the kind: off
    o.opt.extend_mla_flash = true; o.opt.mla_exact_split_min = 1;
    Pass b; b.counts = {2}; b.positions = {600};
    p = plan(o, {MLA_16_512}, b.rows());
    CHECK(p.mla_pos == -1 && !p.mla_xs_split && !p.mla_row_attn);      // no unit row: nothing launched, nothing split
    std::puts("case H ok");
}

static void case_i() {
    // case I: the chunk limits
    KrMultiPlanOpts o = opts(300000, 256, 128);
    o.attn_fast = true;
    const KrMultiPlanRows r{1, 1, 262144, false, nullptr, nullptr};
    KrMultiPlan p = plan(o, {GQA_8_2_64}, r, KR_MP_GQA_CHUNKS);
    CHECK(p.attn_pos == 262144 && p.fd_chunks == 1025 && p.fd_chunk == 256);
    KrMultiPlanRows under = r; under.max_pos = 262143;
    CHECK(plan(o, {GQA_8_2_64}, under).fd_chunks == 1024);
    o = opts(20000, 128, 128);
    o.opt.mla_fast = true;
    const KrMultiPlanRows rm{1, 1, 131072, false, nullptr, nullptr};
    p = plan(o, {MLA_16_512}, rm, KR_MP_MLA_CHUNKS);
    CHECK(p.mla_pos == 131072 && p.mla_chunks == 1025 && p.mla_chunk == 128);
    o.attn_fast = true;      // both over the limit: the GQA one is reported
    p = plan(o, {GQA_8_2_64, MLA_16_512}, rm, KR_MP_GQA_CHUNKS);
    CHECK(p.fd_chunks == 1025 && p.fd_chunk == 128 && p.attn_pos == 131072);
    std::puts("case I ok");
}

static void case_j() {
    // case J: a width two options ask for is built once
    KrMultiPlanOpts o = opts(256, 128, 64);
    o.opt.extend_exact_mfma = true; o.opt.extend_mla_exact_mfma = true;
    Pass j; j.counts = {3, 1}; j.positions = {10, 20};
    const KrMultiPlanLayer mla4{KR_MP_MLA, 4, 0, 0, 512, 0};      // G = 4, as GQA(8, 2, 64)
    KrMultiPlan p = plan(o, {GQA_8_2_64, mla4}, j.rows());
    CHECK(p.gqa_runs == KR_MP_RUNS_XM && p.mla_runs == KR_MP_RUNS_XM && n_tables(p) == 2 && p.tables.size() == 6);
    CHECK(kr_mp_xa(p, 8, 2).off == kr_mp_xa(p, 4, 1).off && kr_mp_xc(p, 8, 2).off == kr_mp_xc(p, 4, 1).off && kr_mp_xa(p, 8, 2).off != kr_mp_xc(p, 8, 2).off);
    CHECK(kr_mp_xa(p, 8, 2).off >= 0 && kr_mp_xc(p, 8, 2).off >= 0);
    const KrMultiPlanLayer gqa_4_2{KR_MP_GQA, 4, 2, 64, 0, 0};      // G = 2: 32 and 16 tokens
    p = plan(o, {GQA_8_2_64, gqa_4_2}, j.rows());
    CHECK(n_tables(p) == 4 && p.xa[4].off >= 0 && p.xc[3].off >= 0 && p.xa[5].off >= 0 && p.xc[4].off >= 0 && p.xa[4].off != p.xc[4].off);
    std::puts("case J ok");
}

// case K: properties over pseudo-random passes
static uint32_t rng_state = 0x2545F491u;
static int rnd(int n) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return (int)(rng_state % (uint32_t)n); }
struct Tab { KrMpSpan sp; std::vector<int32_t> want; };
static void case_k() {
    const int gs[] = {1, 2, 4, 8, 16, 32};
    for (int it = 0; it < 2000; it++) {
        // a store the refusals allow: 0 GQA, 1 MLA, 2 LA + GQA, 3 GQA + MLA
        const int store = rnd(4);
        std::vector<KrMultiPlanLayer> layers;
        const bool has_gqa = store != 1, has_mla = store == 1 || store == 3, has_la = store == 2;
        if (has_la) layers.push_back(KrMultiPlanLayer{KR_MP_LA, 0, 0, 0, 0, 1 + rnd(32)});
        for (int k = 0; has_gqa && k < 1 + rnd(2); k++) { const int nkv = 1 + rnd(4), g = gs[rnd(6)]; layers.push_back(KrMultiPlanLayer{KR_MP_GQA, nkv * g, nkv, 64 << rnd(3), 0, 0}); }
        for (int k = 0; has_mla && k < 1 + rnd(2); k++) layers.push_back(KrMultiPlanLayer{KR_MP_MLA, gs[rnd(6)], 0, 0, rnd(2) ? 512 : 256, 0});
        if (has_la && rnd(2)) layers.push_back(KrMultiPlanLayer{KR_MP_OTHER, 0, 0, 0, 0, 0});
        KrMultiPlanOpts o = opts(64 << rnd(8), 128, 64);
        o.attn_fast = !has_mla && rnd(2); o.opt.mla_fast = has_mla && rnd(2);
        o.opt.extend_flash = has_gqa && !has_mla && rnd(2); o.opt.extend_exact_mfma = has_gqa && !o.opt.extend_flash && rnd(2);
        o.opt.extend_mla_flash = has_mla && rnd(2); o.opt.extend_mla_exact_mfma = has_mla && !o.opt.extend_mla_flash && rnd(2);
        o.opt.extend_la_chunk = has_la && rnd(2);
        o.opt.attn_exact_split = has_gqa && rnd(2); o.opt.mla_exact_split = has_mla && rnd(2);
        o.opt.attn_exact_split_min = 1 + rnd(600); o.opt.mla_exact_split_min = 1 + rnd(600);
        Pass ps; ps.verify = rnd(8) == 0;
        int T = 0;
        for (int i = 0, nf = 1 + rnd(16); i < nf; i++) {
            int c = rnd(3) == 0 ? 1 : 1 + rnd(130);
            if (T + c > 1024) break;
            T += c; ps.counts.push_back(c); ps.positions.push_back(rnd(4000));
        }
        KrMultiPlanRows r = ps.rows();
        if (rnd(10) == 0) { r.counts = nullptr; r.positions = nullptr; r.n = r.n_final; }      // a plain step
        KrMultiPlan p;
        const int rc = kr_multi_plan(o, layers.data(), (int)layers.size(), r, p);
        if (rc != KR_MP_OK) { CHECK(p.fd_chunks > KR_MP_MAX_CHUNKS || p.mla_chunks > KR_MP_MAX_CHUNKS); continue; }
        int nh_max = 1;
        for (const KrMultiPlanLayer& L : layers) if ((L.kind == KR_MP_GQA || L.kind == KR_MP_MLA) && L.nh > nh_max) nh_max = L.nh;
        const bool xm = p.gqa_runs == KR_MP_RUNS_XM || p.mla_runs == KR_MP_RUNS_XM;
        CHECK(p.attn_rows == r.n || p.attn_rows == r.n_final);
        CHECK(p.mla_rows == r.n || p.mla_rows == r.n_final);
        CHECK(!p.need_scores || p.score_bytes >= (size_t)p.attn_rows * nh_max * p.sc_ld * 4);
        CHECK(p.sc_ld % 32 == 0 && (!xm || (p.sc_ld % 64 == 0 && p.need_scores)));
        CHECK(p.sc_ld >= p.attn_pos + 1 && p.n_logits == (r.verify ? r.n : r.n_final));
        if (r.verify || !r.counts) CHECK(no_run_option(p, r));
        // every table: what its builder gives alone
        std::vector<Tab> tabs;
        std::vector<int32_t> one, lt;
        for (int w = 0; w < 8; w++)
            for (const KrMpSpan* sp : {&p.pf[w], &p.xa[w], &p.xc[w]})
                if (sp->off >= 0) { kr_pf_build_tiles(r.n_final, r.counts, 1 << w, one); tabs.push_back(Tab{*sp, one}); }
        for (const KrMultiPlan::Mf& m : p.mf) { kr_mf_build_tiles(r.n_final, r.counts, m.nh, one); tabs.push_back(Tab{m.t, one}); }
        CHECK((p.lc_runs.off >= 0) == (p.lc_tiles.off >= 0) && (p.lc_runs.off >= 0) == (p.lc_nruns > 0));
        if (p.lc_runs.off >= 0) {
            const KrLcStats ls = kr_lc_build(r.n_final, r.counts, one, lt);
            tabs.push_back(Tab{p.lc_runs, one}); tabs.push_back(Tab{p.lc_tiles, lt});
            CHECK(ls.n_runs == p.lc_nruns && ls.n_tiles == p.lc_ntiles && ls.n_short == p.lc_short && p.lc_scratch_floats > 0);
        }
        CHECK((int)tabs.size() == n_tables(p));
        for (size_t a = 0; a < tabs.size(); a++) {
            const KrMpSpan sp = tabs[a].sp;
            CHECK(sp.off % 4 == 0 && sp.n >= 1 && (size_t)sp.off + 2 * (size_t)sp.n <= p.tables.size());      // inside the vector, at a multiple of four ints
            CHECK(tabs[a].want.size() == 2 * (size_t)sp.n);
            for (size_t k = 0; k < tabs[a].want.size(); k++) CHECK(p.tables[(size_t)sp.off + k] == tabs[a].want[k]);
            for (size_t b = 0; b < a; b++) {      // no two distinct tables overlap
                const KrMpSpan sq = tabs[b].sp;
                CHECK(sp.off != sq.off && (sp.off + 2 * sp.n <= sq.off || sq.off + 2 * sq.n <= sp.off));
            }
        }
        // the tables that must be there
        for (const KrMultiPlanLayer& L : layers) {
            if (L.kind == KR_MP_GQA && p.gqa_runs == KR_MP_RUNS_FLASH) CHECK(kr_mp_pf(p, L.nh, L.nkv).off >= 0);
            if (L.kind == KR_MP_GQA && p.gqa_runs == KR_MP_RUNS_XM) CHECK(kr_mp_xa(p, L.nh, L.nkv).off >= 0 && kr_mp_xc(p, L.nh, L.nkv).off >= 0);
            if (L.kind == KR_MP_MLA && p.mla_runs == KR_MP_RUNS_XM) CHECK(kr_mp_xa(p, L.nh, 1).off >= 0 && kr_mp_xc(p, L.nh, 1).off >= 0);
            if (L.kind == KR_MP_MLA) CHECK((kr_mp_mf(p, L.nh).off >= 0) == (p.mla_runs == KR_MP_RUNS_FLASH));
        }
    }
    std::puts("case K ok");
}

int main() {
    case_a_f(); case_c_d(); case_e_f(); case_g_h(); case_i(); case_j(); case_k();
    std::puts("multi plan ok");
    return 0;
}
