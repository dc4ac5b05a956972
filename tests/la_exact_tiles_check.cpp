// la_exact_tiles_check.cpp -- stand-alone check of the tables of a batched pass under "multi_extend_la_exact" (docs/design/36-multi-extend-la-exact.md): the
// builder kr_lx_build (kr_lc_tiles.h) and what the plan (kr_multi_plan.h) makes of it.  Host only, its own main: tests/test_multi_extend_la_exact.py compiles it
// with -fsanitize=address,undefined and runs it.  The flatten the covered rows are counted in is written out here independently: the last token of run i is
// pass row i, the others follow from row n on in call order (docs/design/17-multi-extend.md).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kr_multi_plan.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "la_exact_tiles_check: line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

// the builder alone: every token of every run of >= min in exactly one tile of each width and no token of a shorter run, tiles in call order, t0 ascending
static KrLxStats check_build(const std::vector<int32_t>& counts, int min_given) {
    const int n = (int)counts.size(), min = min_given < 2 ? 2 : min_given;      // a unit row is never staged

    int T = 0;
    for (int c : counts) T += c;
    std::vector<std::vector<int>> row_of((size_t)n);
    int next = n;
    for (int i = 0; i < n; i++)
        for (int t = 0; t < counts[(size_t)i]; t++) row_of[(size_t)i].push_back(t == counts[(size_t)i] - 1 ? i : next++);
    CHECK(next == T);
    std::vector<int32_t> runs{9, 9, 9}, t16{7}, t8{5, 5};          // the builder clears what it is given
    const KrLxStats st = kr_lx_build(n, counts.data(), min_given, runs, t16, t8);
    CHECK((int)runs.size() == 2 * st.n_runs && (int)t16.size() == 2 * st.n16 && (int)t8.size() == 2 * st.n8);
    int want_runs = 0, want_short = 0, want16 = 0, want8 = 0, want_tokens = 0;
    for (int c : counts) { if (c >= min) { want_runs++; want16 += (c + 15) / 16; want8 += (c + 7) / 8; want_tokens += c; } else want_short++; }
    CHECK(st.n_runs == want_runs && st.n_short == want_short && st.n16 == want16 && st.n8 == want8 && st.tokens == want_tokens);
    CHECK(st.n_runs + st.n_short == n);
    // the run table: staged runs in call order, each with its first 16-token tile = the number of such tiles ahead of it
    int prefix = 0, last = -1;
    std::vector<int> staged((size_t)n, 0);
    for (int r = 0; r < st.n_runs; r++) {
        const int run = runs[(size_t)2 * r], first = runs[(size_t)2 * r + 1];
        CHECK(run > last && run < n); last = run;
        CHECK(counts[(size_t)run] >= min && counts[(size_t)run] >= 2);
        CHECK(first == prefix && t16[(size_t)2 * first] == run && t16[(size_t)2 * first + 1] == 0);
        staged[(size_t)run] = 1;
        prefix += (counts[(size_t)run] + 15) / 16;
    }
    CHECK(prefix == st.n16);
    const std::vector<int32_t>* tabs[2] = {&t16, &t8};
    const int widths[2] = {KR_LX_CONV_TOKENS, KR_LX_NORM_TOKENS}, ns[2] = {st.n16, st.n8};
    for (int k = 0; k < 2; k++) {
        std::vector<int> covered((size_t)T, 0);
        int prun = -1, pt0 = 0;
        for (int x = 0; x < ns[k]; x++) {
            const int run = (*tabs[k])[(size_t)2 * x], t0 = (*tabs[k])[(size_t)2 * x + 1];
            CHECK(run >= 0 && run < n && staged[(size_t)run]);
            const int cnt = counts[(size_t)run];
            CHECK(t0 >= 0 && t0 < cnt && t0 % widths[k] == 0);
            if (run == prun) CHECK(t0 == pt0 + widths[k]); else { CHECK(run > prun && t0 == 0); }      // call order, tiles of a run ascending and gapless
            prun = run; pt0 = t0;
            for (int t = t0; t < t0 + widths[k] && t < cnt; t++) covered[(size_t)row_of[(size_t)run][(size_t)t]]++;
        }
        for (int i = 0; i < n; i++)
            for (int t = 0; t < counts[(size_t)i]; t++) CHECK(covered[(size_t)row_of[(size_t)i][(size_t)t]] == staged[(size_t)i]);
    }
    return st;
}

// the plan: a store of two linear-attention layers and a GQA layer between them
static KrMultiPlan plan_of(const std::vector<int32_t>& counts, bool on, int min, bool verify, bool with_counts = true, bool la_chunk = false, bool la_layers = true) {
    const int n_final = (int)counts.size();
    int n = 0;
    std::vector<int32_t> pos;
    for (int c : counts) { n += c; pos.push_back(10 + c - 1); }
    KrMultiPlanOpts o{};
    o.opt.extend_la_exact = on; o.opt.extend_la_exact_min = min; o.opt.extend_la_chunk = la_chunk; o.max_seq = 2048; o.gqa_split_min = 1 << 20; o.mla_split_min = 1 << 20;
    o.opt.attn_exact_split_min = 512; o.opt.mla_exact_split_min = 512; o.fd_chunk = 128; o.mla_chunk = 64;
    const KrMultiPlanLayer layers[3] = {{la_layers ? KR_MP_LA : KR_MP_OTHER, 0, 0, 0, 0, 4}, {KR_MP_GQA, 4, 2, 64, 0, 0}, {la_layers ? KR_MP_LA : KR_MP_OTHER, 0, 0, 0, 0, 8}};
    KrMultiPlan p;
    const KrMultiPlanRows rows{n, n_final, 10 + 1024, verify, with_counts ? counts.data() : nullptr, with_counts ? pos.data() : nullptr};
    CHECK(kr_multi_plan(o, layers, 3, rows, p) == KR_MP_OK);
    return p;
}
static void no_table(const KrMultiPlan& p) { CHECK(p.lx_nruns == 0 && p.lx_short == 0 && p.lx_runs.off < 0 && p.lx_t16.off < 0 && p.lx_t8.off < 0 && p.lx_runs.n == 0 && p.lx_t16.n == 0 && p.lx_t8.n == 0); }

int main() {
    // a plain step has no table
    no_table(plan_of({1, 1, 1}, true, 2, false, false));
    no_table(plan_of({1, 1, 1}, true, 2, false));
    CHECK(plan_of({1, 1, 1}, true, 2, false).tables.empty());
    // a verify pass has no table
    no_table(plan_of({4, 17, 1}, true, 2, true));
    // the option off, or a store without linear-attention layers: none either, and the tables of the pass are what they were
    no_table(plan_of({4, 17, 1}, false, 2, false));
    CHECK(plan_of({4, 17, 1}, false, 2, false).tables.empty());
    no_table(plan_of({4, 17, 1}, true, 2, false, true, false, false));
    // runs at min - 1, min, 16, 17 and 1024
    const int mins[] = {2, 8, 16, 64, 1024};
    for (int min : mins) {
        if (min > 2) { const KrLxStats a = check_build({min - 1}, min); CHECK(a.n_runs == 0 && a.n_short == 1 && a.n16 == 0 && a.n8 == 0); no_table(plan_of({min - 1}, true, min, false)); }
        const KrLxStats b = check_build({min}, min);
        CHECK(b.n_runs == 1 && b.n_short == 0 && b.n16 == (min + 15) / 16 && b.n8 == (min + 7) / 8);
        const KrMultiPlan p = plan_of({min}, true, min, false);
        CHECK(p.lx_nruns == 1 && p.lx_short == 0 && p.lx_runs.n == 1 && p.lx_t16.n == b.n16 && p.lx_t8.n == b.n8);
    }
    { const KrLxStats s = check_build({16}, 2); CHECK(s.n16 == 1 && s.n8 == 2); }
    { const KrLxStats s = check_build({17}, 2); CHECK(s.n16 == 2 && s.n8 == 3); }
    { const KrLxStats s = check_build({1024}, 2); CHECK(s.n16 == 64 && s.n8 == 128 && s.tokens == 1024); }
    { const KrLxStats s = check_build({1}, 0); CHECK(s.n_runs == 0 && s.n_short == 1); }      // a unit row is never staged, whatever the threshold
    { const KrLxStats s = check_build({1, 2}, 1); CHECK(s.n_runs == 1 && s.n_short == 1); }
    // several staged runs among unit rows and shorter runs: counts, order, the runs left to the run kernels
    {
        const std::vector<int32_t> c{1, 2, 33, 1, 3, 16, 17, 170, 5, 1};
        const KrLxStats s = check_build(c, 4);
        CHECK(s.n_runs == 5 && s.n_short == 5 && s.n16 == 3 + 1 + 2 + 11 + 1 && s.n8 == 5 + 2 + 3 + 22 + 1 && s.tokens == 33 + 16 + 17 + 170 + 5);
        const KrMultiPlan p = plan_of(c, true, 4, false);
        CHECK(p.lx_nruns == 5 && p.lx_short == 5 && p.lx_runs.n == 5 && p.lx_t16.n == s.n16 && p.lx_t8.n == s.n8);
        // the three spans lie in the one vector, each at a multiple of four ints, in this order, without overlap
        CHECK(p.lx_runs.off >= 0 && p.lx_runs.off % 4 == 0 && p.lx_t16.off % 4 == 0 && p.lx_t8.off % 4 == 0);
        CHECK(p.lx_runs.off + 2 * p.lx_runs.n <= p.lx_t16.off && p.lx_t16.off + 2 * p.lx_t16.n <= p.lx_t8.off && (size_t)(p.lx_t8.off + 2 * p.lx_t8.n) <= p.tables.size());
        const int32_t* r = p.tables.data() + p.lx_runs.off; const int32_t* a = p.tables.data() + p.lx_t16.off; const int32_t* b = p.tables.data() + p.lx_t8.off;
        const int want_runs[5] = {2, 5, 6, 7, 8}, want_first[5] = {0, 3, 4, 6, 17};
        for (int i = 0; i < 5; i++) CHECK(r[2 * i] == want_runs[i] && r[2 * i + 1] == want_first[i]);
        CHECK(a[0] == 2 && a[1] == 0 && a[2] == 2 && a[3] == 16 && a[4] == 2 && a[5] == 32 && a[6] == 5 && a[7] == 0 && a[8] == 6 && a[9] == 0 && a[10] == 6 && a[11] == 16);
        CHECK(b[0] == 2 && b[1] == 0 && b[2] == 2 && b[3] == 8 && b[8] == 2 && b[9] == 32 && b[10] == 5 && b[11] == 0);
        // every run staged: nothing left to the run kernels
        const KrMultiPlan q = plan_of({4, 9, 100}, true, 4, false);
        CHECK(q.lx_nruns == 3 && q.lx_short == 0);
        // beside the chunked rule's tables (the pass refuses both options; the plan keeps them apart)
        const KrMultiPlan both = plan_of({70, 9}, true, 4, false, true, true);
        CHECK(both.lc_nruns == 1 && both.lx_nruns == 2 && both.lc_runs.off >= 0 && both.lx_runs.off > both.lc_tiles.off);
    }
    // 256 runs of 4 tokens: every one staged at min 2, none at min 5
    {
        const std::vector<int32_t> c256((size_t)256, 4);
        const KrLxStats s = check_build(c256, 2); CHECK(s.n_runs == 256 && s.n16 == 256 && s.n8 == 256);
        const KrLxStats t = check_build(c256, 5); CHECK(t.n_runs == 0 && t.n_short == 256);
    }
    std::vector<int32_t> runs{1}, t16{2}, t8{3};
    const KrLxStats none = kr_lx_build(5, nullptr, 2, runs, t16, t8);      // null counts: one token per run
    CHECK(runs.empty() && t16.empty() && t8.empty() && none.n_runs == 0 && none.n_short == 5 && none.tokens == 0);
    std::puts("la exact tiles ok");
    return 0;
}
