// lc_tiles_check.cpp -- stand-alone check of kr_lc_tiles.h, the table of chunked runs and their sub-chunks of a batched pass under "multi_extend_la_chunk"
// (docs/design/26-multi-extend-la-chunk.md).  Host only, its own main: tests/test_multi_extend_la_chunk.py compiles it with -fsanitize=address,undefined and runs
// it.  The flatten the covered rows are counted in is written out here independently: the last token of run i is pass row i, the others follow from row n on
// in call order (docs/design/17-multi-extend.md).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kr_lc_tiles.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "lc_tiles_check: line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

static void check_pass(const std::vector<int32_t>& counts, int nv) {
    const int n = (int)counts.size();
    int T = 0;
    for (int c : counts) T += c;
    std::vector<std::vector<int>> row_of((size_t)n);
    int next = n;
    for (int i = 0; i < n; i++)
        for (int t = 0; t < counts[(size_t)i]; t++) row_of[(size_t)i].push_back(t == counts[(size_t)i] - 1 ? i : next++);
    CHECK(next == T);
    std::vector<int32_t> runs{9, 9, 9}, tiles{7};                  // the builder clears what it is given
    const KrLcStats st = kr_lc_build(n, counts.data(), runs, tiles);
    CHECK((int)runs.size() == 2 * st.n_runs && (int)tiles.size() == 2 * st.n_tiles);
    int want_runs = 0, want_tiles = 0, want_short = 0, want_tokens = 0;
    for (int c : counts) { if (c >= KR_LC_TOKENS) { want_runs++; want_tiles += (c + 63) / 64; want_tokens += c; } else want_short++; }
    CHECK(st.n_runs == want_runs && st.n_tiles == want_tiles && st.n_short == want_short && st.tokens == want_tokens);
    CHECK(st.n_runs + st.n_short == n);
    // the run table: chunked runs in call order, each with the scratch tile of its sub-chunk 0 = the number of sub-chunks ahead of it
    int prefix = 0, last = -1;
    std::vector<int> first_of((size_t)n, -1);
    for (int r = 0; r < st.n_runs; r++) {
        const int run = runs[(size_t)2 * r], first = runs[(size_t)2 * r + 1];
        CHECK(run > last && run < n); last = run;
        CHECK(counts[(size_t)run] >= KR_LC_TOKENS);
        CHECK(first == prefix);
        first_of[(size_t)run] = first;
        prefix += kr_lc_subs(counts[(size_t)run]);
    }
    CHECK(prefix == st.n_tiles);
    // the tile table: tile x is scratch tile x = first + sub of its run; every token of a chunked run in exactly one tile, no token of a shorter run
    std::vector<int> covered((size_t)T, 0);
    int padded = 0;
    for (int x = 0; x < st.n_tiles; x++) {
        const int run = tiles[(size_t)2 * x], sub = tiles[(size_t)2 * x + 1];
        CHECK(run >= 0 && run < n && first_of[(size_t)run] >= 0);
        const int cnt = counts[(size_t)run];
        CHECK(sub >= 0 && sub < kr_lc_subs(cnt));
        CHECK(x == first_of[(size_t)run] + sub);
        const int nt = kr_lc_sub_tokens(cnt, sub);
        CHECK(nt >= 1 && nt <= KR_LC_TOKENS && (nt == KR_LC_TOKENS || sub == kr_lc_subs(cnt) - 1));      // only the last sub-chunk is partial
        CHECK(sub * KR_LC_TOKENS + nt <= cnt);
        if (sub == kr_lc_subs(cnt) - 1) CHECK(sub * KR_LC_TOKENS + nt == cnt);
        for (int t = sub * KR_LC_TOKENS; t < sub * KR_LC_TOKENS + nt; t++) covered[(size_t)row_of[(size_t)run][(size_t)t]]++;
        padded += KR_LC_TOKENS;
    }
    for (int i = 0; i < n; i++)
        for (int t = 0; t < counts[(size_t)i]; t++) CHECK(covered[(size_t)row_of[(size_t)i][(size_t)t]] == (counts[(size_t)i] >= KR_LC_TOKENS ? 1 : 0));
    // scratch: per padded token and head 128 Y floats, three pairs of bf16 planes of 128 (= 3 x 128 floats) and one G, plus alignment
    CHECK(kr_lc_scratch_floats(st.n_tiles, nv) == (size_t)padded * nv * (4 * 128 + 1) + 4);
    // ... and its carve stays inside: Y, G rounded up to 16 bytes, six planes of 2-byte values
    const size_t tl = (size_t)padded * nv, g_end = tl * 128 + (tl + 3) / 4 * 4, planes_floats = 6 * tl * 128 / 2;
    CHECK(g_end + planes_floats <= kr_lc_scratch_floats(st.n_tiles, nv));
}

int main() {
    CHECK(kr_lc_subs(64) == 1 && kr_lc_subs(65) == 2 && kr_lc_subs(128) == 2 && kr_lc_subs(1024) == 16);
    CHECK(kr_lc_sub_tokens(65, 0) == 64 && kr_lc_sub_tokens(65, 1) == 1 && kr_lc_sub_tokens(200, 3) == 8 && kr_lc_sub_tokens(128, 1) == 64);
    const int nvs[] = {1, 4, 8, 16, 32};
    for (int nv : nvs) {
        check_pass({64}, nv);
        check_pass({63}, nv);                                      // no chunked run: empty tables
        check_pass({1, 1, 1}, nv);
        check_pass({64, 1, 65, 130, 1, 63, 170, 200}, nv);        // partial last sub-chunks, unit rows and a 63-token run between the chunked ones
        check_pass({127, 128, 129, 2, 64}, nv);
        check_pass({1024}, nv);                                    // one run of KR_EXTEND_MAX_TOKENS tokens: 16 sub-chunks
        check_pass({1023}, nv);
        std::vector<int32_t> c256((size_t)256, 4);                 // 256 runs, T = 1024: none chunked
        check_pass(c256, nv);
        std::vector<int32_t> m256((size_t)256, 1);                 // 256 runs, T = 1020: twelve of 64 among unit rows
        for (int i = 0; i < 12; i++) m256[(size_t)(i * 21 + 3)] = 64;
        check_pass(m256, nv);
        m256[3] = 100;                                             // ... T = 1056 is past a pass, but the builder has no limit of its own
        check_pass(m256, nv);
    }
    std::vector<int32_t> runs{1}, tiles{2};
    const KrLcStats none = kr_lc_build(5, nullptr, runs, tiles);    // null counts: one token per run
    CHECK(runs.empty() && tiles.empty() && none.n_runs == 0 && none.n_tiles == 0 && none.n_short == 5 && none.tokens == 0);
    std::puts("lc tiles ok");
    return 0;
}
