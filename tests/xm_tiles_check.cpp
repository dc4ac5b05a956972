// xm_tiles_check.cpp -- stand-alone check of kr_xm_tiles.h, the query-tile tables of a batched pass under "multi_extend_exact_mfma"
// (docs/design/28-multi-extend-exact-mfma.md).  Host only, its own main: tests/test_multi_extend_exact_mfma.py compiles it with -fsanitize=address,undefined and
// runs it.  The tables are kr_pf_tiles.h's at this option's tile widths, tq = 64 / G tokens for the scores pass and 32 / G for the P.V pass, G = 1 .. 32: every
// width from 1 to 64 is walked here, 1 and 2 being widths no other option uses.  The flatten the row map is checked against is written out once more,
// independently: the last token of run i is pass row i, the others follow from row n on in call order (docs/design/17-multi-extend.md).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kr_xm_tiles.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "xm_tiles_check: line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

static void check_pass(const std::vector<int32_t>& counts, const std::vector<int32_t>& positions, int tq) {
    const int n = (int)counts.size();
    int T = 0;
    for (int c : counts) T += c;
    std::vector<std::vector<int>> row_of((size_t)n);
    std::vector<int> off((size_t)n);
    int next = n;
    for (int i = 0; i < n; i++) {
        off[(size_t)i] = next;
        for (int t = 0; t < counts[(size_t)i]; t++) row_of[(size_t)i].push_back(t == counts[(size_t)i] - 1 ? i : next++);
    }
    CHECK(next == T);
    std::vector<int32_t> tiles;
    const KrPfTileStats st = kr_pf_build_tiles(n, counts.data(), tq, tiles);
    CHECK((int)tiles.size() == 2 * st.n_tiles);
    std::vector<int> covered((size_t)T, 0);                       // per pass row: the number of tiles that hold it
    int last_run = -1, last_t0 = -1, want_end = 0, reach = 0;
    for (int k = 0; k < st.n_tiles; k++) {
        const int run = tiles[(size_t)2 * k], t0 = tiles[(size_t)2 * k + 1];
        CHECK(run >= 0 && run < n);
        const int cnt = counts[(size_t)run], pos0 = positions[(size_t)run];
        CHECK(cnt >= 2);                                          // no unit run appears
        CHECK(t0 >= 0 && t0 < cnt && t0 % tq == 0);
        CHECK(run > last_run || (run == last_run && t0 == last_t0 + tq));      // runs in call order, tiles ascending without gaps
        if (run > last_run) CHECK(t0 == 0);
        last_run = run; last_t0 = t0;
        const int end = t0 + tq < cnt ? t0 + tq : cnt;
        for (int t = t0; t < end; t++) {
            const int row = kr_pf_run_row(run, off[(size_t)run], cnt, t);
            CHECK(row == row_of[(size_t)run][(size_t)t] && row >= 0 && row < T);
            covered[(size_t)row]++;
        }
        // the tile's last visible position (p_max of the kernels) lies below the largest kv_end, the bound of the scores pass's grid
        const int p_max = pos0 + end - 1;
        if (p_max + 1 > reach) reach = p_max + 1;
        CHECK(p_max < kr_xm_kv_end_max(n, counts.data(), positions.data()));
    }
    for (int i = 0; i < n; i++) {
        for (int t = 0; t < counts[(size_t)i]; t++) CHECK(covered[(size_t)row_of[(size_t)i][(size_t)t]] == (counts[(size_t)i] >= 2 ? 1 : 0));      // every token of a run of >= 2 exactly once
        if (counts[(size_t)i] >= 2 && positions[(size_t)i] + counts[(size_t)i] > want_end) want_end = positions[(size_t)i] + counts[(size_t)i];
    }
    CHECK(kr_xm_kv_end_max(n, counts.data(), positions.data()) == want_end);      // the largest kv_end: unit runs do not count
    CHECK(reach == want_end);                                     // ... and some tile reaches it
    int want = 0;
    for (int c : counts) if (c >= 2) want += (c + tq - 1) / tq;
    CHECK(st.n_tiles == want);
}

int main() {
    CHECK(kr_xm_tile_tokens_a(16, 2) == 8 && kr_xm_tile_tokens_c(16, 2) == 4 && kr_xm_tile_tokens_a(2, 2) == 64 && kr_xm_tile_tokens_c(2, 2) == 32);
    CHECK(kr_xm_tile_tokens_a(64, 2) == 2 && kr_xm_tile_tokens_c(64, 2) == 1);      // G = 32: a P.V tile holds one token
    for (int tq = 1; tq <= 64; tq++) {
        check_pass({2}, {0}, tq);
        check_pass({1}, {7}, tq);
        check_pass({1, 1, 1}, {3, 0, 9}, tq);                     // a step: no tile at all, kv_end 0
        check_pass({63, 1, 130, 1, 1, 170}, {5, 900, 63, 129, 0, 37}, tq);      // a unit row further out than every run: it does not move the largest kv_end
        check_pass({64, 128, 16, 17, 129}, {64, 0, 1, 2, 3}, tq);
        check_pass({1024}, {100}, tq);                            // T = KR_EXTEND_MAX_TOKENS in one run
        std::vector<int32_t> c256((size_t)256, 4), p256((size_t)256, 11);      // 256 runs, T = 1024
        for (int i = 0; i < 256; i++) p256[(size_t)i] = (i * 37) % 101;
        check_pass(c256, p256, tq);
        for (int i = 0; i < 256; i += 3) c256[(size_t)i] = 1;     // ... a third of them unit rows
        check_pass(c256, p256, tq);
        std::vector<int32_t> mix;                                 // every count 1 .. 44: T = 990
        for (int c = 1; c <= 44; c++) mix.push_back(c);
        check_pass(mix, std::vector<int32_t>(mix.size(), 0), tq);
    }
    CHECK(kr_xm_kv_end_max(3, nullptr, nullptr) == 0);            // null counts: one token per run
    std::puts("xm tiles ok");
    return 0;
}
