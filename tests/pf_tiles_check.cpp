// pf_tiles_check.cpp -- stand-alone check of kr_pf_tiles.h, the query-tile table of a batched pass under "multi_extend_flash"
// (docs/design/25-multi-extend-flash.md).  Host only, its own main: tests/test_multi_extend_flash.py compiles it with -fsanitize=address,undefined and runs it.
// The flatten it checks the row map against is written out here once more, independently: the last token of run i is pass row i, the others follow from row n on
// in call order (docs/design/17-multi-extend.md).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kr_pf_tiles.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "pf_tiles_check: line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

static void check_pass(const std::vector<int32_t>& counts, const std::vector<int32_t>& positions, int tq) {
    const int n = (int)counts.size();
    int T = 0;
    for (int c : counts) T += c;
    // the flatten: row_of[i][t]
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
    int n_unit = 0, n_long = 0, long_tokens = 0, last_run = -1, last_t0 = -1;
    for (int c : counts) { if (c >= 2) { n_long++; long_tokens += c; } else n_unit++; }
    CHECK(st.n_unit == n_unit && st.n_long == n_long && st.long_tokens == long_tokens);
    for (int k = 0; k < st.n_tiles; k++) {
        const int run = tiles[(size_t)2 * k], t0 = tiles[(size_t)2 * k + 1];
        CHECK(run >= 0 && run < n);
        const int cnt = counts[(size_t)run], pos0 = positions[(size_t)run];
        CHECK(cnt >= 2);                                          // no tile for a unit run
        CHECK(t0 >= 0 && t0 < cnt && t0 % tq == 0);
        CHECK(run > last_run || (run == last_run && t0 == last_t0 + tq));      // runs in call order, tiles ascending without gaps
        if (run > last_run) CHECK(t0 == 0);
        last_run = run; last_t0 = t0;
        const int end = t0 + tq < cnt ? t0 + tq : cnt;
        for (int t = t0; t < end; t++) {
            const int row = kr_pf_run_row(run, off[(size_t)run], cnt, t);
            CHECK(row == row_of[(size_t)run][(size_t)t]);         // the row map is the flatten
            CHECK(row >= 0 && row < T);
            covered[(size_t)row]++;
        }
        // the last position any row of the tile sees is its last token's own
        CHECK(kr_pf_tile_kv_end(pos0, cnt, t0, tq) == pos0 + end);
        CHECK(kr_pf_tile_kv_end(pos0, cnt, t0, tq) <= pos0 + cnt);
    }
    for (int i = 0; i < n; i++)
        for (int t = 0; t < counts[(size_t)i]; t++) CHECK(covered[(size_t)row_of[(size_t)i][(size_t)t]] == (counts[(size_t)i] >= 2 ? 1 : 0));
    int want = 0;
    for (int c : counts) if (c >= 2) want += (c + tq - 1) / tq;
    CHECK(st.n_tiles == want);
}

int main() {
    CHECK(kr_pf_tile_tokens(16, 2) == 16 && kr_pf_tile_tokens(8, 2) == 32 && kr_pf_tile_tokens(4, 2) == 64 && kr_pf_tile_tokens(2, 2) == 128 && kr_pf_tile_tokens(128, 1) == 1);
    const int tqs[] = {1, 2, 16, 32, 64, 128};
    for (int tq : tqs) {
        check_pass({2}, {0}, tq);
        check_pass({1}, {7}, tq);
        check_pass({1, 1, 1}, {3, 0, 9}, tq);                     // a step: no tile at all
        check_pass({63, 1, 130, 1, 1, 170}, {5, 64, 63, 129, 0, 37}, tq);      // counts that are no multiples of the tile, unit rows between the runs
        check_pass({64, 128, 16, 17, 129}, {64, 0, 1, 2, 3}, tq);
        check_pass({1024}, {100}, tq);                            // T = KR_EXTEND_MAX_TOKENS in one run
        std::vector<int32_t> c256((size_t)256, 4), p256((size_t)256, 11);      // 256 runs, T = 1024
        check_pass(c256, p256, tq);
        for (int i = 0; i < 256; i += 3) c256[(size_t)i] = 1;     // ... a third of them unit rows
        check_pass(c256, p256, tq);
        std::vector<int32_t> mix;                                 // every count 1 .. 44: T = 990
        for (int c = 1; c <= 44; c++) mix.push_back(c);
        check_pass(mix, std::vector<int32_t>(mix.size(), 0), tq);
    }
    std::vector<int32_t> out{1, 2, 3};
    const KrPfTileStats none = kr_pf_build_tiles(5, nullptr, 16, out);      // null counts: one token per run
    CHECK(out.empty() && none.n_tiles == 0 && none.n_unit == 5 && none.n_long == 0);
    std::puts("pf tiles ok");
    return 0;
}
