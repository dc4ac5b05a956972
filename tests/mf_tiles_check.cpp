// mf_tiles_check.cpp -- stand-alone check of kr_mf_tiles.h, the query-row tile table of a batched pass under "multi_extend_mla_flash"
// (docs/design/27-multi-extend-mla-flash.md).  Host only, its own main: tests/test_multi_extend_mla_flash.py compiles it with -fsanitize=address,undefined and
// runs it.  The flatten it checks the row map against is written out here once more, independently: the last token of run i is pass row i, the others follow from
// row n on in call order (docs/design/17-multi-extend.md).  A (token, head) row of a run is row token * nh + head of its cnt * nh rows.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kr_mf_tiles.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "mf_tiles_check: line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

static void check_pass(const std::vector<int32_t>& counts, int nh) {
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
    const KrMfTileStats st = kr_mf_build_tiles(n, counts.data(), nh, tiles);
    CHECK((int)tiles.size() == 2 * st.n_tiles);
    std::vector<int> covered((size_t)T * (size_t)nh, 0);          // per (pass row, head): the number of tiles that hold it
    int n_unit = 0, n_long = 0, long_tokens = 0, last_run = -1, last_r = -1;
    for (int c : counts) { if (c >= 2) { n_long++; long_tokens += c; } else n_unit++; }
    CHECK(st.n_unit == n_unit && st.n_long == n_long && st.long_tokens == long_tokens);
    for (int k = 0; k < st.n_tiles; k++) {
        const int run = tiles[(size_t)2 * k], r = tiles[(size_t)2 * k + 1];
        CHECK(run >= 0 && run < n);
        const int cnt = counts[(size_t)run], nrows = cnt * nh;
        CHECK(cnt >= 2);                                          // no tile for a unit run
        CHECK(r >= 0 && r * KR_MF_TILE_ROWS < nrows);             // every tile holds a row: no workgroup without work
        CHECK(run > last_run || (run == last_run && r == last_r + 1));      // runs in call order, tiles ascending without gaps
        if (run > last_run) CHECK(r == 0);
        last_run = run; last_r = r;
        const int g0 = r * KR_MF_TILE_ROWS, g1 = g0 + KR_MF_TILE_ROWS < nrows ? g0 + KR_MF_TILE_ROWS : nrows;
        for (int g = g0; g < g1; g++) {
            const int t = g / nh, h = g % nh;
            CHECK(t < cnt);                                       // the row map is asked for tokens of the run only
            const int row = kr_mf_run_row(run, off[(size_t)run], cnt, t);
            CHECK(row == row_of[(size_t)run][(size_t)t]);         // the row map is the flatten
            CHECK(row >= 0 && row < T);
            covered[(size_t)row * (size_t)nh + (size_t)h]++;
        }
        // the tokens of the tile: what the kernel derives from (tile_row, nh); its last token's own position is the last one any row of it sees
        CHECK(kr_mf_tile_first(r, nh) == g0 / nh && kr_mf_tile_last(cnt, r, nh) == (g1 - 1) / nh);
        CHECK(kr_mf_tile_last(cnt, r, nh) < cnt);
    }
    for (int i = 0; i < n; i++)
        for (int t = 0; t < counts[(size_t)i]; t++)
            for (int h = 0; h < nh; h++) CHECK(covered[(size_t)row_of[(size_t)i][(size_t)t] * (size_t)nh + (size_t)h] == (counts[(size_t)i] >= 2 ? 1 : 0));
    int want = 0;
    for (int c : counts) if (c >= 2) want += (c * nh + KR_MF_TILE_ROWS - 1) / KR_MF_TILE_ROWS;
    CHECK(st.n_tiles == want);
}

int main() {
    CHECK(kr_mf_run_tiles(2, 5) == 1 && kr_mf_run_tiles(13, 5) == 2 && kr_mf_run_tiles(1024, 128) == 2048 && kr_mf_run_tiles(4, 16) == 1 && kr_mf_run_tiles(5, 16) == 2);
    const int heads[] = {1, 3, 5, 16, 64, 128};                   // 3, 5: a tile cuts through a token; 64: one token per tile; 128: two tiles per token
    for (int nh : heads) {
        check_pass({2}, nh);
        check_pass({1}, nh);
        check_pass({1, 1, 1}, nh);                                // a step: no tile at all
        check_pass({27, 1, 66, 1, 1, 170}, nh);                   // counts that are no multiples of the tile, unit rows between the runs
        check_pass({2, 27, 32, 66, 170, 131}, nh);
        check_pass({64, 128, 16, 17, 129}, nh);
        check_pass({1024}, nh);                                   // T = KR_EXTEND_MAX_TOKENS in one run
        std::vector<int32_t> c256((size_t)256, 4);                // 256 runs, T = 1024
        check_pass(c256, nh);
        for (int i = 0; i < 256; i += 3) c256[(size_t)i] = 1;     // ... a third of them unit rows
        check_pass(c256, nh);
        std::vector<int32_t> mix;                                 // every count 1 .. 44: T = 990
        for (int c = 1; c <= 44; c++) mix.push_back(c);
        check_pass(mix, nh);
    }
    std::vector<int32_t> out{1, 2, 3};
    const KrMfTileStats none = kr_mf_build_tiles(5, nullptr, 16, out);      // null counts: one token per run
    CHECK(out.empty() && none.n_tiles == 0 && none.n_unit == 5 && none.n_long == 0);
    std::puts("mf tiles ok");
    return 0;
}
