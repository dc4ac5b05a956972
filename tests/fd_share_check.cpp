// fd_share_check.cpp -- the item list of the grouped flash-decode chunk pass (krasis_amd/csrc/kr_fd_share.h) on hand-made rows and tables: a program with its
// own main, built with the host compiler alone (tests/test_multi_attn_fast_share.py builds it with -fsanitize=address,undefined too).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include "kr_fd_share.h"

#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); exit(1); } } while (0)

typedef std::vector<int32_t> V;
typedef std::vector<std::pair<int, V>> Items;      // (chunk, rows)
// the list, checked: every live (row, chunk) pair lies in exactly one item and no other pair in any; a shared chunk is full for each of its rows
static Items build(const KrFdShareRows& r, int chunk, int R) {
    V flat;
    const int n = kr_fd_share_build(r, chunk, R, flat);
    CHECK((size_t)n * KR_FDS_INTS == flat.size());
    Items out;
    std::map<std::pair<int, int>, int> seen;
    for (int i = 0; i < n; i++) {
        const int32_t* it = &flat[(size_t)i * KR_FDS_INTS];
        CHECK(it[1] >= 1 && it[1] <= R);
        out.push_back({it[0], V(it + 2, it + 2 + it[1])});
        for (int k = 0; k < KR_FDS_MAX_ROWS; k++) {
            if (k >= it[1]) { CHECK(it[2 + k] == 0); continue; }
            seen[{it[2 + k], it[0]}]++;
            CHECK(it[1] == 1 || (it[0] + 1) * chunk <= r.positions[it[2 + k]] + 1);
        }
    }
    size_t live = 0;
    for (int b = 0; b < r.n && n; b++)
        for (int c = 0; c * chunk <= r.positions[b] && !(r.in_run && r.in_run[b]); c++) { live++; CHECK((seen[{b, c}] == 1)); }
    CHECK(live == seen.size());
    return out;
}
static bool has(const Items& items, int c, V rows) { return std::find(items.begin(), items.end(), std::make_pair(c, rows)) != items.end(); }

int main() {
    // paged: pages of 32, chunks of 128 = 4 entries each; 6 slots of 12 entries.  Slots 0 .. 3 and 5 share the pages of chunk 0; slot 2 differs in the MIDDLE of
    // chunk 1 (entry 5); slot 4 is unrelated; every slot's last page is its own
    const int stride = 12, shift = 5, chunk = 128;
    V table(6 * stride, -1);
    for (int s = 0; s < 6; s++) for (int e = 0; e < 10; e++) table[s * stride + e] = s == 4 ? 100 + e : e == 8 ? 200 + s : e;
    table[2 * stride + 5] = 77;
    const V slots = {3, 0, 2, 4, 1, 5}, pos = {300, 299, 301, 300, 200, 255};      // row 4: chunk 1 not full (200 < 255); row 5: exactly full
    const KrFdShareRows r{6, slots.data(), pos.data(), nullptr, table.data(), stride, shift};
    const Items it = build(r, chunk, 4);
    CHECK(has(it, 0, {0, 1, 2, 4}) && has(it, 0, {5}) && has(it, 0, {3}));      // cut at R in batch order; the fifth row of the key opens the next item
    CHECK(has(it, 1, {0, 1, 5}) && has(it, 1, {2}) && has(it, 1, {3}) && has(it, 1, {4}));      // a differing id in the middle; a chunk not full for a row
    CHECK(has(it, 2, {0}) && has(it, 2, {1}) && has(it, 2, {2}) && has(it, 2, {3}) && it.size() == 11);      // partial chunks never share
    CHECK(has(build(r, chunk, 8), 0, {0, 1, 2, 4, 5}));
    CHECK(build(r, chunk, 1).empty() && build(r, chunk, 0).empty());      // R < 2: no list
    const V run = {0, 1, 0, 0, 0, 0};      // row 1 belongs to a run: no item names it, the others still share
    const Items ir = build(KrFdShareRows{6, slots.data(), pos.data(), run.data(), table.data(), stride, shift}, chunk, 4);
    CHECK(has(ir, 0, {0, 2, 4, 5}) && has(ir, 1, {0, 5}));
    // unrelated slots, and rows below one chunk: nothing to share, the list is empty; an unmapped entry is never a key
    const V two = {4, 0}, same = {0, 5}, at = {300, 300}, low = {100, 90};
    CHECK(build(KrFdShareRows{2, two.data(), at.data(), nullptr, table.data(), stride, shift}, chunk, 8).empty());
    CHECK(build(KrFdShareRows{2, same.data(), low.data(), nullptr, table.data(), stride, shift}, chunk, 8).empty());
    V holes = table; holes[1] = -1; holes[5 * stride + 1] = -1;
    const Items ih = build(KrFdShareRows{2, same.data(), at.data(), nullptr, holes.data(), stride, shift}, chunk, 8);
    CHECK(ih.size() == 5 && !has(ih, 0, {0, 1}) && has(ih, 1, {0, 1}));
    // flat: the key is the slot -- the token rows of one slot in a verify pass
    const V fs = {7, 7, 7, 2, 2}, fp = {284, 280, 282, 281, 127};
    const Items f = build(KrFdShareRows{5, fs.data(), fp.data(), nullptr, nullptr, 0, 0}, chunk, 8);
    CHECK(has(f, 0, {0, 1, 2}) && has(f, 0, {3, 4}) && has(f, 1, {0, 1, 2}) && has(f, 1, {3}) && f.size() == 8);
    const V big = {5, 6, 5, 9}, ps = {0, 1, 0}, pp = {300, 300, 256};      // pages of 512, two slots that share page 5: chunk 1 of both lies in entry 0
    CHECK(has(build(KrFdShareRows{3, ps.data(), pp.data(), nullptr, big.data(), 2, 9}, chunk, 8), 1, {0, 1, 2}));
    printf("fd share ok\n");
    return 0;
}
