// Stand-alone check of the slot cache view (krasis_amd/csrc/kr_slot_cache.h, docs/design/40-slot-cache-view.md): host only, built with
// -fsanitize=address,undefined and run as a child process by tests/test_multi_paged.py.  Exit status 0 = every check held.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "kr_slot_cache.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main() {
    std::mt19937 rng(20261126u);
    // the map against the formula written out longhand, at every page size the slots take: random tables (-1 = unmapped, read as page 0), random positions
    for (int shift = 5; shift <= 8; shift++) {
        const int tokens = 1 << shift, n_slots = 7, stride = 11, n_pages = 40;
        std::vector<int> table((size_t)n_slots * stride);
        for (int& t : table) t = (int)(rng() % (n_pages + 4)) - 4 < 0 ? -1 : (int)(rng() % n_pages);
        const KrSlotPages pg{table.data(), stride, shift};
        const int mask = kr_slot_mask(shift);
        CHECK(mask == tokens - 1);
        for (int k = 0; k < 4000; k++) {
            const int slot = (int)(rng() % n_slots), p = (int)(rng() % (unsigned)(stride * tokens));
            const int* trow = kr_slot_table_row(pg, (size_t)slot);
            CHECK(trow == table.data() + slot * stride);
            const int entry = table[(size_t)slot * stride + p / tokens];
            const size_t want = (size_t)(entry < 0 ? 0 : entry) * (size_t)tokens + (size_t)(p % tokens);
            CHECK(kr_slot_row<true>(p, trow, shift) == want);
            CHECK(kr_slot_row<false>(p, nullptr, 0) == (size_t)p && kr_slot_row<false>(p, trow, shift) == (size_t)p);      // flat: the position itself
            // the pieces a kernel hoists give the same row
            CHECK(kr_slot_entry(p, shift) == p / tokens && kr_slot_in_page(p, mask) == p % tokens);
            CHECK(kr_slot_page_row(kr_slot_page_id(trow[kr_slot_entry(p, shift)]), p, shift, mask) == want);
            CHECK(kr_slot_page_row(kr_slot_page_id(entry), 0, shift, mask) + (size_t)kr_slot_in_page(p, mask) == want);      // a page's first row, then the row inside it
            CHECK(kr_slot_entries(p, shift, mask) == (p + tokens - 1) / tokens);
        }
    }
    // the byte bases: a slot of a flat cache, the pool itself and a page of a paged one, for either half
    {
        char k[1], v[1];
        const KrSlotCache c{{k, v}, {4096, 1024}, {64, 16}, {nullptr, 0, 0}, 0};
        CHECK(kr_slot_base_off<false>(c, 0, 3) == 3 * 4096 && kr_slot_base_off<false>(c, 1, 3) == 3 * 1024 && kr_slot_base_off<true>(c, 1, 3) == 0);
        CHECK(kr_slot_base<false>(c, 1, 5) == v + 5 * 1024 && kr_slot_base<true>(c, 0, 5) == k && kr_slot_base<false>(c, 0, 9) == k + 9 * 4096);      // the last: unit 9, a page id on a paged cache
    }
    // the predicate on both sides of its boundary: pages of exactly n positions hold a stage of n, pages of half as many do not; flat slots always do
    {
        const int one = 0;
        CHECK(kr_slot_stage_fits(KrSlotPages{nullptr, 0, 0}, 32) && kr_slot_stage_fits(KrSlotPages{nullptr, 0, 0}, 64));
        CHECK(kr_slot_stage_fits(KrSlotPages{&one, 1, 5}, 32) && !kr_slot_stage_fits(KrSlotPages{&one, 1, 4}, 32));
        CHECK(kr_slot_stage_fits(KrSlotPages{&one, 1, 6}, 64) && !kr_slot_stage_fits(KrSlotPages{&one, 1, 5}, 64));
        CHECK(kr_slot_stage_fits(KrSlotPages{&one, 1, 8}, 32) && kr_slot_stage_fits(KrSlotPages{&one, 1, 8}, 64));
        CHECK(!kr_slot_stage_fits(KrSlotPages{&one, 0, 6}, 32) && !kr_slot_stage_fits(KrSlotPages{&one, 1, -1}, 32));      // a table without entries, a negative shift
    }
    std::printf("slot cache ok\n");
    return 0;
}
