// Stand-alone check of the page allocator of paged sequence slots (krasis_amd/csrc/kr_page_pool.h, docs/design/21-paged-slots.md): host only, built with
// -fsanitize=address,undefined and run as a child process by tests/test_multi_paged.py.  Exit status 0 = every check held.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kr_page_pool.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static std::vector<int> pages_of_slot(const KrPagePool& p, int slot) { return std::vector<int>(p.row(slot), p.row(slot) + p.stride); }

int main() {
    KrPagePool p;
    // geometry: a power of two, at least the minimum; at least one page
    for (int bad : {0, 16, 24, 48, -32}) CHECK(p.init(4, 160, bad, 8, 32) == 1);
    CHECK(p.init(4, 160, 32, 0, 32) == 2 && p.init(0, 160, 32, 8, 32) == 3 && p.init(4, 0, 32, 8, 32) == 3);
    CHECK(p.init(4, 160, 32, 8, 32) == 0);
    CHECK(p.paged() && p.shift == 5 && p.stride == 5 && p.n_free == 8 && (int)p.table.size() == 20);
    CHECK(p.pages_of(0) == 0 && p.pages_of(1) == 1 && p.pages_of(32) == 1 && p.pages_of(33) == 2 && p.pages_of(160) == 5);
    for (int s = 0; s < 4; s++) CHECK(p.mapped(s) == 0);

    // lowest id first, in row order; entries already mapped are kept
    std::vector<KrPageChange> log;
    int need = -1, have = -1;
    { const int32_t sl[3] = {2, 0, 3}; const long long len[3] = {33, 1, 0};
      CHECK(p.reserve(3, sl, len, &log, &need, &have) == -1); }
    CHECK((pages_of_slot(p, 2) == std::vector<int>{0, 1, -1, -1, -1}) && (pages_of_slot(p, 0) == std::vector<int>{2, -1, -1, -1, -1}) && p.mapped(3) == 0);
    CHECK(log.size() == 3 && log[0].slot == 2 && log[0].idx == 0 && log[0].page == 0 && log[2].slot == 0 && log[2].page == 2 && p.n_free == 5);
    { const int32_t sl[2] = {0, 2}; const long long len[2] = {64, 64};      // interleaved growth: slot 0 gets 3, slot 2 needs nothing more
      CHECK(p.reserve(2, sl, len, &log, nullptr, nullptr) == -1); }
    CHECK((pages_of_slot(p, 0) == std::vector<int>{2, 3, -1, -1, -1}) && p.n_free == 4 && log.size() == 4);

    // all or nothing: rows 0 and 1 fit (1 + 3 = 4 pages), row 2 brings the call to 5 > 4 free -> row 2 is named and nothing is mapped
    const std::vector<int32_t> before = p.table;
    { const int32_t sl[3] = {2, 1, 3}; const long long len[3] = {96, 96, 1};
      CHECK(p.reserve(3, sl, len, &log, &need, &have) == 2 && need == 5 && have == 4); }
    CHECK(p.table == before && p.n_free == 4 && log.size() == 4);
    { const int32_t sl[1] = {1}; const long long len[1] = {160};      // exhaustion by one row alone
      CHECK(p.reserve(1, sl, len, nullptr, &need, &have) == 0 && need == 5 && have == 4 && p.table == before); }
    { const int32_t sl[2] = {2, 1}; const long long len[2] = {96, 96};      // exactly the pool
      CHECK(p.reserve(2, sl, len, nullptr, nullptr, nullptr) == -1 && p.n_free == 0); }
    CHECK((pages_of_slot(p, 2) == std::vector<int>{0, 1, 4, -1, -1}) && (pages_of_slot(p, 1) == std::vector<int>{5, 6, 7, -1, -1}));
    { const int32_t sl[1] = {3}; const long long len[1] = {1};
      CHECK(p.reserve(1, sl, len, nullptr, &need, &have) == 0 && need == 1 && have == 0); }

    // trim: pages wholly at or past the length go back; a freed low id is the next one handed out, so a slot's ids can be out of order
    std::vector<KrPageChange> freed;
    p.trim(2, 33, &freed);
    CHECK(freed.size() == 1 && freed[0].page == 4 && freed[0].idx == 2 && p.n_free == 1);
    p.trim(2, 32, &freed);
    CHECK(freed.size() == 2 && freed[1].page == 1 && p.mapped(2) == 1 && p.n_free == 2);
    p.trim(2, 32, &freed);      // nothing left to free
    CHECK(freed.size() == 2);
    { const int32_t sl[1] = {1}; const long long len[1] = {160};
      CHECK(p.reserve(1, sl, len, nullptr, nullptr, nullptr) == -1); }
    CHECK((pages_of_slot(p, 1) == std::vector<int>{5, 6, 7, 1, 4}) && p.n_free == 0);
    p.trim(1, 0, &freed);      // length 0 frees all of them
    CHECK(p.mapped(1) == 0 && p.n_free == 5);

    // release of call-mapped pages only: slot 3 holds page idx 2 from before the call; the call maps idx 0, 1, 3, 4 and ends at length 40
    { const int32_t sl[1] = {3}; const long long len[1] = {96};
      CHECK(p.reserve(1, sl, len, nullptr, nullptr, nullptr) == -1); }
    p.trim(3, 0, nullptr);
    CHECK(p.n_free == 5);
    { const int32_t sl[1] = {3}; const long long len[1] = {96};
      CHECK(p.reserve(1, sl, len, nullptr, nullptr, nullptr) == -1); }
    p.give_back(3, 0, nullptr); p.give_back(3, 1, nullptr);      // slot 3: only idx 2 mapped, before the call
    const int kept = p.row(3)[2];
    std::vector<KrPageChange> mine;
    { const int32_t sl[1] = {3}; const long long len[1] = {160};
      CHECK(p.reserve(1, sl, len, &mine, nullptr, nullptr) == -1 && mine.size() == 4 && p.mapped(3) == 5); }
    freed.clear();
    p.release_logged(mine, 3, 40, &freed);      // pages_of(40) = 2: idx 3 and 4 are the call's and wholly past; idx 2 is past too but was mapped before
    CHECK(freed.size() == 2 && p.mapped(3) == 3 && p.row(3)[2] == kept && p.row(3)[0] >= 0 && p.row(3)[1] >= 0 && p.row(3)[3] == -1 && p.row(3)[4] == -1);
    p.release_logged(mine, 3, 40, &freed);      // twice is harmless
    CHECK(freed.size() == 2);
    p.release_logged(mine, 0, 0, &freed);       // another slot's log entries are not this slot's
    CHECK(freed.size() == 2 && p.mapped(0) == 2);

    // the free count always equals the unused pages
    int used = 0;
    for (char u : p.used) used += u;
    int mapped = 0;
    for (int s = 0; s < 4; s++) mapped += p.mapped(s);
    CHECK(used == mapped && p.n_free == p.n_pages - used);

    // a large geometry: max_seq not a multiple of the page
    KrPagePool q;
    CHECK(q.init(3, 32768 + 5, 256, 100, 32) == 0 && q.stride == 129 && q.shift == 8);
    std::puts("page pool ok");
    return 0;
}
