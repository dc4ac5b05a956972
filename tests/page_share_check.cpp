// Stand-alone check of shared pages in the page allocator (krasis_amd/csrc/kr_page_pool.h, docs/design/22-slot-fork.md): reference counts, copy-on-write in
// the all-or-nothing reservation, holds of queued copies.  Host only, built with -fsanitize=address,undefined and run as a child process by
// tests/test_multi_fork.py.  Exit status 0 = every check held.
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "kr_page_pool.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static std::vector<int> ids(const KrPagePool& p, int slot) { return std::vector<int>(p.row(slot), p.row(slot) + p.stride); }
// the invariants of every state: used = referenced or held, n_free = the unused pages, refs = the table entries naming the page, n_shared = pages with refs > 1
static bool consistent(const KrPagePool& p) {
    std::vector<int> cnt((size_t)p.n_pages, 0);
    for (int32_t t : p.table) if (t >= 0) cnt[(size_t)t]++;
    int used = 0, shared = 0;
    for (int i = 0; i < p.n_pages; i++) {
        if (cnt[(size_t)i] != p.refs[(size_t)i] || p.holds[(size_t)i] < 0 || p.tmp[(size_t)i] != 0) return false;
        if ((p.used[(size_t)i] != 0) != (p.refs[(size_t)i] > 0 || p.holds[(size_t)i] > 0)) return false;
        used += p.used[(size_t)i]; shared += p.refs[(size_t)i] > 1;
    }
    return p.n_free == p.n_pages - used && shared == p.n_shared;
}
static int reserve1(KrPagePool& p, int slot, long long from, long long len, std::vector<KrPageChange>* log, int* need = nullptr, int* have = nullptr) {
    const int32_t sl[1] = {slot}; const long long ln[1] = {len}, fr[1] = {from};
    return p.reserve(1, sl, ln, log, need, have, fr);
}

int main() {
    KrPagePool p;
    CHECK(p.init(4, 160, 32, 6, 32) == 0 && consistent(p));
    std::vector<KrPageChange> log, freed;
    // slot 2 holds 70 positions: pages 0, 1, 2
    CHECK(reserve1(p, 2, 0, 70, &log) == -1 && (ids(p, 2) == std::vector<int>{0, 1, 2, -1, -1}) && log.size() == 3 && log[0].src == -1 && p.n_free == 3);

    // share and references: slots 0 and 3 take the two whole pages; the free count does not move
    p.share(2, 0, 2); p.share(2, 3, 2);
    CHECK((ids(p, 0) == std::vector<int>{0, 1, -1, -1, -1}) && (ids(p, 3) == std::vector<int>{0, 1, -1, -1, -1}));
    CHECK(p.refs[0] == 3 && p.refs[1] == 3 && p.refs[2] == 1 && p.n_shared == 2 && p.n_free == 3 && consistent(p));
    // an unmapped entry of the source stays unmapped
    p.share(2, 1, 4);
    CHECK((ids(p, 1) == std::vector<int>{0, 1, 2, -1, -1}) && p.refs[2] == 2 && p.n_shared == 3 && consistent(p));
    p.trim(1, 0, &freed);
    CHECK(freed.size() == 3 && p.mapped(1) == 0 && p.n_free == 3 && p.refs[2] == 1 && p.n_shared == 2 && consistent(p));      // three entries released, no page freed

    // a reservation that writes nothing (from null) and one that writes only past the shared pages leave them shared: appending is the common case
    { const int32_t sl[1] = {0}; const long long ln[1] = {70};
      CHECK(p.reserve(1, sl, ln, &log, nullptr, nullptr) == -1); }
    CHECK((ids(p, 0) == std::vector<int>{0, 1, 3, -1, -1}) && p.refs[0] == 3 && p.n_free == 2);      // lowest free id first, as before
    CHECK(reserve1(p, 3, 64, 71, &log) == -1 && (ids(p, 3) == std::vector<int>{0, 1, 4, -1, -1}) && p.refs[1] == 3 && p.n_free == 1 && consistent(p));

    // copy-on-write: slot 3 writes [40, 50) -> entry 1 becomes a private page, logged with its source and a whole page of rows; the source is held
    log.clear();
    CHECK(reserve1(p, 3, 40, 50, &log) == -1);
    CHECK((ids(p, 3) == std::vector<int>{0, 5, 4, -1, -1}) && log.size() == 1 && log[0].slot == 3 && log[0].idx == 1 && log[0].page == 5 && log[0].src == 1 && log[0].rows == 32);
    CHECK(p.refs[1] == 2 && p.holds[1] == 1 && p.refs[5] == 1 && p.n_free == 0 && consistent(p));
    p.flushed();      // the copy was enqueued
    CHECK(p.holds[1] == 0 && p.used[1] && p.n_free == 0 && consistent(p));

    // copy-on-write counted in all or nothing: no page is free, slot 0 writing at 10 needs one -> refused, table and counts untouched
    const std::vector<int32_t> table = p.table, refs = p.refs;
    int need = -1, have = -1;
    log.clear();
    { const int32_t sl[2] = {2, 0}; const long long ln[2] = {71, 11}, fr[2] = {70, 10};      // row 0 appends in its own page and fits; row 1 does not
      CHECK(p.reserve(2, sl, ln, &log, &need, &have, fr) == 1 && need == 1 && have == 0); }
    CHECK(p.table == table && p.refs == refs && log.empty() && p.n_free == 0 && consistent(p));
    { const int32_t sl[1] = {1}; const long long ln[1] = {1};      // and a plain missing page is refused as ever
      CHECK(p.reserve(1, sl, ln, &log, &need, &have) == 0 && need == 1 && have == 0 && p.table == table); }

    // trim of one holder: slot 3 gives back its private pages 5 and 4, and only a reference of page 0
    freed.clear();
    p.trim(3, 0, &freed);
    CHECK(freed.size() == 3 && p.n_free == 2 && p.refs[0] == 2 && p.used[0] && !p.used[4] && !p.used[5] && consistent(p));

    // two holders of one page write it in the same call: the first takes the copy, the second keeps the page -- one page, not two
    log.clear();
    { const int32_t sl[2] = {0, 2}; const long long ln[2] = {41, 41}, fr[2] = {40, 40};
      CHECK(p.reserve(2, sl, ln, &log, &need, &have, fr) == -1); }
    CHECK(log.size() == 1 && log[0].slot == 0 && log[0].idx == 1 && log[0].page == 4 && log[0].src == 1 && p.row(2)[1] == 1 && p.refs[1] == 1 && p.holds[1] == 1 && p.n_free == 1);

    // a pending copy keeps its source off the free list: the last reference of page 1 goes (trim), the page stays used, and the next reservation takes
    // page 5, not page 1; once the copy is enqueued (or dropped) the page is free
    freed.clear();
    p.trim(2, 32, &freed);      // slot 2 keeps page 0 only
    CHECK(freed.size() == 2 && p.refs[1] == 0 && p.holds[1] == 1 && p.used[1] && p.n_free == 2 && consistent(p));      // page 2 came back, page 1 did not
    CHECK(reserve1(p, 1, 0, 1, &log) == -1 && p.row(1)[0] == 2 && p.n_free == 1);
    CHECK(reserve1(p, 1, 32, 33, &log) == -1 && p.row(1)[1] == 5 && p.n_free == 0);      // page 1 is passed over
    CHECK(reserve1(p, 1, 64, 65, &log, &need, &have) == 0 && need == 1 && have == 0);
    p.flushed();
    CHECK(!p.used[1] && p.n_free == 1 && consistent(p));
    CHECK(reserve1(p, 1, 64, 65, &log) == -1 && p.row(1)[2] == 1);      // lowest free id first order unchanged

    // release_logged gives a copy-on-write mapping back like any other: the entry ends unmapped, not re-attached to the shared page
    p.trim(1, 0, nullptr); p.trim(0, 32, nullptr);
    CHECK((ids(p, 0) == std::vector<int>{0, -1, -1, -1, -1}) && (ids(p, 2) == std::vector<int>{0, -1, -1, -1, -1}) && p.refs[0] == 2 && p.n_free == 5 && consistent(p));
    log.clear();
    CHECK(reserve1(p, 0, 0, 40, &log) == -1 && log.size() == 2 && log[0].src == 0 && log[1].src == -1 && p.refs[0] == 1 && p.holds[0] == 1);
    freed.clear();
    p.release_logged(log, 0, 0, &freed);
    CHECK(freed.size() == 2 && p.mapped(0) == 0 && p.refs[0] == 1 && p.row(2)[0] == 0);
    CHECK(p.holds[0] == 0 && p.pending.empty());      // the dropped mapping left the queue, and its hold went with it (release_logged prunes)
    CHECK(p.n_free == 5 && consistent(p));

    // would_free: the pages a fork may count on when its dsts are released -- a page shared among the dsts alone counts once, one shared with another slot not at all
    p.share(2, 0, 1); p.share(2, 1, 1);
    CHECK(reserve1(p, 0, 32, 40, &log) == -1 && reserve1(p, 3, 0, 1, &log) == -1 && p.n_free == 3);
    p.share(3, 1, 0);
    { const int32_t d[2] = {0, 1}; CHECK(p.would_free(2, d) == 1 && consistent(p)); }      // slot 0's own page; page 0 is slot 2's too
    { const int32_t d[3] = {0, 1, 2}; CHECK(p.would_free(3, d) == 2 && consistent(p)); }

    // the launches of queued copies: no source of a launch is a destination of the same launch
    {
        auto ok = [](const std::vector<int32_t>& dst, const std::vector<int32_t>& src, const std::vector<size_t>& ends) {
            size_t lo = 0;
            for (size_t end : ends) {
                if (end <= lo || end > dst.size()) return false;
                for (size_t i = lo; i < end; i++) for (size_t j = lo; j < end; j++) if (src[i] == dst[j]) return false;
                lo = end;
            }
            return lo == dst.size();
        };
        CHECK(kr_page_copy_launches({}, {}).empty());
        CHECK((kr_page_copy_launches({5, 6, 7}, {1, 1, 2}) == std::vector<size_t>{3}));                  // the common case: one launch
        CHECK((kr_page_copy_launches({5, 6}, {1, 5}) == std::vector<size_t>{1, 2}));                      // a private copy, then a fork's boundary copy out of it
        CHECK((kr_page_copy_launches({5, 6, 7, 8}, {1, 5, 5, 7}) == std::vector<size_t>{1, 3, 4}));
        CHECK((kr_page_copy_launches({5, 6, 7}, {1, 2, 5}) == std::vector<size_t>{2, 3}));
        for (const auto& q : {std::pair<std::vector<int32_t>, std::vector<int32_t>>{{5, 6, 7, 8}, {1, 5, 5, 7}}, {{5, 6, 7}, {1, 2, 5}}, {{4, 5, 6, 7, 8}, {0, 4, 5, 6, 7}}})
            CHECK(ok(q.first, q.second, kr_page_copy_launches(q.first, q.second)));
    }
    // the chain as the allocator produces it: slot 1 shares slot 2's page, takes a private copy (still queued), and its page is then the source of another copy
    {
        KrPagePool q;
        CHECK(q.init(3, 64, 32, 4, 32) == 0);
        const std::vector<KrPageChange>& pend = q.pending;
        CHECK(reserve1(q, 2, 0, 20, nullptr) == -1);
        q.share(2, 1, 1);
        CHECK(reserve1(q, 1, 10, 11, nullptr) == -1 && pend.size() == 2 && pend[1].src == 0 && pend[1].page == 1);
        const int32_t dsts[1] = {0};
        CHECK(q.fork(1, 1, dsts, 8).fits() && pend.size() == 3 && pend[2].page == 2 && pend[2].src == 1 && pend[2].rows == 8 && q.holds[1] == 1);      // a fork of slot 1 inside the page
        const KrPageFlush f = q.flush_plan();
        CHECK((f.copies[0] == std::vector<int32_t>{1, 2}) && (f.copies[1] == std::vector<int32_t>{0, 1}) && (f.ends == std::vector<size_t>{1, 2}));
    }

    // the last holder frees
    for (int s = 0; s < 4; s++) p.trim(s, 0, nullptr);
    CHECK(p.n_free == p.n_pages && p.n_shared == 0 && consistent(p));
    for (int i = 0; i < p.n_pages; i++) CHECK(!p.used[(size_t)i] && !p.refs[(size_t)i] && !p.holds[(size_t)i]);
    CHECK(reserve1(p, 3, 0, 33, &log) == -1 && (ids(p, 3) == std::vector<int>{0, 1, -1, -1, -1}));
    std::puts("page share ok");
    return 0;
}
