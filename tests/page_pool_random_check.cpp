// Stand-alone random check of the page allocator (krasis_amd/csrc/kr_page_pool.h, docs/design/21-paged-slots.md, 22-slot-fork.md): a few thousand seeded calls
// of the members kr_decode_multi.cpp calls -- reservations that append, rewind or write nothing, fork, give_back, trim, release_logged of what a generate
// mapped, flush_plan + flushed, give-backs aimed at entries whose copy is still queued -- with a deliberately naive model beside it: a set of holders per page,
// the lowest free id found by a linear scan, a reservation tried on a copy of the whole state, a queue of its own pruned by its own scan.  After every call the
// two agree on the table, refs, holds, n_free, n_shared, the whole queue and every log; on a refusal on the row, need and have, and nothing has changed.  Every
// flush plan is checked against the model's queue.  Random queued-copy lists go through kr_page_copy_launches.  Host only, built with
// -fsanitize=address,undefined and run as a child process by tests/test_multi_fork.py.  Exit status 0 = every check held.
//   page_pool_random_check [n_calls [seed [n_slots max_seq page_tokens n_pages]]]      prints the refusals, copy-on-write copies, forks and pruned queue entries of
// the run, so a pool size can be tried without a GPU (default: the six slots of 200 positions and pages of 32 of tests/test_multi_paged_random_gpu.py, on 16 pages)
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

#include "kr_page_pool.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "line %d, call %d (%s): %s\n", __LINE__, g_call, g_op, #c); return 1; } } while (0)
static int g_call = 0;
static const char* g_op = "";

struct Rng {      // splitmix64
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
    int below(int n) { return (int)(next() % (uint64_t)n); }               // [0, n)
    int in(int lo, int hi) { return lo + below(hi - lo + 1); }            // [lo, hi]
};

struct Change { int slot, idx, page, src, rows; };
static bool same(const KrPageChange& a, const Change& b) { return a.slot == b.slot && a.idx == b.idx && a.page == b.page && a.src == b.src && a.rows == b.rows; }

// the naive model: who holds each page, nothing cached
struct Model {
    int pt = 0, n_pages = 0, n_slots = 0, stride = 0;
    std::vector<std::vector<int>> table;                      // [slot][idx], -1 = unmapped
    std::vector<std::set<std::pair<int, int>>> holders;       // [page]: the (slot, idx) entries that name it
    std::vector<int> holds;                                   // [page]: queued copies that still read it
    std::vector<Change> mpend;                                // the mappings the device has not seen, in order
    long pruned = 0;                                          // queue entries dropped by prune()
    void init(int slots, int max_seq, int tokens, int pages) {
        pt = tokens; n_pages = pages; n_slots = slots; stride = (max_seq + tokens - 1) / tokens;
        table.assign((size_t)slots, std::vector<int>((size_t)stride, -1));
        holders.assign((size_t)pages, {}); holds.assign((size_t)pages, 0);
    }
    int pages_of(long long len) const { return (int)((len + pt - 1) / pt); }
    bool is_free(int p) const { return holders[(size_t)p].empty() && holds[(size_t)p] == 0; }
    int n_free() const { int c = 0; for (int p = 0; p < n_pages; p++) c += is_free(p); return c; }
    int n_shared() const { int c = 0; for (int p = 0; p < n_pages; p++) c += holders[(size_t)p].size() > 1; return c; }
    int lowest_free() const { for (int p = 0; p < n_pages; p++) if (is_free(p)) return p; return -1; }
    void map(int slot, int idx, int p) { table[(size_t)slot][(size_t)idx] = p; if (p >= 0) holders[(size_t)p].insert({slot, idx}); }
    void unmap(int slot, int idx) { int& t = table[(size_t)slot][(size_t)idx]; if (t >= 0) holders[(size_t)t].erase({slot, idx}); t = -1; }
    // all or nothing by trying it on a copy: rows in order, entries in order; a page the pool cannot give is counted and the try goes on to the end of the row
    int reserve(int n, const int32_t* slots, const long long* lens, const long long* from, std::vector<Change>* log, int* need, int* have) {
        Model m = *this;
        std::vector<Change> mine;
        const int free0 = n_free();
        int takes = 0;
        for (int i = 0; i < n; i++) {
            for (int j = 0, e = pages_of(lens[i]); j < e; j++) {
                const int t = m.table[(size_t)slots[i]][(size_t)j];
                const bool copy = t >= 0 && from && j >= from[i] / pt && m.holders[(size_t)t].size() > 1;
                if (t >= 0 && !copy) continue;
                takes++;
                const int p = m.lowest_free();
                if (copy) { m.unmap(slots[i], j); m.holds[(size_t)t]++; }
                if (p >= 0) m.map(slots[i], j, p);
                mine.push_back(copy ? Change{slots[i], j, p, t, pt} : Change{slots[i], j, p, -1, 0});
            }
            if (takes > free0) { *need = takes; *have = free0; return i; }
        }
        *this = m;
        mpend.insert(mpend.end(), mine.begin(), mine.end());
        log->insert(log->end(), mine.begin(), mine.end());
        return -1;
    }
    // a queued mapping whose entry no longer names its page leaves the queue, and a copy's hold goes with it
    void prune() {
        for (size_t i = 0; i < mpend.size();) {
            const Change c = mpend[i];
            if (table[(size_t)c.slot][(size_t)c.idx] == c.page) { i++; continue; }
            if (c.src >= 0) holds[(size_t)c.src]--;
            mpend.erase(mpend.begin() + (ptrdiff_t)i); pruned++;
        }
    }
    void give_back(int slot, int idx, std::vector<Change>* log) {
        const int t = table[(size_t)slot][(size_t)idx];
        if (t < 0) return;
        unmap(slot, idx);
        log->push_back(Change{slot, idx, t, -1, 0});
    }
    void trim(int slot, long long len, std::vector<Change>* log) { for (int j = pages_of(len); j < stride; j++) give_back(slot, j, log); }
    // the pages that come free when these slots give everything back
    int would_free(const std::vector<int32_t>& slots) const {
        int c = 0;
        for (int p = 0; p < n_pages; p++) {
            if (holders[(size_t)p].empty() || holds[(size_t)p]) continue;
            bool all = true;
            for (const auto& h : holders[(size_t)p]) { bool in = false; for (int32_t s : slots) in |= s == h.first; all &= in; }
            c += all;
        }
        return c;
    }
};

static bool same_logs(const std::vector<KrPageChange>& a, size_t a0, const std::vector<Change>& b, size_t b0);
static bool agree(const KrPagePool& p, const Model& m) {
    if (!same_logs(p.pending, 0, m.mpend, 0)) return false;
    if (p.stride != m.stride || p.n_free != m.n_free() || p.n_shared != m.n_shared()) return false;
    for (int s = 0; s < m.n_slots; s++) for (int j = 0; j < m.stride; j++) if (p.row(s)[j] != m.table[(size_t)s][(size_t)j]) return false;
    for (int q = 0; q < m.n_pages; q++) {
        if (p.refs[(size_t)q] != (int)m.holders[(size_t)q].size() || p.holds[(size_t)q] != m.holds[(size_t)q] || p.tmp[(size_t)q] != 0) return false;
        if ((p.used[(size_t)q] != 0) == m.is_free(q)) return false;
    }
    return true;
}
static bool same_logs(const std::vector<KrPageChange>& a, size_t a0, const std::vector<Change>& b, size_t b0) {
    if (a.size() - a0 != b.size() - b0) return false;
    for (size_t i = 0; a0 + i < a.size(); i++) if (!same(a[a0 + i], b[b0 + i])) return false;
    return true;
}

// random queued-copy lists: the launches concatenated are the queue in order, and no launch reads a page it writes
static int copy_launches(Rng& r) {
    g_op = "copy launches";
    for (int round = 0; round < 400; round++) {
        const int n = r.below(12), pages = r.in(2, 14);
        std::vector<int32_t> dst, src;
        std::vector<char> taken((size_t)pages, 0);
        for (int i = 0; i < n; i++) {      // as the allocator queues them: a destination is a free page -- neither an earlier destination nor an earlier source, which is held
            int d = -1;                    // until the queue is enqueued -- and a source may be an earlier destination
            for (int k = 0; k < pages && d < 0; k++) { const int c = r.below(pages); if (!taken[(size_t)c]) d = c; }
            if (d < 0) break;
            int s = r.below(pages);
            if (s == d) s = (s + 1) % pages;
            taken[(size_t)d] = taken[(size_t)s] = 1; dst.push_back(d); src.push_back(s);
        }
        const std::vector<size_t> ends = kr_page_copy_launches(dst, src);
        CHECK(dst.empty() ? ends.empty() : (!ends.empty() && ends.back() == dst.size()));
        size_t lo = 0;
        for (size_t end : ends) {
            CHECK(end > lo && end <= dst.size());
            for (size_t i = lo; i < end; i++) for (size_t j = lo; j < end; j++) CHECK(src[i] != dst[j]);
            // and a launch is not cut short: the copy that opens the next one reads a page this one writes
            if (end < dst.size()) { bool reads = false; for (size_t j = lo; j < end; j++) reads |= dst[j] == src[end]; CHECK(reads); }
            lo = end;
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    const int n_calls = argc > 1 ? std::atoi(argv[1]) : 4000;
    Rng r{argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1};
    const int n_slots = argc > 6 ? std::atoi(argv[3]) : 6, max_seq = argc > 6 ? std::atoi(argv[4]) : 200, pt = argc > 6 ? std::atoi(argv[5]) : 32, n_pages = argc > 6 ? std::atoi(argv[6]) : 16;
    KrPagePool p;
    Model m;
    CHECK(p.init(n_slots, max_seq, pt, n_pages, 32) == 0);
    m.init(n_slots, max_seq, pt, n_pages);
    CHECK(agree(p, m));
    std::vector<KrPageChange> freed;
    std::vector<Change> mfreed;
    std::vector<int> len((size_t)n_slots, 0);   // what the caller believes each slot holds
    long refusals = 0, cow = 0, forks = 0, fork_refusals = 0, reserves = 0;
    auto distinct = [&](int n, int not_this) {
        std::vector<int32_t> out;
        while ((int)out.size() < n) { const int s = r.below(n_slots); bool dup = s == not_this; for (int32_t o : out) dup |= o == s; if (!dup) out.push_back(s); }
        return out;
    };
    // entries [j0, j1) of slot s were given back by a member of the pool; q0 / holds0 = its queue and holds before the call.  The prune inside that member, checked
    // on the pool alone: no mapping of those entries is queued any more, the queue is the old one without the mappings that are no longer in place, in order, and
    // every copy among those has let go of its source
    auto dropped = [&](int s, int j0, int j1, const std::vector<KrPageChange>& q0, std::vector<int32_t> holds0) {
        size_t k = 0;
        for (const KrPageChange& c : q0) {
            const bool in_place = p.row(c.slot)[c.idx] == c.page;
            if (c.slot == s && c.idx >= j0 && c.idx < j1 && in_place) return false;      // given back: it cannot be
            if (!in_place) { if (c.src >= 0) holds0[(size_t)c.src]--; continue; }
            if (k >= p.pending.size() || p.pending[k].slot != c.slot || p.pending[k].idx != c.idx || p.pending[k].page != c.page || p.pending[k].src != c.src) return false;
            k++;
        }
        return k == p.pending.size() && holds0 == p.holds;
    };
    for (g_call = 0; g_call < n_calls; g_call++) {
        const int op = r.below(100);
        if (op < 45) {      // a reservation over 1 .. 3 rows: appends, rewinds (writes below the slot's length), or one that writes nothing (from null)
            g_op = "reserve";
            const int n = r.in(1, 3 < n_slots ? 3 : n_slots);
            const std::vector<int32_t> sl = distinct(n, -1);
            std::vector<long long> lens((size_t)n), from((size_t)n);
            const bool writes = r.below(8) != 0, logged = r.below(10) != 0;      // logged: the caller keeps the call's mappings too (a generate)
            for (int i = 0; i < n; i++) {
                const int cur = len[(size_t)sl[(size_t)i]];
                from[(size_t)i] = r.below(4) == 0 ? r.below(cur + 1) : cur;
                lens[(size_t)i] = from[(size_t)i] + r.in(1, 70);
                if (lens[(size_t)i] > max_seq) lens[(size_t)i] = max_seq;
                if (from[(size_t)i] >= lens[(size_t)i]) from[(size_t)i] = lens[(size_t)i] - 1;
            }
            int need = -1, have = -1, mneed = -2, mhave = -2;
            const size_t p0 = p.pending.size();
            const std::vector<int32_t> table = p.table, refs = p.refs;
            std::vector<KrPageChange> mine; std::vector<Change> mmine;
            const int bad = p.reserve(n, sl.data(), lens.data(), logged ? &mine : nullptr, &need, &have, writes ? from.data() : nullptr);
            const int mbad = m.reserve(n, sl.data(), lens.data(), writes ? from.data() : nullptr, &mmine, &mneed, &mhave);
            CHECK(bad == mbad);
            reserves++;
            if (bad >= 0) {
                CHECK(need == mneed && have == mhave && need > have);
                CHECK(p.table == table && p.refs == refs && p.pending.size() == p0 && mine.empty());      // nothing mapped, nothing queued, nothing logged
                refusals++;
            } else {
                CHECK(same_logs(p.pending, p0, mmine, 0) && (!logged || same_logs(mine, 0, mmine, 0)));      // queued, and the caller's log is the same mappings
                for (size_t i = p0; i < p.pending.size(); i++) cow += p.pending[i].src >= 0;
                for (int i = 0; i < n; i++) if (writes) len[(size_t)sl[(size_t)i]] = (int)lens[(size_t)i];
                if (logged && r.below(4) == 0) {      // a generate's return: what the call mapped wholly past a row's final length goes back
                    g_op = "release_logged";
                    for (int i = 0; i < n; i++) {
                        const long long fin = from[(size_t)i] + r.below((int)(lens[(size_t)i] - from[(size_t)i]) + 1);
                        freed.clear(); mfreed.clear();
                        p.release_logged(mine, sl[(size_t)i], fin, &freed);
                        for (const KrPageChange& c : mine)
                            if (c.slot == sl[(size_t)i] && c.idx >= m.pages_of(fin) && m.table[(size_t)c.slot][(size_t)c.idx] == c.page) m.give_back(c.slot, c.idx, &mfreed);
                        m.prune();
                        CHECK(same_logs(freed, 0, mfreed, 0) && agree(p, m));
                        if (writes) len[(size_t)sl[(size_t)i]] = (int)fin;
                    }
                }
            }
        } else if (op < 60) {      // a fork: the count alone changes nothing and is the fork's own; a fork that does not fit changes nothing either
            g_op = "fork";
            const int src = r.below(n_slots), n_dst = r.in(1, 3 < n_slots - 1 ? 3 : n_slots - 1);
            const std::vector<int32_t> dsts = distinct(n_dst, src);
            const int seq_len = r.below(8) == 0 ? r.below(max_seq + 1) : r.below(len[(size_t)src] + 1);
            const int full = seq_len / pt, part = seq_len % pt;
            const int edge = part ? m.table[(size_t)src][(size_t)full] : -1;
            const int need = edge >= 0 ? n_dst : 0, gain = m.would_free(dsts), have = m.n_free();
            const KrPageFork fit = p.fork_fit(src, n_dst, dsts.data(), seq_len);
            CHECK(fit.need == need && fit.free == have && fit.gain == gain && fit.fits() == (need <= have + gain) && agree(p, m));
            const KrPageFork did = p.fork(src, n_dst, dsts.data(), seq_len);
            CHECK(did.need == need && did.free == have && did.gain == gain);
            forks++;
            if (need > have + gain) fork_refusals++;      // the model stays as it is, and so must the pool
            else {
                for (int32_t d : dsts) { mfreed.clear(); m.trim(d, 0, &mfreed); }
                m.prune();
                for (int32_t d : dsts) {
                    for (int j = 0; j < full; j++) m.map(d, j, m.table[(size_t)src][(size_t)j]);
                    if (edge >= 0) {
                        const int q = m.lowest_free();
                        CHECK(q >= 0);      // what the count above promised
                        m.map(d, full, q); m.holds[(size_t)edge]++;
                        m.mpend.push_back(Change{d, full, q, edge, part});
                    }
                    len[(size_t)d] = seq_len;
                }
            }
        } else if (op < 72) {      // trim
            g_op = "trim";
            const int s = r.below(n_slots);
            const long long n = r.below(3) == 0 ? 0 : r.below(len[(size_t)s] + 1);
            const std::vector<KrPageChange> q0 = p.pending;
            const std::vector<int32_t> holds0 = p.holds;
            freed.clear(); mfreed.clear();
            p.trim(s, n, &freed); m.trim(s, n, &mfreed); m.prune();
            CHECK(same_logs(freed, 0, mfreed, 0) && dropped(s, m.pages_of(n), p.stride, q0, holds0));
            if (n < len[(size_t)s]) len[(size_t)s] = (int)n;
        } else if (op < 78) {      // one entry given back
            g_op = "give_back";
            const int s = r.below(n_slots), j = r.below(p.stride);
            const std::vector<KrPageChange> q0 = p.pending;
            const std::vector<int32_t> holds0 = p.holds;
            freed.clear(); mfreed.clear();
            p.give_back(s, j, &freed); m.give_back(s, j, &mfreed); m.prune();
            CHECK(same_logs(freed, 0, mfreed, 0) && dropped(s, j, j + 1, q0, holds0));
            if (len[(size_t)s] > j * pt) len[(size_t)s] = j * pt;
        } else if (op < 92) {      // the pass opens: the plan of what goes to the device against the model's queue, then every copy's source is let go, in order
            g_op = "flush";
            const KrPageFlush f = p.flush_plan();
            std::vector<int32_t> zero, cp[3];
            std::vector<int> lo((size_t)n_slots, -1), hi((size_t)n_slots, -1);
            for (size_t k = 0; k < f.ranges.size(); k++) {      // slots ascending, one range each
                const KrPageFlush::Range& g = f.ranges[k];
                CHECK(g.slot >= 0 && g.slot < n_slots && g.lo >= 0 && g.lo <= g.hi && g.hi < p.stride && (k == 0 || f.ranges[k - 1].slot < g.slot));
                lo[(size_t)g.slot] = g.lo; hi[(size_t)g.slot] = g.hi;
            }
            std::vector<char> has((size_t)n_slots, 0);
            for (const Change& c : m.mpend) {
                CHECK(lo[(size_t)c.slot] >= 0 && c.idx >= lo[(size_t)c.slot] && c.idx <= hi[(size_t)c.slot]);      // every queued entry inside its slot's range
                has[(size_t)c.slot] = 1;
                if (c.src < 0) zero.push_back(c.page);
                else { cp[0].push_back(c.page); cp[1].push_back(c.src); cp[2].push_back(c.rows); }
            }
            for (int s = 0; s < n_slots; s++) CHECK(has[(size_t)s] == (lo[(size_t)s] >= 0));      // a slot without queued entries has no range
            CHECK(f.zero == zero && f.copies[0] == cp[0] && f.copies[1] == cp[1] && f.copies[2] == cp[2]);      // exactly the queue, in order
            for (int32_t z : zero) for (int32_t d : cp[0]) CHECK(z != d);      // no page both zeroed and written by a copy
            size_t c0 = 0;
            for (size_t end : f.ends) { CHECK(end > c0 && end <= cp[0].size()); for (size_t i = c0; i < end; i++) for (size_t j = c0; j < end; j++) CHECK(cp[1][i] != cp[0][j]); c0 = end; }
            CHECK(c0 == cp[0].size());
            p.flushed();
            for (int32_t q : cp[1]) m.holds[(size_t)q]--;
            m.mpend.clear();
            CHECK(p.pending.empty());
            for (int q = 0; q < n_pages; q++) CHECK(p.holds[(size_t)q] == 0);
        } else {      // entries leave the queue out of order: a queued entry, a copy where there is one, is given back or trimmed away while earlier ones still wait
            g_op = "give back a queued entry";
            if (p.pending.empty()) continue;
            size_t i = (size_t)r.below((int)p.pending.size());
            for (size_t k = 0; k < p.pending.size(); k++) { const size_t t = (i + k) % p.pending.size(); if (p.pending[t].src >= 0) { i = t; break; } }
            const KrPageChange c = p.pending[i];
            const bool one = r.below(2) == 0;
            const int j1 = one ? c.idx + 1 : p.stride;
            const std::vector<KrPageChange> q0 = p.pending;
            const std::vector<int32_t> holds0 = p.holds;
            const bool held = c.src >= 0 && p.row(c.slot)[c.idx] == c.page;      // a copy still in place: its hold must go with it
            freed.clear(); mfreed.clear();
            if (one) { p.give_back(c.slot, c.idx, &freed); m.give_back(c.slot, c.idx, &mfreed); }
            else { p.trim(c.slot, (long long)c.idx * pt, &freed); m.trim(c.slot, (long long)c.idx * pt, &mfreed); }
            m.prune();
            CHECK(same_logs(freed, 0, mfreed, 0) && dropped(c.slot, c.idx, j1, q0, holds0));
            CHECK(p.pending.size() < q0.size() && (!held || p.holds[(size_t)c.src] < holds0[(size_t)c.src]));
            if (len[(size_t)c.slot] > c.idx * pt) len[(size_t)c.slot] = c.idx * pt;
        }
        CHECK(agree(p, m));
        for (int q = 0; q < n_pages; q++) CHECK(p.holds[(size_t)q] >= 0);
    }
    // everything goes back: the queue empties with the entries, the last holder frees, and the lowest id comes first again
    g_op = "drain";
    for (int s = 0; s < n_slots; s++) { p.trim(s, 0, nullptr); mfreed.clear(); m.trim(s, 0, &mfreed); }
    m.prune();
    CHECK(agree(p, m) && p.pending.empty() && p.n_free == n_pages && p.n_shared == 0);
    if (copy_launches(r)) return 1;
    std::printf("page pool random ok: %d calls, %ld reservations, %ld refused, %ld copy-on-write copies, %ld forks, %ld refused, %ld queue entries pruned\n", n_calls, reserves, refusals, cow,
                forks, fork_refusals, m.pruned);
    return 0;
}
