// kr_page_pool.h -- the page allocator of paged sequence slots (docs/design/21-paged-slots.md): one free list and one page table for every layer's pools, and
// the queue of mappings the device has not seen.  Host only, no HIP types: kr_decode_multi.cpp keeps one in kr_multi_state, mirrors the table to the device and
// carries out flush_plan(); tests/page_pool_check.cpp, page_share_check.cpp and page_pool_random_check.cpp drive these same members under sanitizers.
// Page id p names page p of every pool; table[slot][i] = the page that holds positions [i * page_tokens, (i + 1) * page_tokens) of the slot, -1 = unmapped.
// Pages may be shared between slots (docs/design/22-slot-fork.md): refs[p] = the table entries that name page p.  A write never lands in a page with more
// than one reference: reserve() replaces such a page in a row's write range by a private copy.  holds[p] = the queued copies that still read page p; a page
// is free when it has neither a reference nor a hold.  Every member that gives entries back prunes the queue before it returns: no caller has to remember it.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

// table[slot][idx] became page (a mapping), or gave page back (a release).  A mapping with src >= 0 is a copy: the first `rows` rows of page src go into
// page, the rest of page is zeroed, and src is held (holds[src]) until the copy is enqueued (KrPagePool::flushed) or dropped (prune)
struct KrPageChange { int32_t slot, idx, page, src = -1, rows = 0; };

// queued copies in the order they were queued -> launches whose blocks need no order among themselves: a copy that reads the page an earlier one writes opens
// a new launch.  Returns the end (one past the last copy) of every launch; empty for no copies
inline std::vector<size_t> kr_page_copy_launches(const std::vector<int32_t>& dst, const std::vector<int32_t>& src) {
    std::vector<size_t> ends;
    size_t lo = 0;
    for (size_t i = 0; i < dst.size(); i++)
        for (size_t j = lo; j < i; j++)
            if (dst[j] == src[i]) { ends.push_back(i); lo = i; break; }
    if (!dst.empty()) ends.push_back(dst.size());
    return ends;
}

// KrPagePool::flush_plan: per slot with queued mappings, ascending, its changed table entries [lo, hi]; in queue order, the pages to zero and the copies [dst | src | rows]; the copy launches' ends
struct KrPageFlush { struct Range { int32_t slot, lo, hi; }; std::vector<Range> ranges; std::vector<int32_t> zero, copies[3]; std::vector<size_t> ends; };
// a fork's count: one boundary page per destination (need), out of the free pages and those the destinations give back (gain)
struct KrPageFork { int need, free, gain; bool fits() const { return need <= free + gain; } };

struct KrPagePool {
    int page_tokens = 0, shift = 0, n_pages = 0, n_slots = 0, stride = 0, n_free = 0;      // stride = table entries per slot = ceil(max_seq / page_tokens)
    int n_shared = 0;                // pages with more than one reference
    std::vector<int32_t> table;      // [n_slots][stride]
    std::vector<char> used;          // [n_pages]: 1 = referenced or held
    std::vector<int32_t> refs, holds, tmp;      // [n_pages]; tmp: all zero between calls (the references a call is about to drop, while it counts)
    int hint = 0;                    // no free page has an id below it
    std::vector<KrPageChange> pending;      // mappings the device has not seen, in the order they were made; every copy among them holds its source

    bool paged() const { return page_tokens > 0; }
    // 0: ready; 1: page_tokens is not a power of two >= min_tokens; 2: n_pages < 1; 3: bad slot geometry
    int init(int slots, int max_seq, int tokens, int pages, int min_tokens) {
        if (tokens < min_tokens || (tokens & (tokens - 1))) return 1;
        if (pages < 1) return 2;
        if (slots < 1 || max_seq < 1) return 3;
        page_tokens = tokens; n_pages = pages; n_slots = slots; n_free = pages; hint = 0; n_shared = 0;
        for (shift = 0; (1 << shift) < tokens; shift++) {}
        stride = (int)(((long long)max_seq + tokens - 1) >> shift);
        table.assign((size_t)slots * stride, -1);
        used.assign((size_t)pages, 0); refs.assign((size_t)pages, 0); holds.assign((size_t)pages, 0); tmp.assign((size_t)pages, 0); pending.clear();
        return 0;
    }
    int pages_of(long long len) const { return (int)((len + page_tokens - 1) >> shift); }      // pages that cover positions [0, len)
    int32_t* row(int slot) { return &table[(size_t)slot * stride]; }
    const int32_t* row(int slot) const { return &table[(size_t)slot * stride]; }
    int mapped(int slot) const { int c = 0; for (int i = 0; i < stride; i++) c += row(slot)[i] >= 0; return c; }
    // unmapped entries among the first pages_of(len) of the slot
    int missing(int slot, long long len) const { int c = 0; for (int i = 0, e = pages_of(len); i < e; i++) c += row(slot)[i] < 0; return c; }
    // the lowest free page, taken with one reference (the caller has checked n_free)
    int32_t take() { while (used[(size_t)hint]) hint++; used[(size_t)hint] = 1; refs[(size_t)hint] = 1; n_free--; return hint; }
    void add_ref(int32_t p) { if (++refs[(size_t)p] == 2) n_shared++; }
    void to_free_list(int32_t p) { if (refs[(size_t)p] || holds[(size_t)p]) return; used[(size_t)p] = 0; n_free++; if (p < hint) hint = p; }
    void drop_ref(int32_t p) { if (--refs[(size_t)p] == 1) n_shared--; to_free_list(p); }
    // a queued copy out of page p was enqueued or dropped
    void unhold(int32_t p) { holds[(size_t)p]--; to_free_list(p); }
    void queue(const KrPageChange& c, std::vector<KrPageChange>* log) { pending.push_back(c); if (log) log->push_back(c); }
    // all or nothing: every slots[i] gets the pages that cover [0, lens[i]), lowest free id first in row order, each mapping queued (and logged).  from (may be
    // null: the call writes nothing) = the first position row i writes: a mapped page that covers some of [from[i], lens[i]) and has more than one reference is
    // replaced by a private copy -- a fresh page, logged with src = the shared page and rows = page_tokens, which loses this slot's reference and is held.
    // Returns -1, or the first row that does not fit -- then nothing is mapped; *need = the pages rows 0 .. that row still need, *have = the free pages
    int reserve(int n, const int32_t* slots, const long long* lens, std::vector<KrPageChange>* log, int* need, int* have, const long long* from = nullptr) {
        const bool cow = from && n_shared > 0;
        long long tot = 0;
        int bad = -1;
        for (int i = 0; i < n && bad < 0; i++) {
            tot += missing(slots[i], lens[i]);
            if (cow)      // two rows that hold the same page: the first to write takes the copy, the last keeps the page
                for (int j = (int)(from[i] >> shift), e = pages_of(lens[i]); j < e; j++) {
                    const int32_t t = row(slots[i])[j];
                    if (t >= 0 && refs[(size_t)t] - tmp[(size_t)t] > 1) { tmp[(size_t)t]++; tot++; }
                }
            if (tot > n_free) bad = i;
        }
        if (cow)
            for (int i = 0; i < n; i++)
                for (int j = (int)(from[i] >> shift), e = pages_of(lens[i]); j < e; j++) { const int32_t t = row(slots[i])[j]; if (t >= 0) tmp[(size_t)t] = 0; }
        if (bad >= 0) { if (need) *need = (int)tot; if (have) *have = n_free; return bad; }
        for (int i = 0; i < n; i++)
            for (int j = 0, e = pages_of(lens[i]); j < e; j++) {
                int32_t& t = row(slots[i])[j];
                if (t < 0) { t = take(); queue(KrPageChange{slots[i], j, t}, log); }      // tot <= n_free: a free page exists
                else if (cow && j >= (int)(from[i] >> shift) && refs[(size_t)t] > 1) {
                    const int32_t old = t;
                    holds[(size_t)old]++; drop_ref(old);
                    t = take();
                    queue(KrPageChange{slots[i], j, t, old, page_tokens}, log);
                }
            }
        return -1;
    }
    // dst's first n_entries entries (unmapped before the call) take src's page ids, each mapped one gaining a reference
    void share(int src, int dst, int n_entries) { for (int j = 0; j < n_entries; j++) { const int32_t t = row(dst)[j] = row(src)[j]; if (t >= 0) add_ref(t); } }
    // the pages that would come free if every entry of these (distinct) slots were given back
    int would_free(int n, const int32_t* slots) {
        int c = 0;
        for (int i = 0; i < n; i++)
            for (int j = 0; j < stride; j++) { const int32_t t = row(slots[i])[j]; if (t >= 0 && ++tmp[(size_t)t] == refs[(size_t)t] && !holds[(size_t)t]) c++; }
        for (int i = 0; i < n; i++)
            for (int j = 0; j < stride; j++) { const int32_t t = row(slots[i])[j]; if (t >= 0) tmp[(size_t)t] = 0; }
        return c;
    }
    // the entry loses its page and the page a reference; the page returns to the free list when its last reference (and hold) goes.  The queue is not pruned
    void drop(int slot, int idx, std::vector<KrPageChange>* log) {
        int32_t& t = row(slot)[idx];
        if (t >= 0) { drop_ref(t); if (log) log->push_back(KrPageChange{slot, idx, t}); t = -1; }
    }
    // entries gave their pages back: a queued mapping that is no longer in place is dropped with them, and with it the hold on the page it was to copy from
    void prune() {
        auto gone = [&](const KrPageChange& c) { if (row(c.slot)[c.idx] == c.page) return false; if (c.src >= 0) unhold(c.src); return true; };
        pending.erase(std::remove_if(pending.begin(), pending.end(), gone), pending.end());
    }
    void give_back(int slot, int idx, std::vector<KrPageChange>* log) { drop(slot, idx, log); prune(); }
    // every page of the slot with index >= pages_of(len) back to the pool
    void trim(int slot, long long len, std::vector<KrPageChange>* log) { for (int j = pages_of(len); j < stride; j++) drop(slot, j, log); prune(); }
    // of the mappings a call logged: those of `slot` that lie wholly past its final length and are still in place go back (pages mapped before the call stay)
    void release_logged(const std::vector<KrPageChange>& mine, int slot, long long len, std::vector<KrPageChange>* log) {
        for (const KrPageChange& c : mine) if (c.slot == slot && c.idx >= pages_of(len) && row(slot)[c.idx] == c.page) drop(slot, c.idx, log);
        prune();
    }
    // src's boundary page at seq_len: every destination of a fork gets a copy of its own (-1: seq_len ends a page, or src has none there: nothing to copy)
    int32_t fork_edge(int src, long long seq_len) const { return (seq_len & (page_tokens - 1)) ? row(src)[seq_len >> shift] : -1; }
    // what fork() would need and find; nothing changes
    KrPageFork fork_fit(int src, int n_dst, const int32_t* dsts, long long seq_len) { return KrPageFork{fork_edge(src, seq_len) >= 0 ? n_dst : 0, n_free, would_free(n_dst, dsts)}; }
    // all or nothing: the (distinct, != src) dsts give back what they hold, then each, in argument order, shares src's whole pages below seq_len and takes the
    // lowest free page as its boundary page, queued as a copy of the first seq_len & (page_tokens - 1) rows of src's, which is held.  A fork that does not fit
    // (the count it returns says so) leaves the table, the counts and the queue untouched
    KrPageFork fork(int src, int n_dst, const int32_t* dsts, long long seq_len) {
        const KrPageFork fit = fork_fit(src, n_dst, dsts, seq_len);
        if (!fit.fits()) return fit;
        const int full = (int)(seq_len >> shift), part = (int)(seq_len & (page_tokens - 1)), edge = fork_edge(src, seq_len);
        for (int i = 0; i < n_dst; i++) for (int j = 0; j < stride; j++) drop(dsts[i], j, nullptr);
        prune();
        for (int i = 0; i < n_dst; i++) {
            share(src, dsts[i], full);
            if (edge >= 0) { holds[(size_t)edge]++; queue(KrPageChange{dsts[i], full, row(dsts[i])[full] = take(), edge, part}, nullptr); }
        }
        return fit;
    }
    // what the queue asks of the device, for the caller to carry out; then flushed(): it is enqueued, and what follows on that stream may take the copies' sources
    KrPageFlush flush_plan() const {
        KrPageFlush f;
        std::vector<int32_t> lo((size_t)n_slots, INT32_MAX), hi((size_t)n_slots, -1);
        for (const KrPageChange& c : pending) {
            if (c.src < 0) f.zero.push_back(c.page);
            else { f.copies[0].push_back(c.page); f.copies[1].push_back(c.src); f.copies[2].push_back(c.rows); }
            lo[(size_t)c.slot] = std::min(lo[(size_t)c.slot], c.idx); hi[(size_t)c.slot] = std::max(hi[(size_t)c.slot], c.idx);
        }
        for (int sl = 0; sl < n_slots; sl++) if (hi[(size_t)sl] >= 0) f.ranges.push_back({sl, lo[(size_t)sl], hi[(size_t)sl]});
        f.ends = kr_page_copy_launches(f.copies[0], f.copies[1]); return f;
    }
    void flushed() { for (const KrPageChange& c : pending) if (c.src >= 0) unhold(c.src); pending.clear(); }
};
