// kr_page_pool.h -- the page allocator of paged sequence slots (docs/design/21-paged-slots.md): one free list and one page table for every layer's pools.
// Host only, no HIP types: kr_decode_multi.cpp keeps one in kr_multi_state and mirrors the table to the device; tests/test_multi_paged.py and tests/test_multi_fork.py compile it alone.
// Page id p names page p of every pool; table[slot][i] = the page that holds positions [i * page_tokens, (i + 1) * page_tokens) of the slot, -1 = unmapped.
// Pages may be shared between slots (docs/design/22-slot-fork.md): refs[p] = the table entries that name page p.  A write never lands in a page with more
// than one reference: reserve() replaces such a page in a row's write range by a private copy.  holds[p] = the queued copies that still read page p; a page
// is free when it has neither a reference nor a hold.
#pragma once
#include <stdint.h>

#include <vector>

// table[slot][idx] became page (a mapping), or gave page back (a release).  A mapping with src >= 0 is a copy: the first `rows` rows of page src go into
// page, the rest of page is zeroed, and src is held (holds[src]) until the copy is enqueued or dropped (KrPagePool::unhold)
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

struct KrPagePool {
    int page_tokens = 0, shift = 0, n_pages = 0, n_slots = 0, stride = 0, n_free = 0;      // stride = table entries per slot = ceil(max_seq / page_tokens)
    int n_shared = 0;                // pages with more than one reference
    std::vector<int32_t> table;      // [n_slots][stride]
    std::vector<char> used;          // [n_pages]: 1 = referenced or held
    std::vector<int32_t> refs, holds, tmp;      // [n_pages]; tmp: all zero between calls (the references a call is about to drop, while it counts)
    int hint = 0;                    // no free page has an id below it

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
        used.assign((size_t)pages, 0);
        refs.assign((size_t)pages, 0); holds.assign((size_t)pages, 0); tmp.assign((size_t)pages, 0);
        return 0;
    }
    int pages_of(long long len) const { return (int)((len + page_tokens - 1) >> shift); }      // pages that cover positions [0, len)
    int32_t* row(int slot) { return &table[(size_t)slot * stride]; }
    const int32_t* row(int slot) const { return &table[(size_t)slot * stride]; }
    int mapped(int slot) const { int c = 0; for (int i = 0; i < stride; i++) c += row(slot)[i] >= 0; return c; }
    // unmapped entries among the first pages_of(len) of the slot
    int missing(int slot, long long len) const { int c = 0; for (int i = 0, e = pages_of(len); i < e; i++) c += row(slot)[i] < 0; return c; }
    // the lowest free page, taken with one reference (the caller has checked n_free)
    int32_t take() {
        while (used[(size_t)hint]) hint++;
        used[(size_t)hint] = 1; refs[(size_t)hint] = 1; n_free--;
        return hint;
    }
    void add_ref(int32_t p) { if (++refs[(size_t)p] == 2) n_shared++; }
    void to_free_list(int32_t p) { if (refs[(size_t)p] || holds[(size_t)p]) return; used[(size_t)p] = 0; n_free++; if (p < hint) hint = p; }
    void drop_ref(int32_t p) { if (--refs[(size_t)p] == 1) n_shared--; to_free_list(p); }
    // a queued copy out of page p was enqueued or dropped
    void unhold(int32_t p) { holds[(size_t)p]--; to_free_list(p); }
    // all or nothing: every slots[i] gets the pages that cover [0, lens[i]), lowest free id first in row order, each mapping appended to log.  from (may be
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
                if (t < 0) {
                    t = take();      // tot <= n_free: a free page exists
                    if (log) log->push_back(KrPageChange{slots[i], j, t});
                } else if (cow && j >= (int)(from[i] >> shift) && refs[(size_t)t] > 1) {
                    const int32_t old = t;
                    holds[(size_t)old]++; drop_ref(old);
                    t = take();
                    if (log) log->push_back(KrPageChange{slots[i], j, t, old, page_tokens});
                    else unhold(old);      // nobody will copy
                }
            }
        return -1;
    }
    // dst's first n_entries entries (unmapped before the call) take src's page ids, each mapped one gaining a reference
    void share(int src, int dst, int n_entries) {
        for (int j = 0; j < n_entries; j++) {
            const int32_t t = row(src)[j];
            row(dst)[j] = t;
            if (t >= 0) add_ref(t);
        }
    }
    // the pages that would come free if every entry of these (distinct) slots were given back
    int would_free(int n, const int32_t* slots) {
        int c = 0;
        for (int i = 0; i < n; i++)
            for (int j = 0; j < stride; j++) { const int32_t t = row(slots[i])[j]; if (t >= 0 && ++tmp[(size_t)t] == refs[(size_t)t] && !holds[(size_t)t]) c++; }
        for (int i = 0; i < n; i++)
            for (int j = 0; j < stride; j++) { const int32_t t = row(slots[i])[j]; if (t >= 0) tmp[(size_t)t] = 0; }
        return c;
    }
    // the entry loses its page and the page a reference; the page returns to the free list when its last reference (and hold) goes
    void give_back(int slot, int idx, std::vector<KrPageChange>* log) {
        int32_t& t = row(slot)[idx];
        if (t < 0) return;
        drop_ref(t);
        if (log) log->push_back(KrPageChange{slot, idx, t});
        t = -1;
    }
    // every page of the slot with index >= pages_of(len) back to the pool
    void trim(int slot, long long len, std::vector<KrPageChange>* log) { for (int j = pages_of(len); j < stride; j++) give_back(slot, j, log); }
    // of the mappings a call logged: those of `slot` that lie wholly past its final length and are still in place go back (pages mapped before the call stay)
    void release_logged(const std::vector<KrPageChange>& mine, int slot, long long len, std::vector<KrPageChange>* log) {
        for (const KrPageChange& c : mine)
            if (c.slot == slot && c.idx >= pages_of(len) && row(slot)[c.idx] == c.page) give_back(slot, c.idx, log);
    }
};
