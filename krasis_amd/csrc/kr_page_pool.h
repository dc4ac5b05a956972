// kr_page_pool.h -- the page allocator of paged sequence slots (docs/design/21-paged-slots.md): one free list and one page table for every layer's pools.
// Host only, no HIP types: kr_decode_multi.cpp keeps one in kr_multi_state and mirrors the table to the device; tests/test_multi_paged.py compiles it alone.
// Page id p names page p of every pool; table[slot][i] = the page that holds positions [i * page_tokens, (i + 1) * page_tokens) of the slot, -1 = unmapped.
#pragma once
#include <stdint.h>

#include <vector>

struct KrPageChange { int32_t slot, idx, page; };      // table[slot][idx] became page (a mapping), or gave page back (a release)

struct KrPagePool {
    int page_tokens = 0, shift = 0, n_pages = 0, n_slots = 0, stride = 0, n_free = 0;      // stride = table entries per slot = ceil(max_seq / page_tokens)
    std::vector<int32_t> table;      // [n_slots][stride]
    std::vector<char> used;          // [n_pages]
    int hint = 0;                    // no free page has an id below it

    bool paged() const { return page_tokens > 0; }
    // 0: ready; 1: page_tokens is not a power of two >= min_tokens; 2: n_pages < 1; 3: bad slot geometry
    int init(int slots, int max_seq, int tokens, int pages, int min_tokens) {
        if (tokens < min_tokens || (tokens & (tokens - 1))) return 1;
        if (pages < 1) return 2;
        if (slots < 1 || max_seq < 1) return 3;
        page_tokens = tokens; n_pages = pages; n_slots = slots; n_free = pages; hint = 0;
        for (shift = 0; (1 << shift) < tokens; shift++) {}
        stride = (int)(((long long)max_seq + tokens - 1) >> shift);
        table.assign((size_t)slots * stride, -1);
        used.assign((size_t)pages, 0);
        return 0;
    }
    int pages_of(long long len) const { return (int)((len + page_tokens - 1) >> shift); }      // pages that cover positions [0, len)
    int32_t* row(int slot) { return &table[(size_t)slot * stride]; }
    const int32_t* row(int slot) const { return &table[(size_t)slot * stride]; }
    int mapped(int slot) const { int c = 0; for (int i = 0; i < stride; i++) c += row(slot)[i] >= 0; return c; }
    // unmapped entries among the first pages_of(len) of the slot
    int missing(int slot, long long len) const { int c = 0; for (int i = 0, e = pages_of(len); i < e; i++) c += row(slot)[i] < 0; return c; }
    // all or nothing: every slots[i] gets the pages that cover [0, lens[i]), lowest free id first in row order, each mapping appended to log.  Returns -1, or
    // the first row that does not fit -- then nothing is mapped; *need = the pages rows 0 .. that row still need, *have = the free pages
    int reserve(int n, const int32_t* slots, const long long* lens, std::vector<KrPageChange>* log, int* need, int* have) {
        long long tot = 0;
        for (int i = 0; i < n; i++) {
            tot += missing(slots[i], lens[i]);
            if (tot > n_free) { if (need) *need = (int)tot; if (have) *have = n_free; return i; }
        }
        for (int i = 0; i < n; i++)
            for (int j = 0, e = pages_of(lens[i]); j < e; j++) {
                int32_t& t = row(slots[i])[j];
                if (t >= 0) continue;
                while (used[(size_t)hint]) hint++;      // tot <= n_free: a free page exists
                used[(size_t)hint] = 1; n_free--; t = hint;
                if (log) log->push_back(KrPageChange{slots[i], j, t});
            }
        return -1;
    }
    void give_back(int slot, int idx, std::vector<KrPageChange>* log) {
        int32_t& t = row(slot)[idx];
        if (t < 0) return;
        used[(size_t)t] = 0; n_free++;
        if (t < hint) hint = t;
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
