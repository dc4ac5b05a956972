// kr_fd_share.h -- the item list of the grouped split-KV chunk kernel (kr_multi_flash_share.hip, docs/design/44-multi-attn-fast-share.md), on the host.  No HIP in
// here: the pass (kr_multi_pass, kr_decode_prefill.cpp) and a stand-alone test program (tests/fd_share_check.cpp) include it alike.
// An item is one workgroup's work per KV head: chunk c of the cache rows of rows[0], against the query heads of n_rows rows of the pass.  Rows share an item only
// where the chunk is FULL for each of them and they name the SAME cache rows for it, so every column of the workgroup sees the tiles, the end and the mask it
// saw alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#define KR_FDS_MAX_ROWS 8                          // rows of an item, at most
#define KR_FDS_INTS (2 + KR_FDS_MAX_ROWS)          // an item on the device: [c, n_rows, rows[8]], unused rows 0

// the rows the per-row attention kernels see.  in_run (may be null: none) = what kr_m_row_in_run tests, non-zero for the last token of a run the run kernels
// take.  table null: flat slots, the key of a chunk is the slot; else the pool's host table [n_slots][stride] of pages of page_tokens = 1 << shift positions,
// and the key is the entries over every page the chunk touches
struct KrFdShareRows { int n; const int32_t* slots; const int32_t* positions; const int32_t* in_run; const int32_t* table; int stride, shift; };

// rows per item for G query heads per KV head: the columns of one 32-column matrix instruction, capped
inline int kr_fd_share_width(int G) { const int r = G >= 1 ? 32 / G : 0; return r < KR_FDS_MAX_ROWS ? r : KR_FDS_MAX_ROWS; }

// rows a and b name the same cache rows for positions [p0, p1)
inline bool kr_fd_share_same(const KrFdShareRows& r, int a, int b, int p0, int p1) {
    if (!r.table) return r.slots[a] == r.slots[b];
    const int32_t *ta = r.table + (size_t)r.slots[a] * r.stride, *tb = r.table + (size_t)r.slots[b] * r.stride;
    for (int e = p0 >> r.shift; e <= (p1 - 1) >> r.shift; e++) if (ta[e] < 0 || ta[e] != tb[e]) return false;
    return true;
}

// -> items (KR_FDS_INTS ints each), chunk by chunk and inside a chunk in batch order of their first rows; returns their number.  Every live (row, chunk) pair
// -- c * fd_chunk <= positions[b], b outside a run -- lies in exactly one item.  Rows of one key are cut into items of at most R in batch order.  R < 2, or no
// item of two or more rows: the list is empty and 0 is returned (the pass launches the one-row kernel, as without the list)
inline int kr_fd_share_build(const KrFdShareRows& r, int fd_chunk, int R, std::vector<int32_t>& items) {
    items.clear();
    if (R < 2 || fd_chunk < 1 || r.n < 2) return 0;
    if (R > KR_FDS_MAX_ROWS) R = KR_FDS_MAX_ROWS;
    int max_pos = -1;
    for (int b = 0; b < r.n; b++) if (!(r.in_run && r.in_run[b]) && r.positions[b] > max_pos) max_pos = r.positions[b];
    bool grouped = false;
    std::vector<size_t> open;      // this chunk's items that can still take a row: offsets into items
    for (int c = 0; (long long)c * fd_chunk <= max_pos; c++) {
        const int p0 = c * fd_chunk, p1 = p0 + fd_chunk;
        open.clear();
        for (int b = 0; b < r.n; b++) {
            if ((r.in_run && r.in_run[b]) || p0 > r.positions[b]) continue;
            size_t at = items.size();
            if (p1 <= r.positions[b] + 1) {      // full for row b: the last open item of its key, if any (a full one was closed when it filled)
                size_t k = open.size();
                while (k > 0 && !kr_fd_share_same(r, items[open[k - 1] + 2], b, p0, p1)) k--;
                if (k > 0) { at = open[k - 1]; if (items[at + 1] + 1 == R) open.erase(open.begin() + (ptrdiff_t)(k - 1)); }
                else if (kr_fd_share_same(r, b, b, p0, p1)) open.push_back(at);      // every entry mapped: it may be joined
            }
            if (at == items.size()) { items.resize(at + KR_FDS_INTS, 0); items[at] = c; }
            else grouped = true;
            items[at + 2 + (size_t)items[at + 1]++] = b;
        }
    }
    if (!grouped) items.clear();
    return (int)(items.size() / KR_FDS_INTS);
}
