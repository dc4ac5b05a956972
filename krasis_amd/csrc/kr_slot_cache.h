// kr_slot_cache.h -- where the rows of one layer's slot cache live, stated once for the slot set (kr_decode_multi.cpp), the args builders (kr_decode_prefill.cpp)
// and the kernels (kr_multi*.hip and the shared bodies they call); docs/design/40-slot-cache-view.md.  Host and device: no HIP call, no allocation.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define KR_SC_FN __host__ __device__ __forceinline__
#else
#define KR_SC_FN inline
#endif

// paged slots (docs/design/21-paged-slots.md): table [n_slots][stride] on the device, entry j of a slot = the id of the page that holds its positions
// [j << shift, (j + 1) << shift), -1 = unmapped.  table null: flat slots, and stride / shift are 0
struct KrSlotPages { const int* table; int stride, shift; };

// the cache of one GQA / MLA layer.  Half 0 = K rows (GQA) or latent rows (MLA), half 1 = V rows or rope-key rows.  base[h] = the buffer: [n_slots] units on flat
// slots, a pool of [n_pages] units on paged ones.  unit[h] = the BYTES of one unit: exactly a slot (max_seq rows) when flat, exactly a page (1 << pg.shift rows) when
// paged.  row[h] = the bytes of one position's row.  fp8: elements are E4M3 bytes, else FP16
struct KrSlotCache { void* base[2]; size_t unit[2], row[2]; KrSlotPages pg; int fp8; };

// the table row of a slot
KR_SC_FN const int* kr_slot_table_row(const KrSlotPages& pg, size_t slot) { return pg.table + slot * (size_t)pg.stride; }
// the page map in pieces, for the kernels that hoist a table row or a page id.  mask = kr_slot_mask(shift), taken once ahead of a kernel's loops; then the
// table entry of position p and the entries that cover n positions, p's row inside its page, an entry as a page id (unmapped reads as page 0: the host maps
// every page a pass reads ahead of it), and the pool row of position p of page `page` (p = 0: the page's first row)
KR_SC_FN int kr_slot_mask(int shift) { return (1 << shift) - 1; }
KR_SC_FN int kr_slot_entry(int p, int shift) { return p >> shift; }
KR_SC_FN int kr_slot_entries(int n, int shift, int mask) { return (n + mask) >> shift; }
KR_SC_FN int kr_slot_in_page(int p, int mask) { return p & mask; }
KR_SC_FN int kr_slot_page_id(int entry) { return entry < 0 ? 0 : entry; }
KR_SC_FN size_t kr_slot_page_row(int page, int p, int shift, int mask) { return ((size_t)page << shift) | (size_t)kr_slot_in_page(p, mask); }
// the map itself: the row of position p of a slot whose table row is trow, in a pool (PAGED) or in the slot (flat: the position itself)
template <bool PAGED>
KR_SC_FN size_t kr_slot_row(int p, const int* trow, int shift) {
    if constexpr (PAGED) return kr_slot_page_row(kr_slot_page_id(trow[kr_slot_entry(p, shift)]), p, shift, kr_slot_mask(shift));
    else return (size_t)p;
}
// bytes from base[h] to row 0 of unit u -- a slot, or with <false> on a paged cache a page id -- and that address.  PAGED: row 0 of the pool itself
template <bool PAGED>
KR_SC_FN size_t kr_slot_base_off(const KrSlotCache& c, int h, size_t u) { return PAGED ? 0 : u * c.unit[h]; }
template <bool PAGED>
KR_SC_FN char* kr_slot_base(const KrSlotCache& c, int h, size_t u) { return (char*)c.base[h] + kr_slot_base_off<PAGED>(c, h, u); }
// host: a stage of n positions that starts at a multiple of n never straddles a page (flat slots: always).  What every launcher asks with its own n
inline bool kr_slot_stage_fits(const KrSlotPages& pg, int n) { return !pg.table || (pg.stride >= 1 && pg.shift >= 0 && pg.shift < 31 && (1 << pg.shift) >= n); }
#undef KR_SC_FN
