// kr_slot_image.h -- the host image of one sequence slot (docs/design/38-slot-swap.md): its layout, the checks of its header, and the list of pieces that moves a
// byte range of it out of, or into, a slot's pages.  Host only, no device types: kr_decode_multi.cpp builds the lists and kr_multi_swap.hip carries them out;
// tests/slot_image_check.cpp drives these same functions under sanitizers, with memcpy in place of the kernels.
// An image is a header of 64 bytes, a table of {offset, bytes} per section, then the sections, each at a multiple of 16 bytes, the gaps zero.  Sections 2 l and
// 2 l + 1 belong to store layer l -- GQA: K rows [seq_len][a_row], V rows [seq_len][b_row]; MLA: latent rows, rope-key rows; linear attention: conv state,
// recurrent state; a layer without attention: two empty sections -- and the last one, if the header says so, is the slot's sampler: [temperature f32 | top_k i32 |
// top_p f32 | presence penalty f32 | xorshift64 state u64 | 8 zero bytes | seen bitmap u32 [(vocab + 31) / 32]].  All values little-endian.  The image is canonical:
// position-major, nothing at or past seq_len, nothing of n_slots, max_seq, flat or paged, page_tokens or page ids -- one sequence state, one byte string.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#define KR_SLOT_IMAGE_MAGIC 0x49534C53u      // "SLSI" as the bytes lie in memory
#define KR_SLOT_IMAGE_VERSION 1u
#define KR_SLOT_PIECE_CAP (64u * 1024u)      // bytes of the largest piece, a multiple of 16: a staged range of 4 MiB is at least 64 workgroups, one of 16 MiB at least 256 (the cap itself is unmeasured, docs/design/38-slot-swap.md)
#define KR_SLOT_CHUNK_DEFAULT (4 << 20)      // "slot_swap_chunk_bytes": the smallest of 1, 4, 16, 64, 256 MiB whose export + import time is within 5 % of the best (profiles/slot_swap.txt)
#define KR_SLOT_CHUNK_MIN 1024

enum { KR_SLOT_NONE = 0, KR_SLOT_LA = 1, KR_SLOT_GQA = 2, KR_SLOT_MLA = 3 };      // = ATTN_* (kr_decode_internal.h)
// one store layer: the bytes of one cache row of its two buffers (GQA / MLA), or of its two per-slot states (linear attention); the others 0
struct KrSlotLayerGeo { int32_t kind; uint64_t a_row, b_row, a_state, b_state; };
struct KrSlotGeo { int32_t kv_fp8 = 0, hidden = 0, vocab = 0; std::vector<KrSlotLayerGeo> layers; };

struct KrSlotImageHeader {
    uint32_t magic, version, kv_fp8, seq_len, n_layers, hidden, vocab, has_sampler;
    uint64_t geometry, total_bytes;      // FNV-1a of every layer's [kind, a_row, b_row, a_state, b_state]; the whole image
    uint32_t n_sections, table_offset;   // 2 n_layers + has_sampler; 64
    uint64_t reserved;                   // 0
};
static_assert(sizeof(KrSlotImageHeader) == 64, "the image header is 64 bytes");
struct KrSlotSection { uint64_t offset, bytes; };
#define KR_SLOT_SAMPLER_HEAD 32      // the sampler section's bytes ahead of the seen bitmap: 16 of parameters (host), 8 of state, 8 zero

inline uint64_t kr_slot_geometry_digest(const KrSlotGeo& g) {
    uint64_t h = 0xCBF29CE484222325ull;
    auto eat = [&](uint64_t v) { for (int i = 0; i < 8; i++) { h ^= (v >> (8 * i)) & 0xFF; h *= 0x100000001B3ull; } };
    for (const KrSlotLayerGeo& l : g.layers) { eat((uint64_t)l.kind); eat(l.a_row); eat(l.b_row); eat(l.a_state); eat(l.b_state); }
    return h;
}
inline uint64_t kr_slot_up16(uint64_t v) { return (v + 15) & ~(uint64_t)15; }

// what of an image lives on the device: [off, off + bytes) of the image is `bytes` bytes of pool `pool` -- rows of `row` bytes each, position-major from
// position 0 (row > 0: a GQA / MLA buffer, found through the slot's pages), or one contiguous per-slot buffer (row 0: the "page" is the slot).  Pool 2 l + h =
// buffer h of store layer l; pools 2 n_layers and 2 n_layers + 1 = the samplers' xorshift64 states and seen bitmaps
struct KrSlotSpan { uint64_t off, bytes, row; int32_t pool; };
struct KrSlotLayout {
    KrSlotImageHeader h;
    std::vector<KrSlotSection> sec;
    std::vector<KrSlotSpan> spans;       // ascending, disjoint, none empty; every other payload byte is the host's (the sampler's parameters) or zero
    uint64_t payload = 0, total = 0;     // the sections start here (a multiple of 16); total is one too
    uint64_t sampler = 0;                // the sampler section's offset, 0 = none
};
inline KrSlotLayout kr_slot_image_layout(const KrSlotGeo& g, int seq_len, bool with_sampler) {
    KrSlotLayout L;
    const uint32_t nl = (uint32_t)g.layers.size(), ns = 2 * nl + (with_sampler ? 1u : 0u);
    uint64_t at = L.payload = kr_slot_up16(sizeof(KrSlotImageHeader) + (uint64_t)ns * sizeof(KrSlotSection));
    for (uint32_t l = 0; l < nl; l++) {
        const KrSlotLayerGeo& x = g.layers[l];
        const bool rows = x.kind == KR_SLOT_GQA || x.kind == KR_SLOT_MLA, la = x.kind == KR_SLOT_LA;
        for (int hb = 0; hb < 2; hb++) {
            const uint64_t row = rows ? (hb ? x.b_row : x.a_row) : 0, n = rows ? row * (uint64_t)seq_len : la ? (hb ? x.b_state : x.a_state) : 0;
            L.sec.push_back(KrSlotSection{at, n});
            if (n) L.spans.push_back(KrSlotSpan{at, n, row, (int32_t)(2 * l + hb)});
            at = kr_slot_up16(at + n);
        }
    }
    if (with_sampler) {
        const uint64_t words = ((uint64_t)g.vocab + 31) / 32;
        L.sampler = at;
        L.sec.push_back(KrSlotSection{at, KR_SLOT_SAMPLER_HEAD + words * 4});
        L.spans.push_back(KrSlotSpan{at + 16, 8, 0, (int32_t)(2 * nl)});
        if (words) L.spans.push_back(KrSlotSpan{at + KR_SLOT_SAMPLER_HEAD, words * 4, 0, (int32_t)(2 * nl + 1)});
        at = kr_slot_up16(at + KR_SLOT_SAMPLER_HEAD + words * 4);
    }
    L.total = at;
    L.h = KrSlotImageHeader{KR_SLOT_IMAGE_MAGIC, KR_SLOT_IMAGE_VERSION, (uint32_t)(g.kv_fp8 != 0), (uint32_t)seq_len, nl, (uint32_t)g.hidden, (uint32_t)g.vocab,
                            with_sampler ? 1u : 0u, kr_slot_geometry_digest(g), L.total, ns, (uint32_t)sizeof(KrSlotImageHeader), 0};
    return L;
}
// header and table into the image, and every payload byte that no span covers zeroed (the gaps, the sampler's head: its parameters are the caller's to write)
inline void kr_slot_image_frame(const KrSlotLayout& L, void* image) {
    char* p = (char*)image;
    memcpy(p, &L.h, sizeof(L.h));
    if (!L.sec.empty()) memcpy(p + sizeof(L.h), L.sec.data(), L.sec.size() * sizeof(KrSlotSection));
    uint64_t at = sizeof(L.h) + L.sec.size() * sizeof(KrSlotSection);
    for (const KrSlotSpan& sp : L.spans) { memset(p + at, 0, (size_t)(sp.off - at)); at = sp.off + sp.bytes; }
    memset(p + at, 0, (size_t)(L.total - at));
}

// the checks of an image that need no store.  0: *out is its header; 1: shorter than a header; 2: bad magic; 3: a version this code does not read; 4: total_bytes is
// not `bytes`; 5: a malformed header or table (flags, section count, table offset, a section that is misaligned, out of order or past the end)
inline int kr_slot_image_check(const void* image, size_t bytes, KrSlotImageHeader* out) {
    KrSlotImageHeader h;
    if (!image || bytes < sizeof(h)) return 1;
    memcpy(&h, image, sizeof(h));
    if (h.magic != KR_SLOT_IMAGE_MAGIC) return 2;
    if (h.version != KR_SLOT_IMAGE_VERSION) return 3;
    if (h.total_bytes != (uint64_t)bytes) return 4;
    if (h.kv_fp8 > 1 || h.has_sampler > 1 || h.n_layers > (1u << 20) || h.n_sections != 2 * h.n_layers + h.has_sampler || h.table_offset != sizeof(h) || h.reserved) return 5;
    uint64_t at = kr_slot_up16(sizeof(h) + (uint64_t)h.n_sections * sizeof(KrSlotSection));
    if (at > h.total_bytes || (h.total_bytes & 15)) return 5;
    for (uint32_t i = 0; i < h.n_sections; i++) {
        KrSlotSection sc;
        memcpy(&sc, (const char*)image + sizeof(h) + (size_t)i * sizeof(sc), sizeof(sc));
        if (sc.offset != at || sc.bytes > h.total_bytes - sc.offset) return 5;
        at = kr_slot_up16(sc.offset + sc.bytes);
    }
    if (at != h.total_bytes) return 5;
    if (out) *out = h;
    return 0;
}
// a checked header against the slots it is to enter.  0: fits; 6: another KV element type; 7: another geometry (layers, hidden, vocab or the digest); 8: seq_len
// above max_seq; 5: its table is not the one this geometry gives at its seq_len
inline int kr_slot_image_match(const void* image, const KrSlotImageHeader& h, const KrSlotGeo& g, int max_seq) {
    if (h.kv_fp8 != (uint32_t)(g.kv_fp8 != 0)) return 6;
    if (h.n_layers != g.layers.size() || h.hidden != (uint32_t)g.hidden || h.vocab != (uint32_t)g.vocab || h.geometry != kr_slot_geometry_digest(g)) return 7;
    if (h.seq_len > (uint32_t)max_seq) return 8;
    const KrSlotLayout L = kr_slot_image_layout(g, (int)h.seq_len, h.has_sampler != 0);
    if (L.total != h.total_bytes || (!L.sec.empty() && memcmp((const char*)image + sizeof(h), L.sec.data(), L.sec.size() * sizeof(KrSlotSection)))) return 5;
    return 0;
}

// where a slot's rows lie: paged (page_tokens > 0: table = the slot's table row, entry i = the page of positions [i page_tokens, (i + 1) page_tokens), -1 =
// unmapped) or flat (page_tokens 0: the "page" of every pool is the slot).  A per-slot buffer (span.row 0) is page `slot` either way
struct KrSlotPlace { int32_t slot; int page_tokens; const int32_t* table; };
// `bytes` bytes at page_off of page `page` of pool `pool` (page -1: they read as zero) <-> the same number at range_off of the staged range.  32 bytes, read by
// the kernels of kr_multi_swap.hip as it stands
struct KrSlotPiece { int32_t pool, page; uint64_t page_off, range_off; uint32_t bytes, reserved; };
static_assert(sizeof(KrSlotPiece) == 32, "a piece is 32 bytes");
// the pieces that cover the device bytes of [r0, r1) of the image, appended to *out in image order: none crosses a page, none exceeds KR_SLOT_PIECE_CAP, and
// range_off = the byte's image offset - r0.  r0 and r1 are multiples of 16 (every span starts at one: so does a span's first piece in the range)
inline void kr_slot_pieces(const KrSlotLayout& L, const KrSlotPlace& P, uint64_t r0, uint64_t r1, std::vector<KrSlotPiece>* out) {
    for (const KrSlotSpan& sp : L.spans) {
        const uint64_t lo = std::max(sp.off, r0), hi = std::min(sp.off + sp.bytes, r1);
        if (lo >= hi) continue;
        const bool paged = sp.row && P.page_tokens > 0;
        const uint64_t page_bytes = paged ? sp.row * (uint64_t)P.page_tokens : 0;
        for (uint64_t s = lo - sp.off, e = hi - sp.off; s < e;) {      // s: the byte's offset in the slot's buffer, position-major
            const uint64_t idx = paged ? s / page_bytes : 0, in = paged ? s - idx * page_bytes : s;
            uint64_t n = std::min<uint64_t>(e - s, KR_SLOT_PIECE_CAP);
            if (paged) n = std::min(n, page_bytes - in);
            out->push_back(KrSlotPiece{sp.pool, paged ? P.table[idx] : P.slot, in, sp.off + s - r0, (uint32_t)n, 0});
            s += n;
        }
    }
}
// the ranges of an image: [payload + k chunk, ...) up to total; chunk a multiple of 16
inline uint64_t kr_slot_ranges(const KrSlotLayout& L, uint64_t chunk) { return (L.total - L.payload + chunk - 1) / chunk; }
