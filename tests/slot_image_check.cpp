// slot_image_check.cpp -- stand-alone check of kr_slot_image.h (docs/design/38-slot-swap.md): the image layout, the header checks and the piece lists, with memcpy
// over host "pools" in place of the kernels of kr_multi_swap.hip.  Seeded random geometries; compiled alone, with sanitizers, by tests/test_multi_swap.py.
//   slot_image_check [geometries] [seed]
#include <stdio.h>
#include <stdlib.h>

#include <random>

#include "kr_slot_image.h"

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s (geometry %d)\n", __FILE__, __LINE__, #c, g_case); exit(1); } } while (0)
static int g_case = 0;
typedef std::vector<uint8_t> Bytes;

// one slot set on the host: pool p = n_pages "pages" of page_bytes[p] bytes (a slot of a per-slot buffer or of a flat set, a page of a paged pool)
struct Set {
    int page_tokens = 0, n_slots = 0, n_pages = 0, slot = 0;
    std::vector<int32_t> table;      // the slot's row (paged)
    std::vector<Bytes> pool; std::vector<uint64_t> page_bytes;
    KrSlotPlace place() const { return KrSlotPlace{slot, page_tokens, page_tokens ? table.data() : nullptr}; }
};
static Set make_set(const KrSlotGeo& g, int max_seq, int page_tokens, int slot, const std::vector<char>& hole64, int seq_len, std::mt19937_64& rng, uint8_t fill) {
    Set S;
    S.page_tokens = page_tokens; S.n_slots = 3; S.slot = slot;
    const int stride = page_tokens ? (max_seq + page_tokens - 1) / page_tokens : 0;
    S.n_pages = page_tokens ? 2 * stride + 3 : 0;
    if (page_tokens) {      // a random placement; the entries of a hole stay unmapped, and so does everything past seq_len
        std::vector<int32_t> ids((size_t)S.n_pages);
        for (int i = 0; i < S.n_pages; i++) ids[(size_t)i] = i;
        std::shuffle(ids.begin(), ids.end(), rng);
        S.table.assign((size_t)stride, -1);
        for (int j = 0; j < stride; j++) if (j * page_tokens < seq_len && !hole64[(size_t)(j * page_tokens / 64)]) S.table[(size_t)j] = ids[(size_t)j];
    }
    const size_t nl = g.layers.size(), words = ((size_t)g.vocab + 31) / 32;
    S.pool.resize(2 * nl + 2); S.page_bytes.assign(2 * nl + 2, 0);
    for (size_t l = 0; l < nl; l++)
        for (int h = 0; h < 2; h++) {
            const KrSlotLayerGeo& x = g.layers[l];
            const uint64_t row = h ? x.b_row : x.a_row, state = h ? x.b_state : x.a_state;
            const bool paged = row && page_tokens;
            S.page_bytes[2 * l + h] = row ? row * (uint64_t)(paged ? page_tokens : max_seq) : state;
            S.pool[2 * l + h].assign((size_t)(S.page_bytes[2 * l + h] * (uint64_t)(paged ? S.n_pages : S.n_slots)), fill);
        }
    S.page_bytes[2 * nl] = 8; S.pool[2 * nl].assign(8 * (size_t)S.n_slots, fill);
    S.page_bytes[2 * nl + 1] = words * 4; S.pool[2 * nl + 1].assign(words * 4 * (size_t)S.n_slots, fill);
    return S;
}
// the pieces of every range of `chunk` bytes, checked, and carried out by memcpy: pack (set -> image) or unpack (image -> set)
static void run(const KrSlotLayout& L, Set& S, uint64_t chunk, Bytes& image, bool pack, bool expect_holes) {
    std::vector<int> hits((size_t)L.total, 0);
    Bytes stage((size_t)chunk);
    size_t n_ranges = 0;
    for (uint64_t r0 = L.payload; r0 < L.total; r0 += chunk, n_ranges++) {
        const uint64_t r1 = std::min(r0 + chunk, L.total);
        std::vector<KrSlotPiece> pcs;
        kr_slot_pieces(L, S.place(), r0, r1, &pcs);
        if (pack) std::fill(stage.begin(), stage.end(), (uint8_t)0x5A);      // what no piece writes is garbage: the frame must put it right
        else memcpy(stage.data(), image.data() + r0, (size_t)(r1 - r0));
        for (const KrSlotPiece& p : pcs) {
            CHECK(p.bytes >= 1 && p.bytes <= KR_SLOT_PIECE_CAP);
            CHECK(p.range_off + p.bytes <= r1 - r0);
            CHECK(p.pool >= 0 && (size_t)p.pool < S.pool.size());
            CHECK(p.page_off + p.bytes <= S.page_bytes[(size_t)p.pool]);      // never crosses a page
            for (uint32_t i = 0; i < p.bytes; i++) hits[(size_t)(r0 + p.range_off + i)]++;
            if (p.page < 0) { CHECK(expect_holes); if (pack) memset(stage.data() + p.range_off, 0, p.bytes); continue; }
            uint8_t* at = S.pool[(size_t)p.pool].data() + (size_t)p.page * S.page_bytes[(size_t)p.pool] + p.page_off;
            CHECK((size_t)(at - S.pool[(size_t)p.pool].data()) + p.bytes <= S.pool[(size_t)p.pool].size());
            if (pack) memcpy(stage.data() + p.range_off, at, p.bytes); else memcpy(at, stage.data() + p.range_off, p.bytes);
        }
        if (pack) memcpy(image.data() + r0, stage.data(), (size_t)(r1 - r0));
    }
    CHECK(n_ranges == kr_slot_ranges(L, chunk));
    std::vector<int> want((size_t)L.total, 0);
    for (const KrSlotSpan& sp : L.spans) for (uint64_t i = 0; i < sp.bytes; i++) want[(size_t)(sp.off + i)]++;
    CHECK(hits == want);      // every payload byte of the device exactly once, nothing else
    if (pack) kr_slot_image_frame(L, image.data());
}

int main(int argc, char** argv) {
    const int n_geo = argc > 1 ? atoi(argv[1]) : 60;
    std::mt19937_64 rng(argc > 2 ? (uint64_t)atoll(argv[2]) : 1);
    auto pick = [&](std::initializer_list<uint64_t> xs) { return xs.begin()[rng() % xs.size()]; };
    size_t pieces_capped = 0, images = 0;
    for (g_case = 0; g_case < n_geo; g_case++) {
        KrSlotGeo g;
        g.kv_fp8 = (int)(rng() & 1); g.hidden = 64; g.vocab = (int)pick({1, 31, 32, 33, 500, 1000});
        const int nl = 1 + (int)(rng() % 5), max_seq = (int)pick({70, 120, 200});
        for (int l = 0; l < nl; l++) {
            const int kind = (int)(rng() % 4);      // row sizes include ones that are no multiple of 16
            if (kind == KR_SLOT_LA) g.layers.push_back(KrSlotLayerGeo{kind, 0, 0, pick({40, 256, 1000, 70000}), pick({48, 4096, 100})});
            else if (kind == KR_SLOT_GQA) { const uint64_t r = pick({24, 64, 128, 512, 1024}); g.layers.push_back(KrSlotLayerGeo{kind, r, r, 0, 0}); }
            else if (kind == KR_SLOT_MLA) g.layers.push_back(KrSlotLayerGeo{kind, pick({512, 256, 100}), pick({64, 32, 36}), 0, 0});
            else g.layers.push_back(KrSlotLayerGeo{KR_SLOT_NONE, 0, 0, 0, 0});
        }
        const bool smp = rng() & 1;
        const int pt = (int)pick({32, 64});
        for (int seq_len : {0, 1, pt - 1, pt, pt + 1, max_seq}) {
            const KrSlotLayout L = kr_slot_image_layout(g, seq_len, smp);
            images++;
            CHECK(L.payload % 16 == 0 && L.total % 16 == 0 && L.h.total_bytes == L.total && L.sec.size() == (size_t)(2 * nl + (smp ? 1 : 0)));
            for (const KrSlotSection& sc : L.sec) CHECK(sc.offset % 16 == 0 && sc.offset >= L.payload && sc.offset + sc.bytes <= L.total);
            // the truth: random rows, zero inside the holes (blocks of 64 positions that no paged set maps); random states; the canonical image written directly
            std::vector<char> hole64((size_t)(max_seq / 64 + 1), 0);
            for (char& c : hole64) c = rng() % 4 == 0;
            Bytes truth((size_t)L.total, 0);
            for (const KrSlotSpan& sp : L.spans)
                for (uint64_t i = 0; i < sp.bytes; i++) truth[(size_t)(sp.off + i)] = sp.row && hole64[(size_t)(i / sp.row / 64)] ? 0 : (uint8_t)rng();
            kr_slot_image_frame(L, truth.data());
            if (smp) for (int i = 0; i < 16; i++) truth[(size_t)L.sampler + i] = (uint8_t)(i + 1);      // the parameters are the host's
            // the header checks accept it, and it matches its geometry
            KrSlotImageHeader h;
            CHECK(kr_slot_image_check(truth.data(), truth.size(), &h) == 0 && h.seq_len == (uint32_t)seq_len && h.has_sampler == (smp ? 1u : 0u));
            CHECK(kr_slot_image_match(truth.data(), h, g, max_seq) == 0);
            // a flat set and two paged sets of different page sizes and placements hold the truth: fill them by unpacking it, which is checked on its own below
            Set flat = make_set(g, max_seq, 0, 1, hole64, seq_len, rng, 0xAA), pa = make_set(g, max_seq, 32, 0, hole64, seq_len, rng, 0xAA), pb = make_set(g, max_seq, 64, 2, hole64, seq_len, rng, 0xAA);
            for (Set* S : {&flat, &pa, &pb}) {      // written by hand, not through the pieces: position-major rows into the slot or its pages
                const bool paged = S->page_tokens > 0;
                for (const KrSlotSpan& sp : L.spans)
                    for (uint64_t i = 0; i < sp.bytes; i++) {
                        const uint64_t pb_ = S->page_bytes[(size_t)sp.pool];
                        int64_t page = S->slot; uint64_t in = i;
                        if (sp.row && paged) { page = S->table[(size_t)(i / pb_)]; in = i % pb_; }
                        if (page < 0) { CHECK(truth[(size_t)(sp.off + i)] == 0); continue; }
                        S->pool[(size_t)sp.pool][(size_t)((uint64_t)page * pb_ + in)] = truth[(size_t)(sp.off + i)];
                    }
            }
            for (uint64_t chunk : {(uint64_t)1040, (uint64_t)4096, (uint64_t)1 << 20}) {
                for (Set* S : {&flat, &pa, &pb}) {
                    Bytes image((size_t)L.total, 0xEE);
                    run(L, *S, chunk, image, true, S->page_tokens > 0);
                    if (smp) for (int i = 0; i < 16; i++) image[(size_t)L.sampler + i] = (uint8_t)(i + 1);
                    CHECK(image == truth);      // the canonical image, whatever the placement and the range size
                }
                // unpack into a third placement whose pages read as zero (freshly mapped), then pack again: the same bytes; nothing outside the pieces is written
                std::vector<char> none(hole64.size(), 0);
                Set pc = make_set(g, max_seq, pt, 1, none, seq_len, rng, 0x00);
                const Set before = pc;
                Bytes src = truth;
                run(L, pc, chunk, src, false, false);
                Bytes again((size_t)L.total, 0xEE);
                run(L, pc, chunk, again, true, false);
                if (smp) for (int i = 0; i < 16; i++) again[(size_t)L.sampler + i] = (uint8_t)(i + 1);
                CHECK(again == truth);
                for (size_t p = 0; p < pc.pool.size(); p++) {      // other slots and unmapped pages keep what they had
                    const uint64_t pbytes = pc.page_bytes[p];
                    const bool rows = p < (size_t)(2 * nl) && ((p & 1) ? g.layers[p / 2].b_row : g.layers[p / 2].a_row);
                    for (size_t pg = 0; pbytes && pg < pc.pool[p].size() / pbytes; pg++) {
                        const bool mine = rows ? std::count(pc.table.begin(), pc.table.end(), (int32_t)pg) > 0 : (int)pg == pc.slot;
                        if (!mine) CHECK(!memcmp(pc.pool[p].data() + pg * pbytes, before.pool[p].data() + pg * pbytes, (size_t)pbytes));
                    }
                }
            }
            {   // the cap: a piece list of one range over the whole image
                std::vector<KrSlotPiece> pcs;
                kr_slot_pieces(L, flat.place(), L.payload, L.total, &pcs);
                for (const KrSlotPiece& p : pcs) pieces_capped += p.bytes == KR_SLOT_PIECE_CAP;
            }
            // every corrupted field is refused, with its own code
            auto with = [&](size_t off, uint64_t v, int n) { Bytes b = truth; memcpy(b.data() + off, &v, (size_t)n); return b; };
            auto code = [&](const Bytes& b, size_t bytes) { KrSlotImageHeader hh; const int c = kr_slot_image_check(b.data(), bytes, &hh); return c ? c : kr_slot_image_match(b.data(), hh, g, max_seq); };
            CHECK(code(truth, 63) == 1 && code(truth, truth.size() - 16) == 4);
            CHECK(code(with(0, KR_SLOT_IMAGE_MAGIC ^ 0x100, 4), truth.size()) == 2);
            CHECK(code(with(4, KR_SLOT_IMAGE_VERSION + 1, 4), truth.size()) == 3);
            CHECK(code(with(8, !g.kv_fp8, 4), truth.size()) == 6 && code(with(8, 2, 4), truth.size()) == 5);
            CHECK(code(with(12, (uint64_t)max_seq + 1, 4), truth.size()) == 8);
            CHECK(code(with(16, (uint64_t)nl + 1, 4), truth.size()) == 5 && code(with(20, 65, 4), truth.size()) == 7 && code(with(24, (uint64_t)g.vocab + 1, 4), truth.size()) == 7);
            CHECK(code(with(28, !smp, 4), truth.size()) == 5);
            CHECK(code(with(32, L.h.geometry ^ 1, 8), truth.size()) == 7);
            CHECK(code(with(40, L.total + 16, 8), truth.size()) == 4);
            CHECK(code(with(48, L.h.n_sections + 1, 4), truth.size()) == 5 && code(with(52, 80, 4), truth.size()) == 5 && code(with(56, 1, 8), truth.size()) == 5);
            if (!L.sec.empty()) CHECK(code(with(64, L.sec[0].offset + 16, 8), truth.size()) == 5);
            if (seq_len < max_seq) {      // another seq_len under the same table: the table is not the one this geometry gives (unless no section depends on it)
                bool rows = false;
                for (const KrSlotLayerGeo& x : g.layers) rows |= x.a_row != 0;
                CHECK(code(with(12, (uint64_t)seq_len + 1, 4), truth.size()) == (rows ? 5 : 0));
            }
            KrSlotGeo other = g;      // another geometry with the same section sizes is still refused: the digest
            if (other.layers[0].kind == KR_SLOT_GQA) { other.layers[0].kind = KR_SLOT_MLA; CHECK(kr_slot_image_match(truth.data(), h, other, max_seq) == 7); }
        }
    }
    CHECK(pieces_capped > 0);      // the run reached the cap
    printf("slot image ok: %d geometries, %zu images, %zu pieces at the cap\n", n_geo, images, pieces_capped);
    return 0;
}
