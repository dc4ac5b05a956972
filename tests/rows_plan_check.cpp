// rows_plan_check.cpp -- stand-alone check of kr_rows_plan.h, what a multi-row pass decides about the few-row kernels (docs/design/34-pass-few-rows.md).
// Host only, its own main: tests/test_pass_few_rows.py compiles it with -fsanitize=address,undefined and runs it.  The expected values are written out by
// hand from the rules of the design note (image bytes from the layout: K / 8 records of 16 B, K / 16 pair sums and K / 128 scales rounded up to 16 B, and for
// INT8 matrices K / 16 records of 32 B); none comes from calling the planner.  Each case prints its marker.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kr_rows_plan.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "rows_plan_check: line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

// every row of [0, R) lies in exactly one group, no group exceeds the capacity or the window
static void covers(const KrRowsPlan& p, int R, size_t img, size_t limit) {
    CHECK(p.group >= 1 && p.n_groups >= 1 && p.group <= p.cap && (p.cap == 4 || p.cap == 8 || p.cap == 16));
    CHECK(p.lds == (size_t)p.group * img && p.lds <= limit);
    std::vector<int> hit((size_t)R, 0);
    for (int g = 0; g < p.n_groups; g++) {
        const int r0 = g * p.group;
        CHECK(r0 < R);      // no empty group
        const int nr = R - r0 < p.group ? R - r0 : p.group;
        for (int r = 0; r < nr; r++) hit[(size_t)(r0 + r)]++;
    }
    for (int r = 0; r < R; r++) CHECK(hit[(size_t)r] == 1);
}

int main() {
    // case A: T on both sides of the maximum
    CHECK(kr_rows_use(1, 16, 16, 0) && kr_rows_use(1, 16, 1, 0) && !kr_rows_use(1, 16, 17, 0));
    CHECK(kr_rows_use(1, 4, 4, 0) && !kr_rows_use(1, 4, 5, 0));
    CHECK(!kr_rows_use(0, 16, 5, 0));                                  // the option is off
    CHECK(!kr_rows_use(1, 16, 0, 0) && !kr_rows_use(1, 0, 1, 0) && !kr_rows_use(1, 17, 5, 0));      // nothing outside 1 .. KR_ROWS_MAX
    std::puts("case A ok");

    // case B: the KR_GEMM_FAST bit keeps every pass; the other mode bits (KR_ATTN_FAST 1, KR_DECODE_FAST 4) do not decide
    CHECK(!kr_rows_use(1, 16, 5, 2) && !kr_rows_use(1, 16, 5, 3) && !kr_rows_use(1, 16, 5, 7));
    CHECK(kr_rows_use(1, 16, 5, 1) && kr_rows_use(1, 16, 5, 4));
    std::puts("case B ok");

    // case C: image bytes.  K = 2048: 256 records (4096 B) + 128 + 16 words (576 B) = 4672; INT8: + 128 x 32 = 8768.  K = 128: 256 + (8 + 4 words -> 48 B) = 304
    CHECK(kr_rows_image_bytes(2048, 4) == 4672 && kr_rows_image_bytes(2048, 8) == 8768 && kr_rows_image_bytes(128, 4) == 304 && kr_rows_image_bytes(128, 8) == 560);
    CHECK(kr_rows_image_bytes(4096, 4) == 8192 + 1152 && kr_rows_image_bytes(4096, 8) == 8192 + 1152 + 8192);
    std::puts("case C ok");

    // case D: a big grid keeps all rows in one workgroup; 16 images at K = 2048 take 74 752 B (above the default window, below the limit)
    {
        const KrRowsPlan p = kr_rows_plan(16, 2048, 4, 4096, 0);
        CHECK(p.group == 16 && p.n_groups == 1 && p.cap == 16 && p.lds == 74752 && p.lds > KR_ROWS_LDS_DEFAULT);
        covers(p, 16, 4672, KR_ROWS_LDS_LIMIT);
        const KrRowsPlan q = kr_rows_plan(5, 2048, 4, 4096, 0);
        CHECK(q.group == 5 && q.n_groups == 1 && q.cap == 8);
        const KrRowsPlan one = kr_rows_plan(1, 128, 8, 1, 0);
        CHECK(one.group == 1 && one.n_groups == 1 && one.cap == 4 && one.lds == 560);
    }
    std::puts("case D ok");

    // case E: a K whose 16 images do not fit: K = 4096, INT4 (9344 B) -- 14 fit in 128 KiB, so two balanced groups of 8; INT8 (17 536 B) -- 7 fit, three groups of 6, 6, 4
    {
        const KrRowsPlan p = kr_rows_plan(16, 4096, 4, 4096, 0);
        CHECK(p.group == 8 && p.n_groups == 2 && p.cap == 8 && p.lds == 8 * 9344);
        covers(p, 16, 9344, KR_ROWS_LDS_LIMIT);
        const KrRowsPlan q = kr_rows_plan(16, 4096, 8, 4096, 0);
        CHECK(q.group == 6 && q.n_groups == 3 && q.cap == 8);
        covers(q, 16, 17536, KR_ROWS_LDS_LIMIT);
        // a window of one image: one row per group, never a refusal; below one image: no plan
        const KrRowsPlan r1 = kr_rows_plan(16, 4096, 8, 4096, 0, 17536);
        CHECK(r1.group == 1 && r1.n_groups == 16);
        covers(r1, 16, 17536, 17536);
        CHECK(kr_rows_plan(16, 4096, 8, 4096, 0, 17535).group == 0);
    }
    std::puts("case E ok");

    // case F: a small grid spreads the rows: 64 column workgroups x groups stays below 512 until a group holds 2 rows (64 x 8 = 512)
    {
        const KrRowsPlan p = kr_rows_plan(16, 2048, 4, 64, 0);
        CHECK(p.group == 2 && p.n_groups == 8 && p.cap == 4);
        covers(p, 16, 4672, KR_ROWS_LDS_LIMIT);
        const KrRowsPlan q = kr_rows_plan(16, 2048, 4, 1, 0);      // one column workgroup: one row each
        CHECK(q.group == 1 && q.n_groups == 16);
        const KrRowsPlan f = kr_rows_plan(16, 2048, 4, 64, 16);    // a forced group is kept (the window permitting)
        CHECK(f.group == 16 && f.n_groups == 1);
        const KrRowsPlan f3 = kr_rows_plan(16, 2048, 4, 64, 3);    // ... and balanced: 6 groups of 3, 3, 3, 3, 3, 1
        CHECK(f3.group == 3 && f3.n_groups == 6);
        covers(f3, 16, 4672, KR_ROWS_LDS_LIMIT);
    }
    std::puts("case F ok");

    // case G: properties over every R, several K, both widths, grids and forced groups
    {
        const int Ks[] = {128, 256, 384, 2048, 4096, 8192, 16384};
        for (int K : Ks) for (int bits : {4, 8}) for (int R = 1; R <= KR_ROWS_MAX; R++) for (int wgs : {1, 7, 64, 600}) for (int want = 0; want <= KR_ROWS_MAX; want++) {
            const KrRowsPlan p = kr_rows_plan(R, K, bits, wgs, want);
            const size_t img = kr_rows_image_bytes(K, bits);
            if (img > KR_ROWS_LDS_LIMIT) { CHECK(p.group == 0); continue; }
            covers(p, R, img, KR_ROWS_LDS_LIMIT);
            if (want > 0) CHECK(p.group <= want);
        }
        CHECK(kr_rows_plan(0, 2048, 4, 8, 0).group == 0 && kr_rows_plan(17, 2048, 4, 8, 0).group == 0);      // R out of range
        CHECK(kr_rows_plan(4, 100, 4, 8, 0).group == 0 && kr_rows_plan(4, 2048, 5, 8, 0).group == 0);         // K no multiple of 128, unknown width
    }
    std::puts("case G ok");
    std::puts("rows plan ok");
    return 0;
}
