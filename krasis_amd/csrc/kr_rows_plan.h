// kr_rows_plan.h -- what a multi-row pass decides about the few-row kernels ("pass_few_rows", docs/design/34-pass-few-rows.md), from plain values: whether the
// pass takes them at all (its token rows T against the option's maximum, the store's mode bits) and, per launch, how the rows are split into the row groups of
// gridDim.y so that a group's INT16 images fit the LDS window.  Host only: tests/rows_plan_check.cpp compiles it alone.
#pragma once
#include <stddef.h>

#define KR_ROWS_MAX 16                      // rows of one launch; the option's largest maximum
#define KR_ROWS_MODE_GEMM_FAST 2            // the store's mode bit KR_GEMM_FAST: the tolerance GEMMs keep every pass
#define KR_ROWS_LDS_DEFAULT (64 * 1024)     // dynamic LDS a kernel may ask for without the opt-in (kr_lds_optin.h)
#define KR_ROWS_LDS_LIMIT (128 * 1024)      // ... and with it: a workgroup's images never take more (gfx950: 160 KiB per CU)
#define KR_ROWS_FILL_WGS 512                // auto row groups: halve the group while the grid holds fewer workgroups (two per CU of a 256-CU part)

// bytes of one row's INT16 activation image for a matrix of `bits` (kr_lds_bytes in kr_device.h; the launcher checks the two agree)
static inline size_t kr_rows_image_bytes(int K, int bits) {
    const int tail_words = K / 16 + ((K / 128 + 3) & ~3);
    size_t b = (size_t)(K / 8) * 16 + (size_t)((tail_words + 3) / 4) * 16;
    if (bits == 8) b += (size_t)(K / 16) * 32;
    return b;
}

// the pass-level decision, once per pass and never per chunk: T = the pass's token rows
static inline bool kr_rows_use(int enabled, int max_rows, int T, int mode_bits) {
    if (!enabled || (mode_bits & KR_ROWS_MODE_GEMM_FAST)) return false;
    if (max_rows < 1 || max_rows > KR_ROWS_MAX) return false;
    return T >= 1 && T <= max_rows;
}

struct KrRowsPlan {
    int group;        // rows per workgroup; 0: the launch is not possible (R out of range, one image alone exceeds the limit)
    int n_groups;     // gridDim.y: group g holds rows [g * group, min(R, (g + 1) * group))
    int cap;          // the kernel instantiation's row capacity: 4, 8 or 16, >= group
    size_t lds;       // dynamic LDS of a workgroup: group images
};

// R rows of K values against a matrix of `bits`; col_wgs = workgroups along the columns (gridDim.x); want_group: 0 = auto, else the largest group to use
static inline KrRowsPlan kr_rows_plan(int R, int K, int bits, int col_wgs, int want_group, size_t lds_limit = KR_ROWS_LDS_LIMIT) {
    KrRowsPlan p{0, 0, 0, 0};
    if (R < 1 || R > KR_ROWS_MAX || K < 128 || K % 128 || (bits != 4 && bits != 8)) return p;
    const size_t img = kr_rows_image_bytes(K, bits);
    int fit = (int)(lds_limit / img);
    if (fit < 1) return p;
    if (fit > KR_ROWS_MAX) fit = KR_ROWS_MAX;
    int g = R < fit ? R : fit;
    if (want_group > 0 && want_group < g) g = want_group;
    if (want_group <= 0) while (g > 1 && (long)col_wgs * ((R + g - 1) / g) < KR_ROWS_FILL_WGS) g = (g + 1) / 2;
    const int n = (R + g - 1) / g;
    g = (R + n - 1) / n;      // balanced: no group of one row beside full ones
    p.group = g; p.n_groups = n; p.cap = g <= 4 ? 4 : (g <= 8 ? 8 : 16); p.lds = (size_t)g * img;
    return p;
}
