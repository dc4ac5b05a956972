// kr_multi_mla_pf_flash.hip -- MLA attention of a run of tokens entering a device slot, in tolerance form (kr_decode_set_option "multi_extend_mla_flash",
// docs/design/27-multi-extend-mla-flash.md): causal flash attention on the f16 matrix cores over the slot's [ckv | kpe] rows, one workgroup per 64 (token, head)
// query rows of a run, so the slot's latent cache is streamed once per tile instead of once per (token, 4 heads).  The arithmetic specification is the store's
// own KR_ATTN_FAST prompt pass (kr_mla_flash_kernel, kr_mla_flash.hip): both kernels call the non-SPLIT kr_mla_flash_body (kr_mla_flash_dev.h), so a run carries
// the bits of that prompt pass on its sequence alone, whatever rows share the pass.  The absorption, the prep launch (rope, latent RMSNorm, cache append of every
// row, the run's own among them) and the w_vc projection are the exact pass's, run by the caller (kr_multi.hip) around this one.
#include "kr_mla_flash_dev.h"
#include "kr_lds_optin.h"
#include "kr_multi.h"

// run-local row g = token * nh + head of a run -> its row of q_abs / q_pe / attn_lat: token t of a run is pass row kr_m_run_row(run, off, cnt, t), the flatten of
// docs/design/17-multi-extend.md (the last token sits in row `run`).  The body asks for g < cnt * nh only, so t < cnt
struct KrMfRunRows {
    int run, off, cnt, nh;
    __device__ __forceinline__ int operator()(int g) const { const int t = g / nh; return kr_m_run_row(run, off, cnt, t) * nh + (g - t * nh); }
};

// grid (tiles of the pass's table), 256 threads: workgroup x takes tile x = (run, tile_row), query rows 64 tile_row .. of the run's cnt * nh rows.  The run's
// slot, rows and first position come from the pass's run table and row positions (workgroup-uniform scalar loads); every workgroup of the grid has a tile, and
// none leaves ahead of a barrier.  Flat slots: the slot's row 0 of both caches; PAGED: the pools and the slot's row of the page table.  Bounds: the host built
// the tiles from the run counts it flattened the rows with (64 tile_row < cnt * nh), checked positions[i] + cnt <= the slot's max_seq and mapped every page of
// [0, positions[i] + cnt) before the pass; the body reads cache rows below kv_end = pos0 + (the tile's last token) + 1 <= pos0 + cnt only
template <int KLR, bool FP8, bool PAGED>
__global__ void __launch_bounds__(256) kr_multi_mla_pf_flash_kernel(const KrMultiMlaArgs a) {
    const int* tl = a.mf_tiles + 2 * blockIdx.x;
    const int run = tl[0], tile_row = tl[1];
    const int off = a.mf_runs[3 * run + 1], cnt = a.mf_runs[3 * run + 2];
    const size_t slot = (size_t)a.mf_runs[3 * run];
    const int pos0 = a.positions[kr_m_run_row(run, off, cnt, 0)];
    const KrMfRunRows rows{run, off, cnt, a.nh};
    if constexpr (PAGED) {
        kr_mla_flash_body<KLR, FP8, false, true>(a.q_abs, a.q_pe, a.ckv_cache, a.kpe_cache, pos0, cnt, a.nh, a.sm_scale, a.attn_lat, nullptr, nullptr, tile_row, 0, 0, 0,
                                                 a.page_table + slot * a.page_stride, a.page_shift, rows);
    } else {
        kr_mla_flash_body<KLR, FP8, false>(a.q_abs, a.q_pe, (const char*)a.ckv_cache + slot * a.ckv_stride, (const char*)a.kpe_cache + slot * a.kpe_stride, pos0, cnt, a.nh,
                                           a.sm_scale, a.attn_lat, nullptr, nullptr, tile_row, 0, 0, 0, nullptr, 0, rows);
    }
}

static_assert(KR_PAGE_MIN_TOKENS % MF_TK == 0, "a tile of MF_TK positions lies in one page");

// outside the pass: the body stages 150 KiB (kv_lora_rank 512) or 82 KiB (256) of query, K and V^T tiles, above the default 64 KiB window of a kernel.  The
// window is raised per kernel function, and every instantiation is a function of its own
template <bool PAGED>
static const void* multi_mla_pf_fn(int klr, int fp8) {
    return klr == 512 ? (fp8 ? (const void*)kr_multi_mla_pf_flash_kernel<512, true, PAGED> : (const void*)kr_multi_mla_pf_flash_kernel<512, false, PAGED>)
                      : (fp8 ? (const void*)kr_multi_mla_pf_flash_kernel<256, true, PAGED> : (const void*)kr_multi_mla_pf_flash_kernel<256, false, PAGED>);
}
int kr_multi_mla_pf_prepare(int klr, int fp8, int paged) {
    if (klr != 512 && klr != 256) return 1;
    const size_t lds = klr == 512 ? kr_mla_flash_lds<512>() : kr_mla_flash_lds<256>();
    return kr_lds_optin(paged ? multi_mla_pf_fn<true>(klr, fp8) : multi_mla_pf_fn<false>(klr, fp8), lds);
}

int kr_multi_mla_pf_args_ok(const KrMultiMlaArgs& a) {
    if (a.rd != 64 || (a.klr != 512 && a.klr != 256) || a.nh < 1) return 0;      // kr_launch_mla_flash's rule
    if (!a.mf_runs || !a.mf_tiles || a.mf_ntiles < 1 || !a.attn_lat) return 0;
    return !(a.page_table && (a.page_stride < 1 || (1 << a.page_shift) < MF_TK));      // a tile of MF_TK positions lies in one page
}
int kr_launch_multi_mla_pf_flash(const KrMultiMlaArgs& a, hipStream_t st) {
    if (!kr_multi_mla_pf_args_ok(a)) return 1;
    const dim3 grid(a.mf_ntiles);
#define KR_MMR(K_, F_) do { const size_t lds = kr_mla_flash_lds<K_>(); \
                            if (a.page_table) hipLaunchKernelGGL((kr_multi_mla_pf_flash_kernel<K_, F_, true>), grid, dim3(256), lds, st, a); \
                            else hipLaunchKernelGGL((kr_multi_mla_pf_flash_kernel<K_, F_, false>), grid, dim3(256), lds, st, a); } while (0)
    if (a.klr == 512) { if (a.kv_fp8) KR_MMR(512, true); else KR_MMR(512, false); }
    else { if (a.kv_fp8) KR_MMR(256, true); else KR_MMR(256, false); }
#undef KR_MMR
    return 0;
}
