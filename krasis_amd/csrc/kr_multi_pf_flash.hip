// kr_multi_pf_flash.hip -- GQA attention of a run of tokens entering a device slot, in tolerance form (kr_decode_set_option "multi_extend_flash",
// docs/design/25-multi-extend-flash.md): causal flash attention on the f16 matrix cores over the slot, one workgroup per query tile of 128 / G tokens and KV head,
// so the slot's cache is streamed once per tile instead of once per token.  The arithmetic specification is the store's own KR_ATTN_FAST prompt pass
// (kr_pfm_gqa_flash_kernel / kr_pfm_gqa_flashw_kernel): head_dim 64 instantiates the prompt pass's own kernel template with another tile source, head_dim
// 128 / 256 calls the same device function (both in kr_pfm_flash_dev.h), and the launcher below chooses between the two forms by kr_launch_pfm_gqa_flash's
// rule, so a run carries the bits of that prompt pass on its sequence alone, whatever rows share the pass.  The prep launch (QK-norm, RoPE, cache append of every row, the run's own among them) is the exact pass's kr_multi_gqa_prep_kernel, run by the caller
// before these.
#include "kr_pfm_flash_dev.h"
#include "kr_lds_optin.h"
#include "kr_multi.h"
#include "kr_prefill_ops.h"

// token t of a run is pass row kr_m_run_row(run, off, cnt, t): the flatten of docs/design/17-multi-extend.md
struct KrPfRunRows {
    int i, off, cnt;
    __device__ __forceinline__ int operator()(int t) const { return kr_m_run_row(i, off, cnt, t); }
};

// Tile (run, t0): the run's slot, rows and first position come from the pass's run table and row positions (workgroup-uniform scalar loads).  Flat slots: the
// slot's row 0 of both caches; PAGED: the pools and the slot's row of the page table.  Bounds: the host built the tiles from the run counts it flattened the rows
// with (t0 < cnt), checked positions[i] + cnt <= the slot's max_seq and mapped every page of [0, positions[i] + cnt) before the pass; the kernels read cache rows
// below pos0 + min(t0 + 128 / G, cnt) only

// the four-wave kernel's tile source (kr_pfm_gqa_flash_kernel, kr_pfm_flash_dev.h): workgroup x takes tile x of the pass's table
template <bool FP8, bool PAGED_>
struct KrPfSlotTiles {
    typedef KrMultiGqaArgs Args;
    static constexpr bool PAGED = PAGED_, SLOTS = !PAGED_;
    int C, t0, pos0, run, off; size_t cache_off; const int* ptab; int psh;
    __device__ __forceinline__ KrPfSlotTiles(const Args& a, int, int) {
        const int* tl = a.pf_tiles + 2 * blockIdx.x;
        run = tl[0]; t0 = tl[1];
        const int slot = a.pf_runs[3 * run];
        off = a.pf_runs[3 * run + 1]; C = a.pf_runs[3 * run + 2];
        pos0 = a.positions[row(0)];
        cache_off = PAGED_ ? 0 : (size_t)slot * a.slot_elems * (FP8 ? 1 : 2);      // bytes to the slot's row 0
        ptab = PAGED_ ? a.page_table + (size_t)slot * a.page_stride : nullptr; psh = a.page_shift;
    }
    __device__ __forceinline__ int row(int t) const { return kr_m_run_row(run, off, C, t); }
};

// the wave-specialised body for tile (run, t0) of KV head kvh
template <int HD, bool FP8, bool PAGED>
__device__ __forceinline__ void kr_multi_pf_tile(const KrMultiGqaArgs& a, int run, int t0, int kvh) {
    const int slot = a.pf_runs[3 * run], off = a.pf_runs[3 * run + 1], cnt = a.pf_runs[3 * run + 2];
    const KrPfRunRows rows{run, off, cnt};
    KrPfFlashTile q{a.q_out, a.gate, a.attn_out, a.k_cache, a.v_cache, a.gated, a.nh, a.nkv, a.positions[rows(0)], a.sm_scale};
    if constexpr (PAGED) kr_pfm_flashw_body<HD, FP8, true>(q, cnt, t0, kvh, rows, a.page_table + (size_t)slot * a.page_stride, a.page_shift);
    else {
        const size_t base = (size_t)slot * a.slot_elems * (FP8 ? 1 : 2);      // bytes to the slot's row 0
        q.k_cache = (const char*)a.k_cache + base; q.v_cache = (const char*)a.v_cache + base;
        kr_pfm_flashw_body<HD, FP8>(q, cnt, t0, kvh, rows);
    }
}

// grid (tiles of the pass, nkv), 512 threads: the wave-specialised form takes the table from its end (within a run: the tiles that see the most positions first).
// (head_dim 64: kr_pfm_gqa_flash_kernel<64, FP8, KrPfSlotTiles<FP8, PAGED>>, the prompt pass's own kernel template)
template <int HD, bool FP8, bool PAGED>
__global__ void __launch_bounds__(512, 2) kr_multi_pf_flashw_kernel(const KrMultiGqaArgs a) {
    const int* tl = a.pf_tiles + 2 * (gridDim.x - 1 - blockIdx.x);
    kr_multi_pf_tile<HD, FP8, PAGED>(a, tl[0], tl[1], blockIdx.y);
}

template <bool PAGED>
static const void* multi_pf_fn(int hd, int fp8) {
    return hd == 256 ? (fp8 ? (const void*)kr_multi_pf_flashw_kernel<256, true, PAGED> : (const void*)kr_multi_pf_flashw_kernel<256, false, PAGED>)
         : hd == 128 ? (fp8 ? (const void*)kr_multi_pf_flashw_kernel<128, true, PAGED> : (const void*)kr_multi_pf_flashw_kernel<128, false, PAGED>)
                     : (fp8 ? (const void*)kr_pfm_gqa_flash_kernel<64, true, KrPfSlotTiles<true, PAGED>> : (const void*)kr_pfm_gqa_flash_kernel<64, false, KrPfSlotTiles<false, PAGED>>);
}
// outside the pass: the wave-specialised form stages 77 KiB (head_dim 128) / 143 KiB (head_dim 256), above the default 64 KiB window of a kernel.  The window is
// raised per kernel function, and every instantiation is a function of its own
int kr_multi_pf_prepare(int hd, int fp8, int paged) {
    if (hd != 64 && hd != 128 && hd != 256) return 1;
    const size_t lds = hd >= 128 ? kr_pfm_flashw_lds(hd) : kr_pfm_flash_lds(hd);
    return lds > 64 * 1024 ? kr_lds_optin(paged ? multi_pf_fn<true>(hd, fp8) : multi_pf_fn<false>(hd, fp8), lds) : 0;
}

int kr_multi_pf_args_ok(const KrMultiGqaArgs& a) {
    if (!kr_pfm_gqa_flash_ok(a.nh, a.nkv, a.hd) || !a.pf_runs || !a.pf_tiles || a.pf_ntiles < 1) return 0;
    return !(a.page_table && (a.page_stride < 1 || a.page_shift < 5));      // a tile of FA_TK positions lies in at most two pages
}
int kr_launch_multi_pf_flash(const KrMultiGqaArgs& a, hipStream_t st) {
    if (!kr_multi_pf_args_ok(a)) return 1;
    const dim3 grid(a.pf_ntiles, a.nkv);
    // head_dim >= 128 takes the wave-specialised form: kr_launch_pfm_gqa_flash's rule, part of the bit-identity
#define KR_MPW(H_, F_) do { if (a.page_table) hipLaunchKernelGGL((kr_multi_pf_flashw_kernel<H_, F_, true>), grid, dim3(512), kr_pfm_flashw_lds(H_), st, a); \
                            else hipLaunchKernelGGL((kr_multi_pf_flashw_kernel<H_, F_, false>), grid, dim3(512), kr_pfm_flashw_lds(H_), st, a); } while (0)
#define KR_MPF(H_, F_) do { if (a.page_table) hipLaunchKernelGGL((kr_pfm_gqa_flash_kernel<H_, F_, KrPfSlotTiles<F_, true>>), grid, dim3(256), kr_pfm_flash_lds(H_), st, a, 0); \
                            else hipLaunchKernelGGL((kr_pfm_gqa_flash_kernel<H_, F_, KrPfSlotTiles<F_, false>>), grid, dim3(256), kr_pfm_flash_lds(H_), st, a, 0); } while (0)
    if (a.hd == 256) { if (a.kv_fp8) KR_MPW(256, true); else KR_MPW(256, false); }
    else if (a.hd == 128) { if (a.kv_fp8) KR_MPW(128, true); else KR_MPW(128, false); }
    else { if (a.kv_fp8) KR_MPF(64, true); else KR_MPF(64, false); }
#undef KR_MPW
#undef KR_MPF
    return 0;
}
