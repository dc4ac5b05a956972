// kr_multi_flash_share.hip -- the grouped chunk pass of the batched split-KV flash-decode (kr_decode_set_option "multi_attn_fast_paged" = 2,
// docs/design/44-multi-attn-fast-share.md).  kr_multi_fd_flash_kernel (kr_multi_flash.hip) gives every (chunk, KV head, row) a workgroup, which streams the chunk's
// K and V tiles into LDS for the G = nh / nkv query heads of that one row: at G = 8, 24 of the 32 columns of every v_mfma_f32_32x32x16_f16 are zeros, and rows
// that read the SAME cache rows -- slots forked from one prefix, the token rows of one slot in a verify pass -- fetch, convert and commit the same tiles once
// each.  Here a workgroup takes an ITEM of the pass's list (kr_fd_share.h, built on the host once per pass): a chunk and up to min(8, 32 / G) rows for which
// that chunk is full and names the same cache rows.  The rows sit side by side in the columns of the one body (kr_fd_flash_dev.h, SHARE), the tiles are loaded
// once, and each column runs the operation sequence it runs alone: the partials carry the bits the one-row kernel writes, at the same places, and the merge is
// that kernel's.  Every other live (row, chunk) pair of the pass is an item of one row, so this one launch replaces the one-row launch whole.
#include "kr_fd_flash_dev.h"
#include "kr_fd_share.h"
#include "kr_lds_optin.h"
#include "kr_multi.h"

// grid (items, nkv), 256 threads: workgroup (i, kvh) takes item i = [c, n_rows, rows[8]] on KV head kvh.  K and V are those of rows[0]: its slot, or its
// slot's row of the page table.  The chunk is full for every row of an item of two or more, so the length of rows[0] gives each of them its end,
// c * chunk + chunk; an item of one row ends where its row ends.  The host lists no row of a run (kr_m_row_in_run) and no chunk that starts past its row
template <int HD, bool FP8, bool PAGED>
__global__ void __launch_bounds__(256) kr_multi_fd_share_kernel(const KrMultiGqaArgs a, const int* items, int n_chunks, int chunk) {
    const int* it = items + (size_t)blockIdx.x * KR_FDS_INTS;
    const int b0 = it[2];
    const size_t slot = (size_t)a.slots[b0];
    kr_fd_flash_body<HD, FP8, PAGED, true>(a.positions[b0] + 1, it[0], blockIdx.y, a.q_out, kr_slot_base<PAGED>(a.kv, 0, slot), kr_slot_base<PAGED>(a.kv, 1, slot), a.fd_o,
                                           a.fd_ml, a.nh, a.nkv, a.sm_scale, n_chunks, chunk, PAGED ? kr_slot_table_row(a.kv.pg, slot) : nullptr,
                                           PAGED ? a.kv.pg.shift : 0, it + 2, it[1]);
}

// grid (nh, B), 1024 threads: the merge of kr_multi_flash.hip over the same partials -- the body, the grid and the arguments of kr_multi_fd_merge_kernel, as a
// kernel function of this translation unit (a kernel template is launched where it is defined)
template <int HD>
__global__ void __launch_bounds__(1024) kr_multi_fd_share_merge_kernel(const KrMultiGqaArgs a, int n_chunks, int chunk) {
    const int b = blockIdx.y;
    if (kr_m_row_in_run(a, b)) return;
    kr_fd_merge2_body<HD>(a.positions[b] + 1, blockIdx.x, a.fd_o + (size_t)b * a.nh * n_chunks * HD, a.fd_ml + (size_t)b * a.nh * n_chunks * 2, a.nh, a.nkv,
                          a.gate + (size_t)b * a.nh * HD, a.gated, a.attn_out + (size_t)b * a.nh * HD, nullptr, n_chunks, chunk);
}

static size_t multi_fds_lds(int hd) { return (size_t)FA_TK * (hd * 2 + 16) + (size_t)hd * (FA_TK * 2 + 16); }      // multi_fd_lds (kr_multi_flash.hip): the body's tiles

template <bool PAGED>
static const void* multi_fds_fn(int hd, int fp8) {
    return hd == 256 ? (fp8 ? (const void*)kr_multi_fd_share_kernel<256, true, PAGED> : (const void*)kr_multi_fd_share_kernel<256, false, PAGED>)
         : hd == 128 ? (fp8 ? (const void*)kr_multi_fd_share_kernel<128, true, PAGED> : (const void*)kr_multi_fd_share_kernel<128, false, PAGED>)
                     : (fp8 ? (const void*)kr_multi_fd_share_kernel<64, true, PAGED> : (const void*)kr_multi_fd_share_kernel<64, false, PAGED>);
}
int kr_multi_fd_share_prepare(int hd, int fp8, int paged) {
    const size_t lds = multi_fds_lds(hd);
    return lds > 64 * 1024 ? kr_lds_optin(paged ? multi_fds_fn<true>(hd, fp8) : multi_fds_fn<false>(hd, fp8), lds) : 0;
}

int kr_launch_multi_fd_share(const KrMultiGqaArgs& a, const KrMultiFdShare& sh, int B, int n_chunks, hipStream_t st) {
    if (!kr_multi_fd_ok(a.nh, a.nkv, a.hd) || !a.fd_o || !a.fd_ml || a.fd_chunk < FA_TK || n_chunks < 1 || n_chunks > 1024 || !sh.items || sh.n_items < 1) return 1;
    if (sh.width < 2 || sh.width > kr_fd_share_width(a.nh / a.nkv)) return 1;      // the list was cut for more heads per KV head than this layer has: its rows fit the columns
    if (!kr_slot_stage_fits(a.kv.pg, 32)) return 1;      // a tile of FA_TK positions lies in at most two pages
    const size_t lds = multi_fds_lds(a.hd);
    const dim3 fg(sh.n_items, a.nkv), mg(a.nh, B);
#define KR_MFS(H_, F_) do { if (a.kv.pg.table) hipLaunchKernelGGL((kr_multi_fd_share_kernel<H_, F_, true>), fg, dim3(256), lds, st, a, sh.items, n_chunks, a.fd_chunk); \
                            else hipLaunchKernelGGL((kr_multi_fd_share_kernel<H_, F_, false>), fg, dim3(256), lds, st, a, sh.items, n_chunks, a.fd_chunk); } while (0)
#define KR_MFSM(H_) hipLaunchKernelGGL(kr_multi_fd_share_merge_kernel<H_>, mg, dim3(1024), 0, st, a, n_chunks, a.fd_chunk)
    if (a.hd == 256) { if (a.kv.fp8) KR_MFS(256, true); else KR_MFS(256, false); KR_MFSM(256); }
    else if (a.hd == 128) { if (a.kv.fp8) KR_MFS(128, true); else KR_MFS(128, false); KR_MFSM(128); }
    else { if (a.kv.fp8) KR_MFS(64, true); else KR_MFS(64, false); KR_MFSM(64); }
#undef KR_MFS
#undef KR_MFSM
    return 0;
}
