// kr_multi_mla_flash.hip -- MLA attention of the batched multi-sequence step in tolerance form (kr_decode_set_option "multi_mla_fast",
// docs/design/24-multi-mla-fast.md): split-KV flash-decode on the f16 matrix cores over the rows' slots, flat or paged.  The arithmetic specification is the
// store's own KR_ATTN_FAST step (the SPLIT form of kr_mla_flash_kernel + kr_fd_merge2_kernel): both pairs of kernels call kr_mla_flash_body
// (kr_mla_flash_dev.h) and kr_fd_merge2_body (kr_fd_flash_dev.h), so row b of a step carries the bits of that step on its sequence alone, whatever rows
// share the launch.  The absorption, the prep launch (rope, latent RMSNorm, cache append) and the w_vc projection are the exact step's, run by the caller
// (kr_launch_multi_mla, kr_multi.hip) around these two.
#include "kr_mla_flash_dev.h"
#include "kr_fd_flash_dev.h"
#include "kr_lds_optin.h"
#include "kr_multi.h"

// grid (chunks of the longest row, B), 256 threads: workgroup (c, b) takes chunk c of slot slots[b], which holds positions[b] + 1 rows, against the nh <= 64
// heads of row b (one query tile); one that starts past its row's last position leaves at once (inside the body, before the first barrier).  Partials of
// row b: fd_o + b * n_chunks * nh * KLR as [chunk][head][KLR], fd_ml + b * nh * n_chunks * 2 as [head][n_chunks][2] -- the single-sequence layout inside.
// PAGED: ckv_cache / kpe_cache are the pools and the body walks the slot's row of the page table; the flat instantiation names no table
template <int KLR, bool FP8, bool PAGED>
__global__ void __launch_bounds__(256) kr_multi_mla_flash_kernel(const KrMultiMlaArgs a, int n_chunks, int chunk_tiles) {
    const int c = blockIdx.x, b = blockIdx.y;
    if (kr_m_row_in_run(a, b)) return;      // "multi_extend_mla_flash": the last token of a run of >= 2, attended to by the run kernel (workgroup-uniform, ahead of every barrier)
    const int pos = a.positions[b];
    const float* q_abs = a.q_abs + (size_t)b * a.nh * KLR;
    const float* q_pe = a.q_pe + (size_t)b * a.nh * 64;
    float* fd_o = a.fd_o + (size_t)b * n_chunks * a.nh * KLR;
    float* fd_ml = a.fd_ml + (size_t)b * a.nh * n_chunks * 2;
    const size_t slot = (size_t)a.slots[b];
    if constexpr (PAGED) {
        kr_mla_flash_body<KLR, FP8, true, true>(q_abs, q_pe, a.ckv_cache, a.kpe_cache, pos, 1, a.nh, a.sm_scale, nullptr, fd_o, fd_ml, 0, c, n_chunks, chunk_tiles,
                                                a.page_table + slot * a.page_stride, a.page_shift);
    } else {
        kr_mla_flash_body<KLR, FP8, true>(q_abs, q_pe, (const char*)a.ckv_cache + slot * a.ckv_stride, (const char*)a.kpe_cache + slot * a.kpe_stride, pos, 1, a.nh,
                                          a.sm_scale, nullptr, fd_o, fd_ml, 0, c, n_chunks, chunk_tiles);
    }
}

// grid (nh, B), 1024 threads: head h of row b merges the row's own ceil((positions[b] + 1) / chunk) chunks and writes row b of attn_lat -- what
// kr_launch_mla_flash_decode asks of kr_fd_merge2_kernel (one "KV head", no gate, no image).  Partials are indexed by row, not by slot
template <int KLR>
__global__ void __launch_bounds__(1024) kr_multi_mla_merge_kernel(const KrMultiMlaArgs a, int n_chunks, int chunk) {
    const int b = blockIdx.y;
    if (kr_m_row_in_run(a, b)) return;      // its chunk pass left no partials
    kr_fd_merge2_body<KLR>(a.positions[b] + 1, blockIdx.x, a.fd_o + (size_t)b * n_chunks * a.nh * KLR, a.fd_ml + (size_t)b * a.nh * n_chunks * 2, a.nh, 1, nullptr, 0,
                           a.attn_lat + (size_t)b * a.nh * KLR, nullptr, n_chunks, chunk);
}

static_assert(KR_PAGE_MIN_TOKENS % MF_TK == 0, "a tile of the MLA flash-decode lies in one page");
int kr_multi_mla_fd_ok(int nh, int klr, int rd) { return nh >= 1 && nh <= MF_ROWS && (klr == 512 || klr == 256) && rd == 64; }

// outside the step: the body stages 150 KiB (kv_lora_rank 512) or 82 KiB (256) of query, K and V^T tiles, above the default 64 KiB window of a kernel.  The
// window is raised per kernel function, and every instantiation is a function of its own
template <bool PAGED>
static const void* multi_mla_fd_fn(int klr, int fp8) {
    return klr == 512 ? (fp8 ? (const void*)kr_multi_mla_flash_kernel<512, true, PAGED> : (const void*)kr_multi_mla_flash_kernel<512, false, PAGED>)
                      : (fp8 ? (const void*)kr_multi_mla_flash_kernel<256, true, PAGED> : (const void*)kr_multi_mla_flash_kernel<256, false, PAGED>);
}
int kr_multi_mla_fd_prepare(int klr, int fp8, int paged) {
    if (klr != 512 && klr != 256) return 1;
    const size_t lds = klr == 512 ? kr_mla_flash_lds<512>() : kr_mla_flash_lds<256>();
    return kr_lds_optin(paged ? multi_mla_fd_fn<true>(klr, fp8) : multi_mla_fd_fn<false>(klr, fp8), lds);
}

int kr_launch_multi_mla_fd(const KrMultiMlaArgs& a, int B, hipStream_t st) {
    if (!kr_multi_mla_fd_ok(a.nh, a.klr, a.rd) || !a.fd_o || !a.fd_ml || a.fd_chunk < MF_TK || a.fd_chunk % MF_TK || a.fd_chunks < 1 || a.fd_chunks > 1024) return 1;
    if (a.page_table && (a.page_stride < 1 || (1 << a.page_shift) < MF_TK)) return 1;      // a tile of MF_TK positions lies in one page
    const int n_chunks = a.fd_chunks;
    const dim3 fg(n_chunks, B), mg(a.nh, B);
#define KR_MMF(K_, F_) do { const size_t lds = kr_mla_flash_lds<K_>(); \
                            if (a.page_table) hipLaunchKernelGGL((kr_multi_mla_flash_kernel<K_, F_, true>), fg, dim3(256), lds, st, a, n_chunks, a.fd_chunk / MF_TK); \
                            else hipLaunchKernelGGL((kr_multi_mla_flash_kernel<K_, F_, false>), fg, dim3(256), lds, st, a, n_chunks, a.fd_chunk / MF_TK); } while (0)
#define KR_MMM(K_) hipLaunchKernelGGL(kr_multi_mla_merge_kernel<K_>, mg, dim3(1024), 0, st, a, n_chunks, a.fd_chunk)
    if (a.klr == 512) { if (a.kv_fp8) KR_MMF(512, true); else KR_MMF(512, false); KR_MMM(512); }
    else { if (a.kv_fp8) KR_MMF(256, true); else KR_MMF(256, false); KR_MMM(256); }
#undef KR_MMF
#undef KR_MMM
    return 0;
}
