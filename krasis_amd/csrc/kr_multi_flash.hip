// kr_multi_flash.hip -- GQA attention of the batched multi-sequence step in tolerance form (kr_decode_set_option "multi_attn_fast",
// docs/design/16-multi-attn-fast.md): split-KV flash-decode on the f16 matrix cores over the rows' slots.  The arithmetic specification is the store's own
// KR_ATTN_FAST step (kr_fd_flash_kernel + kr_fd_merge2_kernel, kr_attn_flash.hip): both pairs of kernels call the device functions of kr_fd_flash_dev.h, so
// row b of a step carries the bits of that step on its sequence alone, whatever rows share the launch.  The prep launch (QK-norm, RoPE, cache append) is the
// exact step's kr_multi_gqa_prep_kernel, run by the caller before these two.
#include "kr_fd_flash_dev.h"
#include "kr_lds_optin.h"
#include "kr_multi.h"

// grid (chunks of the longest row, nkv, B), 256 threads: workgroup (c, kvh, b) takes chunk c of KV head kvh of slot slots[b], which holds positions[b] + 1
// rows; one that starts past its row's last position leaves at once (inside the body).  Partials of row b: fd_o + b * nkv * n_chunks * G * HD,
// fd_ml + b * nh * n_chunks * 2, laid out inside as the single-sequence launch's.
// PAGED ("multi_attn_fast_paged", docs/design/23-multi-attn-fast-paged.md): k_cache / v_cache are the pools and the body walks the slot's row of the page
// table; the flat instantiation is the code it was
template <int HD, bool FP8, bool PAGED = false>
__global__ void __launch_bounds__(256) kr_multi_fd_flash_kernel(const KrMultiGqaArgs a, int n_chunks, int chunk) {
    const int b = blockIdx.z;
    if (kr_m_row_in_run(a, b)) return;      // "multi_extend_flash": the run kernels' row (workgroup-uniform, ahead of every barrier)
    const int seq = a.positions[b] + 1;
    if constexpr (PAGED) {
        kr_fd_flash_body<HD, FP8, true>(seq, blockIdx.x, blockIdx.y, a.q_out + (size_t)b * a.nh * HD, a.k_cache, a.v_cache, a.fd_o + (size_t)b * a.nh * n_chunks * HD,
                                        a.fd_ml + (size_t)b * a.nh * n_chunks * 2, a.nh, a.nkv, a.sm_scale, n_chunks, chunk,
                                        a.page_table + (size_t)a.slots[b] * a.page_stride, a.page_shift);
    } else {
        const size_t base = (size_t)a.slots[b] * a.slot_elems * (FP8 ? 1 : 2);      // bytes to the slot's row 0
        kr_fd_flash_body<HD, FP8>(seq, blockIdx.x, blockIdx.y, a.q_out + (size_t)b * a.nh * HD, (const char*)a.k_cache + base, (const char*)a.v_cache + base,
                                  a.fd_o + (size_t)b * a.nh * n_chunks * HD, a.fd_ml + (size_t)b * a.nh * n_chunks * 2, a.nh, a.nkv, a.sm_scale, n_chunks, chunk);
    }
}

// grid (nh, B), 1024 threads: head h of row b merges the row's own ceil((positions[b] + 1) / chunk) chunks, gates, and writes row b of attn_out (f32: the
// o-projection GEMM of the pass reads the rows)
template <int HD>
__global__ void __launch_bounds__(1024) kr_multi_fd_merge_kernel(const KrMultiGqaArgs a, int n_chunks, int chunk) {
    const int b = blockIdx.y;
    if (kr_m_row_in_run(a, b)) return;      // ... which left no partials
    kr_fd_merge2_body<HD>(a.positions[b] + 1, blockIdx.x, a.fd_o + (size_t)b * a.nh * n_chunks * HD, a.fd_ml + (size_t)b * a.nh * n_chunks * 2, a.nh, a.nkv,
                          a.gate + (size_t)b * a.nh * HD, a.gated, a.attn_out + (size_t)b * a.nh * HD, nullptr, n_chunks, chunk);
}

static size_t multi_fd_lds(int hd) { return (size_t)FA_TK * (hd * 2 + 16) + (size_t)hd * (FA_TK * 2 + 16); }

int kr_multi_fd_ok(int nh, int nkv, int hd) { return nkv >= 1 && nh % nkv == 0 && nh / nkv <= 32 && (hd == 64 || hd == 128 || hd == 256); }

// outside the step: head_dim 256 stages 69 KiB of K and V^T tiles, above the default 64 KiB window of a kernel.  The window is raised per kernel function,
// and the paged instantiations are functions of their own
template <bool PAGED>
static const void* multi_fd_fn(int hd, int fp8) {
    return hd == 256 ? (fp8 ? (const void*)kr_multi_fd_flash_kernel<256, true, PAGED> : (const void*)kr_multi_fd_flash_kernel<256, false, PAGED>)
         : hd == 128 ? (fp8 ? (const void*)kr_multi_fd_flash_kernel<128, true, PAGED> : (const void*)kr_multi_fd_flash_kernel<128, false, PAGED>)
                     : (fp8 ? (const void*)kr_multi_fd_flash_kernel<64, true, PAGED> : (const void*)kr_multi_fd_flash_kernel<64, false, PAGED>);
}
int kr_multi_fd_prepare(int hd, int fp8, int paged) {
    const size_t lds = multi_fd_lds(hd);
    return lds > 64 * 1024 ? kr_lds_optin(paged ? multi_fd_fn<true>(hd, fp8) : multi_fd_fn<false>(hd, fp8), lds) : 0;
}

int kr_launch_multi_fd(const KrMultiGqaArgs& a, int B, int n_chunks, hipStream_t st) {
    if (!kr_multi_fd_ok(a.nh, a.nkv, a.hd) || !a.fd_o || !a.fd_ml || a.fd_chunk < FA_TK || n_chunks < 1 || n_chunks > 1024) return 1;
    if (a.page_table && (a.page_stride < 1 || a.page_shift < 5)) return 1;      // a tile of FA_TK positions lies in at most two pages
    const size_t lds = multi_fd_lds(a.hd);
    const dim3 fg(n_chunks, a.nkv, B), mg(a.nh, B);
#define KR_MFF(H_, F_) do { if (a.page_table) hipLaunchKernelGGL((kr_multi_fd_flash_kernel<H_, F_, true>), fg, dim3(256), lds, st, a, n_chunks, a.fd_chunk); \
                            else hipLaunchKernelGGL((kr_multi_fd_flash_kernel<H_, F_, false>), fg, dim3(256), lds, st, a, n_chunks, a.fd_chunk); } while (0)
#define KR_MFM(H_) hipLaunchKernelGGL(kr_multi_fd_merge_kernel<H_>, mg, dim3(1024), 0, st, a, n_chunks, a.fd_chunk)
    if (a.hd == 256) { if (a.kv_fp8) KR_MFF(256, true); else KR_MFF(256, false); KR_MFM(256); }
    else if (a.hd == 128) { if (a.kv_fp8) KR_MFF(128, true); else KR_MFF(128, false); KR_MFM(128); }
    else { if (a.kv_fp8) KR_MFF(64, true); else KR_MFF(64, false); KR_MFM(64); }
#undef KR_MFF
#undef KR_MFM
    return 0;
}
