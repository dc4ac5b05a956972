// kr_mla_flash.hip -- prompt-pass MLA attention on the matrix cores (FAST / tolerance mode, kr_decode_set_attention_mode), and its split-KV form for the
// decode step over a long cache.
//
// The exact MLA prompt pass runs the decode launches with a token dimension: every (head, token) workgroup walks the whole latent cache
// (position x (kv_lora_rank + rope) elements), i.e. the cache is re-read nh x tokens times -- 2.2 k tok/s at 8192 tokens on the V2-Lite shape.
// The flash form streams the cache once per 64 query rows; its arithmetic is kr_mla_flash_body (kr_mla_flash_dev.h), which the batched step's
// kr_multi_mla_flash_kernel (kr_multi_mla_flash.hip) calls too.
#include "kr_lds_optin.h"
#include "kr_mla_flash_dev.h"
#include "kr_decode_ops.h"

// grid (row tiles of 64 query rows); q_abs [C][nh][KLR], q_pe [C][nh][64] (f32, kr_mla_prep_kernel), caches [position][KLR] / [position][64]
// SPLIT (decode over a long cache, one token): grid (row tiles, chunks); a workgroup walks `chunk_tiles` tiles of the cache and leaves the
// un-normalised O rows and (max in log2 units, sum) per head for kr_fd_merge2_kernel (kr_attn_flash.hip); the position comes from a.step.
template <int KLR, bool FP8, bool SPLIT = false>
__global__ void __launch_bounds__(256) kr_mla_flash_kernel(const KrMlaArgs a, int C, int n_chunks = 0, int chunk_tiles = 0) {
    kr_mla_flash_body<KLR, FP8, SPLIT>(a.q_abs, a.q_pe, a.ckv_cache, a.kpe_cache, SPLIT ? a.step->pos : a.pos0, C, a.nh, a.sm_scale, a.attn_lat, a.fd_o, a.fd_ml,
                                       blockIdx.x, SPLIT ? (int)blockIdx.y : 0, n_chunks, chunk_tiles);
}

// raise the dynamic-LDS window (per device, outside graph capture / before the first launch)
void kr_mla_flash_prepare() {
    (void)kr_lds_optin((const void*)kr_mla_flash_kernel<512, false, true>, kr_mla_flash_lds<512>());
    (void)kr_lds_optin((const void*)kr_mla_flash_kernel<512, true, true>, kr_mla_flash_lds<512>());
    (void)kr_lds_optin((const void*)kr_mla_flash_kernel<256, false, true>, kr_mla_flash_lds<256>());
    (void)kr_lds_optin((const void*)kr_mla_flash_kernel<256, true, true>, kr_mla_flash_lds<256>());
    (void)kr_lds_optin((const void*)kr_mla_flash_kernel<512, false>, kr_mla_flash_lds<512>());
    (void)kr_lds_optin((const void*)kr_mla_flash_kernel<512, true>, kr_mla_flash_lds<512>());
    (void)kr_lds_optin((const void*)kr_mla_flash_kernel<256, false>, kr_mla_flash_lds<256>());
    (void)kr_lds_optin((const void*)kr_mla_flash_kernel<256, true>, kr_mla_flash_lds<256>());
}
// prompt pass, n_tok tokens: a.q_abs / a.q_pe / a.attn_lat are the chunk's [n_tok][nh][.] buffers.  non-zero = geometry not covered
int kr_launch_mla_flash(const KrMlaArgs& a, int n_tok, hipStream_t st) {
    if (a.rd != 64 || (a.klr != 512 && a.klr != 256) || a.step) return 1;
    kr_mla_flash_prepare();
    dim3 grid((n_tok * a.nh + MF_ROWS - 1) / MF_ROWS);
    if (a.klr == 512) {
        if (a.kv_fp8) hipLaunchKernelGGL((kr_mla_flash_kernel<512, true>), grid, dim3(256), kr_mla_flash_lds<512>(), st, a, n_tok);
        else hipLaunchKernelGGL((kr_mla_flash_kernel<512, false>), grid, dim3(256), kr_mla_flash_lds<512>(), st, a, n_tok);
    } else {
        if (a.kv_fp8) hipLaunchKernelGGL((kr_mla_flash_kernel<256, true>), grid, dim3(256), kr_mla_flash_lds<256>(), st, a, n_tok);
        else hipLaunchKernelGGL((kr_mla_flash_kernel<256, false>), grid, dim3(256), kr_mla_flash_lds<256>(), st, a, n_tok);
    }
    return 0;
}

// decode over a long cache, FAST mode: split-KV form of the kernel above + the log-sum-exp merge of kr_attn_flash.hip.  nh <= 64 heads (one row
// tile).  non-zero = geometry not covered.  kr_mla_flash_prepare() must have run outside graph capture.
int kr_mla_flash_decode_chunk(int max_seq) { return max_seq > 16384 ? 128 : 64; }
size_t kr_mla_flash_decode_chunks(int max_seq) { const int ch = kr_mla_flash_decode_chunk(max_seq); return ((size_t)max_seq + ch - 1) / ch; }
void kr_launch_fd_merge2(const KrFdFlashArgs& a, int hd, int nch, int chunk, hipStream_t st);   // kr_attn_flash.hip
int kr_launch_mla_flash_decode(const KrMlaArgs& a, int max_seq, hipStream_t st) {
    if (a.rd != 64 || (a.klr != 512 && a.klr != 256) || !a.step || !a.fd_o || !a.fd_ml || a.nh > MF_ROWS) return 1;
    const int chunk = kr_mla_flash_decode_chunk(max_seq), nch = (int)kr_mla_flash_decode_chunks(max_seq);
    if (nch > 1024) return 1;
    dim3 grid(1, nch);
    if (a.klr == 512) {
        if (a.kv_fp8) hipLaunchKernelGGL((kr_mla_flash_kernel<512, true, true>), grid, dim3(256), kr_mla_flash_lds<512>(), st, a, 1, nch, chunk / MF_TK);
        else hipLaunchKernelGGL((kr_mla_flash_kernel<512, false, true>), grid, dim3(256), kr_mla_flash_lds<512>(), st, a, 1, nch, chunk / MF_TK);
    } else {
        if (a.kv_fp8) hipLaunchKernelGGL((kr_mla_flash_kernel<256, true, true>), grid, dim3(256), kr_mla_flash_lds<256>(), st, a, 1, nch, chunk / MF_TK);
        else hipLaunchKernelGGL((kr_mla_flash_kernel<256, false, true>), grid, dim3(256), kr_mla_flash_lds<256>(), st, a, 1, nch, chunk / MF_TK);
    }
    KrFdFlashArgs m{};
    m.step = a.step; m.fd_o = a.fd_o; m.fd_ml = a.fd_ml; m.nh = a.nh; m.nkv = 1; m.gated = 0; m.out = a.attn_lat; m.img_out = nullptr;
    kr_launch_fd_merge2(m, a.klr, nch, chunk, st);
    return 0;
}
