// kr_attn_flash.hip -- prompt-pass GQA attention on the matrix cores (FAST / tolerance mode, kr_decode_set_attention_mode).
//
// The exact prompt pass (kr_prefill_ops.hip: scores -> softmax -> P.V passes over an HBM score scratch) keeps the reference CPU decode's
// operation order per query and runs on the vector ALUs: its cost grows with the square of the prompt (12 GQA layers of a 49 863-token
// prompt: ~2.5e14 flop) and dominates long prompts.  The reference's own GPU prefill uses flashinfer's bf16 flash attention
// (python/krasis/attention.py:612-640) -- i.e. tolerance-level numerics are what the reference itself ships for this step.  This kernel is
// the gfx950 counterpart: causal flash attention over the FP16 / FP8-E4M3 cache with v_mfma_f32_32x32x16_f16, f32 accumulation and f32
// online softmax; q and the probabilities are rounded to f16 (2^-11, eight times finer than the reference's bf16), K / V are exact in f16.
//
// Layout of the computation (one workgroup = 128 query rows = the G query heads of one KV head x 128 / G consecutive tokens, 4 waves x 32 rows,
// so a staged K / V tile serves every head of the group):
//   S^T = K Q^T   : A = K tile rows from LDS ([position][dim], 16-byte reads), B = Q^T kept in registers for the whole KV loop
//                   -> accumulator column = query row = lane % 32: the softmax of a row is a LANE-LOCAL reduction over 32 values plus one
//                   exchange with lane ^ 32 (no cross-lane butterflies), and the rescale factor of O is a per-lane scalar.
//   O^T = V^T P^T : A = V^T tile from LDS ([dim][position], written transposed -- two positions per dword -- while the tile is staged),
//                   B = P^T straight from the S^T accumulators (f16-packed in registers): the k order of an MFMA is free as long as A and
//                   B agree, so B uses the accumulator's own row order {0-3, 8-11} / {4-7, 12-15} and A reads V^T in two 8-byte pieces.
// The V tile of the current 64 positions is fetched while S^T and the softmax run, the next K tile while O^T accumulates (two barriers per tile).
#include "kr_device.h"
#include "kr_libm.h"
#include "kr_lds_optin.h"
#include "kr_prefill_ops.h"
#include "kr_decode_ops.h"

#include "kr_fd_flash_dev.h"
#include "kr_pfm_flash_dev.h"

// the four-wave kernel's tile source for the prompt pass: workgroup x of the launch takes tokens x * 128 / G .. of the chunk of Ck tokens standing at a.pos0; token t
// is row t; the store's own cache holds the sequence (kr_pfm_gqa_flash_kernel itself: kr_pfm_flash_dev.h)
struct KrPfChunkTiles {
    typedef KrPfmGqaArgs Args;
    static constexpr bool PAGED = false, SLOTS = false;
    int C, t0, pos0;
    __device__ __forceinline__ KrPfChunkTiles(const Args& a, int Ck, int tq) : C(Ck), t0(blockIdx.x * tq), pos0(a.pos0) {}
    __device__ __forceinline__ int row(int t) const { return t; }
};

// ------------------------------------------------------------------------------------------------------------------------------------
// Wave-specialised form (head_dim 128 / 256).  Round 3 ran these head sizes as eight waves that all did the same thing in lock step (query tile in LDS, wave
// pairs splitting the positions of a tile, a split-KV merge at the end): every S^T MFMA fetched a K AND a Q fragment from LDS (2 KB per 32 x 32 x 16 MFMA),
// the phases of a tile stood one after the other on both waves of a SIMD (staging 0.9, S^T 0.56, softmax 0.44, P.V 0.56 of 2.64 us) and V reached LDS through
// a transposing register pass (16 conversions + 16 byte permutes + 16 four-byte LDS writes per thread and tile).  Here the two waves of a SIMD do DIFFERENT things:
//   waves 0-3 ("S waves")   own 32 query rows each, Q^T in REGISTERS (no Q in LDS at all): S^T over the 64-position tile, the online softmax (the row
//                           state m, l lives here only), P as f16 rows + the row's rescale factor into LDS (double-buffered); they stage K
//   waves 4-7 ("PV waves")  own HD / 4 output dims each for ALL 128 rows (a V^T fragment serves four row blocks): O^T += V^T P^T one tile BEHIND the S
//                           waves, so the softmax arithmetic of tile t runs under the P.V MFMAs of tile t - 1 on the same SIMD; they stage V, ROW-major like
//                           K -- the transposed fragments come out of gfx950's LDS transpose-read (ds_read_b64_tr_b16)
// No split-KV merge at the end: one softmax stream per row.  V is double-buffered: the PV waves stage V(t) FIRST (their matrix work would only queue behind the S
// waves' S^T on the same SIMD) and run P.V(t - 1) while the S waves are in their softmax.  The S^T accumulators start at -m (the row's running maximum), so once
// the maximum has settled no element needs a subtraction before its exponential and the rescale factor is 1; fragments of both sides are requested several
// MFMAs ahead by hand (one wave of a kind per SIMD: nothing else covers an LDS round trip).
// tools/probes/flash_timing.hip (1024 queries late in a 32 k cache, E4M3, 128 of 256 CUs busy): 355 -> 476 TFLOP/s; per 64-position tile S^T 0.72 | softmax
// 0.56 | K staging 0.40 on the S side, V staging 0.88 (with the fragment requests) | P.V 0.92 on the PV side, 2.28 us in all against 1.02 us of pure MFMA time
// at the 2.0 GHz the chip holds under matrix load (tools/probes/clock_probe.hip).  Tried on the way and not kept: a 32-position tile with K, V and P all
// double-buffered and one barrier per tile (same speed: the waves' own instruction streams, not the barriers, are the limit), S^T(t + 1) issued between the
// pieces of the softmax of tile t in the same wave (slower: the K fragment waits came to stand in front of every piece), K double-buffered instead of V
// (433: P.V and S^T collide on the matrix pipe again).
// ------------------------------------------------------------------------------------------------------------------------------------
template <int HD, bool FP8>
__global__ void __launch_bounds__(512, 2) kr_pfm_gqa_flashw_kernel(const KrPfmGqaArgs a, int C) {      // the body: kr_pfm_flash_dev.h
    // longest rows first: the tail of the launch is made of short workgroups
    kr_pfm_flashw_body<HD, FP8>(a, C, (gridDim.x - 1 - blockIdx.x) * (FA_ROWS / (a.nh / a.nkv)), blockIdx.y, KrPfRowsIdentity());
}

// non-zero = geometry not covered (the caller falls back to the exact passes)
bool kr_pfm_gqa_flash_ok(int nh, int nkv, int hd) {
    const int G = nkv > 0 ? nh / nkv : 0;
    return nkv > 0 && nh % nkv == 0 && G >= 1 && G <= FA_ROWS && (FA_ROWS % G) == 0 && (hd == 64 || hd == 128 || hd == 256);
}

int kr_launch_pfm_gqa_flash(const KrPfmGqaArgs& a, int C, hipStream_t st) {
    const int G = a.nkv > 0 ? a.nh / a.nkv : 0;
    if (!kr_pfm_gqa_flash_ok(a.nh, a.nkv, a.hd)) return 1;
    const int TQ = FA_ROWS / G;
    dim3 grid((C + TQ - 1) / TQ, a.nkv);
    if (a.hd >= 128) {      // wave-specialised form (S waves / PV waves)
        const size_t ldw = kr_pfm_flashw_lds(a.hd);
        const void* fnw = a.hd == 256 ? (a.kv_fp8 ? (const void*)kr_pfm_gqa_flashw_kernel<256, true> : (const void*)kr_pfm_gqa_flashw_kernel<256, false>)
                                      : (a.kv_fp8 ? (const void*)kr_pfm_gqa_flashw_kernel<128, true> : (const void*)kr_pfm_gqa_flashw_kernel<128, false>);
        if (kr_lds_optin(fnw, ldw) == 0) {
#define KR_FAW(H_, F_) hipLaunchKernelGGL((kr_pfm_gqa_flashw_kernel<H_, F_>), grid, dim3(512), ldw, st, a, C)
            if (a.hd == 256) { if (a.kv_fp8) KR_FAW(256, true); else KR_FAW(256, false); }
            else { if (a.kv_fp8) KR_FAW(128, true); else KR_FAW(128, false); }
#undef KR_FAW
            return 0;
        }
        return 1;           // LDS window refused: the caller reports it
    }
    const size_t lds = kr_pfm_flash_lds(a.hd);
    {
        const void* fn = a.kv_fp8 ? (const void*)kr_pfm_gqa_flash_kernel<64, true, KrPfChunkTiles> : (const void*)kr_pfm_gqa_flash_kernel<64, false, KrPfChunkTiles>;
        if (kr_lds_optin(fn, 96 * 1024)) return 1;
    }
#define KR_FA(H_, F_) hipLaunchKernelGGL((kr_pfm_gqa_flash_kernel<H_, F_, KrPfChunkTiles>), grid, dim3(256), lds, st, a, C)
    if (a.kv_fp8) KR_FA(64, true); else KR_FA(64, false);      // head_dim 64: the four-wave form
#undef KR_FA
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// FAST decode attention over a long cache (one token): split-KV flash-decode on the same MFMA forms.
//   kr_fd_flash_kernel  grid (chunks, KV heads): the workgroup stages its chunk's K and V^T tiles (64 positions at a time) ONCE for all G query
//                       heads of the group.  The G heads are accumulator columns 0..G-1 (the other columns of the 32-wide block carry q = 0 and
//                       are never stored: the launch is bound by the K / V stream, not by the MFMAs).  Every wave forms the same S^T and softmax
//                       statistics (32 MFMAs per tile -- cheaper than an exchange) and owns HD / 128 of the O^T dimension blocks.  Output: the
//                       chunk's un-normalised O [G][HD] and (max, sum) per head, max in log2 units.
//   kr_fd_merge2_kernel one workgroup per head: log-sum-exp merge of the chunk partials with independent partial sums (the first version's
//                       single dependent fma per chunk made this launch as long as the partial launch), gate, o-projection image.
// This replaces BOTH the exact scores launch and the first split-KV form (kr_attn_fd.h: exact scores + VALU p.v): at position 32 766 of an
// FP8 cache those were 34 + 36 + 38 us per GQA layer (profiles/r02_decode_32k_fast_fp8_kernel_stats.txt).
// ------------------------------------------------------------------------------------------------------------------------------------
template <int HD, bool FP8>
__global__ void __launch_bounds__(256) kr_fd_flash_kernel(const KrFdFlashArgs a, int n_chunks, int chunk) {      // the body: kr_fd_flash_dev.h
    kr_fd_flash_body<HD, FP8>(a.step->pos + 1, blockIdx.x, blockIdx.y, a.q, a.k_cache, a.v_cache, a.fd_o, a.fd_ml, a.nh, a.nkv, a.sm_scale, n_chunks, chunk);
}

template <int HD>
__global__ void __launch_bounds__(1024) kr_fd_merge2_kernel(const KrFdFlashArgs a, int n_chunks, int chunk) {
    kr_fd_merge2_body<HD>(a.step->pos + 1, blockIdx.x, a.fd_o, a.fd_ml, a.nh, a.nkv, a.gate, a.gated, a.out, a.img_out, n_chunks, chunk);
}

int kr_fd_flash_chunk(int max_seq) { return max_seq > 131072 ? 256 : 128; }      // at most 1024 chunks (the merge gives each a thread)
size_t kr_fd_flash_chunks(int max_seq) { const int ch = kr_fd_flash_chunk(max_seq); return ((size_t)max_seq + ch - 1) / ch; }
// outside graph capture (the windows are per (kernel, device))
int kr_fd_flash_prepare(int hd, int fp8) {
    const size_t lds = (size_t)FA_TK * (hd * 2 + 16) + (size_t)hd * (FA_TK * 2 + 16);
    const void* fn = hd == 256 ? (fp8 ? (const void*)kr_fd_flash_kernel<256, true> : (const void*)kr_fd_flash_kernel<256, false>)
                   : hd == 128 ? (fp8 ? (const void*)kr_fd_flash_kernel<128, true> : (const void*)kr_fd_flash_kernel<128, false>)
                               : (fp8 ? (const void*)kr_fd_flash_kernel<64, true> : (const void*)kr_fd_flash_kernel<64, false>);
    return lds > 64 * 1024 ? kr_lds_optin(fn, lds) : 0;
}
// non-zero = geometry not covered
int kr_launch_fd_flash(const KrFdFlashArgs& a, int hd, int fp8, int max_seq, hipStream_t st) {
    const int G = a.nkv > 0 ? a.nh / a.nkv : 0;
    if (a.nh % a.nkv || G < 1 || G > 32 || (hd != 64 && hd != 128 && hd != 256)) return 1;
    const int chunk = kr_fd_flash_chunk(max_seq), nch = (int)kr_fd_flash_chunks(max_seq);
    if (nch > 1024) return 1;
    const size_t lds = (size_t)FA_TK * (hd * 2 + 16) + (size_t)hd * (FA_TK * 2 + 16);
    dim3 grid(nch, a.nkv);
#define KR_FF(H_, F_) hipLaunchKernelGGL((kr_fd_flash_kernel<H_, F_>), grid, dim3(256), lds, st, a, nch, chunk)
    if (hd == 256) { if (fp8) KR_FF(256, true); else KR_FF(256, false); hipLaunchKernelGGL(kr_fd_merge2_kernel<256>, dim3(a.nh), dim3(1024), 0, st, a, nch, chunk); }
    else if (hd == 128) { if (fp8) KR_FF(128, true); else KR_FF(128, false); hipLaunchKernelGGL(kr_fd_merge2_kernel<128>, dim3(a.nh), dim3(1024), 0, st, a, nch, chunk); }
    else { if (fp8) KR_FF(64, true); else KR_FF(64, false); hipLaunchKernelGGL(kr_fd_merge2_kernel<64>, dim3(a.nh), dim3(1024), 0, st, a, nch, chunk); }
#undef KR_FF
    return 0;
}

void kr_launch_fd_merge2(const KrFdFlashArgs& a, int hd, int nch, int chunk, hipStream_t st) {     // also used by the MLA flash-decode (hd = kv_lora_rank)
    if (hd == 512) hipLaunchKernelGGL(kr_fd_merge2_kernel<512>, dim3(a.nh), dim3(1024), 0, st, a, nch, chunk);
    else if (hd == 256) hipLaunchKernelGGL(kr_fd_merge2_kernel<256>, dim3(a.nh), dim3(1024), 0, st, a, nch, chunk);
    else if (hd == 128) hipLaunchKernelGGL(kr_fd_merge2_kernel<128>, dim3(a.nh), dim3(1024), 0, st, a, nch, chunk);
    else hipLaunchKernelGGL(kr_fd_merge2_kernel<64>, dim3(a.nh), dim3(1024), 0, st, a, nch, chunk);
}
