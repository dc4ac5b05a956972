// kr_multi.h -- kernels of the exact multi-sequence decode step (kr_multi.hip; host side in kr_decode_multi.cpp, docs/design/13-multi-sequence.md).
// Row b of a pass belongs to sequence slot slots[b] at position positions[b]; every per-slot buffer is [n_slots][per-slot elements].
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kr_slot_image.h"

// linear attention over runs of consecutive tokens per slot (the decode step's kr_la_step_kernel arithmetic per token); a step is runs of one token
struct KrMultiLaArgs {
    const float* qkvz; int ld_qkvz; // in-projection rows [rows][ld_qkvz]
    const float* ba; int ld_ba;     // [rows][ld_ba]
    const float *conv_w, *a_log, *dt_bias, *norm_w;
    float* conv_state; size_t conv_stride;     // slot s: conv_state + s * conv_stride, [conv_dim][4]
    float* recur; size_t recur_stride;         // slot s: recur + s * recur_stride, [nv][dk][dv]
    float* conv_out;                           // scratch [rows][conv_dim]: conv + SiLU outputs
    float* out; int ld_out;                    // [rows][ld_out]: gated RMSNorm output, the out-projection's input
    int nk, nv, dk, dv, hr; float scale, eps;
    // the verify form (docs/design/18-multi-verify.md): rec_x set = no state is stored, and per token row b what a replay of the kept tokens needs is
    // recorded instead: rec_x [rows][conv_dim] the pre-conv channel inputs, rec_k [rows][nk * dk] the normalised keys (once per key head), rec_v
    // [rows][nv * dv], rec_ge / rec_be [rows][nv] e^g and beta.  Null: the run form above
    float *rec_x, *rec_k, *rec_v, *rec_ge, *rec_be;
    // "multi_extend_la_exact" (kr_multi_la_exact.hip, docs/design/36-multi-extend-la-exact.md), a non-verify pass with a run of >= lx_min tokens: the two run
    // kernels leave such a run at once; it takes the staged exact form (KrMultiLxArgs below).  0 (the option is off, a verify pass, or every run is shorter): none
    int lx_min;
    // "multi_extend_la_chunk" (kr_multi_la_chunk.hip, docs/design/26-multi-extend-la-chunk.md), a non-verify pass with a run of >= KR_M_LC_MIN tokens: lc_runs =
    // lc_nruns x [run, first scratch tile], those runs in call order; lc_tiles = lc_ntiles x [run, sub], their sub-chunks of 64 tokens (kr_lc_tiles.h; scratch tile
    // x is tile x); lc_short = the number of shorter runs; lc_scratch = kr_pfm_la_chunk_scratch_floats(64 lc_ntiles, nv) floats; lc_o [rows][nv * dv] = the delta
    // rule's output rows ahead of the gated norm.  The two run kernels leave such a run at once and are not launched when lc_short is 0; the run takes the chunked
    // rule of the KR_ATTN_FAST prompt pass.  Null / 0 (the option is off, a verify pass, or every run is shorter): none of this
    const int* lc_runs; const int* lc_tiles; int lc_nruns, lc_ntiles, lc_short; float* lc_scratch; float* lc_o;
};
#define KR_M_LC_MIN 64      // = LC_T (kr_lac_dev.h) = KR_LC_TOKENS (kr_lc_tiles.h): kr_pfm_la_chunk_ok's rule, C >= LC_T
// a run of cnt tokens takes the chunked rule: not a run of the exact run kernels (workgroup-uniform; false whenever lc_runs is null)
__device__ __forceinline__ bool kr_m_run_chunked(const KrMultiLaArgs& a, int cnt) { return a.lc_runs && cnt >= KR_M_LC_MIN; }
// a run of cnt tokens takes the staged exact form: not a run of the run kernels (workgroup-uniform; false whenever lx_min is 0)
__device__ __forceinline__ bool kr_m_run_staged(const KrMultiLaArgs& a, int cnt) { return a.lx_min && cnt >= a.lx_min; }
// "multi_extend_la_exact": what the staged form needs beside KrMultiLaArgs.  runs = n_runs x [run, first 16-token tile], the runs of >= lx_min tokens in call
// order; t16 = n16 x [run, t0], their tiles of 16 tokens (conv launch); t8 = n8 x [run, t0], those of 8 tokens (gated norm) -- kr_lc_tiles.h builds all three;
// n_short = the other runs of the pass (0: the run kernels are not launched); q / k [rows][nv * dk], v / z / o [rows][nv * dv], gexp / beta [rows][nv]: rows of
// the pass's arena, written and read at the staged runs' rows only (o = the delta rule's output ahead of the gated norm)
struct KrMultiLxArgs { const int* runs; const int* t16; const int* t8; int n_runs, n16, n8, n_short; float *q, *k, *v, *z, *gexp, *beta, *o; };
// runs (device) = n_runs x [slot, off, cnt]: run i's tokens are, in order, rows off .. off + cnt - 2 and then row i of qkvz / ba / conv_out / out (cnt 1:
// row i alone).  The slot's conv and recurrent state are loaded once, carried in registers through the run and stored once.  Slots distinct across runs;
// max_cnt = a bound on every cnt, at most 1024 (the gate rows the recurrence kernel keeps in LDS).
// 0: launched; 1: max_cnt out of range or geometry not covered (kd 4 is the caller's check; dk 64 / 128, dv <= 256, dv % 8 == 0)
// x set ("multi_extend_la_exact", a.lx_min its threshold): the run kernels over the shorter runs (none: not launched), the staged form over the others
int kr_launch_multi_la(const KrMultiLaArgs& a, const int* runs, int n_runs, int max_cnt, hipStream_t st, const KrMultiLxArgs* x = nullptr);
// the pass row of token t < cnt of run i (kernels of kr_multi.hip and kr_multi_sample.hip)
__device__ __forceinline__ int kr_m_run_row(int i, int off, int cnt, int t) { return t == cnt - 1 ? i : off + t; }
// the chunked rule of "multi_extend_la_chunk" (after the exact run kernels, which kr_launch_multi_la skips or lets leave those runs): the geometry test
// (dk = dv = 128, nv = nk hr, 16-byte in-projection rows; the tables present); the LDS windows of the two kernels (once per slot set, outside the pass; non-zero =
// refused); prep over (lc_ntiles, nv), the carried conv inputs of every chunked run, scan over (4 nv, lc_nruns), gated norm over the chunked runs' rows
int kr_multi_lc_ok(int dk, int dv, int nk, int nv, int ld_qkvz);
int kr_multi_lc_prepare();
int kr_launch_multi_la_chunk(const KrMultiLaArgs& a, const int* runs, hipStream_t st);
// the staged exact form of "multi_extend_la_exact" (kr_multi_la_exact.hip): the geometry test (kr_launch_pfm_la's: dk 64 / 128, dk <= dv <= 256, dv % 8 == 0,
// 16-byte in-projection rows, nv = nk hr); what the launcher checks of its arguments, asked before anything of the layer is queued; conv over (nk, n16), the
// carried conv inputs over (channels, n_runs), the delta rule over (nv, n_runs), the gated norm over (nv, n8).  0: launched; 1: something not covered
int kr_multi_lx_ok(int dk, int dv, int nk, int nv, int ld_qkvz);
int kr_multi_lx_args_ok(const KrMultiLaArgs& a, const KrMultiLxArgs& x);
int kr_launch_multi_la_exact(const KrMultiLaArgs& a, const KrMultiLxArgs& x, const int* runs, hipStream_t st);

// commit of a verify pass (docs/design/18-multi-verify.md): one linear-attention layer's slot states and the records its verify-form launch left.  A table
// of these lives on the device (kr_multi_state::v_tab)
struct KrMultiLaCommit {
    float* conv_state; size_t conv_stride;     // as KrMultiLaArgs
    float* recur; size_t recur_stride;
    const float *rec_x, *rec_k, *rec_v, *rec_ge, *rec_be;
    int nk, nv, dk, dv, hr;
};
// every slot of runs[0 .. n_runs) advanced by the first n_keep[i] tokens of its run (0: untouched), from the records; runs as above, n_keep on the device.
// One launch per key width present; grid (nv_max, n_runs, n_la) x dv_max threads: the caller has checked dk in {64, 128} and dv <= 256 for every layer
void kr_launch_multi_la_commit(const KrMultiLaCommit* tab, int n_la, bool has64, bool has128, int nv_max, int dv_max, const int* runs, const int* n_keep,
                               int n_runs, hipStream_t st);

// GQA, one token per row: QK-norm + RoPE at the row's position, K / V appended to the row's slot, attention over the slot's rows [0, pos]
struct KrMultiGqaArgs {
    const int* slots; const int* positions;    // [B] device
    const float *q_in, *k_in, *v_in; int ld_q, ld_k, ld_v;
    const float *q_norm, *k_norm; int q_norm_per_head, k_norm_per_head;
    const float *rope_cos, *rope_sin; int rope_half;
    void *k_cache, *v_cache; size_t slot_elems; int kv_fp8;   // slot s: cache + s * slot_elems elements, [max_seq][nkv * hd]
    float *q_out, *gate, *attn_out;            // [B][nh * hd]
    float* scores; int sc_ld;                  // scratch [B][nh][sc_ld], sc_ld >= the longest row's pos + 1 rounded up to 32
    // "multi_attn_exact_split" (kr_multi_split.hip, docs/design/30-multi-attn-exact-split.md): non-zero = wherever a launcher below would launch the exact per-slot
    // attention kernel it launches the scores / softmax / P.V kernels of kr_launch_multi_gqa_split over the same rows instead -- the same bits, the same checks
    // first.  0 (the option is off, or the pass is below "multi_attn_exact_split_min"): the one kernel, as ever
    int xs_split;
    int gated, nh, nkv, hd; float eps, sm_scale;
    // "multi_attn_fast" (kr_multi_flash.hip): split-KV partials [B][nkv][fd_chunks][G][hd] and (max, sum) [B][nh][fd_chunks][2]; fd_chunk positions per
    // chunk, fd_chunks = the longest row's chunk count.  Null: the exact per-slot kernel (scores is not read when they are set).  With page_table set
    // ("multi_attn_fast_paged", docs/design/23-multi-attn-fast-paged.md) the chunk pass reads the pools through the table
    float *fd_o, *fd_ml; int fd_chunk, fd_chunks;
    // paged slots (docs/design/21-paged-slots.md): page_table [n_slots][page_stride] on the device, -1 = unmapped; k_cache / v_cache are then pools
    // [n_pages][1 << page_shift][nkv * hd] and position s of slot b is row (page_table[b][s >> page_shift] << page_shift) | (s & mask).  Null: flat slots
    const int* page_table; int page_stride, page_shift;
    // "multi_extend_flash" (kr_multi_pf_flash.hip, docs/design/25-multi-extend-flash.md), a pass with a run of >= 2 tokens: pf_runs = the pass's run table,
    // pf_nruns x [slot, off, cnt] (above); pf_tiles = pf_ntiles x [run, t0], the query tiles of the runs of >= 2 tokens (kr_pf_tiles.h); pf_units = the number
    // of runs of one token.  The prep launch covers all B rows; the per-row attention kernels above run over the first pf_nruns rows and leave those of a run
    // of >= 2 at once (scores / fd_o / fd_ml are then sized by pf_nruns rows); the runs take causal flash attention over their slots.  Null (the option is
    // off, or every run has one token): none of this, B rows through the per-row kernels
    const int* pf_runs; const int* pf_tiles; int pf_nruns, pf_ntiles, pf_units;
};
// row b < pf_nruns is the last token of a run of >= 2 tokens: not a row of the per-row attention kernels (workgroup-uniform; false whenever pf_runs is null)
__device__ __forceinline__ bool kr_m_row_in_run(const KrMultiGqaArgs& a, int b) { return a.pf_runs && a.pf_runs[3 * b + 2] >= 2; }
// 0: launched; 1: geometry not covered (hd 64 / 128 / 256, nh % nkv == 0), or the dynamic LDS below is over KR_MULTI_GQA_LDS_MAX
int kr_launch_multi_gqa(const KrMultiGqaArgs& a, int B, hipStream_t st);
// "multi_attn_exact_split": the three launches over the first `rows` rows of the pass (after the prep launch), in place of the exact per-slot attention kernel over
// those rows; the rows of runs of >= 2 tokens leave at once as they do there.  0: launched; 1: geometry not covered (what kr_launch_multi_gqa checks)
int kr_launch_multi_gqa_split(const KrMultiGqaArgs& a, int rows, hipStream_t st);
// the run kernels of "multi_extend_flash" (after the prep launch): the geometry test is kr_pfm_gqa_flash_ok's (kr_prefill_ops.h); the LDS window of the kernel a
// layer takes (once per slot set, outside the pass; non-zero = refused; every instantiation is a kernel of its own); grid (a.pf_ntiles, nkv)
int kr_multi_pf_args_ok(const KrMultiGqaArgs& a);      // what kr_launch_multi_pf_flash checks: asked before anything of the layer is queued
int kr_multi_pf_prepare(int hd, int fp8, int paged);
int kr_launch_multi_pf_flash(const KrMultiGqaArgs& a, hipStream_t st);
// "multi_extend_exact_mfma" (kr_multi_xm.hip, docs/design/28-multi-extend-exact-mfma.md), a non-verify pass with a run of >= 2 tokens: those runs take the three
// exact passes of the single-sequence prompt pass over their slots -- scores and P.V on the f32 matrix cores, the exact softmax between them --, bit for bit what
// the per-row kernel gives every token.  What the passes need beside KrMultiGqaArgs travels here (that struct does not grow): tiles_a = n_a x [run, t0], the query
// tiles of 64 / G tokens of the runs of >= 2 (pass A), tiles_c = n_c x [run, t0], those of 32 / G tokens (pass C; kr_pf_tiles.h builds both); inv [B * nh] and tmax
// [B * nh][sc_ld / 32], the softmax's 1 / sum and pass A's row maxima per 32 positions; kv_end = one past the largest position a run of >= 2 reads
struct KrMultiXmArgs { const int* tiles_a; const int* tiles_c; int n_a, n_c; float* inv; float* tmax; int kv_end; };
// the whole GQA section of such a pass: every check, the prep launch over all B rows, the per-row kernels -- the exact one, or the flash-decode pair when a.fd_o is
// set -- over the first n_runs rows when units > 0 (the rows of longer runs leave at once), then passes A, B and C.  runs = the pass's run table, n_runs x [slot,
// off, cnt]; units = its runs of one token; a.pf_* as the caller left them (null / 0): the launcher sets them on its copy.  a.scores covers all B rows at a.sc_ld, a
// multiple of 64 above the pass's largest position.  0: launched; 1: something not covered, nothing queued
int kr_launch_multi_gqa_xm(const KrMultiGqaArgs& a, const KrMultiXmArgs& x, const int* runs, int n_runs, int units, int B, hipStream_t st);
int kr_multi_xm_args_ok(const KrMultiGqaArgs& a, const KrMultiXmArgs& x);      // what kr_launch_multi_xm checks (a.pf_runs set, a.pf_tiles null)
int kr_launch_multi_xm(const KrMultiGqaArgs& a, const KrMultiXmArgs& x, int B, hipStream_t st);      // passes A, B, C alone (after the prep launch)
void kr_launch_multi_xm_softmax(const KrMultiGqaArgs& a, const KrMultiXmArgs& x, int B, hipStream_t st);      // pass B alone: what kr_launch_multi_xm launches second
void kr_launch_multi_xm_pv(const KrMultiGqaArgs& a, const KrMultiXmArgs& x, hipStream_t st);                  // pass C alone (hd 64 / 128 / 256): what it launches third
// dynamic LDS of kr_multi_gqa_attn_kernel in bytes: the G = nh / nkv query rows, four softmax tiles, the P.V tile and, on paged slots, the slot's page-table
// row of page_stride entries (0: flat).  The launcher and kr_decode_slots_create_paged both ask here, so a slot set that is created can be stepped
#define KR_MULTI_GQA_LDS_MAX (64 * 1024)
size_t kr_multi_gqa_lds_bytes(int G, int hd, int page_stride);
// the flash-decode form of the attention launch (after the prep launch): geometry test, the LDS window of its kernel (once, outside the step; non-zero =
// refused; the paged instantiations are kernels of their own), the chunk pass + merge over n_chunks chunks (0: launched; a.page_table set: through the table)
int kr_multi_fd_ok(int nh, int nkv, int hd);
int kr_multi_fd_prepare(int hd, int fp8, int paged);
int kr_launch_multi_fd(const KrMultiGqaArgs& a, int B, int n_chunks, hipStream_t st);

// MLA, one token per row: rope of q_pe, latent RMSNorm + rope of k_pe, both rows appended to the row's slot, attention over the slot's rows [0, pos]
// in the latent space, w_kc absorption before and w_vc projection after (the row-wise launches of the prompt pass)
struct KrMultiMlaArgs {
    const int* slots; const int* positions;    // [B] device
    const float* kv_out; int ld_kv;            // kv_a projection rows [B][ld_kv], [klr | rd] each
    const float* q_full; int ld_q;             // q (or q_b) projection rows [B][ld_q], per head [nd | rd]
    const float *kv_a_norm, *w_kc, *w_vc, *rope_cos, *rope_sin;
    void *ckv_cache, *kpe_cache; size_t ckv_stride, kpe_stride; int kv_fp8;   // slot s: cache + s * stride BYTES, [max_seq][klr] / [max_seq][rd], FP16 or E4M3
    float *q_abs, *q_pe, *attn_lat, *v_proj;   // [B][nh * klr], [B][nh * rd], [B][nh * klr], [B][nh * vhd]
    float* scores; int sc_ld;                  // scratch [B][nh][sc_ld], sc_ld >= the longest row's pos + 1 rounded up to 32
    int nh, klr, nd, rd, vhd; float eps, sm_scale;
    int absorb_done;                           // set by the launch: q_abs came from the matrix-core absorption, the prep launch skips its tiles
    // "multi_mla_exact_split" (kr_multi_mla_split.hip, docs/design/31-multi-mla-exact-split.md): non-zero = wherever a launcher below would launch the exact per-slot
    // attention kernel it launches the scores / softmax / weighted-sum kernels of kr_launch_multi_mla_split over the same rows instead -- the same bits, the same
    // checks first.  0 (the option is off, or the pass is below "multi_mla_exact_split_min"): the one kernel, as ever
    int xs_split;
    // paged slots, as KrMultiGqaArgs: ckv_cache / kpe_cache are pools [n_pages][1 << page_shift][klr] / [..][rd]; a stage of KR_MM_ROWS rows lies in one page
    const int* page_table; int page_stride, page_shift;
    // "multi_mla_fast" (kr_multi_mla_flash.hip, docs/design/24-multi-mla-fast.md): split-KV partials [B][fd_chunks][nh][klr] and (max, sum) [B][nh][fd_chunks][2];
    // fd_chunk positions per chunk, fd_chunks = the longest row's chunk count.  Null: the exact per-slot kernel (scores is not read when they are set).  With
    // page_table set the chunk pass reads the pools through the table
    float *fd_o, *fd_ml; int fd_chunk, fd_chunks;
    // "multi_extend_mla_flash" (kr_multi_mla_pf_flash.hip, docs/design/27-multi-extend-mla-flash.md), a non-verify pass with a run of >= 2 tokens: mf_runs = the
    // pass's run table, mf_nruns x [slot, off, cnt] (above); mf_tiles = mf_ntiles x [run, tile_row], the tiles of 64 (token, head) query rows of the runs of >= 2
    // tokens for this layer's head count (kr_mf_tiles.h); mf_units = the number of runs of one token.  The absorption, the prep launch and the w_vc projection
    // cover all B rows; the per-row attention kernels run over the first mf_nruns rows and leave those of a run of >= 2 at once (scores / fd_o / fd_ml are then
    // sized by mf_nruns rows), and are not launched when mf_units is 0; the runs take causal flash attention over their slots.  Null / 0 (the option is off, a
    // verify pass, or every run has one token): none of this, B rows through the per-row kernels
    const int* mf_runs; const int* mf_tiles; int mf_nruns, mf_ntiles, mf_units;
};
// row b < mf_nruns is the last token of a run of >= 2 tokens: not a row of the per-row MLA attention kernels (workgroup-uniform; false whenever mf_runs is null)
__device__ __forceinline__ bool kr_m_row_in_run(const KrMultiMlaArgs& a, int b) { return a.mf_runs && a.mf_runs[3 * b + 2] >= 2; }
// the geometries the per-slot MLA kernels are specialised for (klr 512 / 256 with rd 64; nd within the prep launch's LDS row)
int kr_multi_mla_ok(int klr, int nd, int rd);
// 0: launched (absorption, prep, attention -- the flash-decode pair when a.fd_o is set --, w_vc projection); 1: geometry not covered
int kr_launch_multi_mla(const KrMultiMlaArgs& a, int B, hipStream_t st);
// "multi_mla_exact_split": the three launches over the first `rows` rows of the pass (after the prep launch, ahead of the w_vc projection), in place of the exact
// per-slot attention kernel over those rows; the rows of runs of >= 2 tokens leave at once as they do there.  0: launched; 1: geometry not covered (what
// kr_launch_multi_mla checks)
int kr_launch_multi_mla_split(const KrMultiMlaArgs& a, int rows, hipStream_t st);
// the flash-decode form of the attention launch (after the prep launch): geometry test (at most 64 heads = one query tile), the LDS window of its kernel
// (once per slot set, outside the pass; non-zero = refused; every instantiation is a kernel of its own), the chunk pass + merge over a.fd_chunks chunks
// (0: launched; a.page_table set: through the table)
int kr_multi_mla_fd_ok(int nh, int klr, int rd);
int kr_multi_mla_fd_prepare(int klr, int fp8, int paged);
int kr_launch_multi_mla_fd(const KrMultiMlaArgs& a, int B, hipStream_t st);
// the run kernel of "multi_extend_mla_flash" (after the prep launch): the geometry test is kr_launch_mla_flash's (kv_lora_rank 512 / 256, rope 64, any head
// count); the LDS window of the kernel a layer takes (once per slot set, outside the pass; non-zero = refused; every instantiation is a kernel of its own);
// grid (a.mf_ntiles)
int kr_multi_mla_pf_args_ok(const KrMultiMlaArgs& a);      // what kr_launch_multi_mla_pf_flash checks: asked before anything of the layer is queued
int kr_multi_mla_pf_prepare(int klr, int fp8, int paged);
int kr_launch_multi_mla_pf_flash(const KrMultiMlaArgs& a, hipStream_t st);
// "multi_extend_mla_exact_mfma" (kr_multi_mla_xm.hip, docs/design/29-multi-extend-mla-exact-mfma.md), a non-verify pass with a run of >= 2 tokens: those runs take
// the three exact passes of the single-sequence MLA prompt pass over their slots -- scores (rope dot, then latent dot) and P.V on the f32 matrix cores, the exact
// softmax between them --, bit for bit what the per-row kernel gives every token.  KrMultiXmArgs as above, at the tile widths 64 / nh (tiles_a) and 32 / nh
// (tiles_c); neither struct grows.
// The whole MLA section of such a pass: every check, the absorption, the prep launch over all B rows, the per-row kernels -- the exact one, or the flash-decode
// pair when a.fd_o is set -- over the first n_runs rows when units > 0 (the rows of longer runs leave at once), passes A (two launches), B and C, the w_vc
// projection over all B rows.  runs = the pass's run table, n_runs x [slot, off, cnt]; units = its runs of one token; a.mf_* as the caller left them (null / 0):
// the launcher sets mf_runs / mf_nruns / mf_units on its copy, mf_tiles stays null.  a.scores covers all B rows at a.sc_ld, a multiple of 64 above the pass's
// largest position.  0: launched; 1: something not covered, nothing queued
int kr_launch_multi_mla_xm(const KrMultiMlaArgs& a, const KrMultiXmArgs& x, const int* runs, int n_runs, int units, int B, hipStream_t st);
int kr_multi_mla_xm_args_ok(const KrMultiMlaArgs& a, const KrMultiXmArgs& x);      // what kr_launch_multi_mla_xm_attn checks (a.mf_runs set, a.mf_tiles null)
int kr_launch_multi_mla_xm_attn(const KrMultiMlaArgs& a, const KrMultiXmArgs& x, int B, hipStream_t st);      // passes A, B, C alone (after the prep launch)

// paged slots: the pools of every layer, and the launch that makes freshly mapped pages read as zero in all of them -- grid (n_pages, n_pools), one launch per pass
#define KR_PAGE_MIN_TOKENS 32      // = KR_MM_ROWS (kr_multi.hip): a stage of the MLA attention kernel never straddles a page
struct KrPagePoolDev { void* base; size_t page_bytes; };
void kr_launch_multi_zero_pages(const KrPagePoolDev* pools, int n_pools, const int* pages, int n_pages, hipStream_t st);
// shared pages (docs/design/22-slot-fork.md): in every pool, copy c = the first rows[c] rows of page src_pages[c] into page dst_pages[c] and zeroes behind them,
// a row being page_bytes / page_tokens bytes -- grid (n_copies, n_pools), one launch.  Also the per-slot linear-attention state of a fork: pools whose "page" is
// a slot, page_tokens 1, rows 1
void kr_launch_multi_copy_pages(const KrPagePoolDev* pools, int n_pools, const int* dst_pages, const int* src_pages, const int* rows, int n_copies, int page_tokens, hipStream_t st);
// slot export / import (kr_multi_swap.hip, docs/design/38-slot-swap.md): one staged byte range of slot images <-> the slots' buffers, one workgroup per piece
// (kr_slot_image.h builds the pieces: pool = an entry of `pools`, whose "page" is a page of a paged GQA / MLA pool and a slot of every other buffer).  pack: the
// pieces' bytes -> stage + range_off, a piece of page -1 as zeroes; unpack: stage + range_off -> the pieces' bytes, nothing else written.  pools, pieces and
// stage on the device; the host keeps every piece inside its page and the staged range
void kr_launch_multi_pack(const KrPagePoolDev* pools, const KrSlotPiece* pieces, int n_pieces, void* stage, hipStream_t st);
void kr_launch_multi_unpack(const KrPagePoolDev* pools, const KrSlotPiece* pieces, int n_pieces, const void* stage, hipStream_t st);

// per row b < B of logits [B][ld]: out[b] = first-maximum argmax of the row's first V values (kr_argmax_kernel's rule)
void kr_launch_multi_argmax(const float* logits, size_t ld, int V, int B, int* out, hipStream_t st);
// accept of a verify pass: ids [rows] = the greedy id of every pass row, tokens [rows] = the token each row consumed.  out[0 .. T) = the ids in caller order
// (the runs concatenated), out[T + i] = n_match of run i: the number of leading draft tokens (tokens 1 .. of the run) that equal the id of the row before
void kr_launch_multi_accept(const int* ids, const int* tokens, const int* runs, int n_runs, int T, int* out, hipStream_t st);
