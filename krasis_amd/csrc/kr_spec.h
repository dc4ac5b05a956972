// kr_spec.h -- kernels of exact speculative greedy decoding (kr_spec.hip; host side in kr_decode_prefill.cpp, docs/design/12-speculative.md)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// one linear-attention layer as the verify pass sees it: the live states, their snapshot from before the pass, and what the pass fed the recurrence
// (rows [0, n) of buffers sized for KR_VERIFY_MAX tokens).  A table of these lives on the device (kr_decode_store::spec_tab).
struct KrSpecLa {
    float* recur; float* conv;                  // live recurrent state [nv][dk][dv], carried conv slots [conv_dim][4]
    float* snap_recur; float* snap_conv;        // the same before the verify pass
    const float* qkvz;                          // in-projection rows [n][ld_qkvz]: the pre-conv channel inputs
    const float* k; const float* v;             // [n][nv*dk], [n][nv*dv]: normalised keys and values as the recurrence read them
    const float* gexp; const float* beta;       // [n][nv]
    int nk, nv, dk, dv, hr, ld_qkvz;
};
// live -> snapshot for every layer of the table, one launch
void kr_launch_spec_snapshot(const KrSpecLa* tab, int n_la, int max_floats, hipStream_t st);
// live = snapshot advanced by tokens [0, n_keep) (n_keep = 0: the snapshot itself).  One launch per key-head width present (has64 / has128);
// grid (nv_max, n_la) x dv_max threads: the caller has checked dk in {64, 128} and dv <= 256 for every layer.
void kr_launch_spec_rollback(const KrSpecLa* tab, int n_la, bool has64, bool has128, int nv_max, int dv_max, int n_keep, hipStream_t st);
// per row r < n of logits [n][ld]: first-maximum argmax (kr_argmax_kernel's rule); the last workgroup writes out[0..n) = the ids, out[n] = the
// number of leading drafts tokens[1..] that equal the preceding row's id.  part: 2 * KR_VERIFY_MAX words; counter: one word, zero between launches.
void kr_launch_spec_accept(const float* logits, size_t ld, int V, int n, const int* tokens, int* out, float* part, unsigned* counter, hipStream_t st);
