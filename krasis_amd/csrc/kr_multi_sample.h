// kr_multi_sample.h -- the batched sampler of the multi-sequence step (kr_multi_sample.hip; host side in kr_decode_multi.cpp,
// docs/design/14-multi-sampling.md).  Row b of a step draws with the sampler of slot rows[b].slot: its parameters, seen-token bitmap and
// xorshift64 state; every row's token equals what kr_launch_sample (or the greedy / penalised-greedy path of kr_decode_generate) gives on that row.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

// what a row does (the three paths of kr_decode_generate's loop; SAMPLE and LOOP are the same draw by two implementations)
enum { KR_MS_GREEDY = 0,   // first maximum of the model's logits (kr_decode_step_multi's id)
       KR_MS_PENALTY = 1,  // temperature 0 with a presence penalty: penalise the seen tokens, first maximum, mark it seen
       KR_MS_SAMPLE = 2,   // the batched draw: penalty, 1 / temperature, top-k (k <= KR_MS_SEL_CAP) by radix select, top-p, xorshift64
       KR_MS_LOOP = 3 };   // the same draw by kr_launch_sample on this row alone (k > KR_MS_SEL_CAP, or the "multi_sample_loop" option)
#define KR_MS_SEL_CAP 4096
struct KrMsRow {
    int mode, slot;        // slot: index of the row's seen bitmap and xorshift64 state
    int k, top_k;          // k = the candidates drawn from (top_k > 0 && top_k < vocab ? top_k : vocab); top_k as given (LOOP)
    float temperature, inv_temp, top_p, penalty;   // inv_temp = 1.0f / temperature, computed on the host as kr_launch_sample does
};
// the verify form (docs/design/19-multi-verify-sample.md): pass row b is token t of run `run` of a verify pass.  It draws as its slot's sampler would after
// t earlier draws that were the run's tokens 1 .. t: those tokens count as seen, the xorshift64 state is advanced t times more
struct KrMsAt { int run, t; };
struct KrMsArgs {
    const float* logits; size_t ld; int V, B;      // the model's logits [B][ld] (read only)
    const KrMsRow* rows_dev; const KrMsRow* rows_host;   // [B], the same rows on the device and on the host
    float* work;                                   // [B][V]: the prepared rows (penalty, temperature; LOOP rows: the raw logits, prepared in place)
    uint64_t* sorted;                              // [B][KR_MS_SEL_CAP]: SAMPLE rows' top-k keys, descending
    uint32_t* seen; size_t seen_words;             // slot s: seen + s * seen_words ((vocab + 31) / 32 words)
    uint64_t* rng;                                 // slot s: rng[s]
    int* ids;                                      // [B] the drawn / greedy ids
    uint64_t* loop_keys; void* loop_temp; size_t loop_temp_bytes; float* loop_probs;   // LOOP rows: kr_launch_sample's scratch (keys [2][V], rocPRIM temp, probs [V])
    // the verify form (runs set; null: a step).  B = the T token rows of the pass, rows / at per pass row, ids per pass row; seen and rng are read only
    const int* runs; const int* tokens;            // device: the pass's run table [n][slot, off, cnt] and the token each pass row consumed [B] (kr_multi.h)
    const KrMsAt* at_dev; const KrMsAt* at_host;   // [B], the same on the device and on the host
    uint32_t* hyp_seen; uint64_t* hyp_rng;         // LOOP rows: one staged bitmap [seen_words] and state, reused row after row in stream order
};
// all B rows, in stream order; returns non-zero on a launch or sort failure
int kr_launch_multi_sample(const KrMsArgs& a, hipStream_t st);
// commit of a verify-form call: run i's slot sampler advanced by its first n_keep[i] draws (ids [T] as that call left them; rows [>= n_runs], row i = run i's)
void kr_launch_ms_commit(const KrMsRow* rows, const int* runs, const int* n_keep, int n_runs, const int* ids, int V, uint32_t* seen, size_t seen_words,
                         uint64_t* rng, hipStream_t st);
