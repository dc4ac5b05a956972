// kr_multi_sample.hip -- sample_from_logits (src/decode.rs:3718-3811) for the B rows of a multi-sequence step in one launch sequence
// (docs/design/14-multi-sampling.md).  The arithmetic specification is the single-row sampler (kr_sampler.hip): each row takes the same
// operations in the same order, so its token, xorshift64 state and seen bitmap are the ones kr_launch_sample / kr_decode_generate give it alone.
//   prepare  grid (V / 256, B): work row = penalty on the slot's seen tokens, *= 1 / temperature (penalised greedy rows: the penalty only)
//   select   grid B, 1024 threads: top-k of the (value, ~index) keys by radix select + LDS bitonic sort (kr_sample_select_kernel), keys computed
//            from the prepared f32 row; per-wave histograms (counts do not depend on the order the keys are counted in)
//   draw     grid B, 256 threads: kr_sample_draw_kernel on the slot's xorshift64 state and seen bitmap
//   argmax   grid B, 1024 threads: greedy rows (first maximum of the model's logits) and penalised greedy rows (of the work row; marks it seen)
// Rows that draw from more than KR_MS_SEL_CAP candidates run kr_launch_sample on their work row, one row after another.
// The verify form (docs/design/19-multi-verify-sample.md) draws the T token rows of a verify pass: row (run i, token t) under the hypothesis that the run's
// tokens 1 .. t were the slot's t draws before it -- those tokens count as seen, the xorshift64 state is the slot's advanced t times more -- and writes no
// sampler state; kr_ms_commit_kernel applies the kept draws.  Each step kernel and its verify-form sibling share one body (the RUN flag).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/krasis_hip.h"
#include "kr_libm.h"
#include "kr_multi.h"
#include "kr_multi_sample.h"
#include "kr_sample_dev.h"
#include "kr_sampler.h"

#define KR_MS_WAVES 16     // waves of the 1024-thread select workgroup

// RUN: row blockIdx.y is token at.t of run at.run; the run's tokens 1 .. t (at most KR_VERIFY_MAX - 1, read once per workgroup into LDS) count as seen.
// Bounds: t < cnt <= KR_VERIFY_MAX (the host's check), so kr_m_run_row(run, off, cnt, j), 1 <= j <= t, is one of the run's own pass rows (< T, the length
// of `tokens`).  The barrier is reached by the whole workgroup: mode and t depend on the row alone
template <bool RUN>
__device__ __forceinline__ void kr_ms_prepare_body(const float* __restrict__ logits, size_t ld, int V, const KrMsRow* __restrict__ rows,
                                                   const uint32_t* __restrict__ seen, size_t seen_words, float* __restrict__ work,
                                                   const KrMsAt* __restrict__ at, const int* __restrict__ runs, const int* __restrict__ tokens) {
    __shared__ int pre[RUN ? KR_VERIFY_MAX : 1];
    const KrMsRow r = rows[blockIdx.y];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    int n_pre = 0;
    if constexpr (RUN) {
        if (r.mode == KR_MS_GREEDY) return;
        if (r.mode != KR_MS_LOOP && r.penalty != 0.0f) {
            const KrMsAt a = at[blockIdx.y];
            n_pre = a.t;
            if ((int)threadIdx.x < n_pre) pre[threadIdx.x] = tokens[kr_m_run_row(a.run, runs[3 * a.run + 1], runs[3 * a.run + 2], (int)threadIdx.x + 1)];
        }
        __syncthreads();
    }
    if (r.mode == KR_MS_GREEDY || i >= V) return;
    float v = logits[(size_t)blockIdx.y * ld + i];
    if (r.mode != KR_MS_LOOP) {            // LOOP rows: kr_launch_sample prepares its row in place
        if (r.penalty != 0.0f) {
            bool hit = (seen[(size_t)r.slot * seen_words + (i >> 5)] >> (i & 31)) & 1u;
            if constexpr (RUN) for (int j = 0; j < n_pre; j++) hit |= pre[j] == i;      // once, however often a token repeats
            if (hit) v -= r.penalty;
        }
        if (r.mode == KR_MS_SAMPLE) v *= r.inv_temp;
    }
    work[(size_t)blockIdx.y * V + i] = v;
}
__global__ void __launch_bounds__(256) kr_ms_prepare_kernel(const float* __restrict__ logits, size_t ld, int V, const KrMsRow* __restrict__ rows,
                                                            const uint32_t* __restrict__ seen, size_t seen_words, float* __restrict__ work) {
    kr_ms_prepare_body<false>(logits, ld, V, rows, seen, seen_words, work, nullptr, nullptr, nullptr);
}
__global__ void __launch_bounds__(256) kr_ms_prepare_run_kernel(const float* __restrict__ logits, size_t ld, int V, const KrMsRow* __restrict__ rows,
                                                                const uint32_t* __restrict__ seen, size_t seen_words, float* __restrict__ work,
                                                                const KrMsAt* __restrict__ at, const int* __restrict__ runs, const int* __restrict__ tokens) {
    kr_ms_prepare_body<true>(logits, ld, V, rows, seen, seen_words, work, at, runs, tokens);
}

// kr_sample_select_kernel on row b's prepared values: the k-th largest key by radix select (most significant byte first), then the keys >= it
// (exactly k: the keys are unique) gathered into LDS and sorted descending.  The histograms are per wave and summed before the bucket walk.
__global__ void __launch_bounds__(1024) kr_ms_select_kernel(const float* __restrict__ work, int V, const KrMsRow* __restrict__ rows,
                                                            uint64_t* __restrict__ sorted) {
    __shared__ uint32_t hist[KR_MS_WAVES][256];
    __shared__ uint64_t cand[KR_MS_SEL_CAP];
    __shared__ uint32_t s_digit, s_above, s_count;
    const KrMsRow r = rows[blockIdx.x];
    if (r.mode != KR_MS_SAMPLE) return;
    const float* row = work + (size_t)blockIdx.x * V;
    const int t = threadIdx.x, w = t >> 6, k = r.k;
    uint64_t prefix = 0; int krem = k;
    for (int p = 7; p >= 0; p--) {
        for (int j = t; j < KR_MS_WAVES * 256; j += 1024) hist[j >> 8][j & 255] = 0;
        __syncthreads();
        const uint64_t himask = p == 7 ? 0ull : (~0ull << (8 * (p + 1)));
        for (int i = t; i < V; i += 1024) { const uint64_t key = kr_sample_key(row[i], i); if ((key & himask) == prefix) atomicAdd(&hist[w][(uint32_t)(key >> (8 * p)) & 255u], 1u); }
        __syncthreads();
        if (t < 256) { uint32_t c = 0; for (int j = 0; j < KR_MS_WAVES; j++) c += hist[j][t]; hist[0][t] = c; }   // thread t owns column t
        __syncthreads();
        if (t < 64) {      // lane l owns digits 255 - 4 l .. 252 - 4 l; counts from the top
            uint32_t c[4], sum = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) { c[j] = hist[0][255 - 4 * t - j]; sum += c[j]; }
            uint32_t incl = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(incl, o); if (t >= o) incl += y; }
            uint32_t above = incl - sum;          // keys in buckets above this lane's
            if (above < (uint32_t)krem && (uint32_t)krem <= incl) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    if ((uint32_t)krem <= above + c[j]) { s_digit = 255 - 4 * t - j; s_above = above; s_count = c[j]; break; }
                    above += c[j];
                }
            }
        }
        __syncthreads();
        prefix |= (uint64_t)s_digit << (8 * p); krem -= (int)s_above;
        const bool all_needed = (int)s_count == krem;
        __syncthreads();
        if (all_needed) break;          // every key of this bucket is taken: the lower bytes cannot matter
    }
    if (t == 0) s_count = 0;
    __syncthreads();
    for (int i = t; i < V; i += 1024) {
        const uint64_t key = kr_sample_key(row[i], i);
        if (key >= prefix) { const uint32_t pos = atomicAdd(&s_count, 1u); if (pos < KR_MS_SEL_CAP) cand[pos] = key; }
    }
    __syncthreads();
    int P = 1; while (P < k) P <<= 1;
    for (int i = k + t; i < P; i += 1024) cand[i] = 0;       // padding sorts last (no real key is 0)
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = t; i < (P >> 1); i += 1024) {
                const int lo = 2 * stride * (i / stride) + (i % stride), hi = lo + stride;
                const bool desc = (lo & size) == 0;
                const uint64_t a = cand[lo], b = cand[hi];
                if ((a < b) == desc) { cand[lo] = b; cand[hi] = a; }
            }
            __syncthreads();
        }
    uint64_t* out = sorted + (size_t)blockIdx.x * KR_MS_SEL_CAP;
    for (int i = t; i < k; i += 1024) out[i] = cand[i];
}

// kr_sample_draw_kernel on row b: exps in parallel, every sum on lane 0 in sorted order, the slot's xorshift64 state and seen bitmap.  RUN: the state is
// the slot's after the at.t earlier draws of the run, neither stored nor the token marked
template <bool RUN>
__device__ __forceinline__ void kr_ms_draw_body(const uint64_t* __restrict__ sorted_all, const float* __restrict__ work, int V,
                                                const KrMsRow* __restrict__ rows, uint64_t* __restrict__ rng, uint32_t* __restrict__ seen,
                                                size_t seen_words, int* __restrict__ ids, const KrMsAt* __restrict__ at) {
    __shared__ float probs[KR_MS_SEL_CAP];
    __shared__ float s_inv;
    const KrMsRow r = rows[blockIdx.x];
    if (r.mode != KR_MS_SAMPLE) return;
    const uint64_t* sorted = sorted_all + (size_t)blockIdx.x * KR_MS_SEL_CAP;
    const float* logits = work + (size_t)blockIdx.x * V;
    const int t = threadIdx.x, k = r.k;
    const float top_p = r.top_p;
    const int i0 = (int)(0xFFFFFFFFu - (uint32_t)sorted[0]);
    const float mx = logits[i0];
    for (int i = t; i < k; i += 256) { const int idx = (int)(0xFFFFFFFFu - (uint32_t)sorted[i]); probs[i] = kr_expf(logits[idx] - mx); }
    __syncthreads();
    if (t == 0) {
        float sum = 0.0f;
        for (int i = 0; i < k; i++) sum += probs[i];
        s_inv = 1.0f / sum;
    }
    __syncthreads();
    const float inv_sum = s_inv;
    for (int i = t; i < k; i += 256) probs[i] *= inv_sum;
    __syncthreads();
    if (t != 0) return;
    int cutoff = k;
    if (top_p < 1.0f) {
        float cum = 0.0f;
        for (int i = 0; i < k; i++) { cum += probs[i]; if (cum >= top_p) { cutoff = i + 1; break; } }
    }
    if (cutoff < k) {
        float ns = 0.0f;
        for (int i = 0; i < cutoff; i++) ns += probs[i];
        const float inv_ns = 1.0f / ns;
        for (int i = 0; i < cutoff; i++) probs[i] *= inv_ns;
    }
    uint64_t x = rng[r.slot];
    if constexpr (RUN) for (int j = at[blockIdx.x].t; j > 0; j--) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; }
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    if constexpr (!RUN) rng[r.slot] = x;
    const float rr = (float)((double)x / 18446744073709551615.0);
    int pick = -1; float cum = 0.0f;
    for (int i = 0; i < cutoff; i++) { cum += probs[i]; if (rr < cum) { pick = i; break; } }
    if (pick < 0) pick = cutoff - 1;
    const int tok = (int)(0xFFFFFFFFu - (uint32_t)sorted[pick]);
    ids[blockIdx.x] = tok;
    if constexpr (!RUN) if ((unsigned)tok < (unsigned)V) atomicOr(&seen[(size_t)r.slot * seen_words + (tok >> 5)], 1u << (tok & 31));
}
__global__ void __launch_bounds__(256) kr_ms_draw_kernel(const uint64_t* __restrict__ sorted_all, const float* __restrict__ work, int V,
                                                         const KrMsRow* __restrict__ rows, uint64_t* __restrict__ rng, uint32_t* __restrict__ seen,
                                                         size_t seen_words, int* __restrict__ ids) {
    kr_ms_draw_body<false>(sorted_all, work, V, rows, rng, seen, seen_words, ids, nullptr);
}
__global__ void __launch_bounds__(256) kr_ms_draw_run_kernel(const uint64_t* __restrict__ sorted_all, const float* __restrict__ work, int V,
                                                             const KrMsRow* __restrict__ rows, uint64_t* __restrict__ rng, int* __restrict__ ids,
                                                             const KrMsAt* __restrict__ at) {
    kr_ms_draw_body<true>(sorted_all, work, V, rows, rng, nullptr, 0, ids, at);
}

// greedy rows: first maximum of the model's logits; penalised greedy rows: of the work row, then the token is marked seen (RUN: nothing is marked)
template <bool RUN>
__device__ __forceinline__ void kr_ms_argmax_body(const float* __restrict__ logits, size_t ld, const float* __restrict__ work, int V,
                                                  const KrMsRow* __restrict__ rows, uint32_t* __restrict__ seen, size_t seen_words, int* __restrict__ ids) {
    const KrMsRow r = rows[blockIdx.x];
    if (r.mode != KR_MS_GREEDY && r.mode != KR_MS_PENALTY) return;
    const float* row = r.mode == KR_MS_GREEDY ? logits + (size_t)blockIdx.x * ld : work + (size_t)blockIdx.x * V;
    const int idx = kr_row_argmax_1024(row, V);
    if (threadIdx.x != 0) return;
    ids[blockIdx.x] = idx;
    if constexpr (!RUN) if (r.mode == KR_MS_PENALTY && idx < V) atomicOr(&seen[(size_t)r.slot * seen_words + (idx >> 5)], 1u << (idx & 31));
}
__global__ void __launch_bounds__(1024) kr_ms_argmax_kernel(const float* __restrict__ logits, size_t ld, const float* __restrict__ work, int V,
                                                            const KrMsRow* __restrict__ rows, uint32_t* __restrict__ seen, size_t seen_words,
                                                            int* __restrict__ ids) {
    kr_ms_argmax_body<false>(logits, ld, work, V, rows, seen, seen_words, ids);
}
__global__ void __launch_bounds__(1024) kr_ms_argmax_run_kernel(const float* __restrict__ logits, size_t ld, const float* __restrict__ work, int V,
                                                                const KrMsRow* __restrict__ rows, int* __restrict__ ids) {
    kr_ms_argmax_body<true>(logits, ld, work, V, rows, nullptr, 0, ids);
}

// a LOOP row of the verify form: the slot's sampler as the run's at.t earlier draws would have left it, into scratch that kr_launch_sample may mark and
// advance freely.  One workgroup; each thread ORs the prefix tokens' bits into the words it copies (no second pass, no barrier).  Bounds as in the prepare
// kernel; a token >= V (never: the host checked) would match no word
__global__ void __launch_bounds__(1024) kr_ms_stage_kernel(const uint32_t* __restrict__ seen_slot, int words, const uint64_t* __restrict__ rng_slot,
                                                           const int* __restrict__ runs, const int* __restrict__ tokens, int run, int t,
                                                           uint32_t* __restrict__ hyp_seen, uint64_t* __restrict__ hyp_rng) {
    const int off = runs[3 * run + 1], cnt = runs[3 * run + 2];
    for (int w = threadIdx.x; w < words; w += 1024) {
        uint32_t v = seen_slot[w];
        for (int j = 1; j <= t; j++) { const int tok = tokens[kr_m_run_row(run, off, cnt, j)]; if ((tok >> 5) == w) v |= 1u << (tok & 31); }
        hyp_seen[w] = v;
    }
    if (threadIdx.x == 0) {
        uint64_t x = *rng_slot;
        for (int j = 0; j < t; j++) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; }
        *hyp_rng = x;
    }
}

// commit of a sampled verify: thread i applies the first n_keep[i] draws of run i to its slot's sampler -- the ids of the kept rows marked seen (the modes
// that mark: all but plain greedy), the xorshift64 state advanced once per kept draw (the modes that draw).  rows[i] is the run's last token row: every row
// of a run carries the run's slot and mode.  Bounds: t < n_keep <= n_match + 1 <= cnt (the host's check), rows through kr_m_run_row; slots are distinct
// across runs, so no two threads touch the same words
__global__ void __launch_bounds__(256) kr_ms_commit_kernel(const KrMsRow* __restrict__ rows, const int* __restrict__ runs, const int* __restrict__ n_keep,
                                                           int n_runs, const int* __restrict__ ids, int V, uint32_t* __restrict__ seen, size_t seen_words,
                                                           uint64_t* __restrict__ rng) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_runs) return;
    const int keep = n_keep[i];
    const KrMsRow r = rows[i];
    if (keep <= 0 || r.mode == KR_MS_GREEDY) return;
    const int off = runs[3 * i + 1], cnt = runs[3 * i + 2];
    for (int t = 0; t < keep; t++) {
        const int tok = ids[kr_m_run_row(i, off, cnt, t)];
        if ((unsigned)tok < (unsigned)V) atomicOr(&seen[(size_t)r.slot * seen_words + (tok >> 5)], 1u << (tok & 31));
    }
    if (r.mode == KR_MS_PENALTY) return;
    uint64_t x = rng[r.slot];
    for (int t = 0; t < keep; t++) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; }
    rng[r.slot] = x;
}
void kr_launch_ms_commit(const KrMsRow* rows, const int* runs, const int* n_keep, int n_runs, const int* ids, int V, uint32_t* seen, size_t seen_words,
                         uint64_t* rng, hipStream_t st) {
    hipLaunchKernelGGL(kr_ms_commit_kernel, dim3((n_runs + 255) / 256), dim3(256), 0, st, rows, runs, n_keep, n_runs, ids, V, seen, seen_words, rng);
}

int kr_launch_multi_sample(const KrMsArgs& a, hipStream_t st) {
    bool any_prep = false, any_sample = false, any_argmax = false;
    for (int b = 0; b < a.B; b++) {
        const int m = a.rows_host[b].mode;
        any_prep |= m != KR_MS_GREEDY; any_sample |= m == KR_MS_SAMPLE; any_argmax |= m == KR_MS_GREEDY || m == KR_MS_PENALTY;
    }
    const bool run = a.runs != nullptr;      // the verify form: no launch below writes sampler state
    if (any_prep) {
        const dim3 g((a.V + 255) / 256, a.B);
        if (run) hipLaunchKernelGGL(kr_ms_prepare_run_kernel, g, dim3(256), 0, st, a.logits, a.ld, a.V, a.rows_dev, a.seen, a.seen_words, a.work, a.at_dev, a.runs, a.tokens);
        else hipLaunchKernelGGL(kr_ms_prepare_kernel, g, dim3(256), 0, st, a.logits, a.ld, a.V, a.rows_dev, a.seen, a.seen_words, a.work);
        if (hipGetLastError() != hipSuccess) return 1;
    }
    if (any_sample) {
        hipLaunchKernelGGL(kr_ms_select_kernel, dim3(a.B), dim3(1024), 0, st, (const float*)a.work, a.V, a.rows_dev, a.sorted);
        if (hipGetLastError() != hipSuccess) return 1;
        if (run) hipLaunchKernelGGL(kr_ms_draw_run_kernel, dim3(a.B), dim3(256), 0, st, (const uint64_t*)a.sorted, (const float*)a.work, a.V, a.rows_dev, a.rng, a.ids, a.at_dev);
        else hipLaunchKernelGGL(kr_ms_draw_kernel, dim3(a.B), dim3(256), 0, st, (const uint64_t*)a.sorted, (const float*)a.work, a.V, a.rows_dev, a.rng, a.seen, a.seen_words, a.ids);
        if (hipGetLastError() != hipSuccess) return 1;
    }
    if (any_argmax) {
        if (run) hipLaunchKernelGGL(kr_ms_argmax_run_kernel, dim3(a.B), dim3(1024), 0, st, a.logits, a.ld, (const float*)a.work, a.V, a.rows_dev, a.ids);
        else hipLaunchKernelGGL(kr_ms_argmax_kernel, dim3(a.B), dim3(1024), 0, st, a.logits, a.ld, (const float*)a.work, a.V, a.rows_dev, a.seen, a.seen_words, a.ids);
        if (hipGetLastError() != hipSuccess) return 1;
    }
    for (int b = 0; b < a.B; b++) {        // the per-row path: exact by construction (the single-row sampler on this row's work copy and slot state)
        const KrMsRow& r = a.rows_host[b];
        if (r.mode != KR_MS_LOOP) continue;
        uint32_t* seen = a.seen + (size_t)r.slot * a.seen_words;
        uint64_t* rng = a.rng + r.slot;
        if (run) {      // ... and on a staged copy of the slot's sampler in the verify form
            hipLaunchKernelGGL(kr_ms_stage_kernel, dim3(1), dim3(1024), 0, st, (const uint32_t*)seen, (int)a.seen_words, (const uint64_t*)rng, a.runs, a.tokens,
                               a.at_host[b].run, a.at_host[b].t, a.hyp_seen, a.hyp_rng);
            if (hipGetLastError() != hipSuccess) return 1;
            seen = a.hyp_seen; rng = a.hyp_rng;
        }
        if (kr_launch_sample(a.work + (size_t)b * a.V, a.V, r.temperature, r.top_k, r.top_p, r.penalty, seen, a.loop_keys, a.loop_keys + a.V, a.loop_temp,
                             a.loop_temp_bytes, a.loop_probs, rng, a.ids + b, st))
            return 1;
    }
    return 0;
}
