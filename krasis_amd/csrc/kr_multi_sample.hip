// kr_multi_sample.hip -- sample_from_logits (src/decode.rs:3718-3811) for the B rows of a multi-sequence step in one launch sequence
// (docs/design/14-multi-sampling.md).  The arithmetic specification is the single-row sampler (kr_sampler.hip): each row takes the same
// operations in the same order, so its token, xorshift64 state and seen bitmap are the ones kr_launch_sample / kr_decode_generate give it alone.
//   prepare  grid (V / 256, B): work row = penalty on the slot's seen tokens, *= 1 / temperature (penalised greedy rows: the penalty only)
//   select   grid B, 1024 threads: top-k of the (value, ~index) keys by radix select + LDS bitonic sort (kr_sample_select_kernel), keys computed
//            from the prepared f32 row; per-wave histograms (counts do not depend on the order the keys are counted in)
//   draw     grid B, 256 threads: kr_sample_draw_kernel on the slot's xorshift64 state and seen bitmap
//   argmax   grid B, 1024 threads: greedy rows (first maximum of the model's logits) and penalised greedy rows (of the work row; marks it seen)
// Rows that draw from more than KR_MS_SEL_CAP candidates run kr_launch_sample on their work row, one row after another.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kr_libm.h"
#include "kr_multi_sample.h"
#include "kr_sample_dev.h"
#include "kr_sampler.h"

#define KR_MS_WAVES 16     // waves of the 1024-thread select workgroup

__global__ void __launch_bounds__(256) kr_ms_prepare_kernel(const float* __restrict__ logits, size_t ld, int V, const KrMsRow* __restrict__ rows,
                                                            const uint32_t* __restrict__ seen, size_t seen_words, float* __restrict__ work) {
    const KrMsRow r = rows[blockIdx.y];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (r.mode == KR_MS_GREEDY || i >= V) return;
    float v = logits[(size_t)blockIdx.y * ld + i];
    if (r.mode != KR_MS_LOOP) {            // LOOP rows: kr_launch_sample prepares its row in place
        if (r.penalty != 0.0f && ((seen[(size_t)r.slot * seen_words + (i >> 5)] >> (i & 31)) & 1u)) v -= r.penalty;
        if (r.mode == KR_MS_SAMPLE) v *= r.inv_temp;
    }
    work[(size_t)blockIdx.y * V + i] = v;
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

// kr_sample_draw_kernel on row b: exps in parallel, every sum on lane 0 in sorted order, the slot's xorshift64 state and seen bitmap
__global__ void __launch_bounds__(256) kr_ms_draw_kernel(const uint64_t* __restrict__ sorted_all, const float* __restrict__ work, int V,
                                                         const KrMsRow* __restrict__ rows, uint64_t* __restrict__ rng, uint32_t* __restrict__ seen,
                                                         size_t seen_words, int* __restrict__ ids) {
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
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    rng[r.slot] = x;
    const float rr = (float)((double)x / 18446744073709551615.0);
    int pick = -1; float cum = 0.0f;
    for (int i = 0; i < cutoff; i++) { cum += probs[i]; if (rr < cum) { pick = i; break; } }
    if (pick < 0) pick = cutoff - 1;
    const int tok = (int)(0xFFFFFFFFu - (uint32_t)sorted[pick]);
    ids[blockIdx.x] = tok;
    if ((unsigned)tok < (unsigned)V) atomicOr(&seen[(size_t)r.slot * seen_words + (tok >> 5)], 1u << (tok & 31));
}

// greedy rows: first maximum of the model's logits; penalised greedy rows: of the work row, then the token is marked seen
__global__ void __launch_bounds__(1024) kr_ms_argmax_kernel(const float* __restrict__ logits, size_t ld, const float* __restrict__ work, int V,
                                                            const KrMsRow* __restrict__ rows, uint32_t* __restrict__ seen, size_t seen_words,
                                                            int* __restrict__ ids) {
    const KrMsRow r = rows[blockIdx.x];
    if (r.mode != KR_MS_GREEDY && r.mode != KR_MS_PENALTY) return;
    const float* row = r.mode == KR_MS_GREEDY ? logits + (size_t)blockIdx.x * ld : work + (size_t)blockIdx.x * V;
    const int idx = kr_row_argmax_1024(row, V);
    if (threadIdx.x != 0) return;
    ids[blockIdx.x] = idx;
    if (r.mode == KR_MS_PENALTY && idx < V) atomicOr(&seen[(size_t)r.slot * seen_words + (idx >> 5)], 1u << (idx & 31));
}

int kr_launch_multi_sample(const KrMsArgs& a, hipStream_t st) {
    bool any_prep = false, any_sample = false, any_argmax = false;
    for (int b = 0; b < a.B; b++) {
        const int m = a.rows_host[b].mode;
        any_prep |= m != KR_MS_GREEDY; any_sample |= m == KR_MS_SAMPLE; any_argmax |= m == KR_MS_GREEDY || m == KR_MS_PENALTY;
    }
    if (any_prep) {
        hipLaunchKernelGGL(kr_ms_prepare_kernel, dim3((a.V + 255) / 256, a.B), dim3(256), 0, st, a.logits, a.ld, a.V, a.rows_dev, a.seen, a.seen_words, a.work);
        if (hipGetLastError() != hipSuccess) return 1;
    }
    if (any_sample) {
        hipLaunchKernelGGL(kr_ms_select_kernel, dim3(a.B), dim3(1024), 0, st, (const float*)a.work, a.V, a.rows_dev, a.sorted);
        if (hipGetLastError() != hipSuccess) return 1;
        hipLaunchKernelGGL(kr_ms_draw_kernel, dim3(a.B), dim3(256), 0, st, (const uint64_t*)a.sorted, (const float*)a.work, a.V, a.rows_dev, a.rng, a.seen, a.seen_words, a.ids);
        if (hipGetLastError() != hipSuccess) return 1;
    }
    if (any_argmax) {
        hipLaunchKernelGGL(kr_ms_argmax_kernel, dim3(a.B), dim3(1024), 0, st, a.logits, a.ld, (const float*)a.work, a.V, a.rows_dev, a.seen, a.seen_words, a.ids);
        if (hipGetLastError() != hipSuccess) return 1;
    }
    for (int b = 0; b < a.B; b++) {        // the per-row path: exact by construction (the single-row sampler on this row's work copy and slot state)
        const KrMsRow& r = a.rows_host[b];
        if (r.mode != KR_MS_LOOP) continue;
        if (kr_launch_sample(a.work + (size_t)b * a.V, a.V, r.temperature, r.top_k, r.top_p, r.penalty, a.seen + (size_t)r.slot * a.seen_words,
                             a.loop_keys, a.loop_keys + a.V, a.loop_temp, a.loop_temp_bytes, a.loop_probs, a.rng + r.slot, a.ids + b, st))
            return 1;
    }
    return 0;
}
