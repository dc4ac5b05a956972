// kr_multi_softmax_dev.h -- the softmax of one score row by one wave, shared by the per-slot attention kernels of kr_multi.hip and the softmax launch of
// "multi_attn_exact_split" (kr_multi_split.hip).  One copy: the steps and their order are the specification of both.
#pragma once
#include "kr_device.h"
#include "kr_libm.h"
#include "kr_exact_dev.h"

// ---- softmax of one score row by one wave (decode.rs:4245-4254) -----------------------------------------------------------------------------------
// rowp[0, seq) in place: the maximum, libm exp of (score - max), the sum of the exponentials in position order -- by lane 0 over LDS tiles of
// KR_MG_TILE floats (tw: this wave's tile; zero padding to a multiple of 32 leaves a sum of exponentials unchanged) -- and the scale by its reciprocal.
// It contains workgroup barriers: EVERY thread of the workgroup calls it, the same number of times; a wave without a row passes on = false (and any
// valid row pointer) and only keeps the barriers.
#define KR_MG_TILE 1024      // softmax-sum tile per wave (floats)
__device__ __forceinline__ void kr_m_wave_softmax(float* rowp, int seq, float* tw, bool on, int lane) {
    const int seq32 = (seq + 31) & ~31;
    float mx = -__builtin_inff();
    if (on) for (int s = lane; s < seq; s += 64) mx = fmaxf(mx, rowp[s]);
    mx = kr_wave_max(mx);
    if (on) for (int s = lane; s < seq; s += 64) rowp[s] = kr_expf(rowp[s] - mx);
    __syncthreads();
    float se = 0.0f;
    for (int s0 = 0; s0 < seq32; s0 += KR_MG_TILE) {
        const int n = min(KR_MG_TILE, seq32 - s0);
        if (on) for (int i = lane; i < n; i += 64) tw[i] = s0 + i < seq ? rowp[s0 + i] : 0.0f;
        __syncthreads();
        if (on && lane == 0) se = kr_seq_sum(tw, n, se);
        __syncthreads();
    }
    se = __shfl(se, 0);
    const float inv = 1.0f / se;
    if (on) for (int s = lane; s < seq; s += 64) rowp[s] *= inv;
}
