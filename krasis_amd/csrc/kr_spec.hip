// kr_spec.hip -- the device side of exact speculative greedy decoding (docs/design/12-speculative.md): the accept kernel of the verify pass and the
// snapshot / rollback of the linear-attention states.  A verify pass is the exact prompt pass over [last token, d1 .. dk]; its per-row greedy ids
// are those of the decode step (same logits bits, same first-maximum rule), so accepting the longest agreeing prefix reproduces plain greedy
// decoding.  The prompt pass advances the conv / recurrent states in place over all k + 1 tokens: when fewer are kept, the rollback recomputes
// the kept tokens' updates from the snapshot taken before the pass, in the decode step's order (KV rows need nothing: attention at position p
// reads positions <= p only, and the next pass overwrites the rest).
#include "../../include/krasis_hip.h"
#include "kr_spec.h"

// ---- accept: per-row argmax + draft comparison ---------------------------------------------------------------------------------------------------
// grid n (one 1024-thread workgroup per logits row).  The (value desc, index asc) rule of kr_argmax_kernel (kr_decode_ops.hip): a total order on the
// row's values, so any reduction tree returns the decode step's first maximum.  The workgroup that finishes last (device-scope counter, reset for the
// next pass) reads every row's id and compares the drafts: out = [greedy[0..n), n_match], one DtoH for the host.
__global__ void __launch_bounds__(1024) kr_spec_accept_kernel(const float* __restrict__ x, size_t ld, int V, int n, const int* __restrict__ tokens, int* out,
                                                              float* part_v, int* part_i, unsigned* counter) {
    __shared__ float bv[16]; __shared__ int bi[16]; __shared__ int s_last;
    const int r = blockIdx.x;
    const float* row = x + (size_t)r * ld;
    float v = -__builtin_inff(); int idx = 0x7FFFFFFF;
    for (int i = threadIdx.x; i < V; i += 1024) { const float t = row[i]; if (t > v || (t == v && i < idx)) { v = t; idx = i; } }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(v, off); const int oi = __shfl_xor(idx, off);
        if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
    }
    if ((threadIdx.x & 63) == 0) { bv[threadIdx.x >> 6] = v; bi[threadIdx.x >> 6] = idx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; w++) if (bv[w] > v || (bv[w] == v && bi[w] < idx)) { v = bv[w]; idx = bi[w]; }
        __hip_atomic_store(part_v + r, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(part_i + r, idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned prev = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        s_last = prev == (unsigned)n - 1;
        if (s_last) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (!s_last || threadIdx.x >= 64) return;
    // one wave: lane i < n holds row i's id; n_match = the first i >= 1 with tokens[i] != greedy[i - 1], minus one (n - 1 when every draft agrees)
    const int lane = threadIdx.x;
    const int g = lane < n ? __hip_atomic_load(part_i + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
    const int gprev = __shfl_up(g, 1);
    const bool miss = lane >= 1 && lane < n && tokens[lane] != gprev;
    const unsigned long long m = __ballot(miss);
    if (lane < n) out[lane] = g;
    if (lane == 0) out[n] = m ? (int)__builtin_ctzll(m) - 1 : n - 1;
}

// ---- snapshot: live -> snap for every linear-attention layer ------------------------------------------------------------------------------------
// grid (x, layers), 256 threads; 16-byte copies (both state sizes are multiples of 4 floats: dk % 8 == 0, 4 conv slots per channel)
__global__ void __launch_bounds__(256) kr_spec_snapshot_kernel(const KrSpecLa* __restrict__ tab) {
    const KrSpecLa E = tab[blockIdx.y];
    const size_t nr = (size_t)E.nv * E.dk * E.dv / 4, nc = (size_t)(2 * E.nk * E.dk + E.nv * E.dv);     // float4 counts: recurrent state, conv slots
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nr + nc; i += stride) {
        if (i < nr) reinterpret_cast<float4*>(E.snap_recur)[i] = reinterpret_cast<const float4*>(E.recur)[i];
        else reinterpret_cast<float4*>(E.snap_conv)[i - nr] = reinterpret_cast<const float4*>(E.conv)[i - nr];
    }
}

// ---- rollback: live = snapshot advanced by the kept tokens ----------------------------------------------------------------------------------------
// grid (value head, layer), dv threads: thread j owns column j of head h's state, S[i] = state[h][i][j], in registers.  Per kept token the decode
// step's update (decode.rs:1293; the order kr_pfm_la_recur_kernel keeps, kr_prefill_ops.hip): S[i] *= e^g, kv = fma chain over i of S[i] k[i] from 0,
// delta = (v - kv) * beta, S[i] = fma(k[i], delta, S[i]) -- the output chain is not needed.  Then the carried conv slots: slot j = X(n_keep - 4 + j),
// X(i < 0) = the snapshot's slot 4 + i (kr_pfm_la_conv_state_kernel), the workgroups of a layer striding over its channels.
template <int DK>
__global__ void __launch_bounds__(256) kr_spec_rollback_kernel(const KrSpecLa* __restrict__ tab, int n_keep) {
    const KrSpecLa E = tab[blockIdx.y];
    if (E.dk != DK) return;                                   // another launch takes the layers of the other key width
    const int h = blockIdx.x, j = threadIdx.x, nv = E.nv, dv = E.dv;
    if (h < nv && j < dv) {
        const size_t base = (size_t)h * DK * dv + j;
        float S[DK];
#pragma unroll
        for (int i = 0; i < DK; i++) S[i] = E.snap_recur[base + (size_t)i * dv];
        for (int t = 0; t < n_keep; t++) {
            const float* kr = E.k + (size_t)t * nv * DK + (size_t)h * DK;
            const float ge = E.gexp[(size_t)t * nv + h], bt = E.beta[(size_t)t * nv + h], vj = E.v[(size_t)t * nv * dv + (size_t)h * dv + j];
            float kv = 0.0f;
#pragma unroll
            for (int i = 0; i < DK; i++) { S[i] = S[i] * ge; kv = __builtin_fmaf(S[i], kr[i], kv); }
            const float delta = (vj - kv) * bt;
#pragma unroll
            for (int i = 0; i < DK; i++) S[i] = __builtin_fmaf(kr[i], delta, S[i]);
        }
#pragma unroll
        for (int i = 0; i < DK; i++) E.recur[base + (size_t)i * dv] = S[i];
    }
    const int key_dim = E.nk * E.dk, conv_dim = 2 * key_dim + nv * dv, group_dim = 2 * E.dk + 2 * dv * E.hr;
    for (int ch = blockIdx.x * blockDim.x + threadIdx.x; ch < conv_dim; ch += gridDim.x * blockDim.x) {
        int kh, off;
        if (ch < key_dim) { kh = ch / E.dk; off = ch % E.dk; }
        else if (ch < 2 * key_dim) { kh = (ch - key_dim) / E.dk; off = E.dk + (ch - key_dim) % E.dk; }
        else { const int vh = (ch - 2 * key_dim) / dv, i = (ch - 2 * key_dim) % dv; kh = vh / E.hr; off = 2 * E.dk + (vh % E.hr) * dv + i; }
        const float* cs = E.snap_conv + (size_t)ch * 4;
        float nslot[4];
#pragma unroll
        for (int q = 0; q < 4; q++) { const int i = n_keep - 4 + q; nslot[q] = i >= 0 ? E.qkvz[(size_t)i * E.ld_qkvz + (size_t)kh * group_dim + off] : cs[4 + i]; }
        *reinterpret_cast<float4*>(E.conv + (size_t)ch * 4) = float4{nslot[0], nslot[1], nslot[2], nslot[3]};
    }
}

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
void kr_launch_spec_accept(const float* logits, size_t ld, int V, int n, const int* tokens, int* out, float* part, unsigned* counter, hipStream_t st) {
    hipLaunchKernelGGL(kr_spec_accept_kernel, dim3(n), dim3(1024), 0, st, logits, ld, V, n, tokens, out, part, (int*)(part + KR_VERIFY_MAX), counter);
}
void kr_launch_spec_snapshot(const KrSpecLa* tab, int n_la, int max_floats, hipStream_t st) {
    int bx = (max_floats / 4 + 255) / 256;
    bx = bx < 1 ? 1 : (bx > 64 ? 64 : bx);                    // 64 x layers workgroups, grid-stride inside
    hipLaunchKernelGGL(kr_spec_snapshot_kernel, dim3(bx, n_la), dim3(256), 0, st, tab);
}
void kr_launch_spec_rollback(const KrSpecLa* tab, int n_la, bool has64, bool has128, int nv_max, int dv_max, int n_keep, hipStream_t st) {
    if (has128) hipLaunchKernelGGL(kr_spec_rollback_kernel<128>, dim3(nv_max, n_la), dim3(dv_max), 0, st, tab, n_keep);
    if (has64) hipLaunchKernelGGL(kr_spec_rollback_kernel<64>, dim3(nv_max, n_la), dim3(dv_max), 0, st, tab, n_keep);
}
