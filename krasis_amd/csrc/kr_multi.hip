// kr_multi.hip -- the device side of the exact multi-sequence decode step (docs/design/13-multi-sequence.md).  Every row of a step belongs to its
// own sequence slot; these kernels replace the two layer sections that tie rows to one sequence (the linear-attention recurrence and GQA
// attention) with per-row forms over the slots.  The arithmetic specification is the decode step (kr_decode_ops.hip): the same operations in the
// same order, so each row's results carry the bits kr_decode_step gives on that sequence alone.
#include "kr_device.h"
#include "kr_libm.h"
#include "kr_multi.h"
#include "kr_sample_dev.h"

// hsum over 8 consecutive lanes in the order of the reference's hsum (kr_decode_ops.hip kr_hsum8)
__device__ __forceinline__ float kr_m_hsum8(float v) {
    v = v + __shfl_xor(v, 4);
    v = v + __shfl_xor(v, 1);
    v = v + __shfl_xor(v, 2);
    return v;
}
// sum of squares of x[0..n) (n % 8 == 0): lane l < 8 chains fma over elements b * 8 + l, ascending b, then hsum8 (kr_sumsq_chain8)
__device__ __forceinline__ float kr_m_sumsq8(const float* x, int n, int l) {
    float acc = 0.0f;
    for (int b = 0; b < n / 8; b++) { const float v = x[b * 8 + l]; acc = __builtin_fmaf(v, v, acc); }
    return kr_m_hsum8(acc);
}

// ---- linear attention ----------------------------------------------------------------------------------------------------------------------------
// conv1d (kernel 4) + SiLU of every channel of row b, and the shift of the slot's carried inputs.  grid (conv_dim / 256, B), 256 threads.
// Channel layout (decode.rs:3815): q [0, key_dim), k [key_dim, 2 key_dim), v [2 key_dim, conv_dim); the in-projection row holds per key head
// [q (dk) | k (dk) | v (hr dv) | z (hr dv)].
__global__ void __launch_bounds__(256) kr_multi_la_conv_kernel(const KrMultiLaArgs a) {
    const int b = blockIdx.y, ch = blockIdx.x * 256 + threadIdx.x;
    const int dk = a.dk, dv = a.dv, hr = a.hr, key_dim = a.nk * dk, conv_dim = 2 * key_dim + a.nv * dv, group_dim = 2 * dk + 2 * dv * hr;
    if (ch >= conv_dim) return;
    int kh, off;
    if (ch < key_dim) { kh = ch / dk; off = ch % dk; }
    else if (ch < 2 * key_dim) { kh = (ch - key_dim) / dk; off = dk + (ch - key_dim) % dk; }
    else { const int vh = (ch - 2 * key_dim) / dv, i = (ch - 2 * key_dim) % dv; kh = vh / hr; off = 2 * dk + (vh % hr) * dv + i; }
    const float x = a.qkvz[(size_t)b * a.ld_qkvz + (size_t)kh * group_dim + off];
    float4* cs = reinterpret_cast<float4*>(a.conv_state + (size_t)a.slots[b] * a.conv_stride) + ch;
    const float4 s = *cs, w = reinterpret_cast<const float4*>(a.conv_w)[ch];
    *cs = float4{s.y, s.z, s.w, x};
    const float co = s.y * w.x + s.z * w.y + s.w * w.z + x * w.w;
    a.conv_out[(size_t)b * conv_dim + ch] = co * kr_sigmoid_poly5(co);      // fast_silu_avx2
}

// gates, L2 norms, the gated delta rule on the slot's state and the head's gated RMSNorm.  grid (nv, B), dv threads: thread j owns column j of
// value head h of row b's slot, the whole column (DK values) in registers.  The operations and order of kr_la_step_kernel (kr_decode_ops.hip).
template <int DK>
__global__ void __launch_bounds__(256) kr_multi_la_recur_kernel(const KrMultiLaArgs a) {
    __shared__ float qc[DK], kc[DK], rr[256], nrm[2], gb[2], rms_s;
    const int h = blockIdx.x, b = blockIdx.y, j = threadIdx.x, dv = a.dv, hr = a.hr, kh = h / hr, r = h - kh * hr;
    const int key_dim = a.nk * DK, conv_dim = 2 * key_dim + a.nv * dv, group_dim = 2 * DK + 2 * dv * hr;
    // the head's state slice through one buffer descriptor (workgroup-uniform): voffset = the thread's column, row i by scalar offset -- no
    // per-row address registers next to the DK-register column
    const __amdgpu_buffer_rsrc_t srd = __builtin_amdgcn_make_buffer_rsrc(a.recur + (size_t)a.slots[b] * a.recur_stride + (size_t)h * DK * dv, 0, DK * dv * 4, 0x00020000);
    float c[DK];
#pragma unroll
    for (int i = 0; i < DK; i++) c[i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(srd, j * 4, i * dv * 4, 0));
    const float* co = a.conv_out + (size_t)b * conv_dim;
    for (int i = j; i < DK; i += dv) { qc[i] = co[kh * DK + i]; kc[i] = co[key_dim + kh * DK + i]; }
    const float vj = co[2 * key_dim + h * dv + j];
    const float* src = a.qkvz + (size_t)b * a.ld_qkvz + (size_t)kh * group_dim;
    const float zz = src[2 * DK + hr * dv + r * dv + j], wn = a.norm_w[(size_t)h * dv + j];
    if (j == 0) {      // gates (decode.rs:3891-3901)
        const float* ba = a.ba + (size_t)b * a.ld_ba;
        const float b_raw = ba[kh * 2 * hr + r], a_p = ba[kh * 2 * hr + hr + r];
        gb[1] = 1.0f / (1.0f + kr_expf(-b_raw));
        const float ap_dt = a_p + a.dt_bias[h];
        const float softplus = ap_dt > 20.0f ? ap_dt : kr_logf(1.0f + kr_expf(ap_dt));
        const float g = -(kr_expf(a.a_log[h])) * softplus;
        gb[0] = kr_expf(g);
    }
    __syncthreads();
    if (j < 16) {      // L2 norms: lanes 0-7 -> q, lanes 8-15 -> k (decode.rs:3909-3945)
        const int which = j >> 3, l = j & 7;
        const float ss = kr_m_sumsq8(which ? kc : qc, DK, l);
        if (l == 0) nrm[which] = ss > 0.0f ? 1.0f / sqrtf(ss) : 0.0f;
    }
    __syncthreads();
    {
        const float inv_q = nrm[0] * a.scale, inv_k = nrm[1] * 1.0f;
        for (int i = j; i < DK; i += dv) { qc[i] = qc[i] * inv_q; kc[i] = kc[i] * inv_k; }
    }
    __syncthreads();
    // kv = sum_i fma(S[i] e^g, k[i]); delta = (v - kv) beta; S' = fma(k, delta, S e^g); o = sum_i fma(S', q)
    const float g_exp = gb[0], beta_h = gb[1];
    // 16 elements of k (and q) per block out of LDS; the scheduling barriers keep the compiler from hoisting every read next to the column
    float kv = 0.0f;
#pragma unroll
    for (int i0 = 0; i0 < DK; i0 += 16) {
        float kk[16];
#pragma unroll
        for (int u = 0; u < 16; u++) kk[u] = kc[i0 + u];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 16; u++) { c[i0 + u] = c[i0 + u] * g_exp; kv = __builtin_fmaf(c[i0 + u], kk[u], kv); }
        __builtin_amdgcn_sched_barrier(0);
    }
    const float delta = (vj - kv) * beta_h;
    float ob = 0.0f;
#pragma unroll
    for (int i0 = 0; i0 < DK; i0 += 16) {
        float kk[16], qq[16];
#pragma unroll
        for (int u = 0; u < 16; u++) { kk[u] = kc[i0 + u]; qq[u] = qc[i0 + u]; }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 16; u++) {
            const float sn = __builtin_fmaf(kk[u], delta, c[i0 + u]);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(sn), srd, j * 4, (i0 + u) * dv * 4, 0);
            ob = __builtin_fmaf(sn, qq[u], ob);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    rr[j] = ob;
    __syncthreads();
    if (j < 8) { const float ss = kr_m_sumsq8(rr, dv, j); if (j == 0) rms_s = 1.0f / sqrtf(ss / (float)dv + a.eps); }
    __syncthreads();
    const float normed = (ob * rms_s) * wn;
    a.out[(size_t)b * a.ld_out + (size_t)h * dv + j] = (zz * kr_sigmoid_poly5(zz)) * normed;
}

int kr_launch_multi_la(const KrMultiLaArgs& a, int B, hipStream_t st) {
    if ((a.dk != 64 && a.dk != 128) || a.dv < 8 || a.dv > 256 || a.dv % 8 || a.nv != a.nk * a.hr) return 1;
    const int conv_dim = 2 * a.nk * a.dk + a.nv * a.dv;
    hipLaunchKernelGGL(kr_multi_la_conv_kernel, dim3((conv_dim + 255) / 256, B), dim3(256), 0, st, a);
    if (a.dk == 128) hipLaunchKernelGGL(kr_multi_la_recur_kernel<128>, dim3(a.nv, B), dim3(a.dv), 0, st, a);
    else hipLaunchKernelGGL(kr_multi_la_recur_kernel<64>, dim3(a.nv, B), dim3(a.dv), 0, st, a);
    return 0;
}

// ---- GQA -----------------------------------------------------------------------------------------------------------------------------------------
// decode.rs:2873-2966 per row: gated split, per-head RMS norm (scalar sequential sum), half-split RoPE at the row's position, K / V into the row's
// slot.  grid (nh + nkv, B), 256 threads (hd <= 256).  The exact branch of kr_gqa_prep_kernel.
__global__ void __launch_bounds__(256) kr_multi_gqa_prep_kernel(const KrMultiGqaArgs a) {
    __shared__ float x[256]; __shared__ float rms_s;
    const int hb = blockIdx.x, row = blockIdx.y, d = threadIdx.x, hd = a.hd, pos = a.positions[row];
    const bool is_q = hb < a.nh;
    const int h = is_q ? hb : hb - a.nh;
    const float* q_in = a.q_in + (size_t)row * a.ld_q;
    if (is_q) {
        float* gate = a.gate + (size_t)row * a.nh * hd;
        if (a.gated) { if (d < hd) { x[d] = q_in[(size_t)h * hd * 2 + d]; gate[(size_t)h * hd + d] = q_in[(size_t)h * hd * 2 + hd + d]; } }
        else if (d < hd) x[d] = q_in[(size_t)h * hd + d];
    } else if (d < hd) x[d] = a.k_in[(size_t)row * a.ld_k + (size_t)h * hd + d];
    __syncthreads();
    const float* nw = is_q ? a.q_norm : a.k_norm;
    if (nw) {
        if (d == 0) {
            float ss = 0.0f;
            for (int i = 0; i < hd; i++) ss += x[i] * x[i];
            rms_s = 1.0f / sqrtf(ss / (float)hd + a.eps);
        }
        __syncthreads();
        const int per_head = is_q ? a.q_norm_per_head : a.k_norm_per_head;
        if (d < hd) x[d] = x[d] * (rms_s * nw[(per_head ? h * hd : 0) + d]);
        __syncthreads();
    }
    const int d2 = a.rope_half;
    float val = d < hd ? x[d] : 0.0f;
    if (d < 2 * d2) {
        const float c = a.rope_cos[(size_t)pos * d2 + (d % d2)], s = a.rope_sin[(size_t)pos * d2 + (d % d2)];
        if (d < d2) val = x[d] * c - x[d2 + d] * s;        // x1*cos - x2*sin
        else val = x[d] * c + x[d - d2] * s;               // x2*cos + x1*sin
    }
    if (d < hd) {
        if (is_q) a.q_out[(size_t)row * a.nh * hd + (size_t)h * hd + d] = val;
        else {
            const size_t o = (size_t)a.slots[row] * a.slot_elems + (size_t)pos * a.nkv * hd + (size_t)h * hd + d;
            kr_kv_store(a.k_cache, o, val, a.kv_fp8);
            kr_kv_store(a.v_cache, o, a.v_in[(size_t)row * a.ld_v + (size_t)h * hd + d], a.kv_fp8);
        }
    }
}

// decode.rs:4194 per row: the G = nh / nkv query heads of KV head kvh over the slot's rows [0, pos].  grid (nkv, B), 256 threads; every K and V row
// of the sequence is read once for the G heads.  Scores: 8 lanes per position, lane l chains fma over elements e * 8 + l (ascending e) and the
// 8-lane hsum -- one K row in registers serves all G heads.  Softmax: one wave per head (rounds of 4 heads): max, libm exp in place, the
// position-ordered sum over LDS tiles by one lane (zero padding to a multiple of 32 leaves a sum of exponentials unchanged), the scale by the
// reciprocal.  P.V: thread t owns output d = t % hd of heads t / hd, t / hd + 256 / hd, ..: one fma per position, ascending.
#define KR_MG_TILE 1024      // softmax-sum tile per wave (floats)
#define KR_MG_PT 64          // positions per P.V stage
#define KR_MG_ACC 16         // heads per thread and pass of the P.V loop
template <int NB, bool FP8>
__global__ void __launch_bounds__(256) kr_multi_gqa_attn_kernel(const KrMultiGqaArgs a) {
    constexpr int HD = NB * 8;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int G = a.nh / a.nkv;
    float* qs = sm;                                  // [G][HD]
    float* tile = qs + (size_t)G * HD;               // [4][KR_MG_TILE]
    float* pt = tile + 4 * KR_MG_TILE;               // [G][KR_MG_PT]
    const int kvh = blockIdx.x, row = blockIdx.y, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int pos = a.positions[row], seq = pos + 1, kvs = a.nkv * HD;
    const size_t kv0 = (size_t)a.slots[row] * a.slot_elems + (size_t)kvh * HD;      // element of (position 0, this KV head) in the slot
    float* sc = a.scores + ((size_t)row * a.nh + (size_t)kvh * G) * a.sc_ld;        // [G][sc_ld]
    const float* q = a.q_out + (size_t)row * a.nh * HD + (size_t)kvh * G * HD;
    for (int i = t; i < G * HD; i += 256) qs[i] = q[i];
    __syncthreads();
    // ---- scores
    {
        const int l = t & 7, grp = t >> 3;
        for (int s = grp; s < seq; s += 32) {
            float kr[NB];
#pragma unroll
            for (int e = 0; e < NB; e++) kr[e] = kr_kv_load(a.k_cache, kv0 + (size_t)s * kvs + e * 8 + l, FP8);
            for (int g = 0; g < G; g++) {
                float acc = 0.0f;
#pragma unroll
                for (int e = 0; e < NB; e++) acc = __builtin_fmaf(qs[g * HD + e * 8 + l], kr[e], acc);
                acc = kr_m_hsum8(acc);
                if (l == 0) sc[(size_t)g * a.sc_ld + s] = acc * a.sm_scale;
            }
        }
    }
    __syncthreads();
    // ---- softmax, one wave per head
    const int seq32 = (seq + 31) & ~31;
    float* tw = tile + w * KR_MG_TILE;
    for (int g0 = 0; g0 < G; g0 += 4) {
        const int g = g0 + w;
        const bool on = g < G;
        float* rowp = sc + (size_t)(on ? g : 0) * a.sc_ld;
        float mx = -__builtin_inff();
        if (on) for (int s = lane; s < seq; s += 64) mx = fmaxf(mx, rowp[s]);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
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
    __syncthreads();
    // ---- P.V
    constexpr int TPH = 256 / HD;                    // threads per output column: heads are dealt round-robin over them
    const int d = t % HD, hg = t / HD;
    const float* gate = a.gate + (size_t)row * a.nh * HD + (size_t)kvh * G * HD;
    float* out = a.attn_out + (size_t)row * a.nh * HD + (size_t)kvh * G * HD;
    for (int gp = 0; gp < G; gp += KR_MG_ACC * TPH) {      // heads gp + hg + k * TPH, k < KR_MG_ACC
        float o[KR_MG_ACC];
#pragma unroll
        for (int k = 0; k < KR_MG_ACC; k++) o[k] = 0.0f;
        for (int s0 = 0; s0 < seq; s0 += KR_MG_PT) {
            const int n = min(KR_MG_PT, seq - s0);
            __syncthreads();
            for (int i = t; i < G * KR_MG_PT; i += 256) { const int g = i / KR_MG_PT, s = i % KR_MG_PT; pt[i] = s < n ? sc[(size_t)g * a.sc_ld + s0 + s] : 0.0f; }
            __syncthreads();
            for (int s1 = 0; s1 < n; s1 += 16) {
                float v[16];
#pragma unroll
                for (int u = 0; u < 16; u++) v[u] = kr_kv_load(a.v_cache, kv0 + (size_t)(s0 + min(s1 + u, n - 1)) * kvs + d, FP8);
#pragma unroll
                for (int u = 0; u < 16; u++) {
#pragma unroll
                    for (int k = 0; k < KR_MG_ACC; k++) {
                        const int g = gp + hg + k * TPH;
                        if (g < G && s1 + u < n) o[k] = __builtin_fmaf(pt[g * KR_MG_PT + s1 + u], v[u], o[k]);
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < KR_MG_ACC; k++) {
            const int g = gp + hg + k * TPH;
            if (g < G) {
                float ov = o[k];
                if (a.gated) { const float gt = gate[(size_t)g * HD + d]; ov *= 1.0f / (1.0f + kr_expf(-gt)); }
                out[(size_t)g * HD + d] = ov;
            }
        }
    }
}

int kr_launch_multi_gqa(const KrMultiGqaArgs& a, int B, hipStream_t st) {
    if ((a.hd != 64 && a.hd != 128 && a.hd != 256) || a.nkv < 1 || a.nh % a.nkv || a.sc_ld % 32) return 1;
    const int G = a.nh / a.nkv;
    const size_t lds = ((size_t)G * a.hd + 4 * KR_MG_TILE + (size_t)G * KR_MG_PT) * 4;
    if (lds > 64 * 1024) return 1;
    hipLaunchKernelGGL(kr_multi_gqa_prep_kernel, dim3(a.nh + a.nkv, B), dim3(256), 0, st, a);
#define KR_MGA(NB_, F_) hipLaunchKernelGGL((kr_multi_gqa_attn_kernel<NB_, F_>), dim3(a.nkv, B), dim3(256), lds, st, a)
    if (a.kv_fp8) { if (a.hd == 256) KR_MGA(32, true); else if (a.hd == 128) KR_MGA(16, true); else KR_MGA(8, true); }
    else { if (a.hd == 256) KR_MGA(32, false); else if (a.hd == 128) KR_MGA(16, false); else KR_MGA(8, false); }
#undef KR_MGA
    return 0;
}

// ---- per-row greedy id ---------------------------------------------------------------------------------------------------------------------------
// grid B, 1024 threads per row: kr_argmax_kernel's first maximum (kr_row_argmax_1024)
__global__ void __launch_bounds__(1024) kr_multi_argmax_kernel(const float* __restrict__ x, size_t ld, int V, int* __restrict__ out) {
    const int idx = kr_row_argmax_1024(x + (size_t)blockIdx.x * ld, V);
    if (threadIdx.x == 0) out[blockIdx.x] = idx;
}
void kr_launch_multi_argmax(const float* logits, size_t ld, int V, int B, int* out, hipStream_t st) {
    hipLaunchKernelGGL(kr_multi_argmax_kernel, dim3(B), dim3(1024), 0, st, logits, ld, V, out);
}
