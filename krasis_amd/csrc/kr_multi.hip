// kr_multi.hip -- the device side of the exact multi-sequence decode step (docs/design/13-multi-sequence.md).  Every row of a step belongs to its
// own sequence slot; these kernels replace the two layer sections that tie rows to one sequence (the linear-attention recurrence and GQA
// attention) with per-row forms over the slots.  The arithmetic specification is the decode step (kr_decode_ops.hip): the same operations in the
// same order, so each row's results carry the bits kr_decode_step gives on that sequence alone.
#include "kr_device.h"
#include "kr_libm.h"
#include "kr_exact_dev.h"
#include "kr_multi.h"
#include "kr_multi_softmax_dev.h"      // kr_m_wave_softmax, KR_MG_TILE
#include "kr_mla_dev.h"
#include "kr_decode_ops.h"
#include "kr_router.h"
#include "kr_sample_dev.h"

// ---- linear attention ----------------------------------------------------------------------------------------------------------------------------
// Run i of a pass is `cnt` consecutive tokens of one slot: runs[3 i] = the slot, runs[3 i + 1] = off, runs[3 i + 2] = cnt.  Its tokens sit, in order, in
// pass rows off .. off + cnt - 2 and, the last one, in row i (the pass keeps every run's last token in the first rows for the lm_head); a step is runs of
// one token, row i alone.  The two kernels below carry the slot's state through the run in registers: per token the operations and order of
// kr_la_step_kernel (kr_decode_ops.hip), the state loaded once before the first token and stored once after the last.
// (kr_m_run_row, kr_multi.h, is that mapping.)

// conv1d (kernel 4) + SiLU of every channel of the run's rows, and the shift of the slot's carried inputs.  grid (conv_dim / 256, runs), 256 threads:
// thread = channel, the slot's four carried inputs in registers for the whole run.  Channel layout (decode.rs:3815): q [0, key_dim), k [key_dim, 2 key_dim),
// v [2 key_dim, conv_dim); the in-projection row holds per key head [q (dk) | k (dk) | v (hr dv) | z (hr dv)].
// VERIFY (docs/design/18-multi-verify.md): the same outputs for every token, the channel's inputs recorded per row, the slot's carried inputs left as they are.
template <bool VERIFY>
__global__ void __launch_bounds__(256) kr_multi_la_conv_kernel(const KrMultiLaArgs a, const int* __restrict__ runs) {
    const int i = blockIdx.y, ch = blockIdx.x * 256 + threadIdx.x;
    const int dk = a.dk, dv = a.dv, hr = a.hr, key_dim = a.nk * dk, conv_dim = 2 * key_dim + a.nv * dv, group_dim = 2 * dk + 2 * dv * hr;
    if (ch >= conv_dim) return;
    int kh, off;
    if (ch < key_dim) { kh = ch / dk; off = ch % dk; }
    else if (ch < 2 * key_dim) { kh = (ch - key_dim) / dk; off = dk + (ch - key_dim) % dk; }
    else { const int vh = (ch - 2 * key_dim) / dv, e = (ch - 2 * key_dim) % dv; kh = vh / hr; off = 2 * dk + (vh % hr) * dv + e; }
    const int slot = runs[3 * i], row0 = runs[3 * i + 1], cnt = runs[3 * i + 2];
    if constexpr (!VERIFY) if (kr_m_run_chunked(a, cnt)) return;      // "multi_extend_la_chunk": the chunked rule's run (workgroup-uniform; this kernel has no barrier; never in a verify pass)
    if constexpr (!VERIFY) if (kr_m_run_staged(a, cnt)) return;       // "multi_extend_la_exact": the staged form's run (the same)
    const float* xin = a.qkvz + (size_t)kh * group_dim + off;
    float4* cs = reinterpret_cast<float4*>(a.conv_state + (size_t)slot * a.conv_stride) + ch;
    float4 s = *cs;
    const float4 w = reinterpret_cast<const float4*>(a.conv_w)[ch];
    for (int t = 0; t < cnt; t++) {
        const int b = kr_m_run_row(i, row0, cnt, t);
        const float x = xin[(size_t)b * a.ld_qkvz];
        a.conv_out[(size_t)b * conv_dim + ch] = kr_conv4_silu(s.y, s.z, s.w, x, w);
        if constexpr (VERIFY) a.rec_x[(size_t)b * conv_dim + ch] = x;
        s = float4{s.y, s.z, s.w, x};
    }
    if constexpr (!VERIFY) *cs = s;
}

// gates, L2 norms, the gated delta rule on the slot's state and the head's gated RMSNorm.  grid (nv, runs), dv threads: thread j keeps column j of value
// head h of the run's slot (DK registers) from the first token to the last, read and written through one buffer descriptor (workgroup-uniform: voffset =
// the thread's column, row i by scalar offset -- no per-row address registers next to the column).  The gates of all the run's tokens (e^g, beta: exp / log chains that depend on the ba row alone) are
// computed first, a token per thread, into LDS -- before the column is loaded, so their temporaries never sit next to it.  Barriers of the token loop (five
// per token): a token's reads of qc / kc / nrm all precede its fourth barrier (after rr is written) and its reads of rr precede the fifth; every thread passes
// both before any thread starts the next token, whose first LDS writes are qc / kc.  rms_s is read after the fifth barrier and next written after the next
// token's fourth, by which time every thread has passed that token's first.
// VERIFY (docs/design/18-multi-verify.md): the same outputs for every token; the column is not stored, and per token row the normalised key (by the first value
// head of each key head, each thread the elements it scaled itself: no barrier is added), the value, e^g and beta are recorded for kr_multi_la_commit_kernel.
#define KR_M_RUN_MAX 1024      // tokens per run (LDS gate rows); = KR_EXTEND_MAX_TOKENS
template <int DK, bool VERIFY>
__global__ void __launch_bounds__(256) kr_multi_la_recur_kernel(const KrMultiLaArgs a, const int* __restrict__ runs) {
    __shared__ float qc[DK], kc[DK], rr[256], nrm[2], rms_s, ge[KR_M_RUN_MAX], be[KR_M_RUN_MAX];
    const int h = blockIdx.x, ri = blockIdx.y, j = threadIdx.x, dv = a.dv, hr = a.hr, kh = h / hr, r = h - kh * hr;
    const int key_dim = a.nk * DK, conv_dim = 2 * key_dim + a.nv * dv, group_dim = 2 * DK + 2 * dv * hr;
    const int slot = runs[3 * ri], row0 = runs[3 * ri + 1], cnt = runs[3 * ri + 2];
    if constexpr (!VERIFY) if (kr_m_run_chunked(a, cnt)) return;      // "multi_extend_la_chunk": the chunked rule's run (workgroup-uniform, ahead of every barrier; never in a verify pass)
    if constexpr (!VERIFY) if (kr_m_run_staged(a, cnt)) return;       // "multi_extend_la_exact": the staged form's run (the same)
    for (int t = j; t < cnt; t += dv) {      // gates (decode.rs:3891-3901)
        const float* ba = a.ba + (size_t)kr_m_run_row(ri, row0, cnt, t) * a.ld_ba;
        const float b_raw = ba[kh * 2 * hr + r], a_p = ba[kh * 2 * hr + hr + r];
        float g; kr_la_gate(b_raw, a_p, a.dt_bias[h], a.a_log[h], be[t], g);
        ge[t] = kr_expf(g);
    }
    const __amdgpu_buffer_rsrc_t srd = __builtin_amdgcn_make_buffer_rsrc(a.recur + (size_t)slot * a.recur_stride + (size_t)h * DK * dv, 0, DK * dv * 4, 0x00020000);
    float c[DK];
#pragma unroll
    for (int i = 0; i < DK; i++) c[i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(srd, j * 4, i * dv * 4, 0));
    const float wn = a.norm_w[(size_t)h * dv + j];
#pragma unroll 1
    for (int t = 0; t < cnt; t++) {
        const int b = kr_m_run_row(ri, row0, cnt, t);
        const float* co = a.conv_out + (size_t)b * conv_dim;
#pragma unroll 1
        for (int i = j; i < DK; i += dv) { qc[i] = co[kh * DK + i]; kc[i] = co[key_dim + kh * DK + i]; }
        const float vj = co[2 * key_dim + h * dv + j];
        const float zz = a.qkvz[(size_t)b * a.ld_qkvz + (size_t)kh * group_dim + 2 * DK + hr * dv + r * dv + j];
        __syncthreads();      // (first token: also the gate rows)
        if (j < 16) {      // L2 norms: lanes 0-7 -> q, lanes 8-15 -> k (decode.rs:3909-3945)
            const int which = j >> 3, l = j & 7;
            const float ss = kr_sumsq8<0, 0>(which ? kc : qc, DK, l);
            if (l == 0) nrm[which] = kr_l2_inv(ss);
        }
        __syncthreads();
        {
            const float inv_q = nrm[0] * a.scale, inv_k = nrm[1] * 1.0f;
#pragma unroll 1
            for (int i = j; i < DK; i += dv) {
                qc[i] = qc[i] * inv_q; kc[i] = kc[i] * inv_k;
                if constexpr (VERIFY) if (r == 0) a.rec_k[((size_t)b * a.nk + kh) * DK + i] = kc[i];
            }
        }
        __syncthreads();
        if constexpr (VERIFY) {
            a.rec_v[((size_t)b * a.nv + h) * dv + j] = vj;
            if (j == 0) { a.rec_ge[(size_t)b * a.nv + h] = ge[t]; a.rec_be[(size_t)b * a.nv + h] = be[t]; }
        }
        // kv = sum_i fma(S[i] e^g, k[i]); delta = (v - kv) beta; S' = fma(k, delta, S e^g); o = sum_i fma(S', q)
        const float g_exp = ge[t], beta_h = be[t];
        float kv = 0.0f;
#pragma unroll
        for (int i0 = 0; i0 < DK; i0 += 16) {
            float kk[16];
#pragma unroll
            for (int u = 0; u < 16; u++) kk[u] = kc[i0 + u];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < 16; u++) { c[i0 + u] = c[i0 + u] * g_exp; kv = __builtin_fmaf(c[i0 + u], kk[u], kv); }
            asm volatile("" : "+v"(kv));      // the block's chain ends here: the next block's LDS reads are not gathered ahead of it
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
                c[i0 + u] = __builtin_fmaf(kk[u], delta, c[i0 + u]);      // the new state stays in the column
                ob = __builtin_fmaf(c[i0 + u], qq[u], ob);
            }
            asm volatile("" : "+v"(ob));
            __builtin_amdgcn_sched_barrier(0);
        }
        rr[j] = ob;
        __syncthreads();
        if (j < 8) { const float ss = kr_sumsq8<0, 0>(rr, dv, j); if (j == 0) rms_s = kr_rms_inv(ss, dv, a.eps); }
        __syncthreads();
        a.out[(size_t)b * a.ld_out + (size_t)h * dv + j] = kr_gated_norm_out(ob, rms_s, wn, zz);
    }
    if constexpr (!VERIFY) {
#pragma unroll
        for (int i = 0; i < DK; i++) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(c[i]), srd, j * 4, i * dv * 4, 0);
    }
}

// commit of a verify pass: the slot of run ri advanced by the first n_keep[ri] tokens of the run, from the records of the verify-form launches above.  grid
// (value head, run, linear-attention layer), dv_max threads, one launch per key width (a workgroup of a layer of the other width returns).  Thread j < dv of
// head h < nv loads column j of the slot's state through the run kernel's buffer descriptor, applies per kept token the run kernel's update in its order
// (c[i] *= e^g; kv = fma chain over ascending i from 0; delta = (v - kv) beta; c[i] = fma(k[i], delta, c[i]) -- the output chain is not needed) and stores the
// column once.  Then the carried conv inputs: input q of a channel = x(n_keep - 4 + q), x(i < 0) = the slot's old input 4 + i (kr_spec_rollback_kernel's rule);
// the workgroups of (run, layer) stride over the layer's channels, each channel read and written by one thread.  No LDS, no barrier; a run that keeps nothing
// returns at once.  Bounds: rows come from the run table the verify pass itself indexed the records with (kr_m_run_row), t < n_keep <= cnt; the column's
// descriptor covers exactly head h's [DK][dv] block of the slot.
template <int DK>
__global__ void __launch_bounds__(256) kr_multi_la_commit_kernel(const KrMultiLaCommit* __restrict__ tab, const int* __restrict__ runs, const int* __restrict__ n_keep) {
    const KrMultiLaCommit E = tab[blockIdx.z];
    if (E.dk != DK) return;
    const int ri = blockIdx.y, keep = n_keep[ri];
    if (keep <= 0) return;
    const int slot = runs[3 * ri], row0 = runs[3 * ri + 1], cnt = runs[3 * ri + 2];
    const int h = blockIdx.x, j = threadIdx.x, nv = E.nv, dv = E.dv;
    if (h < nv && j < dv) {
        const __amdgpu_buffer_rsrc_t srd = __builtin_amdgcn_make_buffer_rsrc(E.recur + (size_t)slot * E.recur_stride + (size_t)h * DK * dv, 0, DK * dv * 4, 0x00020000);
        float c[DK];
#pragma unroll
        for (int i = 0; i < DK; i++) c[i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(srd, j * 4, i * dv * 4, 0));
#pragma unroll 1
        for (int t = 0; t < keep; t++) {
            const size_t b = (size_t)kr_m_run_row(ri, row0, cnt, t);
            const float* kr = E.rec_k + (b * E.nk + h / E.hr) * DK;
            const float g_exp = E.rec_ge[b * nv + h], beta_h = E.rec_be[b * nv + h], vj = E.rec_v[(b * nv + h) * dv + j];
            float kv = 0.0f;
#pragma unroll
            for (int i = 0; i < DK; i++) { c[i] = c[i] * g_exp; kv = __builtin_fmaf(c[i], kr[i], kv); }
            const float delta = (vj - kv) * beta_h;
#pragma unroll
            for (int i = 0; i < DK; i++) c[i] = __builtin_fmaf(kr[i], delta, c[i]);
        }
#pragma unroll
        for (int i = 0; i < DK; i++) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(c[i]), srd, j * 4, i * dv * 4, 0);
    }
    const int conv_dim = 2 * E.nk * DK + nv * dv;
    float4* cs = reinterpret_cast<float4*>(E.conv_state + (size_t)slot * E.conv_stride);
    for (int ch = blockIdx.x * blockDim.x + threadIdx.x; ch < conv_dim; ch += gridDim.x * blockDim.x) {
        const float4 o = cs[ch];
        float ns[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int i = keep - 4 + q, p = 4 + i;      // p in [1, 3] when i < 0 (keep >= 1)
            ns[q] = i >= 0 ? E.rec_x[(size_t)kr_m_run_row(ri, row0, cnt, i) * conv_dim + ch] : (p == 1 ? o.y : p == 2 ? o.z : o.w);
        }
        cs[ch] = float4{ns[0], ns[1], ns[2], ns[3]};
    }
}
void kr_launch_multi_la_commit(const KrMultiLaCommit* tab, int n_la, bool has64, bool has128, int nv_max, int dv_max, const int* runs, const int* n_keep,
                               int n_runs, hipStream_t st) {
    if (has128) hipLaunchKernelGGL(kr_multi_la_commit_kernel<128>, dim3(nv_max, n_runs, n_la), dim3(dv_max), 0, st, tab, runs, n_keep);
    if (has64) hipLaunchKernelGGL(kr_multi_la_commit_kernel<64>, dim3(nv_max, n_runs, n_la), dim3(dv_max), 0, st, tab, runs, n_keep);
}

int kr_launch_multi_la(const KrMultiLaArgs& a, const int* runs, int n_runs, int max_cnt, hipStream_t st, const KrMultiLxArgs* x) {
    if (max_cnt < 1 || max_cnt > KR_M_RUN_MAX) return 1;
    if ((a.dk != 64 && a.dk != 128) || a.dv < 8 || a.dv > 256 || a.dv % 8 || a.nv != a.nk * a.hr) return 1;
    const int conv_dim = 2 * a.nk * a.dk + a.nv * a.dv;
    const dim3 cg((conv_dim + 255) / 256, n_runs), rg(a.nv, n_runs);
    if (a.rec_x) {      // the verify form: records instead of state
        if (!a.rec_k || !a.rec_v || !a.rec_ge || !a.rec_be) return 1;
        hipLaunchKernelGGL(kr_multi_la_conv_kernel<true>, cg, dim3(256), 0, st, a, runs);
        if (a.dk == 128) hipLaunchKernelGGL((kr_multi_la_recur_kernel<128, true>), rg, dim3(a.dv), 0, st, a, runs);
        else hipLaunchKernelGGL((kr_multi_la_recur_kernel<64, true>), rg, dim3(a.dv), 0, st, a, runs);
        return 0;
    }
    // "multi_extend_la_chunk", a pass with a run of >= 64 tokens: the run kernels over the shorter runs (none: not launched), then the chunked rule over the
    // others.  Every check that can refuse the layer stands ahead of the first launch, which advances slot state: a layer fails whole
    if (a.lc_runs && (!kr_multi_lc_ok(a.dk, a.dv, a.nk, a.nv, a.ld_qkvz) || !a.lc_tiles || !a.lc_scratch || !a.lc_o || a.lc_nruns < 1 || a.lc_ntiles < a.lc_nruns)) return 1;
    // "multi_extend_la_exact", a pass with a run of >= a.lx_min tokens: the same shape -- the run kernels over the shorter runs, the staged form over the others
    if ((x != nullptr) != (a.lx_min != 0) || (x && (a.lc_runs || !kr_multi_lx_args_ok(a, *x)))) return 1;
    if (x && x->n_short == 0) return kr_launch_multi_la_exact(a, *x, runs, st);      // every run is staged: the run kernels are not launched
    if (!a.lc_runs || a.lc_short > 0) {
        hipLaunchKernelGGL(kr_multi_la_conv_kernel<false>, cg, dim3(256), 0, st, a, runs);
        if (a.dk == 128) hipLaunchKernelGGL((kr_multi_la_recur_kernel<128, false>), rg, dim3(a.dv), 0, st, a, runs);
        else hipLaunchKernelGGL((kr_multi_la_recur_kernel<64, false>), rg, dim3(a.dv), 0, st, a, runs);
    }
    if (a.lc_runs) return kr_launch_multi_la_chunk(a, runs, st);
    if (x) return kr_launch_multi_la_exact(a, *x, runs, st);
    return 0;
}

// ---- softmax of one score row by one wave: kr_m_wave_softmax and KR_MG_TILE, in kr_multi_softmax_dev.h (shared with kr_multi_split.hip) ----------------------------

// ---- GQA -----------------------------------------------------------------------------------------------------------------------------------------
// decode.rs:2873-2966 per row: gated split, per-head RMS norm (scalar sequential sum), half-split RoPE at the row's position, K / V into the row's
// slot.  grid (nh + nkv, B), 256 threads (hd <= 256).  The exact branch of kr_gqa_prep_kernel.
// PAGED (docs/design/21-paged-slots.md): the row lands in the page of the slot's table that holds its position; the flat instantiation is the code above it
template <bool PAGED>
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
            rms_s = kr_rms_inv(ss, hd, a.eps);
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
            size_t o;
            if constexpr (PAGED) {
                const int pg = max(a.page_table[(size_t)a.slots[row] * a.page_stride + (pos >> a.page_shift)], 0);      // mapped by the host before the pass
                o = (((size_t)pg << a.page_shift) | (size_t)(pos & ((1 << a.page_shift) - 1))) * a.nkv * hd + (size_t)h * hd + d;
            } else o = (size_t)a.slots[row] * a.slot_elems + (size_t)pos * a.nkv * hd + (size_t)h * hd + d;
            kr_kv_store(a.k_cache, o, val, a.kv_fp8);
            kr_kv_store(a.v_cache, o, a.v_in[(size_t)row * a.ld_v + (size_t)h * hd + d], a.kv_fp8);
        }
    }
}

// decode.rs:4194 per row: the G = nh / nkv query heads of KV head kvh over the slot's rows [0, pos].  grid (nkv, B), 256 threads; every K and V row
// of the sequence is read once for the G heads.  Scores: 8 lanes per position, lane l chains fma over elements e * 8 + l (ascending e) and the
// 8-lane hsum -- one K row in registers serves all G heads.  Softmax: one wave per head (rounds of 4 heads), kr_m_wave_softmax.
// P.V: thread t owns output d = t % hd of heads t / hd, t / hd + 256 / hd, ..: one fma per position, ascending.
#define KR_MG_PT 64          // positions per P.V stage
#define KR_MG_ACC 16         // heads per thread and pass of the P.V loop
// PAGED: the slot's table slice for [0, seq) is loaded into LDS once, and position s is row (page << shift) | (s & mask) of the pools; the loops and their
// order are the flat kernel's
template <int NB, bool FP8, bool PAGED>
__global__ void __launch_bounds__(256) kr_multi_gqa_attn_kernel(const KrMultiGqaArgs a) {
    constexpr int HD = NB * 8;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int G = a.nh / a.nkv;
    float* qs = sm;                                  // [G][HD]
    float* tile = qs + (size_t)G * HD;               // [4][KR_MG_TILE]
    float* pt = tile + 4 * KR_MG_TILE;               // [G][KR_MG_PT]
    const int kvh = blockIdx.x, row = blockIdx.y, t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (kr_m_row_in_run(a, row)) return;      // "multi_extend_flash": the last token of a run of >= 2, attended to by the run kernels (workgroup-uniform, ahead of every barrier)
    const int pos = a.positions[row], seq = pos + 1, kvs = a.nkv * HD;
    const size_t kv0 = PAGED ? (size_t)kvh * HD : (size_t)a.slots[row] * a.slot_elems + (size_t)kvh * HD;      // element of (position 0, this KV head) in the slot (paged: in a page)
    const int* pgt = reinterpret_cast<const int*>(pt + (size_t)G * KR_MG_PT);      // PAGED: [ceil(seq / page_tokens)] page ids of the slot
    const int psh = PAGED ? a.page_shift : 0, pmask = (1 << psh) - 1;
    if constexpr (PAGED) {
        const int* src = a.page_table + (size_t)a.slots[row] * a.page_stride;
        int* dst = reinterpret_cast<int*>(pt + (size_t)G * KR_MG_PT);
        for (int i = t; i < ((seq + pmask) >> psh); i += 256) dst[i] = max(src[i], 0);      // every page of [0, seq) was mapped by the host before the pass
    }
    // element of (position s, this KV head)
    auto kvat = [&](int s) -> size_t {
        if constexpr (PAGED) return kv0 + (((size_t)pgt[s >> psh] << psh) | (size_t)(s & pmask)) * kvs;
        else return kv0 + (size_t)s * kvs;
    };
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
            for (int e = 0; e < NB; e++) kr[e] = kr_kv_load(a.k_cache, kvat(s) + e * 8 + l, FP8);
            for (int g = 0; g < G; g++) {
                float acc = 0.0f;
#pragma unroll
                for (int e = 0; e < NB; e++) acc = __builtin_fmaf(qs[g * HD + e * 8 + l], kr[e], acc);
                acc = kr_hsum8(acc);
                if (l == 0) sc[(size_t)g * a.sc_ld + s] = acc * a.sm_scale;
            }
        }
    }
    __syncthreads();
    // ---- softmax, one wave per head
    float* tw = tile + w * KR_MG_TILE;
    for (int g0 = 0; g0 < G; g0 += 4) {
        const int g = g0 + w;
        const bool on = g < G;
        kr_m_wave_softmax(sc + (size_t)(on ? g : 0) * a.sc_ld, seq, tw, on, lane);
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
                for (int u = 0; u < 16; u++) v[u] = kr_kv_load(a.v_cache, kvat(s0 + min(s1 + u, n - 1)) + d, FP8);
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

size_t kr_multi_gqa_lds_bytes(int G, int hd, int page_stride) {
    return ((size_t)G * hd + 4 * KR_MG_TILE + (size_t)G * KR_MG_PT + (size_t)page_stride) * 4;
}

static int multi_gqa_runs(const KrMultiGqaArgs& a, int B, size_t lds, hipStream_t st);      // below
int kr_launch_multi_gqa(const KrMultiGqaArgs& a, int B, hipStream_t st) {
    if ((a.hd != 64 && a.hd != 128 && a.hd != 256) || a.nkv < 1 || a.nh % a.nkv || a.sc_ld % 32) return 1;
    const int G = a.nh / a.nkv;
    const size_t lds = kr_multi_gqa_lds_bytes(G, a.hd, a.page_table ? a.page_stride : 0);
    if (a.pf_tiles) return multi_gqa_runs(a, B, lds, st);
    if (a.fd_o) {
        // "multi_attn_fast" / "multi_attn_fast_paged": the same prep launch, then split-KV flash-decode over the slots, flat or paged (kr_multi_flash.hip)
        if (!kr_multi_fd_ok(a.nh, a.nkv, a.hd) || !a.fd_ml || a.fd_chunks < 1 || a.fd_chunks > 1024) return 1;
        if (a.page_table) {
            if (a.page_stride < 1 || a.page_shift < 5) return 1;
            hipLaunchKernelGGL(kr_multi_gqa_prep_kernel<true>, dim3(a.nh + a.nkv, B), dim3(256), 0, st, a);
        } else hipLaunchKernelGGL(kr_multi_gqa_prep_kernel<false>, dim3(a.nh + a.nkv, B), dim3(256), 0, st, a);
        return kr_launch_multi_fd(a, B, a.fd_chunks, st);
    }
    if (lds > KR_MULTI_GQA_LDS_MAX) return 1;
#define KR_MGA(NB_, F_, P_) hipLaunchKernelGGL((kr_multi_gqa_attn_kernel<NB_, F_, P_>), dim3(a.nkv, B), dim3(256), lds, st, a)
#define KR_MGA_HD(F_, P_) do { if (a.hd == 256) KR_MGA(32, F_, P_); else if (a.hd == 128) KR_MGA(16, F_, P_); else KR_MGA(8, F_, P_); } while (0)
    if (a.page_table) {
        if (a.page_stride < 1 || a.page_shift < 5) return 1;
        hipLaunchKernelGGL(kr_multi_gqa_prep_kernel<true>, dim3(a.nh + a.nkv, B), dim3(256), 0, st, a);
        if (a.xs_split) return kr_launch_multi_gqa_split(a, B, st);      // "multi_attn_exact_split": the same bits from three launches (kr_multi_split.hip)
        if (a.kv_fp8) KR_MGA_HD(true, true); else KR_MGA_HD(false, true);
        return 0;
    }
    hipLaunchKernelGGL(kr_multi_gqa_prep_kernel<false>, dim3(a.nh + a.nkv, B), dim3(256), 0, st, a);
    if (a.xs_split) return kr_launch_multi_gqa_split(a, B, st);
    if (a.kv_fp8) KR_MGA_HD(true, false); else KR_MGA_HD(false, false);
#undef KR_MGA_HD
#undef KR_MGA
    return 0;
}

// "multi_extend_flash", a pass with a run of >= 2 tokens (docs/design/25-multi-extend-flash.md): the prep launch over all B rows as ever; the per-row attention
// kernels -- the exact one, or the flash-decode pair when a.fd_o is set -- over the first pf_nruns rows, where every unit row lies (the rows of longer runs
// leave at once), and not at all without a unit row; then the run kernels over the query tiles
static int multi_gqa_runs(const KrMultiGqaArgs& a, int B, size_t lds, hipStream_t st) {
    // every check first: the prep launch appends rows to the slots, and a layer fails whole
    if (a.pf_nruns < 1 || a.pf_nruns > B || a.pf_units < 0 || a.pf_units >= a.pf_nruns || !kr_multi_pf_args_ok(a)) return 1;
    if (a.page_table && (a.page_stride < 1 || a.page_shift < 5)) return 1;
    if (a.pf_units && a.fd_o && (!kr_multi_fd_ok(a.nh, a.nkv, a.hd) || !a.fd_ml || a.fd_chunk < 64 || a.fd_chunks < 1 || a.fd_chunks > 1024)) return 1;
    if (a.pf_units && !a.fd_o && lds > KR_MULTI_GQA_LDS_MAX) return 1;
    if (a.page_table) hipLaunchKernelGGL(kr_multi_gqa_prep_kernel<true>, dim3(a.nh + a.nkv, B), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(kr_multi_gqa_prep_kernel<false>, dim3(a.nh + a.nkv, B), dim3(256), 0, st, a);
    if (a.pf_units) {
        if (a.fd_o) {
            if (kr_launch_multi_fd(a, a.pf_nruns, a.fd_chunks, st)) return 1;
        } else if (a.xs_split) {      // "multi_attn_exact_split": the unit rows' attention as three launches
            if (kr_launch_multi_gqa_split(a, a.pf_nruns, st)) return 1;
        } else {
#define KR_MGR(NB_, F_, P_) hipLaunchKernelGGL((kr_multi_gqa_attn_kernel<NB_, F_, P_>), dim3(a.nkv, a.pf_nruns), dim3(256), lds, st, a)
#define KR_MGR_HD(F_, P_) do { if (a.hd == 256) KR_MGR(32, F_, P_); else if (a.hd == 128) KR_MGR(16, F_, P_); else KR_MGR(8, F_, P_); } while (0)
            if (a.page_table) { if (a.kv_fp8) KR_MGR_HD(true, true); else KR_MGR_HD(false, true); }
            else { if (a.kv_fp8) KR_MGR_HD(true, false); else KR_MGR_HD(false, false); }
#undef KR_MGR_HD
#undef KR_MGR
        }
    }
    return kr_launch_multi_pf_flash(a, st);
}

// "multi_extend_exact_mfma", a non-verify pass with a run of >= 2 tokens (docs/design/28-multi-extend-exact-mfma.md): the prep launch over all B rows as ever; the
// per-row attention kernels over the first n_runs rows, where every unit row lies (kr_m_row_in_run: the rows of longer runs leave at once), and not at all without
// a unit row; then the three exact passes over the runs' query tiles (kr_multi_xm.hip).  pf_tiles stays null: kr_launch_multi_gqa never comes here by itself
int kr_launch_multi_gqa_xm(const KrMultiGqaArgs& a0, const KrMultiXmArgs& x, const int* runs, int n_runs, int units, int B, hipStream_t st) {
    KrMultiGqaArgs a = a0;
    a.pf_runs = runs; a.pf_nruns = n_runs; a.pf_units = units; a.pf_tiles = nullptr; a.pf_ntiles = 0;
    // every check first: the prep launch appends rows to the slots, and a layer fails whole
    if ((a.hd != 64 && a.hd != 128 && a.hd != 256) || a.nkv < 1 || a.nh % a.nkv || a.sc_ld % 32) return 1;
    const size_t lds = kr_multi_gqa_lds_bytes(a.nh / a.nkv, a.hd, a.page_table ? a.page_stride : 0);
    if (n_runs < 1 || n_runs > B || units < 0 || units >= n_runs || !kr_multi_xm_args_ok(a, x)) return 1;
    if (units && a.fd_o && (!kr_multi_fd_ok(a.nh, a.nkv, a.hd) || !a.fd_ml || a.fd_chunk < 64 || a.fd_chunks < 1 || a.fd_chunks > 1024)) return 1;
    if (units && !a.fd_o && lds > KR_MULTI_GQA_LDS_MAX) return 1;
    if (a.page_table) hipLaunchKernelGGL(kr_multi_gqa_prep_kernel<true>, dim3(a.nh + a.nkv, B), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(kr_multi_gqa_prep_kernel<false>, dim3(a.nh + a.nkv, B), dim3(256), 0, st, a);
    if (units) {
        if (a.fd_o) {
            if (kr_launch_multi_fd(a, n_runs, a.fd_chunks, st)) return 1;
        } else if (a.xs_split) {      // "multi_attn_exact_split": the unit rows' attention as three launches
            if (kr_launch_multi_gqa_split(a, n_runs, st)) return 1;
        } else {
#define KR_MGX(NB_, F_, P_) hipLaunchKernelGGL((kr_multi_gqa_attn_kernel<NB_, F_, P_>), dim3(a.nkv, n_runs), dim3(256), lds, st, a)
#define KR_MGX_HD(F_, P_) do { if (a.hd == 256) KR_MGX(32, F_, P_); else if (a.hd == 128) KR_MGX(16, F_, P_); else KR_MGX(8, F_, P_); } while (0)
            if (a.page_table) { if (a.kv_fp8) KR_MGX_HD(true, true); else KR_MGX_HD(false, true); }
            else { if (a.kv_fp8) KR_MGX_HD(true, false); else KR_MGX_HD(false, false); }
#undef KR_MGX_HD
#undef KR_MGX
        }
    }
    return kr_launch_multi_xm(a, x, B, st);
}

// ---- MLA (docs/design/15-multi-mla.md) -----------------------------------------------------------------------------------------------------------
// The arithmetic specification is kr_mla_prep_kernel / kr_mla_attn_kernel (kr_mla.hip); the sections of the prep launch are the shared device
// functions of kr_mla_dev.h.  grid (nh * klr / 64 + 1, B) -- or (nh + 1, B) when the matrix-core absorption has produced q_abs -- 64 threads:
// workgroups below the last: absorption tile (h, jt) of row b, the jt == 0 one also ropes q_pe[h] at the row's position; the last: latent RMSNorm,
// k_pe rope, both rows stored at the row's position of the row's slot.
// PAGED: kr_mla_append_row receives the base of the page that holds the position, and the position inside it
template <bool FP8, bool PAGED>
__global__ void __launch_bounds__(64) kr_multi_mla_prep_kernel(const KrMultiMlaArgs a) {
    __shared__ float sh[640];
    const int row = blockIdx.y, pos = a.positions[row];
    const int tiles = a.absorb_done ? 1 : a.klr / 64, nb_abs = a.nh * tiles, hd = a.nd + a.rd;
    if ((int)blockIdx.x < nb_abs) {
        const int h = blockIdx.x / tiles, jt = blockIdx.x % tiles;
        const float* qh = a.q_full + (size_t)row * a.ld_q + (size_t)h * hd;
        if (!a.absorb_done) kr_mla_absorb_tile(qh, a.w_kc + (size_t)h * a.nd * a.klr, a.q_abs + ((size_t)row * a.nh + h) * a.klr, jt * 64 + (int)threadIdx.x, a.nd, a.klr, sh);
        if (jt == 0) kr_mla_rope_qpe(qh, a.q_pe + ((size_t)row * a.nh + h) * a.rd, a.rope_cos, a.rope_sin, pos, a.nd, a.rd / 2);
        return;
    }
    const size_t slot = (size_t)a.slots[row];
    if constexpr (PAGED) {      // ckv_stride / kpe_stride = bytes of one page; the rope tables are still read at the position itself
        const size_t pg = (size_t)max(a.page_table[slot * a.page_stride + (pos >> a.page_shift)], 0);      // mapped by the host before the pass
        kr_mla_append_row<FP8>(a.kv_out + (size_t)row * a.ld_kv, a.kv_a_norm, a.rope_cos, a.rope_sin, (char*)a.ckv_cache + pg * a.ckv_stride,
                               (char*)a.kpe_cache + pg * a.kpe_stride, pos, a.klr, a.rd, a.eps, sh, pos & ((1 << a.page_shift) - 1));
    } else {
        kr_mla_append_row<FP8>(a.kv_out + (size_t)row * a.ld_kv, a.kv_a_norm, a.rope_cos, a.rope_sin, (char*)a.ckv_cache + slot * a.ckv_stride,
                               (char*)a.kpe_cache + slot * a.kpe_stride, pos, a.klr, a.rd, a.eps, sh);
    }
}

// Attention of KR_MM_HG heads of row b over the slot's rows [0, pos].  grid (ceil(nh / KR_MM_HG), B), 512 threads.  The latent + rope rows are
// shared by every head of the row: KR_MM_ROWS of them at a time are fetched with 16-byte buffer loads (num_records = the row's current length: rows
// past it read as zero), committed to LDS while the next stage's loads are in flight, and serve all heads of the group.
//   scores: 16 lanes per (position, head) pair -- kr_dot2acc over klr + kr_dot2acc over rd, x sm_scale (the query slice stays in registers) -- into the
//           row's global score rows, so the form (and its bits) does not depend on the slot capacity
//   softmax: one wave per head (kr_m_wave_softmax)
//   weighted sum: the rows staged again; thread t owns latent element t % klr of heads t / klr + k * (512 / klr): one fma per position, ascending
#define KR_MM_ROWS 32
#define KR_MM_HG 4
static_assert(KR_PAGE_MIN_TOKENS % KR_MM_ROWS == 0, "a stage of the MLA attention kernel lies in one page");
// PAGED: a stage lies in one page (page_tokens is a multiple of KR_MM_ROWS), so each stage builds its two descriptors from that page's base with
// num_records = the page's rows below the current length; a stage past the end or in an unmapped page gets num_records 0 and reads zeros
template <bool FP8, int NBC, bool PAGED>
__global__ void __launch_bounds__(512) kr_multi_mla_attn_kernel(const KrMultiMlaArgs a) {
    constexpr int klr = NBC * 8, NBR = 8, rd = NBR * 8, esz = FP8 ? 1 : 2, HG = KR_MM_HG, ROWS = KR_MM_ROWS;
    constexpr int CPR_C = klr * esz / 16, CPR_R = rd * esz / 16, pitch = (klr + rd) * esz + 16, NLC = ROWS * CPR_C / 512;
    static_assert(ROWS * CPR_C % 512 == 0 && ROWS * CPR_R <= 512 && 512 % klr == 0 && HG % (512 / klr) == 0 && ROWS * HG <= 512 && 32 % HG == 0, "work split");
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* qa = sm;                                  // [HG][klr]
    float* qp = qa + HG * klr;                       // [HG][rd]
    float* tile = qp + HG * rd;                      // [4][KR_MG_TILE]
    float* pt = tile + 4 * KR_MG_TILE;               // [ROWS][HG]
    unsigned char* stage = reinterpret_cast<unsigned char*>(pt + ROWS * HG);      // [ROWS][pitch]
    const int row = blockIdx.y, hg0 = blockIdx.x * HG, nhg = min(HG, a.nh - hg0), t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (kr_m_row_in_run(a, row)) return;      // "multi_extend_mla_flash": the last token of a run of >= 2, attended to by the run kernel (workgroup-uniform, ahead of every barrier)
    const int seq = a.positions[row] + 1, nst = (seq + ROWS - 1) / ROWS;
    const size_t slot = (size_t)a.slots[row];
    float* sc = a.scores + ((size_t)row * a.nh + hg0) * a.sc_ld;                  // [nhg][sc_ld]
    const __amdgpu_buffer_rsrc_t srd_c = __builtin_amdgcn_make_buffer_rsrc((char*)a.ckv_cache + (PAGED ? 0 : slot * a.ckv_stride), 0, PAGED ? 0 : seq * klr * esz, 0x00020000);
    const __amdgpu_buffer_rsrc_t srd_r = __builtin_amdgcn_make_buffer_rsrc((char*)a.kpe_cache + (PAGED ? 0 : slot * a.kpe_stride), 0, PAGED ? 0 : seq * rd * esz, 0x00020000);
    // PAGED: the page of stage s0 (a multiple of ROWS) -> its id made wave-uniform for the descriptors (-1: none) and the rows of it that are below seq
    const int psh = PAGED ? a.page_shift : 0, pmask = (1 << psh) - 1;
    const int* ptab = PAGED ? a.page_table + slot * a.page_stride : nullptr;
    auto page_of = [&](int s0, int& nrec) -> int {
        int pg = -1;
        if (s0 < seq) pg = ptab[s0 >> psh];
        pg = __builtin_amdgcn_readfirstlane(pg);
        nrec = pg >= 0 ? min(1 << psh, seq - (s0 & ~pmask)) : 0;
        return max(pg, 0);
    };
    // unconditional loads: rows at or past the current length are outside the descriptors and read as zero
    struct Regs { u32x4 c[NLC]; u32x4 r; };
    const int rrow = t / CPR_R, rcol = t % CPR_R;
    const bool has_r = t < ROWS * CPR_R;
    auto issue_c = [&](Regs& R, int s0) {
        __amdgpu_buffer_rsrc_t srd = srd_c; int r0 = s0;      // the descriptor and the first row of the stage inside it
        if constexpr (PAGED) {
            int nrec; const int pg = page_of(s0, nrec);
            srd = __builtin_amdgcn_make_buffer_rsrc((char*)a.ckv_cache + (size_t)pg * a.ckv_stride, 0, nrec * klr * esz, 0x00020000);
            r0 = s0 & pmask;
        }
#pragma unroll
        for (int i = 0; i < NLC; i++) {
            const int c = t + 512 * i, r = c / CPR_C, col = c % CPR_C;
            R.c[i] = __builtin_amdgcn_raw_buffer_load_b128(srd, (r0 + r) * klr * esz + col * 16, 0, 0);
        }
    };
    auto issue_r = [&](Regs& R, int s0) {
        __amdgpu_buffer_rsrc_t srd = srd_r; int r0 = s0;
        if constexpr (PAGED) {
            int nrec; const int pg = page_of(s0, nrec);
            srd = __builtin_amdgcn_make_buffer_rsrc((char*)a.kpe_cache + (size_t)pg * a.kpe_stride, 0, nrec * rd * esz, 0x00020000);
            r0 = s0 & pmask;
        }
        R.r = __builtin_amdgcn_raw_buffer_load_b128(srd, has_r ? (r0 + rrow) * rd * esz + rcol * 16 : 0x7FFFFFF0, 0, 0);
    };
    auto commit_c = [&](const Regs& R) {
#pragma unroll
        for (int i = 0; i < NLC; i++) {
            const int c = t + 512 * i, r = c / CPR_C, col = c % CPR_C;
            *reinterpret_cast<u32x4*>(stage + r * pitch + col * 16) = R.c[i];
        }
    };
    auto commit_r = [&](const Regs& R) { if (has_r) *reinterpret_cast<u32x4*>(stage + rrow * pitch + klr * esz + rcol * 16) = R.r; };
    Regs rg;
    issue_c(rg, 0); issue_r(rg, 0);
    for (int i = t; i < nhg * klr; i += 512) qa[i] = a.q_abs[((size_t)row * a.nh + hg0) * klr + i];
    for (int i = t; i < nhg * rd; i += 512) qp[i] = a.q_pe[((size_t)row * a.nh + hg0) * rd + i];
    __syncthreads();
    // ---- scores (kr_mla_scores_kernel's lane roles): lane c16 = (accumulator a2, AVX lane l) owns the 8-blocks i % 2 == a2, ascending
    {
        const int c16 = t & 15, a2 = c16 >> 3, l = c16 & 7, g = t >> 4, hh = g % HG, prow = g / HG;
        const bool hon = hh < nhg;
        constexpr int NQC = NBC / 2, NQR = NBR / 2;
        float qc[NQC], qr[NQR];
#pragma unroll
        for (int u = 0; u < NQC; u++) qc[u] = hon ? qa[hh * klr + (2 * u + a2) * 8 + l] : 0.0f;
#pragma unroll
        for (int u = 0; u < NQR; u++) qr[u] = hon ? qp[hh * rd + (2 * u + a2) * 8 + l] : 0.0f;
        float* out = sc + (size_t)(hon ? hh : 0) * a.sc_ld;
        for (int st = 0; st < nst; st++) {
            if (st) __syncthreads();                 // the previous stage has been consumed
            commit_c(rg); commit_r(rg);
            issue_c(rg, (st + 1) * ROWS); issue_r(rg, (st + 1) * ROWS);      // past the end: zeros, never used
            __syncthreads();
            const int s0 = st * ROWS;
#pragma unroll 1
            for (int pass = 0; pass < ROWS / (32 / HG); pass++) {
                const int r = prow + (32 / HG) * pass;
                if (!hon || s0 + r >= seq) continue;          // uniform over the 16 lanes of a pair
                const unsigned char* srow = stage + r * pitch;
                float kc[NQC], kr[NQR];
#pragma unroll
                for (int u = 0; u < NQC; u++) kc[u] = kr_stage_val<FP8>(srow, (2 * u + a2) * 8 + l);
#pragma unroll
                for (int u = 0; u < NQR; u++) kr[u] = kr_stage_val<FP8>(srow + klr * esz, (2 * u + a2) * 8 + l);
                float acc = 0.0f;
#pragma unroll
                for (int u = 0; u < NQC; u++) acc = __builtin_fmaf(qc[u], kc[u], acc);
                float v = kr_mla_pair_hsum(acc, a2);
                acc = 0.0f;
#pragma unroll
                for (int u = 0; u < NQR; u++) acc = __builtin_fmaf(qr[u], kr[u], acc);
                v += kr_mla_pair_hsum(acc, a2);
                v *= a.sm_scale;
                if (c16 == 0) out[s0 + r] = v;
            }
        }
    }
    issue_c(rg, 0);                                  // the first stage of the weighted sum rides under the softmax
    __syncthreads();
    // ---- softmax: wave w < nhg takes head hg0 + w
    {
        const bool on = w < nhg;
        kr_m_wave_softmax(sc + (size_t)(on ? w : 0) * a.sc_ld, seq, tile + (w & 3) * KR_MG_TILE, on, lane);
    }
    // ---- weighted sum
    constexpr int TPH = 512 / klr, KH = HG / TPH;    // threads per latent element; heads per thread: hq + k * TPH
    const int j = t % klr, hq = t / klr;
    float o[KH];
#pragma unroll
    for (int k = 0; k < KH; k++) o[k] = 0.0f;
    for (int st = 0; st < nst; st++) {
        __syncthreads();                             // the scaled score rows are written / the previous stage has been consumed
        commit_c(rg);
        issue_c(rg, (st + 1) * ROWS);
        const int s0 = st * ROWS, n = min(ROWS, seq - s0);
        if (t < ROWS * HG) { const int r = t / HG, h = t % HG; pt[t] = (r < n && h < nhg) ? sc[(size_t)h * a.sc_ld + s0 + r] : 0.0f; }
        __syncthreads();
        for (int r = 0; r < n; r += 8) {             // n <= ROWS and r % 8 == 0: rows r .. r + 7 are inside the stage
            float vv[8], pp[8][KH];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                vv[u] = kr_stage_val<FP8>(stage + (r + u) * pitch, j);
#pragma unroll
                for (int k = 0; k < KH; k++) pp[u][k] = pt[(r + u) * HG + hq + k * TPH];
            }
#pragma unroll
            for (int u = 0; u < 8; u++)
                if (r + u < n) {
#pragma unroll
                    for (int k = 0; k < KH; k++) o[k] = __builtin_fmaf(pp[u][k], vv[u], o[k]);
                }
        }
    }
#pragma unroll
    for (int k = 0; k < KH; k++) {
        const int h = hq + k * TPH;
        if (h < nhg) a.attn_lat[((size_t)row * a.nh + hg0 + h) * klr + j] = o[k];
    }
}
template <bool FP8, int NBC> static constexpr size_t kr_multi_mla_lds() {
    return ((size_t)KR_MM_HG * (NBC * 8 + 64) + 4 * KR_MG_TILE + KR_MM_ROWS * KR_MM_HG) * 4 + (size_t)KR_MM_ROWS * ((NBC * 8 + 64) * (FP8 ? 1 : 2) + 16);
}

int kr_multi_mla_ok(int klr, int nd, int rd) { return (klr == 512 || klr == 256) && rd == 64 && nd >= 1 && nd <= 640; }

// "multi_extend_mla_flash", a pass with a run of >= 2 tokens (docs/design/27-multi-extend-mla-flash.md): the absorption, the prep launch and the w_vc projection
// over all B rows as ever; the per-row attention kernels -- the exact one, or the flash-decode pair when a.fd_o is set -- over the first mf_nruns rows, where
// every unit row lies (the rows of longer runs leave at once), and not at all without a unit row; the run kernel over the query tiles
static int multi_mla_runs(KrMultiMlaArgs& a, int B, hipStream_t st) {
    // every check first: the prep launch appends rows to the slots, and a layer fails whole
    if (a.mf_nruns < 1 || a.mf_nruns > B || a.mf_units < 0 || a.mf_units >= a.mf_nruns || !kr_multi_mla_pf_args_ok(a)) return 1;
    if (a.mf_units && a.fd_o && (!kr_multi_mla_fd_ok(a.nh, a.klr, a.rd) || !a.fd_ml || a.fd_chunk < 32 || a.fd_chunk % 32 || a.fd_chunks < 1 || a.fd_chunks > 1024)) return 1;
    if (a.mf_units && !a.fd_o && (!a.scores || a.sc_ld < 32)) return 1;
    a.absorb_done = B >= 32 && kr_launch_mla_absorb_mfma(a.q_full, a.ld_q, a.nd + a.rd, a.nd, a.w_kc, a.klr, a.q_abs, B, a.nh, st) == 0;
    const dim3 pg(a.nh * (a.absorb_done ? 1 : a.klr / 64) + 1, B), ag((a.nh + KR_MM_HG - 1) / KR_MM_HG, a.mf_nruns);
    const bool rows = a.mf_units && !a.fd_o && !a.xs_split;      // the exact per-row kernel has a row to take ("multi_mla_exact_split": the three launches below)
#define KR_MRP(F_, P_) hipLaunchKernelGGL((kr_multi_mla_prep_kernel<F_, P_>), pg, dim3(64), 0, st, a)
#define KR_MRA(F_, NBC_, P_) hipLaunchKernelGGL((kr_multi_mla_attn_kernel<F_, NBC_, P_>), ag, dim3(512), (kr_multi_mla_lds<F_, NBC_>()), st, a)
#define KR_MRA_ALL(P_) do { \
    if (a.kv_fp8) { KR_MRP(true, P_); if (!rows) break; if (a.klr == 512) KR_MRA(true, 64, P_); else KR_MRA(true, 32, P_); } \
    else { KR_MRP(false, P_); if (!rows) break; if (a.klr == 512) KR_MRA(false, 64, P_); else KR_MRA(false, 32, P_); } } while (0)
    if (a.page_table) KR_MRA_ALL(true); else KR_MRA_ALL(false);
#undef KR_MRA_ALL
#undef KR_MRA
#undef KR_MRP
    if (a.mf_units && a.fd_o && kr_launch_multi_mla_fd(a, a.mf_nruns, st)) return 1;
    if (a.mf_units && !a.fd_o && a.xs_split && kr_launch_multi_mla_split(a, a.mf_nruns, st)) return 1;      // "multi_mla_exact_split": the unit rows' attention as three launches
    if (kr_launch_multi_mla_pf_flash(a, st)) return 1;
    if (B >= 32 && kr_launch_mla_wvc_mfma(a.w_vc, a.attn_lat, a.v_proj, B, a.nh, a.vhd, a.klr, st) == 0) return 0;
    KrMlaArgs m{};
    m.step = nullptr; m.pos0 = 0; m.kv_out = a.kv_out; m.ld_kv = a.ld_kv; m.q_full = a.q_full; m.ld_q = a.ld_q; m.w_vc = a.w_vc;
    m.q_abs = a.q_abs; m.q_pe = a.q_pe; m.attn_lat = a.attn_lat; m.v_proj = a.v_proj; m.nh = a.nh; m.klr = a.klr; m.nd = a.nd; m.rd = a.rd; m.vhd = a.vhd;
    kr_launch_mla_wvc(m, st, B);
    return 0;
}

int kr_launch_multi_mla(const KrMultiMlaArgs& a_in, int B, hipStream_t st) {
    KrMultiMlaArgs a = a_in;
    if (!kr_multi_mla_ok(a.klr, a.nd, a.rd) || a.nh < 1 || a.sc_ld % 32) return 1;
    if (a.page_table && (a.page_stride < 1 || (1 << a.page_shift) < KR_MM_ROWS)) return 1;      // a stage must not straddle a page
    static_assert(kr_multi_mla_lds<false, 64>() <= 64 * 1024, "the attention kernel stays inside the default 64 KiB LDS window");
    // "multi_mla_fast" (a.fd_o set): the same absorption and prep launch, then split-KV flash-decode over the slots, flat or paged
    // (kr_multi_mla_flash.hip) in place of the attention kernel; checked before anything is launched
    if (a.fd_o && (!kr_multi_mla_fd_ok(a.nh, a.klr, a.rd) || !a.fd_ml || a.fd_chunk < 32 || a.fd_chunk % 32 || a.fd_chunks < 1 || a.fd_chunks > 1024)) return 1;
    if (a.mf_tiles) return multi_mla_runs(a, B, st);      // "multi_extend_mla_flash", a pass with a run of >= 2 tokens
    // the w_kc absorption, row-wise: from 32 rows on the matrix cores (one fma chain per output, the prompt pass's launch), the prep launch's tiles below
    a.absorb_done = B >= 32 && kr_launch_mla_absorb_mfma(a.q_full, a.ld_q, a.nd + a.rd, a.nd, a.w_kc, a.klr, a.q_abs, B, a.nh, st) == 0;
    const dim3 pg(a.nh * (a.absorb_done ? 1 : a.klr / 64) + 1, B), ag((a.nh + KR_MM_HG - 1) / KR_MM_HG, B);
#define KR_MMP(F_, P_) hipLaunchKernelGGL((kr_multi_mla_prep_kernel<F_, P_>), pg, dim3(64), 0, st, a)
#define KR_MMA(F_, NBC_, P_) hipLaunchKernelGGL((kr_multi_mla_attn_kernel<F_, NBC_, P_>), ag, dim3(512), (kr_multi_mla_lds<F_, NBC_>()), st, a)
#define KR_MMA_ALL(P_) do { \
    if (a.kv_fp8) { KR_MMP(true, P_); if (a.fd_o) break; if (a.xs_split) break; if (a.klr == 512) KR_MMA(true, 64, P_); else KR_MMA(true, 32, P_); } \
    else { KR_MMP(false, P_); if (a.fd_o) break; if (a.xs_split) break; if (a.klr == 512) KR_MMA(false, 64, P_); else KR_MMA(false, 32, P_); } } while (0)
    if (a.page_table) KR_MMA_ALL(true); else KR_MMA_ALL(false);
#undef KR_MMA_ALL
#undef KR_MMA
#undef KR_MMP
    if (a.fd_o && kr_launch_multi_mla_fd(a, B, st)) return 1;
    if (!a.fd_o && a.xs_split && kr_launch_multi_mla_split(a, B, st)) return 1;      // "multi_mla_exact_split": the attention as three launches, flat or paged
    // the w_vc projection, row-wise: the prompt pass's matrix-core launch from 32 rows, the decode launch with a token dimension below
    if (B >= 32 && kr_launch_mla_wvc_mfma(a.w_vc, a.attn_lat, a.v_proj, B, a.nh, a.vhd, a.klr, st) == 0) return 0;
    KrMlaArgs m{};
    m.step = nullptr; m.pos0 = 0; m.kv_out = a.kv_out; m.ld_kv = a.ld_kv; m.q_full = a.q_full; m.ld_q = a.ld_q; m.w_vc = a.w_vc;
    m.q_abs = a.q_abs; m.q_pe = a.q_pe; m.attn_lat = a.attn_lat; m.v_proj = a.v_proj; m.nh = a.nh; m.klr = a.klr; m.nd = a.nd; m.rd = a.rd; m.vhd = a.vhd;
    kr_launch_mla_wvc(m, st, B);
    return 0;
}

// "multi_extend_mla_exact_mfma", a non-verify pass with a run of >= 2 tokens (docs/design/29-multi-extend-mla-exact-mfma.md): the absorption, the prep launch and the
// w_vc projection over all B rows as ever; the per-row attention kernels over the first n_runs rows, where every unit row lies (kr_m_row_in_run: the rows of
// longer runs leave at once), and not at all without a unit row; the three exact passes over the runs' query tiles (kr_multi_mla_xm.hip).  mf_tiles stays null:
// kr_launch_multi_mla never goes to multi_mla_runs by itself
int kr_launch_multi_mla_xm(const KrMultiMlaArgs& a0, const KrMultiXmArgs& x, const int* runs, int n_runs, int units, int B, hipStream_t st) {
    KrMultiMlaArgs a = a0;
    a.mf_runs = runs; a.mf_nruns = n_runs; a.mf_units = units; a.mf_tiles = nullptr; a.mf_ntiles = 0;
    // every check first: the prep launch appends rows to the slots, and a layer fails whole
    if (!kr_multi_mla_ok(a.klr, a.nd, a.rd) || a.nh < 1 || a.sc_ld % 32) return 1;
    if (a.page_table && (a.page_stride < 1 || (1 << a.page_shift) < KR_MM_ROWS)) return 1;      // a stage of the per-row kernel must not straddle a page
    if (n_runs < 1 || n_runs > B || units < 0 || units >= n_runs || !kr_multi_mla_xm_args_ok(a, x)) return 1;
    if (units && a.fd_o && (!kr_multi_mla_fd_ok(a.nh, a.klr, a.rd) || !a.fd_ml || a.fd_chunk < 32 || a.fd_chunk % 32 || a.fd_chunks < 1 || a.fd_chunks > 1024)) return 1;
    a.absorb_done = B >= 32 && kr_launch_mla_absorb_mfma(a.q_full, a.ld_q, a.nd + a.rd, a.nd, a.w_kc, a.klr, a.q_abs, B, a.nh, st) == 0;
    const dim3 pg(a.nh * (a.absorb_done ? 1 : a.klr / 64) + 1, B), ag((a.nh + KR_MM_HG - 1) / KR_MM_HG, n_runs);
    const bool rows = units && !a.fd_o && !a.xs_split;      // the exact per-row kernel has a row to take ("multi_mla_exact_split": the three launches below)
#define KR_MXP(F_, P_) hipLaunchKernelGGL((kr_multi_mla_prep_kernel<F_, P_>), pg, dim3(64), 0, st, a)
#define KR_MXR(F_, NBC_, P_) hipLaunchKernelGGL((kr_multi_mla_attn_kernel<F_, NBC_, P_>), ag, dim3(512), (kr_multi_mla_lds<F_, NBC_>()), st, a)
#define KR_MXR_ALL(P_) do { \
    if (a.kv_fp8) { KR_MXP(true, P_); if (!rows) break; if (a.klr == 512) KR_MXR(true, 64, P_); else KR_MXR(true, 32, P_); } \
    else { KR_MXP(false, P_); if (!rows) break; if (a.klr == 512) KR_MXR(false, 64, P_); else KR_MXR(false, 32, P_); } } while (0)
    if (a.page_table) KR_MXR_ALL(true); else KR_MXR_ALL(false);
#undef KR_MXR_ALL
#undef KR_MXR
#undef KR_MXP
    if (units && a.fd_o && kr_launch_multi_mla_fd(a, n_runs, st)) return 1;
    if (units && !a.fd_o && a.xs_split && kr_launch_multi_mla_split(a, n_runs, st)) return 1;      // "multi_mla_exact_split": the unit rows' attention as three launches
    if (kr_launch_multi_mla_xm_attn(a, x, B, st)) return 1;
    if (B >= 32 && kr_launch_mla_wvc_mfma(a.w_vc, a.attn_lat, a.v_proj, B, a.nh, a.vhd, a.klr, st) == 0) return 0;
    KrMlaArgs m{};
    m.step = nullptr; m.pos0 = 0; m.kv_out = a.kv_out; m.ld_kv = a.ld_kv; m.q_full = a.q_full; m.ld_q = a.ld_q; m.w_vc = a.w_vc;
    m.q_abs = a.q_abs; m.q_pe = a.q_pe; m.attn_lat = a.attn_lat; m.v_proj = a.v_proj; m.nh = a.nh; m.klr = a.klr; m.nd = a.nd; m.rd = a.rd; m.vhd = a.vhd;
    kr_launch_mla_wvc(m, st, B);
    return 0;
}

// ---- paged slots: freshly mapped pages read as zero in every pool (docs/design/21-paged-slots.md).  grid (n_pages, n_pools), 256 threads; page_bytes % 16 == 0
__global__ void __launch_bounds__(256) kr_multi_zero_pages_kernel(const KrPagePoolDev* __restrict__ pools, const int* __restrict__ pages) {
    const KrPagePoolDev P = pools[blockIdx.y];
    uint4* dst = reinterpret_cast<uint4*>((char*)P.base + (size_t)pages[blockIdx.x] * P.page_bytes);
    const size_t n = P.page_bytes / 16;
    for (size_t i = threadIdx.x; i < n; i += 256) dst[i] = make_uint4(0u, 0u, 0u, 0u);
}
void kr_launch_multi_zero_pages(const KrPagePoolDev* pools, int n_pools, const int* pages, int n_pages, hipStream_t st) {
    if (n_pools < 1 || n_pages < 1) return;
    hipLaunchKernelGGL(kr_multi_zero_pages_kernel, dim3(n_pages, n_pools), dim3(256), 0, st, pools, pages);
}
// ---- shared pages (docs/design/22-slot-fork.md): copy c of pool p = the first rows[c] * (page_bytes / page_tokens) bytes of page src[c] into page dst[c], the
// rest of dst[c] zeroed -- a destination page is written whole.  grid (n_copies, n_pools), 256 threads.  The body moves 16 bytes per thread and step; the one
// vector the split may fall inside (rope-key rows of rd E4M3 bytes) keeps the source's bytes below the split.  A pool whose pages are not 16-byte aligned
// (a per-slot state buffer of an odd geometry) goes byte by byte.
__device__ __forceinline__ uint32_t kr_low_bytes(uint32_t v, int keep) { return keep >= 4 ? v : keep <= 0 ? 0u : v & ((1u << (8 * keep)) - 1u); }
__global__ void __launch_bounds__(256) kr_multi_copy_pages_kernel(const KrPagePoolDev* __restrict__ pools, const int* __restrict__ dst_pages, const int* __restrict__ src_pages,
                                                                  const int* __restrict__ rows, int page_tokens) {
    const KrPagePoolDev P = pools[blockIdx.y];
    char* dst = (char*)P.base + (size_t)dst_pages[blockIdx.x] * P.page_bytes;
    const char* src = (const char*)P.base + (size_t)src_pages[blockIdx.x] * P.page_bytes;
    const size_t split = (size_t)min(max(rows[blockIdx.x], 0), page_tokens) * (P.page_bytes / (size_t)page_tokens);      // bytes copied; zero from there on
    if ((P.page_bytes | (size_t)P.base) & 15) {
        for (size_t i = threadIdx.x; i < P.page_bytes; i += 256) dst[i] = i < split ? src[i] : (char)0;
        return;
    }
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    uint4* d4 = reinterpret_cast<uint4*>(dst);
    const size_t n = P.page_bytes / 16, whole = split / 16;
    for (size_t i = threadIdx.x; i < n; i += 256) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (i < whole) v = s4[i];
        else if (i * 16 < split) {      // i == whole and the split is inside this vector
            const int keep = (int)(split - i * 16);
            const uint4 t = s4[i];
            v = make_uint4(kr_low_bytes(t.x, keep), kr_low_bytes(t.y, keep - 4), kr_low_bytes(t.z, keep - 8), kr_low_bytes(t.w, keep - 12));
        }
        d4[i] = v;
    }
}
void kr_launch_multi_copy_pages(const KrPagePoolDev* pools, int n_pools, const int* dst_pages, const int* src_pages, const int* rows, int n_copies, int page_tokens, hipStream_t st) {
    if (n_pools < 1 || n_copies < 1 || page_tokens < 1) return;
    hipLaunchKernelGGL(kr_multi_copy_pages_kernel, dim3(n_copies, n_pools), dim3(256), 0, st, pools, dst_pages, src_pages, rows, page_tokens);
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

// ---- accept of a verify pass (docs/design/18-multi-verify.md) ------------------------------------------------------------------------------------
// one thread per run walks it through kr_m_run_row: the ids into caller order (run i starts at off - n_runs + i: off counts the n_runs last-token rows plus
// the earlier runs' other tokens), n_match = the draft tokens before the first that differs from the id of the row before it
__global__ void __launch_bounds__(256) kr_multi_accept_kernel(const int* __restrict__ ids, const int* __restrict__ tokens, const int* __restrict__ runs, int n_runs,
                                                              int T, int* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_runs) return;
    const int off = runs[3 * i + 1], cnt = runs[3 * i + 2], src = off - n_runs + i;
    int m = cnt - 1, prev = 0;
    for (int t = 0; t < cnt; t++) {
        const int b = kr_m_run_row(i, off, cnt, t);
        if (t >= 1 && m == cnt - 1 && tokens[b] != prev) m = t - 1;
        prev = ids[b];
        out[src + t] = prev;
    }
    out[T + i] = m;
}
void kr_launch_multi_accept(const int* ids, const int* tokens, const int* runs, int n_runs, int T, int* out, hipStream_t st) {
    hipLaunchKernelGGL(kr_multi_accept_kernel, dim3((n_runs + 255) / 256), dim3(256), 0, st, ids, tokens, runs, n_runs, T, out);
}
