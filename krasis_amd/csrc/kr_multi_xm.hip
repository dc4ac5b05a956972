// kr_multi_xm.hip -- GQA attention of a run of tokens entering a device slot, EXACT, on the f32 matrix cores (kr_decode_set_option "multi_extend_exact_mfma",
// docs/design/28-multi-extend-exact-mfma.md).  The three passes of the exact single-sequence prompt pass placed on the runs of a batched pass:
//   A  scores   kr_xm_scores_body (kr_xm_dev.h, the text of kr_pfm_gqa_scores_mfma_kernel): 8 fma lanes per (query, position), the reference's add tree, * sm_scale
//   B  softmax  max -> libm exp -> sum in position order -> 1 / sum (the steps of kr_pfm_gqa_softmax_kernel with tmax); the rows stay as exponentials
//   C  P.V      kr_xm_pv_body (the text of kr_pfm_gqa_pv_mfma_kernel): one fma chain per output over ascending positions with p = e * inv, then the sigmoid gate
// value for value what kr_multi_gqa_attn_kernel computes for every token of the run one by one -- but a slot's K rows are staged once per 64 / G query tokens and
// its V rows once per 32 / G, not once per token.  The prep launch (QK-norm, RoPE, cache append of every row, the run's own among them) is the exact pass's
// kr_multi_gqa_prep_kernel, run by the caller before these.
//
// Bounds.  The host built the tile tables from the run counts it flattened the rows with (t0 < cnt), checked positions[i] + cnt <= the slot's max_seq and mapped
// every page of [0, positions[i] + cnt) before the pass.  A tile reads cache rows at positions <= p_max = pos0 + min(t0 + tile, cnt) - 1 only (later rows of a
// stage re-read p_max), so a flat slot is read below its max_seq and a table row below page_stride; score rows are written and read at columns <= the row's own
// position < sc_ld, pass C's 64-column stage loads end at ((p_max >> 6) + 1) * 64 <= sc_ld (a multiple of 64 that exceeds the pass's largest position), tmax at
// block <= p_max >> 5 < sc_ld / 32; every row index is a pass row < n.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kr_exact_dev.h"
#include "kr_multi.h"
#include "kr_prefill_ops.h"
#include "kr_xm_dev.h"

// token t of a run is pass row kr_m_run_row(run, off, cnt, t): the flatten of docs/design/17-multi-extend.md
struct KrXmRunRows {
    int i, off, cnt;
    __device__ __forceinline__ int operator()(int t) const { return kr_m_run_row(i, off, cnt, t); }
};

// Tile (run, t0) of a table: the run's slot, rows and first position come from the pass's run table and row positions (workgroup-uniform loads).  Flat slots:
// the slot's row 0 of both caches; PAGED: the pools and the slot's row of the page table
template <bool FP8, bool PAGED>
struct KrXmSlotTile {
    KrXmSeq q; KrXmRunRows rows; int t0; const int* ptab;
    __device__ __forceinline__ KrXmSlotTile(const KrMultiGqaArgs& a, const int* tl) {
        const int run = tl[0];
        t0 = tl[1];
        const int slot = a.pf_runs[3 * run];
        rows = KrXmRunRows{run, a.pf_runs[3 * run + 1], a.pf_runs[3 * run + 2]};
        const size_t base = PAGED ? 0 : (size_t)slot * a.slot_elems * (FP8 ? 1 : 2);      // bytes to the slot's row 0
        q = KrXmSeq{a.q_out, a.gate, a.attn_out, (const char*)a.k_cache + base, (const char*)a.v_cache + base, a.gated, a.nh, a.nkv, a.positions[rows(0)], rows.cnt, a.sm_scale};
        ptab = PAGED ? a.page_table + (size_t)slot * a.page_stride : nullptr;
    }
};

// pass A: grid (position tiles of 64 up to the pass's largest kv_end, x.n_a query tiles of 64 / G tokens, nkv), 256 threads.  A tile whose p_lo lies past its last
// visible position leaves inside the body, ahead of every barrier
template <bool FP8, bool PAGED>
__global__ void __launch_bounds__(256, 2) kr_multi_xm_scores_kernel(const KrMultiGqaArgs a, const KrMultiXmArgs x) {
    __shared__ __attribute__((aligned(16))) float Qs[64 * XM_LDF];
    __shared__ __attribute__((aligned(16))) float Ks[64 * XM_LDF];
    const KrXmSlotTile<FP8, PAGED> tl(a, x.tiles_a + 2 * blockIdx.y);
    kr_xm_scores_body<FP8, PAGED>(tl.q, a.hd, tl.t0, blockIdx.x * 64, blockIdx.z, tl.rows, tl.ptab, a.page_shift, a.scores, a.sc_ld, x.tmax, Qs, Ks);
}

// pass B: one wave per (pass row, head), seq = positions[row] + 1.  A row b < pf_nruns whose run has one token is a unit row of the per-row kernels and leaves at
// once (wave-uniform; there is no workgroup barrier in here).  The steps and their order are kr_pfm_gqa_softmax_kernel's with tmax (kr_prefill_ops.hip): the
// maximum over pass A's per-32-position maxima (a maximum is the same in whatever order it is taken), e = exp(s - max) by kr_expf stored in place, the sum in
// position order by lane 0, inv = 1 / sum; the row stays as exponentials
__global__ void __launch_bounds__(256) kr_multi_xm_softmax_kernel(const KrMultiGqaArgs a, const KrMultiXmArgs x, int rows) {
    __shared__ __attribute__((aligned(16))) float buf[4][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, row = blockIdx.x * 4 + wave;
    if (row >= rows) return;
    const int b = row / a.nh;
    if (b < a.pf_nruns && a.pf_runs[3 * b + 2] < 2) return;
    const int seq = a.positions[b] + 1;
    float* s = a.scores + (size_t)row * a.sc_ld;
    float mx = -__builtin_inff();
    const float* tm = x.tmax + (size_t)row * (a.sc_ld >> 5);
    for (int k = lane; k < (seq + 31) >> 5; k += 64) mx = fmaxf(mx, tm[k]);
    mx = kr_wave_max(mx);
    float se = 0.0f;
    for (int p0 = 0; p0 < seq; p0 += 64) {
        const int p = p0 + lane;
        float e = 0.0f;
        if (p < seq) { e = kr_expf(s[p] - mx); s[p] = e; }
        buf[wave][lane] = e;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier();
        if (lane == 0) {
            const int n = min(64, seq - p0);
            if (n == 64) {
                const float4* b4 = reinterpret_cast<const float4*>(buf[wave]);
#pragma unroll
                for (int u = 0; u < 16; u++) { const float4 v = b4[u]; se += v.x; se += v.y; se += v.z; se += v.w; }
            } else for (int u = 0; u < n; u++) se += buf[wave][u];
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier();
    }
    const float iv = __shfl(1.0f / se, 0);
    if (lane == 0) x.inv[row] = iv;
}

// pass C: grid (x.n_c query tiles of 32 / G tokens, nkv), 256 threads
template <bool FP8, int HD, bool PAGED>
__global__ void __launch_bounds__(256) kr_multi_xm_pv_kernel(const KrMultiGqaArgs a, const KrMultiXmArgs x) {
    __shared__ __attribute__((aligned(16))) float Ps[32 * (64 + 4)];
    __shared__ __attribute__((aligned(16))) char Vs[64 * (HD * (FP8 ? 1 : 2) + 64)];
    const KrXmSlotTile<FP8, PAGED> tl(a, x.tiles_c + 2 * blockIdx.x);
    kr_xm_pv_body<FP8, HD, 64, PAGED>(tl.q, tl.t0, blockIdx.y, tl.rows, tl.ptab, a.page_shift, a.scores, a.sc_ld, x.inv, Ps, Vs);
}

// what kr_launch_multi_xm checks: asked before anything of the layer is queued
int kr_multi_xm_args_ok(const KrMultiGqaArgs& a, const KrMultiXmArgs& x) {
    KrPfmGqaArgs g{};
    g.nh = a.nh; g.nkv = a.nkv; g.hd = a.hd;
    if (a.nkv < 1 || !kr_pfm_gqa_exact_mfma_ok(g)) return 0;
    if (!a.pf_runs || a.pf_tiles || !a.scores || a.sc_ld < 64 || a.sc_ld % 64) return 0;      // pass C reads stages of 64 score columns
    if (!x.tiles_a || !x.tiles_c || x.n_a < 1 || x.n_c < 1 || x.n_a > 65535 || !x.inv || !x.tmax || x.kv_end < 2 || x.kv_end > a.sc_ld) return 0;
    return !(a.page_table && (a.page_stride < 1 || a.page_shift < 5));
}
// passes B and C on their own: the MLA runs of "multi_extend_mla_exact_mfma" take them behind a scores pass of their own (kr_multi_mla_xm.hip) through a view of
// the layer with nkv = 1, hd = kv_lora_rank 256.  The caller has checked what kr_multi_xm_args_ok checks
void kr_launch_multi_xm_softmax(const KrMultiGqaArgs& a, const KrMultiXmArgs& x, int B, hipStream_t st) {
    const int rows = B * a.nh;
    hipLaunchKernelGGL(kr_multi_xm_softmax_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, a, x, rows);
}
void kr_launch_multi_xm_pv(const KrMultiGqaArgs& a, const KrMultiXmArgs& x, hipStream_t st) {
    const dim3 gc(x.n_c, a.nkv);
#define KR_XC(F_, H_) do { if (a.page_table) hipLaunchKernelGGL((kr_multi_xm_pv_kernel<F_, H_, true>), gc, dim3(256), 0, st, a, x); \
                           else hipLaunchKernelGGL((kr_multi_xm_pv_kernel<F_, H_, false>), gc, dim3(256), 0, st, a, x); } while (0)
    if (a.hd == 256) { if (a.kv_fp8) KR_XC(true, 256); else KR_XC(false, 256); }
    else if (a.hd == 128) { if (a.kv_fp8) KR_XC(true, 128); else KR_XC(false, 128); }
    else { if (a.kv_fp8) KR_XC(true, 64); else KR_XC(false, 64); }
#undef KR_XC
}
int kr_launch_multi_xm(const KrMultiGqaArgs& a, const KrMultiXmArgs& x, int B, hipStream_t st) {
    if (!kr_multi_xm_args_ok(a, x) || B < 1) return 1;
    const dim3 ga((x.kv_end + 63) / 64, x.n_a, a.nkv);
#define KR_XA(F_, P_) hipLaunchKernelGGL((kr_multi_xm_scores_kernel<F_, P_>), ga, dim3(256), 0, st, a, x)
    if (a.page_table) { if (a.kv_fp8) KR_XA(true, true); else KR_XA(false, true); }
    else { if (a.kv_fp8) KR_XA(true, false); else KR_XA(false, false); }
#undef KR_XA
    kr_launch_multi_xm_softmax(a, x, B, st);
    kr_launch_multi_xm_pv(a, x, st);
    return 0;
}
