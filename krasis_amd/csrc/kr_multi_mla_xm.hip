// kr_multi_mla_xm.hip -- MLA attention of a run of tokens entering a device slot, EXACT, on the f32 matrix cores (kr_decode_set_option
// "multi_extend_mla_exact_mfma", docs/design/29-multi-extend-mla-exact-mfma.md).  The three passes of the exact single-sequence MLA prompt pass (kr_launch_mla,
// kr_mla.hip) placed on the runs of a batched pass:
//   A  scores   kr_xm_mla_scores_body (kr_xm_mla_dev.h, the text of kr_mla_scores_mfma_kernel), two launches: dot16(q_pe, kpe), then (dot16(q_abs, ckv) + that) * sm_scale
//   B  softmax  kr_multi_xm_softmax_kernel (kr_multi_xm.hip) through a KrMultiGqaArgs view of the layer: nkv = 1, hd = klr, v_cache = the latent cache
//   C  P.V      kr_xm_pv_body (kr_xm_dev.h) over the same view: one fma chain per latent element over ascending positions with p = e * inv.  kv_lora_rank 256 takes
//               kr_multi_xm_pv_kernel<.., 256, ..>; 512 the kernel below, 32 positions a stage (the V tile must fit the static LDS window)
// value for value what kr_multi_mla_attn_kernel computes for every token of the run one by one -- but the slot's rope-key and latent rows are staged once per
// 64 / nh query tokens (A) and its latent rows once per 32 / nh (C), not once per (token, 4 heads).  The absorption, the prep launch (which appends the run's own
// rows first) and the w_vc projection are the exact pass's, run by kr_launch_multi_mla_xm (kr_multi.hip) around these.
//
// Bounds.  The host built the tile tables from the run counts it flattened the rows with (t0 < cnt), checked positions[i] + cnt <= the slot's max_seq and mapped
// every page of [0, positions[i] + cnt) before the pass.  A tile reads cache rows at positions <= p_max = pos0 + min(t0 + tile, cnt) - 1 only (later rows of a
// stage re-read p_max), so a flat slot is read below its max_seq and a table row below page_stride; score rows are written and read at columns <= the row's own
// position < sc_ld, pass C's 32-column stage loads end at ((p_max >> 5) + 1) * 32 <= sc_ld (a multiple of 64 that exceeds the pass's largest position), tmax at
// block <= p_max >> 5 < sc_ld / 32; every row index is a pass row < n.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kr_multi.h"
#include "kr_prefill_ops.h"
#include "kr_xm_mla_dev.h"

// token t of a run is pass row kr_m_run_row(run, off, cnt, t): the flatten of docs/design/17-multi-extend.md
struct KrMlaXmRunRows {
    int i, off, cnt;
    __device__ __forceinline__ int operator()(int t) const { return kr_m_run_row(i, off, cnt, t); }
};

// pass A: grid (position tiles of 64 up to the pass's largest kv_end, x.n_a query tiles of 64 / nh tokens), 256 threads.  Tile (run, t0) of the table: the run's
// slot, rows and first position come from the pass's run table and row positions (workgroup-uniform loads).  A tile whose p_lo lies past its last visible
// position leaves inside the body, ahead of every barrier
template <bool FP8, bool ROPE, bool PAGED>
__global__ void __launch_bounds__(256) kr_multi_mla_xm_scores_kernel(const KrMultiMlaArgs a, const KrMultiXmArgs x) {
    __shared__ __attribute__((aligned(16))) float As[64 * XM_LDF];
    __shared__ __attribute__((aligned(16))) float Bs[64 * XM_LDF];
    const int* tl = x.tiles_a + 2 * blockIdx.y;
    const int run = tl[0], t0 = tl[1], slot = a.mf_runs[3 * run];
    const KrMlaXmRunRows rows{run, a.mf_runs[3 * run + 1], a.mf_runs[3 * run + 2]};
    const char* kb = reinterpret_cast<const char*>(ROPE ? a.kpe_cache : a.ckv_cache) + (PAGED ? 0 : (size_t)slot * (ROPE ? a.kpe_stride : a.ckv_stride));
    const int* ptab = PAGED ? a.page_table + (size_t)slot * a.page_stride : nullptr;
    kr_xm_mla_scores_body<FP8, ROPE, PAGED>(ROPE ? a.q_pe : a.q_abs, kb, a.nh, ROPE ? a.rd : a.klr, a.positions[rows(0)], rows.cnt, t0, blockIdx.x * 64, rows, ptab,
                                            a.page_shift, a.sm_scale, a.scores, a.sc_ld, x.tmax, As, Bs);
}

// pass C for kv_lora_rank 512: grid (x.n_c query tiles of 32 / nh tokens), 256 threads; a = the KrMultiGqaArgs view (nkv = 1, hd = 512, gated = 0)
template <bool FP8, bool PAGED>
__global__ void __launch_bounds__(256) kr_multi_mla_xm_pv512_kernel(const KrMultiGqaArgs a, const KrMultiXmArgs x) {
    __shared__ __attribute__((aligned(16))) float Ps[32 * (32 + 4)];
    __shared__ __attribute__((aligned(16))) char Vs[32 * (512 * (FP8 ? 1 : 2) + 64)];
    const int* tl = x.tiles_c + 2 * blockIdx.x;
    const int run = tl[0], t0 = tl[1], slot = a.pf_runs[3 * run];
    const KrMlaXmRunRows rows{run, a.pf_runs[3 * run + 1], a.pf_runs[3 * run + 2]};
    const size_t base = PAGED ? 0 : (size_t)slot * a.slot_elems * (FP8 ? 1 : 2);      // bytes to the slot's row 0
    const KrXmSeq q{a.q_out, a.gate, a.attn_out, (const char*)a.k_cache + base, (const char*)a.v_cache + base, a.gated, a.nh, a.nkv, a.positions[rows(0)], rows.cnt, a.sm_scale};
    const int* ptab = PAGED ? a.page_table + (size_t)slot * a.page_stride : nullptr;
    kr_xm_pv_body<FP8, 512, 32, PAGED>(q, t0, 0, rows, ptab, a.page_shift, a.scores, a.sc_ld, x.inv, Ps, Vs);
}

// what kr_launch_multi_mla_xm_attn checks: asked before anything of the layer is queued (a.mf_runs set, a.mf_tiles null)
int kr_multi_mla_xm_args_ok(const KrMultiMlaArgs& a, const KrMultiXmArgs& x) {
    if (!kr_mla_exact_mfma_ok(a.nh, a.klr, a.rd)) return 0;
    if (!a.mf_runs || a.mf_tiles || !a.scores || a.sc_ld < 64 || a.sc_ld % 64) return 0;      // the row maxima are per 32 positions, a 256-wide pass C reads stages of 64 score columns
    if (!x.tiles_a || !x.tiles_c || x.n_a < 1 || x.n_c < 1 || x.n_a > 65535 || !x.inv || !x.tmax || x.kv_end < 2 || x.kv_end > a.sc_ld) return 0;
    return !(a.page_table && (a.page_stride < 1 || a.page_shift < 5));
}
// passes A (two launches), B and C alone (after the prep launch)
int kr_launch_multi_mla_xm_attn(const KrMultiMlaArgs& a, const KrMultiXmArgs& x, int B, hipStream_t st) {
    if (!kr_multi_mla_xm_args_ok(a, x) || B < 1) return 1;
    const dim3 ga((x.kv_end + 63) / 64, x.n_a);
#define KR_MXA(F_, R_, P_) hipLaunchKernelGGL((kr_multi_mla_xm_scores_kernel<F_, R_, P_>), ga, dim3(256), 0, st, a, x)
#define KR_MXA2(F_, P_) do { KR_MXA(F_, true, P_); KR_MXA(F_, false, P_); } while (0)
    if (a.page_table) { if (a.kv_fp8) KR_MXA2(true, true); else KR_MXA2(false, true); }
    else { if (a.kv_fp8) KR_MXA2(true, false); else KR_MXA2(false, false); }
#undef KR_MXA2
#undef KR_MXA
    // the GQA view of the layer: one KV head whose K = V rows are the latent rows
    KrMultiGqaArgs g{};
    g.slots = a.slots; g.positions = a.positions; g.k_cache = a.ckv_cache; g.v_cache = a.ckv_cache; g.slot_elems = a.ckv_stride / (a.kv_fp8 ? 1 : 2); g.kv_fp8 = a.kv_fp8;
    g.attn_out = a.attn_lat; g.scores = a.scores; g.sc_ld = a.sc_ld; g.gated = 0; g.nh = a.nh; g.nkv = 1; g.hd = a.klr; g.sm_scale = a.sm_scale;
    g.page_table = a.page_table; g.page_stride = a.page_stride; g.page_shift = a.page_shift;
    g.pf_runs = a.mf_runs; g.pf_nruns = a.mf_nruns; g.pf_units = a.mf_units; g.pf_tiles = nullptr; g.pf_ntiles = 0;
    kr_launch_multi_xm_softmax(g, x, B, st);
    if (a.klr == 256) { kr_launch_multi_xm_pv(g, x, st); return 0; }
#define KR_MXC(F_) do { if (a.page_table) hipLaunchKernelGGL((kr_multi_mla_xm_pv512_kernel<F_, true>), dim3(x.n_c), dim3(256), 0, st, g, x); \
                        else hipLaunchKernelGGL((kr_multi_mla_xm_pv512_kernel<F_, false>), dim3(x.n_c), dim3(256), 0, st, g, x); } while (0)
    if (a.kv_fp8) KR_MXC(true); else KR_MXC(false);
#undef KR_MXC
    return 0;
}
