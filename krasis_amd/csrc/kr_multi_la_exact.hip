// kr_multi_la_exact.hip -- linear attention of a run of >= "multi_extend_la_exact_min" tokens entering a device slot, in the staged exact form of the store's own
// prompt pass (kr_decode_set_option "multi_extend_la_exact", docs/design/36-multi-extend-la-exact.md): conv + SiLU + gates + L2 norms parallel over (key head, 16
// tokens), the carried conv inputs, the delta rule alone in the serial loop (the output chain of token t and the kv chain of token t + 1 interleaved, rows by
// LDS-DMA, one barrier per token), the gated RMSNorm parallel over tokens -- instead of the run kernels' walk with five barriers per token.  The four launches
// instantiate the prompt pass's own kernel templates (kr_pfm_la_dev.h) with another placement; no arithmetic is stated here.  Per value that arithmetic is the
// decode step's, as the run kernels' is: no bit of any call changes.
#include "kr_pfm_la_dev.h"
#include "kr_multi.h"
#include "kr_lc_tiles.h"

static_assert(KR_LX_CONV_TOKENS == PFC_WT && KR_LX_NORM_TOKENS == PFG_TT, "the host's tiles are the kernels'");

// where a workgroup's tokens lie in a batched pass.  conv: workgroup (., y) takes tile y of t16 = tokens t0 .. t0 + 15 of run `run`; gated norm: tile y of t8;
// conv state and delta rule: workgroups (., r) take staged run r of the run table.  The run's slot, rows and length come from the pass's run table [slot, off,
// cnt] (workgroup-uniform scalar loads, ahead of every loop); token t is pass row kr_m_run_row(run, off, cnt, t): the flatten of docs/design/17-multi-extend.md,
// the last token in row `run` -- the conv window's taps inside the run go through it too, those before its first token come from the slot's carried inputs.
// Bounds: the host built the three tables from the counts it flattened the rows with, so t0 < cnt and every row is a row of the pass; the kernels ask for row(t)
// with t < C = cnt only (the delta rule's phantom token re-reads row cnt - 1); the state descriptor covers one head's [dk][dv] block of the slot
struct KrPfmLaSlot {
    struct ConvArgs { KrPfmLaArgs a; const int* runs; const int* tab; size_t conv_stride; };      // a.conv_state: the slots' base; tab: t16 (conv) / the run table (conv state)
    struct RecurArgs { KrPfmLaRecurArgs r; const int* runs; const int* tab; size_t recur_stride; };      // r.state: the slots' base; tab: the run table
    struct NormPlace { const int* runs; const int* tab; };                                         // tab: t8
    int C, t0, run, off, slot; size_t stride;
    static __device__ __forceinline__ const KrPfmLaArgs& la(const ConvArgs& A) { return A.a; }
    static __device__ __forceinline__ const KrPfmLaRecurArgs& rec(const RecurArgs& A) { return A.r; }
    static __device__ __forceinline__ KrPfmLaSlot place(const int* runs, int run, int t0, size_t stride) {
        return KrPfmLaSlot{runs[3 * run + 2], t0, run, runs[3 * run + 1], runs[3 * run], stride};
    }
    static __device__ __forceinline__ KrPfmLaSlot conv(const ConvArgs& A) { const int* tl = A.tab + 2 * blockIdx.y; return place(A.runs, tl[0], tl[1], A.conv_stride); }
    static __device__ __forceinline__ KrPfmLaSlot cstate(const ConvArgs& A) { return place(A.runs, A.tab[2 * blockIdx.y], 0, A.conv_stride); }
    static __device__ __forceinline__ KrPfmLaSlot recur(const RecurArgs& A) { return place(A.runs, A.tab[2 * blockIdx.y], 0, A.recur_stride); }
    static __device__ __forceinline__ KrPfmLaSlot norm(const NormPlace& P, int) { const int* tl = P.tab + 2 * blockIdx.y; return place(P.runs, tl[0], tl[1], 0); }
    __device__ __forceinline__ int row(int t) const { return kr_m_run_row(run, off, C, t); }
    __device__ __forceinline__ float* cs(const KrPfmLaArgs& a) const { return a.conv_state + (size_t)slot * stride; }
    __device__ __forceinline__ float* state(const KrPfmLaRecurArgs& r) const { return r.state + (size_t)slot * stride; }
};

int kr_multi_lx_ok(int dk, int dv, int nk, int nv, int ld_qkvz) {
    return (dk == 64 || dk == 128) && dv >= dk && dv <= 256 && dv % 8 == 0 && nk >= 1 && nv == nk * (nv / nk) && ld_qkvz % 4 == 0;
}
int kr_multi_lx_args_ok(const KrMultiLaArgs& m, const KrMultiLxArgs& x) {
    return kr_multi_lx_ok(m.dk, m.dv, m.nk, m.nv, m.ld_qkvz) && m.nv == m.nk * m.hr && m.ld_out == m.nv * m.dv && m.lx_min >= 2 && x.runs && x.t16 && x.t8 && x.n_runs >= 1 &&
           x.n16 >= x.n_runs && x.n8 >= x.n16 && x.n_short >= 0 && x.q && x.k && x.v && x.z && x.gexp && x.beta && x.o;
}

int kr_launch_multi_la_exact(const KrMultiLaArgs& m, const KrMultiLxArgs& x, const int* runs, hipStream_t st) {
    if (!kr_multi_lx_args_ok(m, x)) return 1;
    KrPfmLaArgs a{};
    a.qkvz = m.qkvz; a.ld_qkvz = m.ld_qkvz; a.ba = m.ba; a.ld_ba = m.ld_ba; a.conv_state = m.conv_state; a.conv_w = m.conv_w; a.a_log = m.a_log; a.dt_bias = m.dt_bias;
    a.scale = m.scale; a.q = x.q; a.k = x.k; a.v = x.v; a.z = x.z; a.gexp = x.gexp; a.beta = x.beta; a.nk = m.nk; a.nv = m.nv; a.dk = m.dk; a.dv = m.dv; a.hr = m.hr;
    const int conv_dim = 2 * m.nk * m.dk + m.nv * m.dv;
    hipLaunchKernelGGL(kr_pfm_la_conv_kernel<KrPfmLaSlot>, dim3(m.nk, x.n16), dim3(256), (size_t)(2 * PFC_WT * m.dk + 2 * PFC_WT) * 4, st, KrPfmLaSlot::ConvArgs{a, runs, x.t16, m.conv_stride});
    hipLaunchKernelGGL(kr_pfm_la_conv_state_kernel<KrPfmLaSlot>, dim3((conv_dim + 255) / 256, x.n_runs), dim3(256), 0, st, KrPfmLaSlot::ConvArgs{a, runs, x.runs, m.conv_stride});      // behind the conv launch: it read the old inputs
    const KrPfmLaSlot::RecurArgs r{KrPfmLaRecurArgs{m.recur, x.q, x.k, x.v, x.gexp, x.beta, x.o, m.nv, m.dv, 0}, runs, x.runs, m.recur_stride};
    if (m.dk == 128) hipLaunchKernelGGL((kr_pfm_la_recur_kernel<128, KrPfmLaSlot>), dim3(m.nv, x.n_runs), dim3(m.dv), 0, st, r);
    else hipLaunchKernelGGL((kr_pfm_la_recur_kernel<64, KrPfmLaSlot>), dim3(m.nv, x.n_runs), dim3(m.dv), 0, st, r);
    // z: the copy [rows][nv * dv] the conv launch made (z_hr = nv: one block); the rows of the other runs hold the run kernel's output and are not touched
    hipLaunchKernelGGL(kr_pfm_gated_norm_kernel<KrPfmLaSlot>, dim3(m.nv, x.n8), dim3(256), 0, st, (const float*)x.o, (const float*)x.z, (size_t)m.nv * m.dv, m.nv, 0, m.norm_w, m.out, m.nv, m.dv, 0, m.eps,
                       KrPfmLaSlot::NormPlace{runs, x.t8});
    return 0;
}
