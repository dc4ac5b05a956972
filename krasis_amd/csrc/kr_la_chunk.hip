// kr_la_chunk.hip -- FAST-mode prompt pass of the gated delta rule (linear-attention layers): sub-chunks of 64 tokens in closed form.
//
// The reference recurrence (src/decode.rs:1293 restated per token in kr_pfm_la_recur_kernel, which stays the exact / default path) is
//     S <- a_t S;  d = b_t (v_t - S^T k_t);  S <- S + k_t d^T;  o_t = S^T q_t            (a_t = e^{g_t}, b_t = beta_t, S is [dk][dv])
// i.e. S_t = (I - b_t k_t k_t^T) a_t S_{t-1} + b_t k_t v_t^T: two dk-long dependent fma chains per token, 1.67 ms per 1024-token launch on
// MI355X (52.6 % of the FAST prompt pass, profiles/r02_prefill_fast_8192_kernel_stats.txt).  Over a sub-chunk of T = 64 tokens with
// G_t = sum_{r<=t} g_r the same map is (WY form):
//     (I + L) [W | Y] = [diag(b e^G) K | diag(b) V],   L[t][j] = b_t e^{G_t - G_j} (k_t . k_j)   (j < t)          -> forward substitution
//     U  = Y - W S_0                                                                                            (the 64 "delta" rows)
//     O  = (diag(e^G) Q - B W) S_0 + B Y,          B[t][j] = e^{G_t - G_j} (q_t . k_j)   (j <= t)
//     S' = e^{G_T} S_0 + (diag(e^{G_T - G}) K)^T U
// Only the two products with S_0 are sequential over sub-chunks.  Two launches:
//   kr_lac_prep_kernel  grid (sub-chunks, heads): everything that does not need the state -- K K^T, Q K^T on the f32 MFMA, the triangular
//                       solve in registers (one column of [W | Y] per thread, L rows broadcast from LDS), Q' = e^G Q - B W and O_0 = B Y.
//   kr_lac_scan_kernel  grid (heads x 4 column slices of the state): walks the sub-chunks; per step U = Y - W S, O = O_0 + Q' S (four 32x32
//                       blocks, one per wave) and S <- e^{G_T} S + K'^T U (four blocks), the next sub-chunk's tiles in flight in registers.
// Every product runs on the bf16 MFMA with its f32 operands split into two bf16 values (x = hi + lo, hi = bf16(x), lo = bf16(x - hi)) and
// acc += hi.hi + hi.lo + lo.hi: three v_mfma_f32_32x32x16_bf16 (96 matrix-pipe cycles per 16 k) instead of eight v_mfma_f32_32x32x2_f32 (512),
// products exact to ~2^-17 relative, f32 accumulation, f32 exponent range.  The prep kernel splits in registers (lc_blk_s); W, Q' and K^T leave it
// already split into planes (and K transposed), so the SCAN -- the sequential part -- stages them with plain 16-byte copies (lc_blk3); only the state
// slice and the delta rows are split inside the scan (16 values per lane and step).  Round 2 ran everything on v_mfma_f32_32x32x2_f32.
// (tolerance mode: tests/test_attn_fast_gpu.py states the bound.)  All exponents are differences G_t - G_j <= 0: nothing overflows, and a
// decay that underflows gives 0, not NaN (g is clamped at -80 per token).
#include <hip/hip_runtime.h>
#include "kr_lds_optin.h"
#include "kr_device.h"
#include "kr_libm.h"
#include "kr_exact_dev.h"
#include "kr_prefill_ops.h"

#include "kr_lac_dev.h"      // the two kernels: one text for this pass and for the runs of a batched pass (kr_multi_la_chunk.hip)

// where a workgroup's sub-chunk lies in the prompt pass: sub-chunk x of the chunk, token t is row t, scratch tile = sub-chunk, the store's own states
struct KrLacChunk {
    typedef KrLacArgs Args;
    int sub, C, n_sub;
    static __device__ __forceinline__ const KrLacArgs& lac(const Args& A) { return A; }
    static __device__ __forceinline__ KrLacChunk prep(const Args& A) { return KrLacChunk{(int)blockIdx.x, A.C, A.n_sub}; }
    static __device__ __forceinline__ KrLacChunk scan(const Args& A) { return KrLacChunk{0, A.C, A.n_sub}; }
    __device__ __forceinline__ int tile() const { return sub; }
    __device__ __forceinline__ int tile0() const { return 0; }
    __device__ __forceinline__ int row(int t) const { return t; }
    __device__ __forceinline__ const float* conv(const KrLacArgs& a) const { return a.conv_state; }
    __device__ __forceinline__ float* state(const KrLacArgs& a) const { return a.state; }
};

// floats of scratch per padded token (a multiple of 64 tokens) and head: Y rows, the bf16 plane pairs of W, Q', K^T (2 + 2 bytes per value each), one G
size_t kr_pfm_la_chunk_scratch_floats(int C, int nv) { const size_t c64 = ((size_t)C + LC_T - 1) / LC_T * LC_T; return c64 * nv * (4 * LC_D + 1) + 4; }   // Y (f32), three pairs of bf16 planes, G
bool kr_pfm_la_chunk_ok(int dk, int dv, int C) { return dk == LC_D && dv == LC_D && C >= LC_T; }

// > 64 KB of dynamic LDS is an opt-in per device (and not allowed inside a stream capture: the prompt pass is never captured)
static int lac_prepare() {
    return kr_lds_optin(reinterpret_cast<const void*>(kr_lac_prep_kernel<KrLacChunk>), LC_PREP_LDS) || kr_lds_optin(reinterpret_cast<const void*>(kr_lac_scan_kernel<KrLacChunk>), LC_SCAN_LDS);
}

// fused != 0: the prep launch forms q / k / v and the gates from the in-projection's output itself (no conv launch ran); `between` (may be null) is called between the
// two launches, on the stream -- the carried conv slots are advanced there, AFTER the prep launch has read the old ones
int kr_launch_pfm_la_chunked(const KrPfmLaArgs& p, float* state, float* out, float* scratch, int C, hipStream_t st, const KrPfSync* sy, int fused, void (*between)(const KrPfmLaArgs&, int, hipStream_t, const KrPfSync*)) {
    if (!kr_pfm_la_chunk_ok(p.dk, p.dv, C) || !scratch) return 1;
    if (fused && (p.nv != p.nk * p.hr || p.ld_qkvz % 4)) return 1;
    if (lac_prepare()) return 1;
    KrLacArgs a{};
    a.fused = fused; a.qkvz = p.qkvz; a.ld_qkvz = p.ld_qkvz; a.ba = p.ba; a.ld_ba = p.ld_ba; a.conv_state = p.conv_state; a.conv_w = p.conv_w; a.a_log = p.a_log; a.dt_bias = p.dt_bias;
    a.scale = p.scale; a.nk = p.nk; a.hr = p.hr;
    a.q = p.q; a.k = p.k; a.v = p.v; a.gexp = p.gexp; a.beta = p.beta; a.nv = p.nv; a.C = C; a.n_sub = (C + LC_T - 1) / LC_T;
    const size_t tiles = (size_t)a.n_sub * p.nv * LC_T;
    a.Y = scratch; a.G = a.Y + tiles * LC_D;
    uint16_t* pl = reinterpret_cast<uint16_t*>(a.G + ((tiles + 3) / 4) * 4);        // planes start 16-byte aligned
    a.Wh = pl; a.Wl = a.Wh + tiles * LC_D; a.Qh = a.Wl + tiles * LC_D; a.Ql = a.Qh + tiles * LC_D; a.Kh = a.Ql + tiles * LC_D; a.Kl = a.Kh + tiles * LC_D;
    a.out = out; a.state = state;
    hipLaunchKernelGGL(kr_lac_prep_kernel<KrLacChunk>, dim3(a.n_sub, p.nv), dim3(LC_PTH), LC_PREP_LDS, st, a);
    if (between) between(p, C, st, sy);
    if (sy) kr_pf_wait(st, sy->wait_b);      // only the scan reads the state the previous chunk of the prompt leaves
    hipLaunchKernelGGL(kr_lac_scan_kernel<KrLacChunk>, dim3(p.nv * 4), dim3(256), LC_SCAN_LDS, st, a);
    return 0;
}
