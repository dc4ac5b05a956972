// kr_multi_la_chunk.hip -- linear attention of a run of >= 64 tokens entering a device slot, in tolerance form (kr_decode_set_option "multi_extend_la_chunk",
// docs/design/26-multi-extend-la-chunk.md): the gated delta rule in closed form over sub-chunks of 64 tokens on the bf16 matrix cores instead of the exact run
// kernels' walk token by token.  The arithmetic specification is the store's own KR_ATTN_FAST prompt pass in its fused form (kr_launch_pfm_la with
// "la_conv_fused" = 1): the prep and scan launches instantiate that pass's own kernel templates (kr_lac_dev.h) with another placement, and the two small kernels
// below restate kr_pfm_la_conv_state_kernel and kr_pfm_gated_norm_kernel (kr_prefill_ops.hip) over the pass's rows with the same operations in the same order, so
// a run carries the bits of that prompt pass on its sequence alone, whatever rows share the pass.
#include "kr_lac_dev.h"
#include "kr_lds_optin.h"
#include "kr_multi.h"
#include "kr_lc_tiles.h"

static_assert(KR_M_LC_MIN == LC_T && KR_LC_TOKENS == LC_T, "one threshold: kr_pfm_la_chunk_ok's C >= LC_T");

struct KrLacSlotArgs {
    KrLacArgs lac;                              // as the prompt pass fills it, fused form; conv_state, state, C and n_sub are not read
    const int* runs;                            // the pass's run table, [slot, off, cnt] per run (kr_multi.h)
    const int* lc_runs; const int* lc_tiles;    // [run, first scratch tile] per chunked run; [run, sub] per sub-chunk (kr_lc_tiles.h)
    float* conv_state; size_t conv_stride;      // as KrMultiLaArgs
    float* recur; size_t recur_stride;
};

// where a workgroup's sub-chunk lies in a batched pass.  prep: workgroup x takes tile x of the table = sub-chunk `sub` of run `run`, scratch tile x; scan:
// workgroups (., r) take chunked run r, whose sub-chunk 0 is scratch tile lc_runs[2 r + 1].  The run's slot, rows and length come from the pass's run table
// (workgroup-uniform scalar loads); token t is pass row kr_m_run_row(run, off, cnt, t): the flatten of docs/design/17-multi-extend.md, the last token in row
// `run` -- the 7-row conv window of the prep goes through it too.  Bounds: the host built both tables from the counts it flattened the rows with, so sub <
// ceil(cnt / 64), every row is a row of the pass, and the scratch holds lc_ntiles tiles; the kernels ask for row(t) with t < C only
struct KrLacSlot {
    typedef KrLacSlotArgs Args;
    int sub, C, n_sub, run, off, t0; const float* cs; float* st;
    static __device__ __forceinline__ const KrLacArgs& lac(const Args& A) { return A.lac; }
    static __device__ __forceinline__ KrLacSlot place(const Args& A, int run, int sub, int t0) {
        const int slot = A.runs[3 * run], off = A.runs[3 * run + 1], cnt = A.runs[3 * run + 2];
        return KrLacSlot{sub, cnt, (cnt + LC_T - 1) / LC_T, run, off, t0, A.conv_state + (size_t)slot * A.conv_stride, A.recur + (size_t)slot * A.recur_stride};
    }
    static __device__ __forceinline__ KrLacSlot prep(const Args& A) { const int* tl = A.lc_tiles + 2 * blockIdx.x; return place(A, tl[0], tl[1], (int)blockIdx.x); }
    static __device__ __forceinline__ KrLacSlot scan(const Args& A) { const int* rn = A.lc_runs + 2 * blockIdx.y; return place(A, rn[0], 0, rn[1]); }
    __device__ __forceinline__ int tile() const { return t0; }
    __device__ __forceinline__ int tile0() const { return t0; }
    __device__ __forceinline__ int row(int t) const { return kr_m_run_row(run, off, C, t); }
    __device__ __forceinline__ const float* conv(const KrLacArgs&) const { return cs; }
    __device__ __forceinline__ float* state(const KrLacArgs&) const { return st; }
};

// the carried conv inputs of every chunked run after it: input j of a channel = X(cnt - 4 + j), kr_pfm_la_conv_state_kernel's rule.  cnt >= 64: all four come
// from the run's rows.  Launched BEHIND the prep launch, which reads the old ones.  grid (conv_dim / 256, chunked runs), thread = channel
__global__ void __launch_bounds__(256) kr_multi_lc_conv_state_kernel(const KrMultiLaArgs a, const int* __restrict__ runs) {
    const int run = a.lc_runs[2 * blockIdx.y], ch = blockIdx.x * 256 + threadIdx.x;
    const int key_dim = a.nk * a.dk, conv_dim = 2 * key_dim + a.nv * a.dv, group_dim = 2 * a.dk + 2 * a.dv * a.hr;
    if (ch >= conv_dim) return;
    const int slot = runs[3 * run], row0 = runs[3 * run + 1], cnt = runs[3 * run + 2];
    int kh, off;
    if (ch < key_dim) { kh = ch / a.dk; off = ch % a.dk; }
    else if (ch < 2 * key_dim) { kh = (ch - key_dim) / a.dk; off = a.dk + (ch - key_dim) % a.dk; }
    else { const int vh = (ch - 2 * key_dim) / a.dv, i = (ch - 2 * key_dim) % a.dv; kh = vh / a.hr; off = 2 * a.dk + (vh % a.hr) * a.dv + i; }
    float n[4];
#pragma unroll
    for (int j = 0; j < 4; j++) n[j] = a.qkvz[(size_t)kr_m_run_row(run, row0, cnt, cnt - 4 + j) * a.ld_qkvz + (size_t)kh * group_dim + off];
    reinterpret_cast<float4*>(a.conv_state + (size_t)slot * a.conv_stride)[ch] = float4{n[0], n[1], n[2], n[3]};
}

// gated RMSNorm + SiLU gate of the chunked runs' rows: kr_pfm_gated_norm_kernel's arithmetic (a wave per (token, head) row in a wave-private LDS slice, the sum
// of squares as the reference's 8-lane chain, no workgroup barrier), z read where the in-projection left it.  grid (nv, 8 per sub-chunk tile): workgroup (h, y)
// takes tokens 8 (y & 7) .. + 8 of tile y >> 3, two per wave.  The rows of the other runs already hold the exact run kernel's output and are not touched
__global__ void __launch_bounds__(256) kr_multi_lc_gated_norm_kernel(const KrMultiLaArgs a, const int* __restrict__ runs) {
    __shared__ __attribute__((aligned(16))) float rs[4][256 + 8];
    const int h = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, dv = a.dv;
    const int* tl = a.lc_tiles + 2 * (blockIdx.y >> 3);
    const int run = tl[0], sub = tl[1], row0 = runs[3 * run + 1], cnt = runs[3 * run + 2];
    float* r = rs[wave];
    const int nc = dv / 4;
    const size_t zoff = (size_t)(h / a.hr) * (2 * a.dk + 2 * dv * a.hr) + 2 * a.dk + a.hr * dv + (size_t)(h % a.hr) * dv;
    const bool act = lane < nc;
    const float4 wv = act ? *reinterpret_cast<const float4*>(a.norm_w + (size_t)h * dv + 4 * lane) : float4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int tw = 0; tw < 2; tw++) {
        const int t = sub * LC_T + (blockIdx.y & 7) * 8 + tw * 4 + wave;
        if (t >= cnt) break;                                      // wave-uniform
        const size_t b = (size_t)kr_m_run_row(run, row0, cnt, t);
        float4 v = float4{0.0f, 0.0f, 0.0f, 0.0f}, zz = v;
        if (act) { v = *reinterpret_cast<const float4*>(a.lc_o + b * a.nv * dv + (size_t)h * dv + 4 * lane); zz = *reinterpret_cast<const float4*>(a.qkvz + b * a.ld_qkvz + zoff + 4 * lane); *reinterpret_cast<float4*>(r + 4 * lane) = v; }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier();
        if (lane < 8) { const float ss = kr_sumsq8<8, 0>(r, dv, lane); if (lane == 0) r[256] = kr_rms_inv(ss, dv, a.eps); }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier();
        const float rms = r[256];
        if (act) {
            float4 ov;
            ov.x = kr_gated_norm_out(v.x, rms, wv.x, zz.x); ov.y = kr_gated_norm_out(v.y, rms, wv.y, zz.y);
            ov.z = kr_gated_norm_out(v.z, rms, wv.z, zz.z); ov.w = kr_gated_norm_out(v.w, rms, wv.w, zz.w);
            *reinterpret_cast<float4*>(a.out + b * a.ld_out + (size_t)h * dv + 4 * lane) = ov;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier();      // the slice is rewritten by the wave's next row
    }
}

int kr_multi_lc_ok(int dk, int dv, int nk, int nv, int ld_qkvz) { return dk == LC_D && dv == LC_D && nk >= 1 && nv == nk * (nv / nk) && ld_qkvz % 4 == 0; }
// outside the pass: both kernels stage more than the default 64 KiB window of a kernel (134 KiB / 130 KiB).  The window is raised per kernel function, and
// every instantiation is a function of its own
int kr_multi_lc_prepare() {
    return kr_lds_optin(reinterpret_cast<const void*>(kr_lac_prep_kernel<KrLacSlot>), LC_PREP_LDS) || kr_lds_optin(reinterpret_cast<const void*>(kr_lac_scan_kernel<KrLacSlot>), LC_SCAN_LDS);
}

int kr_launch_multi_la_chunk(const KrMultiLaArgs& m, const int* runs, hipStream_t st) {
    if (!kr_multi_lc_ok(m.dk, m.dv, m.nk, m.nv, m.ld_qkvz) || !m.lc_runs || !m.lc_tiles || !m.lc_scratch || !m.lc_o || m.lc_nruns < 1 || m.lc_ntiles < m.lc_nruns) return 1;
    KrLacSlotArgs A{};
    KrLacArgs& a = A.lac;
    a.fused = 1; a.qkvz = m.qkvz; a.ld_qkvz = m.ld_qkvz; a.ba = m.ba; a.ld_ba = m.ld_ba; a.conv_w = m.conv_w; a.a_log = m.a_log; a.dt_bias = m.dt_bias;
    a.scale = m.scale; a.nk = m.nk; a.hr = m.hr; a.nv = m.nv;
    const size_t tiles = (size_t)m.lc_ntiles * m.nv * LC_T;      // the carve of kr_launch_pfm_la_chunked, over the pass's tiles
    a.Y = m.lc_scratch; a.G = a.Y + tiles * LC_D;
    uint16_t* pl = reinterpret_cast<uint16_t*>(a.G + ((tiles + 3) / 4) * 4);        // planes start 16-byte aligned
    a.Wh = pl; a.Wl = a.Wh + tiles * LC_D; a.Qh = a.Wl + tiles * LC_D; a.Ql = a.Qh + tiles * LC_D; a.Kh = a.Ql + tiles * LC_D; a.Kl = a.Kh + tiles * LC_D;
    a.out = m.lc_o;
    A.runs = runs; A.lc_runs = m.lc_runs; A.lc_tiles = m.lc_tiles;
    A.conv_state = m.conv_state; A.conv_stride = m.conv_stride; A.recur = m.recur; A.recur_stride = m.recur_stride;
    const int conv_dim = 2 * m.nk * m.dk + m.nv * m.dv;
    hipLaunchKernelGGL(kr_lac_prep_kernel<KrLacSlot>, dim3(m.lc_ntiles, m.nv), dim3(LC_PTH), LC_PREP_LDS, st, A);
    hipLaunchKernelGGL(kr_multi_lc_conv_state_kernel, dim3((conv_dim + 255) / 256, m.lc_nruns), dim3(256), 0, st, m, runs);      // behind the prep launch: it read the old inputs
    hipLaunchKernelGGL(kr_lac_scan_kernel<KrLacSlot>, dim3(m.nv * 4, m.lc_nruns), dim3(256), LC_SCAN_LDS, st, A);
    hipLaunchKernelGGL(kr_multi_lc_gated_norm_kernel, dim3(m.nv, m.lc_ntiles * 8), dim3(256), 0, st, m, runs);
    return 0;
}
