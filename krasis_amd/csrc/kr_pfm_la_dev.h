// kr_pfm_la_dev.h -- the four kernels of the exact staged linear attention (causal conv + SiLU + gates + L2 norms; the carried conv inputs; the gated delta rule
// token by token; the gated RMSNorm) as kernel templates over WHERE a workgroup's tokens lie, so that two callers share one text: the store's own exact prompt
// pass (kr_prefill_ops.hip: token t is row t, the store's own states, tile y of the grid first -- every member of its `Where` a compile-time identity) and the
// runs of a batched pass over device slots under "multi_extend_la_exact" (kr_multi_la_exact.hip, docs/design/36-multi-extend-la-exact.md: tiles and runs of the
// pass's tables, rows through the flatten of the pass, states in the run's slot).  Per value the arithmetic is the decode step's, so a run carries the bits the
// run kernels of kr_multi.hip give it.
// `Where` gives three argument types and, per kernel, the placement of this workgroup:
//   ConvArgs, la(ConvArgs) -> the KrPfmLaArgs in it     conv(A):    C, t0 = the first of the workgroup's 16 tokens     cstate(A): C
//   RecurArgs, rec(RecurArgs) -> KrPfmLaRecurArgs       recur(A):   C
//   NormPlace                                           norm(P, C): C, t0 = the first of the workgroup's 8 tokens (the gated norm keeps its scalar arguments and
//                                                       takes the placement as one more: as one struct its pointers lose `__restrict__`, two registers more)
//   C        tokens of the chunk / run                  row(t)     the row of token t < C in qkvz / ba / q / k / v / z / gexp / beta / recur / out
//   cs(a)    the four carried conv inputs per channel, [conv_dim][4]        state(r)   the recurrent state [nv][DK][dv]
// They are kernel templates, not device functions inlined into one-line kernels (kr_lac_dev.h, docs/design/25-multi-extend-flash.md).
#pragma once
#include <hip/hip_runtime.h>
#include "kr_device.h"
#include "kr_libm.h"
#include "kr_exact_dev.h"
#include "kr_prefill_ops.h"

struct KrPfmLaRecurArgs {
    float* state;                                      // [nv][DK][dv]
    const float *q, *k, *v, *gexp, *beta;              // [rows][nv * DK] x2, [rows][nv * dv], [rows][nv] x2
    float* out;                                        // [rows][nv * dv]
    int nv, dv, C;
};

// ---- linear attention: causal conv + SiLU + L2 norms + gates for every token (decode.rs:3815-3945) -------------------------
// grid (nk, tiles of 16 tokens): a workgroup takes one key head and SIXTEEN consecutive tokens, as two tiles of eight; a thread takes FOUR consecutive channels of one tile
// and walks them down the 8 tokens with the 4-tap window in registers: 11 row reads of 16 bytes per lane (round 2-4: one channel per thread, 4-byte reads -- the
// launch moved 180 MB per 2731-token chunk at 1.1 TB/s, 5.9 % of the tolerance prompt pass).  Tap j of token t is X(t-3+j): a chunk row for >= 0, the carried conv
// state slot 4+i for i < 0.  Per value the arithmetic is unchanged: the tap products are added left to right, SiLU with the degree-5 sigmoid, the two L2 norms as
// 8-lane fma chains over the head's conv outputs.  Needs dk % 4 == 0, dv % 4 == 0 and ld_qkvz % 4 == 0 (the launchers refuse other shapes); any channel count and
// any hr: the channel-quad loop, the z copy and the gate block all stride over the workgroup's threads.
#define PFC_TT 8
#define PFC_WT 16      // tokens per workgroup
template <class Where>
__global__ void __launch_bounds__(256) kr_pfm_la_conv_kernel(typename Where::ConvArgs A) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const KrPfmLaArgs& a = Where::la(A);
    const Where W = Where::conv(A);
    const int C = W.C;
    const int kh = blockIdx.x, w0 = W.t0, dk = a.dk, dv = a.dv, hr = a.hr, nk = a.nk;
    const int nw = C - w0 < PFC_WT ? C - w0 : PFC_WT;                       // tokens of this workgroup
    const int group_dim = 2 * dk + 2 * dv * hr, key_dim = nk * dk, nvdk = a.nv * dk, nvdv = a.nv * dv;
    float* qc = sm; float* kc = sm + PFC_WT * dk; float* nrm = sm + 2 * PFC_WT * dk;       // [16][dk], [16][dk], [16][2]
    const int nch = 2 * dk + hr * dv, nq = nch / 4;
    const int half = threadIdx.x >> 7, t0 = w0 + half * PFC_TT;               // this thread's token tile
    const int nt = C - t0 < PFC_TT ? (C - t0 < 0 ? 0 : C - t0) : PFC_TT;
    for (int cq = threadIdx.x & 127; cq < nq; cq += 128) {
        const int c = cq * 4;
        int ch, off;
        if (c < dk) { ch = kh * dk + c; off = c; }
        else if (c < 2 * dk) { ch = key_dim + kh * dk + (c - dk); off = c; }
        else { const int r = (c - 2 * dk) / dv, i = (c - 2 * dk) % dv; ch = 2 * key_dim + (kh * hr + r) * dv + i; off = 2 * dk + r * dv + i; }
        const float* cs = W.cs(a) + (size_t)ch * 4;
        float4 cw[4];
#pragma unroll
        for (int q = 0; q < 4; q++) cw[q] = *reinterpret_cast<const float4*>(a.conv_w + (size_t)(ch + q) * 4);
        const float* col = a.qkvz + (size_t)kh * group_dim + off;
        float4 x[PFC_TT + 3];                       // X(t0 - 3) .. X(t0 + 7) of the four channels, all requested before the first use
#pragma unroll
        for (int j = 0; j < PFC_TT + 3; j++) {
            const int i = t0 - 3 + j;
            if (i < 0) x[j] = float4{cs[4 + i], cs[8 + i], cs[12 + i], cs[16 + i]};        // slot 4 + i of channels ch .. ch + 3 (first tile of the chunk only)
            else x[j] = i < C ? *reinterpret_cast<const float4*>(col + (size_t)W.row(i) * a.ld_qkvz) : float4{0.0f, 0.0f, 0.0f, 0.0f};
        }
#pragma unroll
        for (int tt = 0; tt < PFC_TT; tt++)
            if (tt < nt) {
                const float4 co = float4{kr_conv4_silu(x[tt].x, x[tt + 1].x, x[tt + 2].x, x[tt + 3].x, cw[0]), kr_conv4_silu(x[tt].y, x[tt + 1].y, x[tt + 2].y, x[tt + 3].y, cw[1]),
                                         kr_conv4_silu(x[tt].z, x[tt + 1].z, x[tt + 2].z, x[tt + 3].z, cw[2]), kr_conv4_silu(x[tt].w, x[tt + 1].w, x[tt + 2].w, x[tt + 3].w, cw[3])};
                const int wt = half * PFC_TT + tt;
                if (c < dk) *reinterpret_cast<float4*>(qc + wt * dk + c) = co;
                else if (c < 2 * dk) *reinterpret_cast<float4*>(kc + wt * dk + (c - dk)) = co;
                else *reinterpret_cast<float4*>(a.v + (size_t)W.row(t0 + tt) * nvdv + (ch - 2 * key_dim)) = co;
            }
    }
    for (int c = threadIdx.x; c < nw * hr * dv / 4; c += 256) {
        const int e = c * 4, tt = e / (hr * dv), rem = e % (hr * dv), r = rem / dv, i = rem % dv;
        const size_t b = (size_t)W.row(w0 + tt);
        *reinterpret_cast<float4*>(a.z + b * nvdv + (size_t)(kh * hr + r) * dv + i) =
            *reinterpret_cast<const float4*>(a.qkvz + b * a.ld_qkvz + (size_t)kh * group_dim + 2 * dk + hr * dv + r * dv + i);
    }
    for (int gi = threadIdx.x; gi < nw * hr; gi += 256) {   // decode.rs:3891-3901; strided: 16 tokens x hr value heads per key head can exceed the 256 threads (hr > 16)
        const int tt = gi / hr, r = gi % hr, vh = kh * hr + r;
        const size_t t = (size_t)W.row(w0 + tt);
        const float* ba = a.ba + t * a.ld_ba;
        const float b_raw = ba[kh * 2 * hr + r], a_p = ba[kh * 2 * hr + hr + r];
        float g; kr_la_gate(b_raw, a_p, a.dt_bias[vh], a.a_log[vh], a.beta[t * a.nv + vh], g);
        a.gexp[t * a.nv + vh] = kr_expf(g);   // decode.rs:1293 decays the state by exp(g)
    }
    __syncthreads();
    if (threadIdx.x < 16 * PFC_WT) {            // 8 lanes per (token, q | k) chain
        const int tt = threadIdx.x >> 4, which = (threadIdx.x >> 3) & 1, l = threadIdx.x & 7;
        if (tt < nw) {
            const float ss = kr_sumsq8<8, 0>((which ? kc : qc) + tt * dk, dk, l);
            if (l == 0) nrm[tt * 2 + which] = kr_l2_inv(ss);
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < nw * hr * dk / 4; c += 256) {
        const int e = c * 4, tt = e / (hr * dk), rem = e % (hr * dk), r = rem / dk, i = rem % dk, vh = kh * hr + r;
        const float inv_q = nrm[tt * 2] * a.scale, inv_k = nrm[tt * 2 + 1] * 1.0f;
        const float4 qv = *reinterpret_cast<const float4*>(qc + tt * dk + i), kv = *reinterpret_cast<const float4*>(kc + tt * dk + i);
        const size_t b = (size_t)W.row(w0 + tt);
        *reinterpret_cast<float4*>(a.q + b * nvdk + (size_t)vh * dk + i) = float4{qv.x * inv_q, qv.y * inv_q, qv.z * inv_q, qv.w * inv_q};
        *reinterpret_cast<float4*>(a.k + b * nvdk + (size_t)vh * dk + i) = float4{kv.x * inv_k, kv.y * inv_k, kv.z * inv_k, kv.w * inv_k};
    }
}

// carried conv state after the chunk: slot j = X(C-4+j).  Launched AFTER the conv kernel (it reads the old slots).  one thread per channel (blockIdx.x over them)
template <class Where>
__global__ void kr_pfm_la_conv_state_kernel(typename Where::ConvArgs A) {
    const KrPfmLaArgs& a = Where::la(A);
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    const int key_dim = a.nk * a.dk, conv_dim = 2 * key_dim + a.nv * a.dv;
    if (ch >= conv_dim) return;
    const Where W = Where::cstate(A);
    const int C = W.C;
    const int group_dim = 2 * a.dk + 2 * a.dv * a.hr;
    int kh, off;
    if (ch < key_dim) { kh = ch / a.dk; off = ch % a.dk; }
    else if (ch < 2 * key_dim) { kh = (ch - key_dim) / a.dk; off = a.dk + (ch - key_dim) % a.dk; }
    else { const int vh = (ch - 2 * key_dim) / a.dv, i = (ch - 2 * key_dim) % a.dv; kh = vh / a.hr; off = 2 * a.dk + (vh % a.hr) * a.dv + i; }
    float* cs = W.cs(a) + (size_t)ch * 4;
    float n[4];
#pragma unroll
    for (int j = 0; j < 4; j++) { const int i = C - 4 + j; n[j] = i >= 0 ? a.qkvz[(size_t)W.row(i) * a.ld_qkvz + (size_t)kh * group_dim + off] : cs[4 + i]; }
#pragma unroll
    for (int j = 0; j < 4; j++) cs[j] = n[j];
}

// ---- gated delta rule over the chunk (decode.rs:1293): one thread per state column, the column lives in registers ------------
// grid (nv [, runs]), dv threads.  Per token: kv = chain_i fma(S[i]*e^g, k[i]); delta = (v - kv)*beta; S[i] = fma(k[i], delta, S[i]*e^g); o = chain_i fma(S[i], q[i]).
// The two DK-long fma chains per token are inherent to the reference order, and a dependent v_fmac issues only every ~15 cycles on this part: run one after the other they
// cost 2 x DK x 15 cycles per token (1.8 us at DK = 128: the round-5 form).  Round 6: the OUTPUT chain of token t and the kv chain of token t + 1 are independent once
// S(t)[i] exists, so they advance together, element by element -- update S[i] with delta_t, step o_t, decay S[i] by e^g(t+1), step kv_(t+1): four instructions per element,
// two chains in each other's latency shadow; every value is produced by the same operation in the same order as before (bit-identical).  Behind the last token runs a
// phantom one with e^g = 1 (S * 1.0f is S) whose chain nobody reads.  The rows (k, q, v) and the two gate scalars of a token reach an LDS ring of RS slots by LDS-DMA
// (global_load_lds_dword: lane i's word lands at M0 + 4 i), requested three tokens ahead: no staging registers, one loop body; the state slice is addressed through a
// buffer descriptor (scalar row offsets) so that no per-row 64-bit addresses stay live across the loop.
// (Measured earlier and slower: LDS-staged token blocks; one packed fma advancing both chains on a {S*e^g, S} register pair -- 2 x DK registers; the same interleave with
// the rows prefetched into rotating register sets -- three copies of the loop, 328 registers.)
// Bounds: W.row is asked for t < C only (the phantom token re-reads row C - 1), and the descriptor covers exactly head h's [DK][dv] block of W.state.
__device__ __forceinline__ void pfm_dma4(uint32_t lds_dst, const void* gptr) {      // this lane's 4 bytes at gptr -> lds_dst + 4 * lane; not counted by the compiler's waits
    unsigned keep;
    lds_dst = __builtin_amdgcn_readfirstlane(lds_dst);
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 2\n\tglobal_load_lds_dword %2, off\n\ts_mov_b32 m0, %0" : "=&s"(keep) : "s"(lds_dst), "v"(gptr) : "memory");
}
template <int DK, class Where>
__global__ void __launch_bounds__(256) kr_pfm_la_recur_kernel(typename Where::RecurArgs A) {
    constexpr int RS = 5, ROW = 256;                 // ring slots; floats per row region (dv <= 256)
    constexpr int SLOT = 3 * ROW + 128;              // floats per slot: k row, q row, v row, e^g at [3 ROW], beta at [3 ROW + 1] (wave 0's other lanes land behind them), a 64-word dump at [3 ROW + 64]
    __shared__ __attribute__((aligned(16))) float ring[RS][SLOT];
    const KrPfmLaRecurArgs& R = Where::rec(A);
    const Where W = Where::recur(A);                 // workgroup-uniform: the run's table entries come by scalar loads, ahead of the loop
    const float* __restrict__ q = R.q; const float* __restrict__ k = R.k; const float* __restrict__ v = R.v;
    const float* __restrict__ gexp = R.gexp; const float* __restrict__ beta = R.beta; float* __restrict__ out = R.out;
    const int nv = R.nv, dv = R.dv, C = W.C;
    const int h = blockIdx.x, j = threadIdx.x, lane = j & 63, wv = __builtin_amdgcn_readfirstlane(j >> 6), nvdk = nv * DK, nvdv = nv * dv;
    float S[DK];
    const __amdgpu_buffer_rsrc_t srd = __builtin_amdgcn_make_buffer_rsrc(W.state(R) + (size_t)h * DK * dv, 0, DK * dv * 4, 0x00020000);
#pragma unroll
    for (int i = 0; i < DK; i++) S[i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(srd, j * 4, i * dv * 4, 0));
    const uint32_t ring0 = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)&ring[0][0];
    const bool kq_wave = wv * 64 < DK;                                   // wave-uniform: this wave's columns have k / q words
    const int jk = kq_wave ? j : lane;                                    // other waves fetch (harmless) words into the slot's spare area: every wave issues 5 DMAs per token
    auto request = [&](int tt, int slot) {           // token tt (clamped: a phantom token behind the chunk re-reads the last one; its gates are forced below)
        const size_t tc = (size_t)W.row(tt < C ? tt : C - 1);
        const uint32_t base = ring0 + (uint32_t)slot * (SLOT * 4), dump = base + (3 * ROW + 64) * 4;
        pfm_dma4(kq_wave ? base + wv * 256 : dump, k + tc * nvdk + (size_t)h * DK + jk);
        pfm_dma4(kq_wave ? base + ROW * 4 + wv * 256 : dump, q + tc * nvdk + (size_t)h * DK + jk);
        pfm_dma4(base + 2 * ROW * 4 + wv * 256, v + tc * nvdv + (size_t)h * dv + j);
        pfm_dma4(wv == 0 ? base + 3 * ROW * 4 : dump, (lane == 0 ? gexp : beta) + tc * nv + h);      // wave 0: lane 0 -> e^g, lane 1 -> beta (lanes 2 .. 63 land behind them, unread)
        pfm_dma4(dump, beta + tc * nv + h);                                                          // filler: every wave issues exactly 5 requests per token (the wait below counts them)
    };
    request(0, 0); request(1, 1); request(2, 2);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // prologue: decay + kv chain of token 0 alone
    float delta;
    {
        const float4* k4 = reinterpret_cast<const float4*>(&ring[0][0]);
        const float ge0 = ring[0][3 * ROW], bt0 = ring[0][3 * ROW + 1], vj0 = ring[0][2 * ROW + j];
        float kv = 0.0f;
#pragma unroll
        for (int u = 0; u < DK / 4; u++) {
            const float4 kk = k4[u];
            float* Sb = S + 4 * u;
            Sb[0] = Sb[0] * ge0; kv = __builtin_fmaf(Sb[0], kk.x, kv);
            Sb[1] = Sb[1] * ge0; kv = __builtin_fmaf(Sb[1], kk.y, kv);
            Sb[2] = Sb[2] * ge0; kv = __builtin_fmaf(Sb[2], kk.z, kv);
            Sb[3] = Sb[3] * ge0; kv = __builtin_fmaf(Sb[3], kk.w, kv);
        }
        delta = (vj0 - kv) * bt0;
    }
    int slot = 0;
    for (int t = 0; t < C; t++) {
        // token t: S update + output chain of token t, together with decay + kv chain of token t + 1; blocks of 16 elements, the next block's rows leave LDS while the
        // current block's steps run (the scheduling fences keep the reads from sinking next to their uses)
        const int s1 = slot + 1 >= RS ? slot + 1 - RS : slot + 1, s3 = slot + 3 >= RS ? slot + 3 - RS : slot + 3;
        request(t + 3, s3);          // slot s3 held token t - 2: last read two barriers ago
        const float4* k4 = reinterpret_cast<const float4*>(&ring[slot][0]); const float4* q4 = reinterpret_cast<const float4*>(&ring[slot][ROW]);
        const float4* n4 = reinterpret_cast<const float4*>(&ring[s1][0]);
        const bool has_next = t + 1 < C;
        const float ge1 = has_next ? ring[s1][3 * ROW] : 1.0f, bt1 = ring[s1][3 * ROW + 1], vj1 = ring[s1][2 * ROW + j];
        float ob = 0.0f, kv = 0.0f;
        float4 ka[4] = {k4[0], k4[1], k4[2], k4[3]}, qa[4] = {q4[0], q4[1], q4[2], q4[3]}, na[4] = {n4[0], n4[1], n4[2], n4[3]};
#pragma unroll
        for (int b = 0; b < DK / 16; b++) {
            float4 kb[4] = {ka[0], ka[1], ka[2], ka[3]}, qb[4] = {qa[0], qa[1], qa[2], qa[3]}, nb[4] = {na[0], na[1], na[2], na[3]};
            if (b + 1 < DK / 16) {
#pragma unroll
                for (int u = 0; u < 4; u++) { kb[u] = k4[4 * b + 4 + u]; qb[u] = q4[4 * b + 4 + u]; nb[u] = n4[4 * b + 4 + u]; }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < 4; u++) {
                float* Sb = S + 16 * b + 4 * u;
                const float kk[4] = {ka[u].x, ka[u].y, ka[u].z, ka[u].w}, qq[4] = {qa[u].x, qa[u].y, qa[u].z, qa[u].w}, nn[4] = {na[u].x, na[u].y, na[u].z, na[u].w};
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    Sb[e] = __builtin_fmaf(kk[e], delta, Sb[e]); ob = __builtin_fmaf(Sb[e], qq[e], ob);
                    Sb[e] = Sb[e] * ge1; kv = __builtin_fmaf(Sb[e], nn[e], kv);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < 4; u++) { ka[u] = kb[u]; qa[u] = qb[u]; na[u] = nb[u]; }
        }
        out[(size_t)W.row(t) * nvdv + (size_t)h * dv + j] = ob;
        delta = (vj1 - kv) * bt1;
        // the next token reads slots t + 1 and t + 2: this wave's requests for token t + 2 (issued one token ago) are older than its 5 requests for t + 3 and the two
        // output stores since -- at most 7 vector-memory operations may still be in flight
        asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
        __syncthreads();
        slot = s1;
    }
#pragma unroll
    for (int i = 0; i < DK; i++) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(S[i]), srd, j * 4, i * dv * 4, 0);
}

// ---- gated RMSNorm + SiLU gate per (token, head) (decode.rs:3979) ----------------------------------------------------------------
// grid (nv, tiles of 8 tokens), 256 threads: a WAVE takes one (token, head) row at a time (two rows per wave: 8 tokens per workgroup), the row in a wave-private LDS slice,
// the sum of squares as the reference's 8-lane chain + hsum (kr_sumsq8) on lanes 0..7, no workgroup barrier.  (Rounds 1-5: one workgroup of dv threads per
// (token, head) -- 262 144 workgroups of two waves for an 8192-token chunk, 140 us against ~80 us of traffic.)  z may sit inside the in-projection's output
// (z_ld = its row stride, z_head = floats between the z blocks of consecutive value heads): the stand-alone copy of z is then never made.
#define PFG_TT 8
template <class Where>
__global__ void __launch_bounds__(256) kr_pfm_gated_norm_kernel(const float* __restrict__ recur, const float* __restrict__ z, size_t z_ld, int z_hr, int z_kstride, const float* __restrict__ w,
                                                               float* __restrict__ out, int nv, int dv, int C_, float eps, typename Where::NormPlace P) {
    __shared__ __attribute__((aligned(16))) float rs[4][256 + 8];
    const Where W = Where::norm(P, C_);
    const int C = W.C;
    const int h = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* r = rs[wave];
    const int nc = dv / 4;                                          // 16-byte chunks of a row (dv % 8 == 0, dv <= 256: one chunk per lane at most)
    // z of value head h: block (h / z_hr) of z_kstride floats, then head h % z_hr inside it (plain [C][nv * dv] rows: z_hr = nv, one block)
    const size_t zoff = (size_t)(h / z_hr) * z_kstride + (size_t)(h % z_hr) * dv;
    const bool act = lane < nc;
    const float4 wv = act ? *reinterpret_cast<const float4*>(w + (size_t)h * dv + 4 * lane) : float4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int tw = 0; tw < PFG_TT / 4; tw++) {
        const int t = W.t0 + tw * 4 + wave;
        if (t >= C) break;                                        // wave-uniform
        const int b = W.row(t);
        const size_t o = (size_t)b * nv * dv + (size_t)h * dv;
        float4 v = float4{0.0f, 0.0f, 0.0f, 0.0f}, zz = v;
        if (act) { v = *reinterpret_cast<const float4*>(recur + o + 4 * lane); zz = *reinterpret_cast<const float4*>(z + (size_t)b * z_ld + zoff + 4 * lane); *reinterpret_cast<float4*>(r + 4 * lane) = v; }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier();
        if (lane < 8) { const float ss = kr_sumsq8<8, 0>(r, dv, lane); if (lane == 0) r[256] = kr_rms_inv(ss, dv, eps); }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier();
        const float rms = r[256];
        if (act) {
            float4 ov;
            ov.x = kr_gated_norm_out(v.x, rms, wv.x, zz.x); ov.y = kr_gated_norm_out(v.y, rms, wv.y, zz.y);
            ov.z = kr_gated_norm_out(v.z, rms, wv.z, zz.z); ov.w = kr_gated_norm_out(v.w, rms, wv.w, zz.w);
            *reinterpret_cast<float4*>(out + o + 4 * lane) = ov;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier();      // the slice is rewritten by the wave's next row
    }
}
