// kr_moe_decode.hip -- memory-bound M=1..few MoE expert path for gfx950 (MI355X).
//
// Replaces (bit-exactly) the reference's CPU decode experts:
//   moe_forward_unified (src/moe.rs:572-715) -> expert_forward_unified (src/moe.rs:184-380)
//   -> expert_matmul_int4/int8_transposed_integer (src/kernel/avx2.rs:1066,1477),
//   quantize_activation_int16 (avx2.rs:234), silu_quantize_int16_avx2 (avx2.rs:2310).
//
// Shape of the computation on the GPU:
//   * a wave owns 8 output columns; each column is served by 8 lanes that split every 128-wide
//     quantization group 16/16/.. between them.  One `global_load_dwordx4` per lane per group pair
//     => every wave-level load is 1 KiB of contiguous, streamed-once (non-temporal) HBM.
//   * integer dot products are exact: a(i16) = AH*256 + AL, nibbles stay unsigned,
//     sum(q*a) = 256*sdot4(q,AH) + udot4(q,AL), minus 8*sum(a) for the INT4 offset.
//   * the per-group i32 sums are reduced over the 8 lanes with DPP adds and folded into the
//     column's f32 accumulator with ONE fma per group, in group order -- the same chain as
//     _mm256_fmadd_ps(group_f32, w_scale*a_scale, out) in the reference, hence bit-identical.
#include "kr_device.h"
#include "kr_kernels.h"
#include "kr_matvec_dev.h"
#include "kr_libm.h"
#include "kr_exact_dev.h"
#include <cstdio>

#define KR_BLOCK 256
#define KR_WAVES (KR_BLOCK / 64)

#include "kr_matvec_tile_dev.h"      // the prologues and the per-wave tile (shared with kr_rows_matvec.hip)

// ------------------------------------------------------------------------------------------
// Cooperative tile: the KR_WAVES waves of a workgroup SPLIT THE K RANGE of one 8-column tile.
//
// Measured on MI355X (tools/probes/launch_floor.hip, matvec_timing.hip): a dependent launch in a replayed graph costs ~1.55 us and
// cold HBM loads add almost nothing, but every instruction on a wave's serial path costs ~3.5 ns -- a wave that walks all K/128 groups
// of its tile executes ~1000 dependent instructions, which IS the kernel's duration.  The integer group sums are order-free, so wave w
// computes the sums of groups [w*gw, (w+1)*gw) only; (f32(isum), bf16(w_scale)*a_scale) pairs go through LDS and 8 lanes replay the
// reference's one-fma-per-group chain in group order (avx2.rs:1162-1176): bit-identical, a quarter of the serial path.
// ------------------------------------------------------------------------------------------
#define KR_GMAX 8        // groups per wave whose weights are requested up front (K <= 4096 with 4 waves; longer K loops)
#define KR_NG_MAX 128    // groups per row the exchange buffer holds (K <= 16384)
struct KrXch { float2 v[8][KR_NG_MAX + 2]; };   // [column][group] = (f32(isum), bf16(w_scale) * a_scale)

template <int BITS> struct KrCo;
template <> struct KrCo<4> { u32x2 w[KR_GMAX]; uint32_t sc[KR_GMAX]; int g0, g1; };
template <> struct KrCo<8> { u32x4 w[KR_GMAX]; uint32_t sc[KR_GMAX]; int g0, g1; };

template <int BITS>
__device__ __forceinline__ void kr_co_fetch(KrCo<BITS>& p, const void* qbase, const uint32_t* sbase, const KrMatDev& m, int tile, int lane, int gb) {
#pragma unroll
    for (int u = 0; u < KR_GMAX; u++) {
        const int g = gb + u;
        if (g < p.g1) {
            if constexpr (BITS == 4) p.w[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(qbase) + (((size_t)tile * m.ngp + (g >> 1)) * 64 + lane) * 2 + (g & 1));
            else p.w[u] = kr_ldg_nt(reinterpret_cast<const u32x4*>(qbase) + ((size_t)tile * m.ng + g) * 64 + lane);
            p.sc[u] = kr_ldg_nt(sbase + ((size_t)tile * m.ngp + (g >> 1)) * 8 + (lane >> 3));
        }
    }
}
template <int BITS>
__device__ __forceinline__ void kr_co_preload(KrCo<BITS>& p, const void* qbase, const uint32_t* sbase, const KrMatDev& m, int tile, int lane, int wave) {
    const int gw = (m.ng + KR_WAVES - 1) / KR_WAVES;
    p.g0 = wave * gw; p.g1 = p.g0 + gw < m.ng ? p.g0 + gw : m.ng;
    kr_co_fetch<BITS>(p, qbase, sbase, m, tile, lane, p.g0);
}

// phase 1 (all waves): this wave's group sums -> LDS.  Call after the activation image is complete (workgroup barrier).
template <int BITS>
__device__ __forceinline__ void kr_co_sums(KrCo<BITS>& p, const void* qbase, const uint32_t* sbase, const KrMatDev& m, int tile, const KrActLds& L, KrXch& X, int lane) {
    const int l8 = lane & 7, col = lane >> 3;
    for (int gb = p.g0; gb < p.g1; gb += KR_GMAX) {
        if (gb > p.g0) kr_co_fetch<BITS>(p, qbase, sbase, m, tile, lane, gb);
#pragma unroll
        for (int u = 0; u < KR_GMAX; u++) {
            const int g = gb + u;
            if (g < p.g1) {
                int isum;
                if constexpr (BITS == 4) isum = kr_red8_add_i32(kr_group_i4(p.w[u].x, p.w[u].y, g, l8, L));
                else isum = kr_red8_add_i32(kr_group_i8(p.w[u], g, l8, L));
                const uint32_t sbits = (g & 1) ? (p.sc[u] >> 16) : (p.sc[u] & 0xFFFFu);
                if (l8 == 0) X.v[col][g] = make_float2((float)isum, __uint_as_float(sbits << 16) * L.ascale[g]);   // comb: avx2.rs:1171
            }
        }
    }
}
// phase 2 (after a workgroup barrier): lane c < 8 of wave 0 folds column c in group order
__device__ __forceinline__ float kr_co_chain(const KrXch& X, int ng, int col, bool fused) {
    float acc = 0.0f;
    int g = 0;
    for (; g + 4 <= ng; g += 4) {
        const float2 t0 = X.v[col][g], t1 = X.v[col][g + 1], t2 = X.v[col][g + 2], t3 = X.v[col][g + 3];
        if (fused) { acc = __builtin_fmaf(t0.x, t0.y, acc); acc = __builtin_fmaf(t1.x, t1.y, acc); acc = __builtin_fmaf(t2.x, t2.y, acc); acc = __builtin_fmaf(t3.x, t3.y, acc); }
        else { acc = acc + t0.x * t0.y; acc = acc + t1.x * t1.y; acc = acc + t2.x * t2.y; acc = acc + t3.x * t3.y; }      // avx2.rs:1201
    }
    for (; g < ng; g++) { const float2 t = X.v[col][g]; acc = fused ? __builtin_fmaf(t.x, t.y, acc) : (acc + t.x * t.y); }
    return acc;
}

// ------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------

extern __shared__ __attribute__((aligned(16))) u32x4 kr_smem[];

struct KrSlot { const void* q13; const uint32_t* s13; const void* q2; const uint32_t* s2; int inter; bool shared; bool valid; };

__device__ __forceinline__ KrSlot kr_resolve_slot(const KrMoeArgs& a, int b, int slot) {
    KrSlot r;
    r.shared = slot >= a.topk;
    if (r.shared) {
        r.valid = true; r.inter = a.I_shared;
        r.q13 = a.sw13.q; r.s13 = a.sw13.s; r.q2 = a.sw2.q; r.s2 = a.sw2.s;
    } else {
        const int e = a.ids[(size_t)b * a.topk + slot];
        const int lo = a.e_hi > 0 ? a.e_lo : 0, hi = a.e_hi > 0 ? a.e_hi : a.E;
        r.valid = e >= lo && e < hi; r.inter = a.I;
        const size_t ee = (size_t)(r.valid ? e - a.e_sub : 0);
        r.q13 = reinterpret_cast<const char*>(a.w13.q) + ee * a.w13.q_stride;
        r.s13 = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(a.w13.s) + ee * a.w13.s_stride);
        r.q2 = reinterpret_cast<const char*>(a.w2.q) + ee * a.w2.q_stride;
        r.s2 = reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(a.w2.s) + ee * a.w2.s_stride);
    }
    return r;
}

// pre-built activation image (global memory, byte layout == the LDS image for INT4 weights) -> LDS.  INT8 weights read the same INT16
// values in natural byte order (kr_store_chunk<true>): that second plane set is a byte permutation of the record, formed on the way in.
// Two phases (see kr_vec_load): the first KR_IMG_PRE records of a thread are requested by kr_image_load, before the caller's weight records.
#define KR_IMG_PRE 3
struct KrImgPre { u32x4 r[KR_IMG_PRE]; };
__device__ __forceinline__ void kr_image_load(const void* img, int K, KrImgPre& P) {
    const int n16 = (int)(kr_lds_bytes(K, false) / 16);
    const u32x4* src = reinterpret_cast<const u32x4*>(img);
#pragma unroll
    for (int j = 0; j < KR_IMG_PRE; j++)
        if (j == 0 || n16 > j * KR_BLOCK) { const int i = threadIdx.x + j * KR_BLOCK; P.r[j] = src[i < n16 ? i : n16 - 1]; }
}
template <int BITS>
__device__ __forceinline__ void kr_image_put(const u32x4 r, int i, int K, u32x4* smem, const KrActLds& L) {
    smem[i] = r;
    if constexpr (BITS == 8) {
        if (i < K / 8) {         // record of chunk i: x / y = high bytes of the even / odd values, z / w = low bytes
            uint32_t* p = reinterpret_cast<uint32_t*>(L.planes8) + (i >> 1) * 8 + (i & 1) * 2;
            p[0] = __builtin_amdgcn_perm(r.y, r.x, 0x05010400u);
            p[1] = __builtin_amdgcn_perm(r.y, r.x, 0x07030602u);
            p[4] = __builtin_amdgcn_perm(r.w, r.z, 0x05010400u) ^ 0x80808080u;    // (low byte) - 128 as i8
            p[5] = __builtin_amdgcn_perm(r.w, r.z, 0x07030602u) ^ 0x80808080u;
        }
    }
}
template <int BITS>
__device__ __forceinline__ void kr_image_copy(const void* img, int K, u32x4* smem, const KrActLds& L, const KrImgPre& P) {
    const int n16 = (int)(kr_lds_bytes(K, false) / 16);
    const u32x4* src = reinterpret_cast<const u32x4*>(img);
#pragma unroll
    for (int j = 0; j < KR_IMG_PRE; j++) { const int i = threadIdx.x + j * KR_BLOCK; if (i < n16) kr_image_put<BITS>(P.r[j], i, K, smem, L); }
    for (int i = threadIdx.x + KR_IMG_PRE * KR_BLOCK; i < n16; i += KR_BLOCK) kr_image_put<BITS>(src[i], i, K, smem, L);
}

// stage 1: gu[b][slot][0..2I) = W13 . q(act[b])      grid = (tile groups, n_slots, B)
// The shared slot may carry one extra tile: the shared expert's sigmoid-gate row (decode.rs:3379-3390), N = 1.
template <int BITS>
__global__ void __launch_bounds__(KR_BLOCK) kr_moe_w13_kernel(const void* p_img_bf16, const void* p_img_f32, int p_H, int p_topk, int p_shared_decode, int p_B,
                                                              const KrMoeArgs a, int tiles_per_wave) {      // leading scalars: preloaded (see kr_matvec_coop_kernel)
    const int slot = blockIdx.y, b = blockIdx.z;
    // the activation (image or vector) is requested first: it depends on nothing this launch reads, the weight records wait for the routing record
    const bool round_bf16 = !(slot >= p_topk && p_shared_decode);
    const void* img = p_B == 1 ? (round_bf16 ? p_img_bf16 : p_img_f32) : nullptr;   // pre-built by the router launch
    KrImgPre IP; KrVecPre VP;
    if (img) kr_image_load(img, p_H, IP);
    else if (a.act_f32) kr_vec_load(a.act_f32 + (size_t)b * a.H, a.H, VP);
    else kr_vec_load(a.act + (size_t)b * a.H, a.H, VP);
    const KrSlot sl = kr_resolve_slot(a, b, slot);
    if (!sl.valid) return;
    const KrMatDev& m = sl.shared ? a.sw13 : a.w13;
    const int ntiles = (m.N + 7) / 8;
    const bool with_gate = sl.shared && a.sgate.q != nullptr;
    const int tile0 = (blockIdx.x * KR_WAVES) * tiles_per_wave;
    if (tile0 >= ntiles + (with_gate ? 1 : 0)) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int first = tile0 + wave * tiles_per_wave;
    KrPre pre;
    const bool gate_wave = with_gate && first == ntiles;
    if (first < ntiles) kr_preload<BITS>(pre, sl.q13, sl.s13, m, first, lane, 0);
    else if (gate_wave) kr_preload<BITS>(pre, a.sgate.q, a.sgate.s, a.sgate, 0, lane, 0);   // the gate row has the width of the launch (host check)
    const KrActLds L = kr_carve_lds(kr_smem, a.H, BITS == 8);
    if (img) kr_image_copy<BITS>(img, a.H, kr_smem, L, IP);
    else if (a.act_f32) kr_prologue_quant_f32<BITS == 8>(a.act_f32 + (size_t)b * a.H, a.H, L, round_bf16, VP);
    else kr_prologue_quant<uint16_t, BITS == 8>(a.act + (size_t)b * a.H, a.H, L, VP);
    __syncthreads();
    float* gu = a.gu + ((size_t)b * a.n_slots + slot) * a.gu_ld;
    for (int t = 0; t < tiles_per_wave; t++) {
        const int tile = first + t;
        if (tile < ntiles) {
            const float acc = kr_matvec_tile<BITS>(pre, t == 0, sl.q13, sl.s13, m, tile, L, lane);
            const int col = tile * 8 + (lane >> 3);
            if ((lane & 7) == 0 && col < m.N) gu[col] = acc;
        } else if (with_gate && tile == ntiles) {
            const float acc = kr_matvec_tile<BITS>(pre, t == 0, a.sgate.q, a.sgate.s, a.sgate, 0, L, lane);
            if (lane == 0) a.gate_out[b] = acc;
        }
    }
}

// stage 2: eo[b][slot][0..H) = W2 . q(act_fn(gu[b][slot]))
template <int BITS, int ACT>
__global__ void __launch_bounds__(KR_BLOCK) kr_moe_w2_kernel(const float* p_gu, int p_n_slots, int p_gu_ld, int p_I, int p_I_shared, int p_topk, const KrMoeArgs a, int tiles_per_wave) {
    const int slot = blockIdx.y, b = blockIdx.z;
    const float* gu = p_gu + ((size_t)b * p_n_slots + slot) * p_gu_ld;
    KrHidPre HP;
    kr_hidden_load(gu, slot >= p_topk ? p_I_shared : p_I, HP);      // the slot's gate | up values first (kr_vec_load; preloaded arguments), then the routing record and the weights
    const KrSlot sl = kr_resolve_slot(a, b, slot);
    if (!sl.valid) return;
    const KrMatDev& m = sl.shared ? a.sw2 : a.w2;
    const int ntiles = (m.N + 7) / 8;
    const int tile0 = (blockIdx.x * KR_WAVES) * tiles_per_wave;
    if (tile0 >= ntiles) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int first = tile0 + wave * tiles_per_wave;
    KrPre pre;
    if (first < ntiles) kr_preload<BITS>(pre, sl.q2, sl.s2, m, first, lane, 0);
    const KrActLds L = kr_carve_lds(kr_smem, sl.inter, BITS == 8);
    if (sl.shared && a.shared_decode) kr_prologue_hidden<KR_ACT_SILU_MUL, BITS == 8>(gu, sl.inter, a.swiglu_limit, a.alpha, L, HP);
    else kr_prologue_hidden<ACT, BITS == 8>(gu, sl.inter, a.swiglu_limit, a.alpha, L, HP);
    __syncthreads();
    float* eo = a.eo + ((size_t)b * a.n_slots + slot) * a.H;
    for (int t = 0; t < tiles_per_wave; t++) {
        const int tile = first + t;
        if (tile >= ntiles) break;
        const float acc = kr_matvec_tile<BITS>(pre, t == 0, sl.q2, sl.s2, m, tile, L, lane);
        const int col = tile * 8 + (lane >> 3);
        if ((lane & 7) == 0 && col < m.N) eo[col] = acc;
    }
}

// stages 2 + 3 of the DECODE STEP in one launch (B == 1, round 5): one workgroup per 8-column tile of the output, ONE WAVE PER SLOT.  Every wave quantizes its slot's hidden
// values into a wave-private image (the arithmetic of kr_prologue_hidden, chunk = lane), runs the exact per-wave tile (kr_matvec_tile: the reference's chain order) and
// leaves its 8 column sums in LDS; lanes 0 .. 7 of wave 0 then form the step's MoE output in routing order -- sum_i w_i * eo_i (moe.rs:661-667), * rsf, + shared *
// sigmoid(gate) (decode.rs:3343-3402): the arithmetic the next layer's fused add + RMSNorm launch used to run over (topk + 1) rows of H floats pulled through ONE CU.
// That launch now reads `out` like any hidden vector (KrNormSrc mode 0).  Expert-parallel decode keeps stage 2 alone (its per-slot rows are all-reduced).
template <int BITS, int ACT>
// (the pointers of the first requests and the widths are leading scalar arguments: preloaded into SGPRs, see kr_matvec_coop_kernel)
__global__ void __launch_bounds__(1024) kr_moe_w2c_kernel(const float* p_gu, const int32_t* p_ids, const float* p_wts, const float* p_gate_val, int p_gu_ld, int p_I, int p_I_shared,
                                                         int p_topk, int p_img16, float* p_out, const KrMoeArgs a) {
    __shared__ float s_e[16][8];
    const int slot = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, tile = blockIdx.x;
    const bool shared = slot >= p_topk;
    const int inter = shared ? p_I_shared : p_I, nch = inter / 8;
    const float* gu = p_gu + (size_t)slot * p_gu_ld;
    // the slot's gate | up values first, the routing record and the weight records behind them (a wave's memory counter is in-order)
    float pg[8], pu[8];
    { const int c = lane < nch ? lane : nch - 1; kr_load8(gu, c, pg); kr_load8(gu + inter, c, pu); }
    float wv = 0.0f; int idv = -1; float gval = 0.0f;
    if (slot == 0) {      // the combine's operands: lane s holds slot s
        const int sc = lane < p_topk ? lane : p_topk - 1;
        wv = p_wts[sc]; idv = p_ids[sc];
        if (p_gate_val) gval = p_gate_val[0];
    }
    KrSlot sl;      // kr_resolve_slot for b = 0, no expert-parallel slice (the launcher refuses one)
    {
        const int e = shared ? 0 : p_ids[slot];
        sl.shared = shared; sl.inter = inter; sl.valid = shared || (e >= 0 && e < a.E);
        const size_t ee = (size_t)(sl.valid ? e : 0);
        sl.q2 = shared ? a.sw2.q : (const void*)(reinterpret_cast<const char*>(a.w2.q) + ee * a.w2.q_stride);
        sl.s2 = shared ? a.sw2.s : reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(a.w2.s) + ee * a.w2.s_stride);
        sl.q13 = nullptr; sl.s13 = nullptr;
    }
    const KrMatDev& m = shared ? a.sw2 : a.w2;
    KrPre pre;
    if (sl.valid) kr_preload<BITS>(pre, sl.q2, sl.s2, m, tile, lane, 0);
    const KrActLds L = kr_carve_lds(kr_smem + (size_t)slot * p_img16, inter, BITS == 8);
    if (sl.valid) {
        const bool mul = shared && a.shared_decode;      // the decode store's shared expert: silu * up with f32::round (KR_ACT_SILU_MUL)
        for (int c = lane; c < nch; c += 64) {
            float g[8], u[8], h[8];
            if (c == lane) {
#pragma unroll
                for (int i = 0; i < 8; i++) { g[i] = pg[i]; u[i] = pu[i]; }
            } else { kr_load8(gu, c, g); kr_load8(gu + inter, c, u); }
            float mx = 0.0f;
#pragma unroll
            for (int i = 0; i < 8; i++) {
                if (ACT == KR_ACT_GPTOSS && !mul) {  // moe.rs:272-280
                    float gate = g[i], up = u[i];
                    if (gate > a.swiglu_limit) gate = a.swiglu_limit;
                    if (up > a.swiglu_limit) up = a.swiglu_limit;
                    if (up < -a.swiglu_limit) up = -a.swiglu_limit;
                    const float glu = gate * kr_sigmoid_poly5_scalar(gate * a.alpha);
                    h[i] = (up + 1.0f) * glu;
                } else {                      // avx2.rs:2331-2333 / decode.rs:1731-1733
                    const float silu = g[i] * kr_sigmoid_poly5(g[i]);
                    h[i] = silu * u[i];
                }
                mx = fmaxf(mx, fabsf(h[i]));
            }
            float scale, inv;
            kr_group_scale(mx, scale, inv);
            int q[8];
            if (ACT == KR_ACT_SILU_FUSED && !mul) kr_quant8<true>(h, inv, q);   // _mm256_cvtps_epi32
            else kr_quant8<false>(h, inv, q);                                    // f32::round
            kr_store_chunk<BITS == 8>(L, c, q);
            if ((c & 15) == 0) L.ascale[c >> 4] = scale;
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the image is wave-private: the wave's own LDS writes are complete before its reads, no workgroup barrier
    float acc = 0.0f;
    if (sl.valid) acc = kr_matvec_tile<BITS>(pre, true, sl.q2, sl.s2, m, tile, L, lane);
    if ((lane & 7) == 0) s_e[slot][lane >> 3] = acc;
    __syncthreads();
    if (slot == 0) {
        const int c8 = lane & 7, col = tile * 8 + c8;
        float o = 0.0f;
#pragma unroll
        for (int s2 = 0; s2 < 16; s2++) if (s2 < p_topk) {      // v_readlane with a constant lane: one instruction per operand
            const float w = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, wv), s2)); const int id = __builtin_amdgcn_readlane(idv, s2);
            if (id >= 0) o += w * s_e[s2][c8];
        }
        if (a.rsf != 1.0f) o *= a.rsf;
        if (a.n_slots > p_topk) {
            float sh = s_e[p_topk][c8];
            if (p_gate_val) sh *= 1.0f / (1.0f + kr_expf(-gval));
            o = o + sh;
        }
        if (lane < 8 && col < a.H) p_out[col] = o;
    }
}

// stage 3: out[b][j] = sum_i w_i * eo_i[j] in routing order (moe.rs:661-667); then rsf*out + shared (moe.rs:703-706)
__global__ void __launch_bounds__(KR_BLOCK) kr_moe_combine_kernel(const KrMoeArgs a) {
    const int b = blockIdx.y;
    const int j = blockIdx.x * KR_BLOCK + threadIdx.x;
    if (j >= a.H) return;
    const float* eo = a.eo + (size_t)b * a.n_slots * a.H;
    float acc = 0.0f;
    for (int s = 0; s < a.topk; s++) {
        { const int id = a.ids[(size_t)b * a.topk + s]; if (id < 0 || id >= a.E) continue; }
        const float w = a.wts[(size_t)b * a.topk + s];
        acc += w * eo[(size_t)s * a.H + j];
    }
    if (a.n_slots > a.topk) acc = a.rsf * acc + eo[(size_t)a.topk * a.H + j];
    if (a.out_bf16) reinterpret_cast<uint16_t*>(a.out)[(size_t)b * a.H + j] = kr_f32_to_bf16(acc);
    else reinterpret_cast<float*>(a.out)[(size_t)b * a.H + j] = acc;
}

// y_i[N_i] = W_i . quant(x[K]) for up to KR_MAX_MULTI matrices that share the same input vector (q|k|v, qkvz|ba, ...):
// one launch, one activation prologue per workgroup, tiles of all matrices in one grid.
template <typename T, int BITS>
__global__ void __launch_bounds__(KR_BLOCK) kr_matvec_kernel(const KrMultiMat mm, const T* x, int tiles_per_wave, int act_mode) {
    const int total = mm.tile_end[mm.n - 1];
    const int tile0 = (blockIdx.x * KR_WAVES) * tiles_per_wave;
    if (tile0 >= total) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int first = tile0 + wave * tiles_per_wave;
    int mi = 0;
    while (mi + 1 < mm.n && first >= mm.tile_end[mi]) mi++;
    const int K = mm.m[0].ng * 128;
    KrHidPre HP; KrVecPre VP;
    if (act_mode == KR_ACT_SILU_MUL) kr_hidden_load(reinterpret_cast<const float*>(x), K, HP); else kr_vec_load(x, K, VP);      // the input first, the weight records behind it (kr_vec_load)
    KrPre pre;
    if (first < total) kr_preload<BITS>(pre, mm.m[mi].q, mm.m[mi].s, mm.m[mi], first - (mi ? mm.tile_end[mi - 1] : 0), lane, 0);
    const KrActLds L = kr_carve_lds(kr_smem, K, BITS == 8);
    if (act_mode == KR_ACT_SILU_MUL) kr_prologue_hidden<KR_ACT_SILU_MUL, BITS == 8>(reinterpret_cast<const float*>(x), K, 0.0f, 0.0f, L, HP);
    else kr_prologue_quant<T, BITS == 8>(x, K, L, VP);
    __syncthreads();
    for (int t = 0; t < tiles_per_wave; t++) {
        const int gt = first + t;
        if (gt >= total) break;
        while (mi + 1 < mm.n && gt >= mm.tile_end[mi]) mi++;
        const KrMatDev& m = mm.m[mi];
        const int tile = gt - (mi ? mm.tile_end[mi - 1] : 0);
        const float acc = kr_matvec_tile<BITS>(pre, t == 0, m.q, m.s, m, tile, L, lane);
        const int col = tile * 8 + (lane >> 3);
        if ((lane & 7) == 0 && col < m.N) mm.y[mi][col] = acc;
    }
}

// Cooperative form of the multi-matrix matvec (used for mid-sized projections fed by a pre-built activation image): the waves of a
// workgroup split the K range of a tile (see "Cooperative tile" above); a workgroup walks `tpb` consecutive tiles.
// x_kind / act_mode: kept in the signature (leading scalars, preloaded); the input of this kernel is always the pre-built INT16 image in global memory (x_kind 2)
// LA = true (exact decode step, linear-attention layers; tpb == 1): the in-projection's EPILOGUE is the layer's conv1d + SiLU + conv-state shift (decode.rs:3815-3890) and
// -- every output row of in_proj_qkvz is one conv channel (or a z value), formed by the one lane that holds the row's sum, with the arithmetic of kr_la_step_kernel
// (the in_proj_ba rows are stored as they are: the recurrence launch forms the gates from them while its state streams in).  The recurrence then runs one workgroup per VALUE head (kr_la_step_kernel<.., false>): twice the CUs pull the
// state.  The lane's conv state / weights / gate parameters are requested with the input image, ahead of the weight records (a wave's memory counter is in-order).
template <typename T, int BITS, bool LA = false>
// (x, K and the modes are leading scalar arguments: the Makefile asks for them to be preloaded into SGPRs, so the input request leaves without a scalar round trip to
//  the argument block -- see kr_decode_fast.hip)
__global__ void __launch_bounds__(KR_BLOCK) kr_matvec_coop_kernel(const T* x, int Kp, int tpb, int act_mode, int x_kind, const KrMultiMat mm, const KrCoLa la) {
    __shared__ KrXch X[2];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int K = Kp;
    // the input is always the pre-built INT16 image (the launchers pass x_kind = 2): the vector forms of the per-wave kernel above are not instantiated here -- as
    // run-time branches they cost this kernel 25 registers (78 -> 54: six -> eight workgroups per CU)
    (void)act_mode; (void)x_kind;
    KrImgPre IP;
    kr_image_load(x, K, IP);      // the input first, the weight records behind it (kr_vec_load)
    const int total = mm.tile_end[mm.n - 1], gt0 = blockIdx.x * tpb;      // (the launcher's grid has no workgroup past the last tile)
    int mi = 0;
    while (mi + 1 < mm.n && gt0 >= mm.tile_end[mi]) mi++;
    KrCo<BITS> cur;
    kr_co_preload<BITS>(cur, mm.m[mi].q, mm.m[mi].s, mm.m[mi], gt0 - (mi ? mm.tile_end[mi - 1] : 0), lane, wave);
    // LA: what the epilogue lane of this workgroup's tile (wave 0, lanes 0 .. 7) will do with its row -- worked out (two integer divisions) BEHIND the request for the
    // tile's weight records: wave 0 also carries a quarter of the tile's sums
    int la_kind = -1, la_dst = 0;      // 0 q / k channel -> qk_out, 1 v channel -> v_out, 2 z -> z_out; -1: plain store (the in_proj_ba rows: the recurrence launch forms the gates)
    float4 la_cs = {0.0f, 0.0f, 0.0f, 0.0f}, la_cw = la_cs; int la_ch = 0;
    __shared__ int la_park[3][8];      // the three indices wait in LDS while the sums run (three more live registers cost the kernel a workgroup per CU)
    if (LA && wave == 0) {
        const int col = (gt0 - (mi ? mm.tile_end[mi - 1] : 0)) * 8 + (lane & 7);
        if (mi == la.conv_mi && col < mm.m[mi].N) {
            const int nt = la.hr * la.dv, group_dim = 2 * la.dk + 2 * nt, key_dim = la.nk * la.dk;
            const int kh = col / group_dim, cc = col - kh * group_dim;
            if (cc < la.dk) { la_kind = 0; la_ch = kh * la.dk + cc; la_dst = kh * 2 * la.dk + cc; }
            else if (cc < 2 * la.dk) { la_kind = 0; la_ch = key_dim + kh * la.dk + (cc - la.dk); la_dst = kh * 2 * la.dk + cc; }
            else if (cc < 2 * la.dk + nt) { la_kind = 1; la_ch = 2 * key_dim + kh * nt + (cc - 2 * la.dk); la_dst = kh * nt + (cc - 2 * la.dk); }
            else { la_kind = 2; la_dst = kh * nt + (cc - 2 * la.dk - nt); }
        }
        if (lane < 8) { la_park[0][lane] = la_kind; la_park[1][lane] = la_dst; la_park[2][lane] = la_ch; }
    }
    const KrActLds L = kr_carve_lds(kr_smem, K, BITS == 8);
    kr_image_copy<BITS>(x, K, kr_smem, L, IP);
    __syncthreads();
    for (int t = 0; t < (LA ? 1 : tpb); t++) {      // LA: one tile per workgroup (the launcher), nothing of a next tile stays live across the epilogue
        const int gt = gt0 + t;
        if (gt >= total) break;
        const KrMatDev& m = mm.m[mi];
        const int tile = gt - (mi ? mm.tile_end[mi - 1] : 0);
        int mn = mi;
        KrCo<BITS> nxt;
        const bool more = !LA && t + 1 < tpb && gt + 1 < total;
        if (more) {   // the next tile's weights are requested before this tile's sums are formed
            while (mn + 1 < mm.n && gt + 1 >= mm.tile_end[mn]) mn++;
            kr_co_preload<BITS>(nxt, mm.m[mn].q, mm.m[mn].s, mm.m[mn], gt + 1 - (mn ? mm.tile_end[mn - 1] : 0), lane, wave);
        }
        KrXch& Xc = X[t & 1];
        kr_co_sums<BITS>(cur, m.q, m.s, m, tile, L, Xc, lane);
        if (LA && wave == 0) {      // the epilogue's operands, requested once the weight registers are free (held across the sums they cost the kernel two workgroups per CU)
            la_kind = la_park[0][lane & 7]; la_dst = la_park[1][lane & 7]; la_ch = la_park[2][lane & 7];      // written by this wave: no barrier needed
            la_cs = reinterpret_cast<const float4*>(la.conv_state)[la_ch]; la_cw = reinterpret_cast<const float4*>(la.conv_w)[la_ch];      // clamped to channel 0 when unused: never masked
        }
        __syncthreads();      // one barrier per tile: the exchange buffer alternates, so the chain of tile t overlaps the sums of tile t + 1
        if (wave == (t & (KR_WAVES - 1)) && lane < 8) {
            const int col = tile * 8 + lane;
            const float acc = kr_co_chain(Xc, m.ng, lane, col < m.n_fma);
            if (LA && la_kind >= 0) {      // (tpb == 1: t == 0, this is wave 0 and `col` the row the operands above were requested for)
                if (la_kind <= 1) {        // depthwise conv1d (kernel 4) over the shifted state, SiLU (fast_silu_avx2); the state shift is this lane's alone
                    reinterpret_cast<float4*>(la.conv_state)[la_ch] = float4{la_cs.y, la_cs.z, la_cs.w, acc};
                    const float co = kr_conv4_silu(la_cs.y, la_cs.z, la_cs.w, acc, la_cw);
                    if (la_kind == 0) la.qk_out[la_dst] = co; else la.v_out[la_dst] = co;
                } else la.z_out[la_dst] = acc;
            } else if (col < m.N) mm.y[mi][col] = acc;
        }
        if (more) { cur = nxt; mi = mn; }
    }
}

// ------------------------------------------------------------------------------------------
// host launchers
// ------------------------------------------------------------------------------------------

static int kr_pick_tpw(int K, int ntiles) {
    // keep >= ~1 KiB/lane-instruction streams but give short-K matrices more columns per wave
    int tpw = K >= 2048 ? 1 : (K >= 1024 ? 2 : 4);
    while (tpw > 1 && (ntiles + KR_WAVES * tpw - 1) / (KR_WAVES * tpw) < 32) tpw >>= 1;
    return tpw;
}

void kr_launch_moe_w13(const KrMoeArgs& a, hipStream_t st) {
    const bool has_shared = a.n_slots > a.topk;
    int nt = (a.w13.N + 7) / 8;
    if (has_shared && (a.sw13.N + 7) / 8 + (a.sgate.q ? 1 : 0) > nt) nt = (a.sw13.N + 7) / 8 + (a.sgate.q ? 1 : 0);
    const int tpw = kr_pick_tpw(a.H, nt);
    dim3 grid((nt + KR_WAVES * tpw - 1) / (KR_WAVES * tpw), a.n_slots, a.B);
    const size_t lds = kr_lds_bytes(a.H, a.w13.bits == 8);
    if (a.w13.bits == 4) hipLaunchKernelGGL(kr_moe_w13_kernel<4>, grid, dim3(KR_BLOCK), lds, st, a.act_img_bf16, a.act_img, a.H, a.topk, a.shared_decode, a.B, a, tpw);
    else hipLaunchKernelGGL(kr_moe_w13_kernel<8>, grid, dim3(KR_BLOCK), lds, st, a.act_img_bf16, a.act_img, a.H, a.topk, a.shared_decode, a.B, a, tpw);
}

void kr_launch_moe_w2(const KrMoeArgs& a, hipStream_t st) {
    const bool has_shared = a.n_slots > a.topk;
    const int nt = (a.H + 7) / 8;
    const int imax = has_shared && a.I_shared > a.I ? a.I_shared : a.I;
    const int tpw = kr_pick_tpw(a.I, nt);
    dim3 grid((nt + KR_WAVES * tpw - 1) / (KR_WAVES * tpw), a.n_slots, a.B);
    const size_t lds = kr_lds_bytes(imax, a.w2.bits == 8);
#define KR_W2(B_, A_) hipLaunchKernelGGL((kr_moe_w2_kernel<B_, A_>), grid, dim3(KR_BLOCK), lds, st, a.gu, a.n_slots, a.gu_ld, a.I, a.I_shared, a.topk, a, tpw)
    if (a.w2.bits == 4) {
        if (a.act_mode == KR_ACT_SILU_FUSED) KR_W2(4, KR_ACT_SILU_FUSED);
        else if (a.act_mode == KR_ACT_GPTOSS) KR_W2(4, KR_ACT_GPTOSS);
        else KR_W2(4, KR_ACT_SILU_MUL);
    } else {
        if (a.act_mode == KR_ACT_SILU_FUSED) KR_W2(8, KR_ACT_SILU_FUSED);
        else if (a.act_mode == KR_ACT_GPTOSS) KR_W2(8, KR_ACT_GPTOSS);
        else KR_W2(8, KR_ACT_SILU_MUL);
    }
#undef KR_W2
}

// stages 2 + 3 of the decode step in one launch (kr_moe_w2c_kernel); non-zero = geometry not covered (the caller keeps kr_launch_moe_w2 + the combine inside the next norm launch)
int kr_launch_moe_w2c(const KrMoeArgs& a, const float* gate_val, float* out, hipStream_t st) {
    const bool has_shared = a.n_slots > a.topk;
    if (a.B != 1 || a.n_slots < 1 || a.n_slots > 16 || a.topk < 1 || a.H % 8 || a.I % 128 || (has_shared && (a.I_shared % 128 || a.sw2.bits != a.w2.bits)) || a.e_hi > 0) return 1;
    // the GPT-OSS activation of this kernel is a hand copy of kr_prologue_hidden's branch that no bit-exact decode test reaches (the oracle's decode driver has no
    // GPT-OSS model): such layers keep the per-slot launch + the combine inside the next norm launch, which the kr_moe_forward tests cover
    if (a.act_mode == KR_ACT_GPTOSS) return 1;
    const int imax = has_shared && a.I_shared > a.I ? a.I_shared : a.I;
    const size_t img = (kr_lds_bytes(imax, a.w2.bits == 8) + 15) / 16 * 16, lds = img * a.n_slots;
    if (lds > 60 * 1024) return 1;
    dim3 grid(a.H / 8), block(64 * a.n_slots);
#define KR_W2C(B_, A_) hipLaunchKernelGGL((kr_moe_w2c_kernel<B_, A_>), grid, block, lds, st, a.gu, a.ids, a.wts, gate_val, a.gu_ld, a.I, a.I_shared, a.topk, (int)(img / 16), out, a)
    if (a.w2.bits == 4) {
        if (a.act_mode == KR_ACT_SILU_FUSED) KR_W2C(4, KR_ACT_SILU_FUSED);
        else KR_W2C(4, KR_ACT_SILU_MUL);
    } else {
        if (a.act_mode == KR_ACT_SILU_FUSED) KR_W2C(8, KR_ACT_SILU_FUSED);
        else KR_W2C(8, KR_ACT_SILU_MUL);
    }
#undef KR_W2C
    return 0;
}

void kr_launch_moe_combine(const KrMoeArgs& a, hipStream_t st) {
    dim3 grid((a.H + KR_BLOCK - 1) / KR_BLOCK, a.B);
    hipLaunchKernelGGL(kr_moe_combine_kernel, grid, dim3(KR_BLOCK), 0, st, a);
}

void kr_launch_moe_decode(const KrMoeArgs& a, hipStream_t st) {
    kr_launch_moe_w13(a, st);
    kr_launch_moe_w2(a, st);
    kr_launch_moe_combine(a, st);
}

// exact decode step, linear-attention layers: in_proj_qkvz | in_proj_ba from the INT16 image with the conv / gate epilogue (kr_matvec_coop_kernel<.., LA = true>);
// non-zero = geometry not covered (the caller keeps kr_launch_multi_matvec + the one-launch kr_la_step)
int kr_launch_multi_matvec_la(const KrMatDev* mats, float* const* ys, int n, const void* x_img, const KrCoLa& la, hipStream_t st) {
    KrMultiMat mm{};
    mm.n = n;
    int total = 0;
    for (int i = 0; i < n; i++) { mm.m[i] = mats[i]; mm.y[i] = ys[i]; total += (mats[i].N + 7) / 8; mm.tile_end[i] = total; if (mats[i].bits != mats[0].bits || mats[i].ng != mats[0].ng) return 1; }
    if (n > KR_MAX_MULTI || total > 3072 || la.conv_mi < 0 || la.conv_mi >= n) return 1;      // one tile per workgroup
    if (mats[la.conv_mi].N != la.nk * (2 * la.dk + 2 * la.hr * la.dv)) return 1;
    const int bits = mats[0].bits;
    const size_t lds = kr_lds_bytes(mats[0].ng * 128, bits == 8);
    if (bits == 4) hipLaunchKernelGGL((kr_matvec_coop_kernel<float, 4, true>), dim3(total), dim3(KR_BLOCK), lds, st, (const float*)x_img, mats[0].ng * 128, 1, -1, 2, mm, la);
    else hipLaunchKernelGGL((kr_matvec_coop_kernel<float, 8, true>), dim3(total), dim3(KR_BLOCK), lds, st, (const float*)x_img, mats[0].ng * 128, 1, -1, 2, mm, la);
    return 0;
}

void kr_launch_multi_matvec(const KrMatDev* mats, float* const* ys, int n, const void* x, int x_is_f32, hipStream_t st, int act_mode) {
    // x_is_f32: 0 bf16 vector, 1 f32 vector, 2 pre-built INT16 image (kr_act_image_bytes(K) bytes) -> cooperative kernel
    KrMultiMat mm{};
    mm.n = n;
    int total = 0;
    for (int i = 0; i < n; i++) { mm.m[i] = mats[i]; mm.y[i] = ys[i]; total += (mats[i].N + 7) / 8; mm.tile_end[i] = total; }
    const int bits = mats[0].bits;
    const size_t lds = kr_lds_bytes(mats[0].ng * 128, bits == 8);
    if (x_is_f32 == 2) {
        int tpb = 1;
        while ((total + tpb - 1) / tpb > 3072) tpb *= 2;
        if (bits == 4) hipLaunchKernelGGL((kr_matvec_coop_kernel<float, 4>), dim3((total + tpb - 1) / tpb), dim3(KR_BLOCK), lds, st, (const float*)x, mats[0].ng * 128, tpb, act_mode, 2, mm, KrCoLa{});
        else hipLaunchKernelGGL((kr_matvec_coop_kernel<float, 8>), dim3((total + tpb - 1) / tpb), dim3(KR_BLOCK), lds, st, (const float*)x, mats[0].ng * 128, tpb, act_mode, 2, mm, KrCoLa{});
        return;
    }
    const int tpw = kr_pick_tpw(mats[0].K, total);
    dim3 grid((total + KR_WAVES * tpw - 1) / (KR_WAVES * tpw));
    if (x_is_f32) {
        if (bits == 4) hipLaunchKernelGGL((kr_matvec_kernel<float, 4>), grid, dim3(KR_BLOCK), lds, st, mm, (const float*)x, tpw, act_mode);
        else hipLaunchKernelGGL((kr_matvec_kernel<float, 8>), grid, dim3(KR_BLOCK), lds, st, mm, (const float*)x, tpw, act_mode);
    } else {
        if (bits == 4) hipLaunchKernelGGL((kr_matvec_kernel<uint16_t, 4>), grid, dim3(KR_BLOCK), lds, st, mm, (const uint16_t*)x, tpw, act_mode);
        else hipLaunchKernelGGL((kr_matvec_kernel<uint16_t, 8>), grid, dim3(KR_BLOCK), lds, st, mm, (const uint16_t*)x, tpw, act_mode);
    }
}

void kr_launch_matvec(const KrMatDev& m, const void* x, int x_is_f32, float* y, hipStream_t st, int act_mode) {
    kr_launch_multi_matvec(&m, &y, 1, x, x_is_f32, st, act_mode);
}

// ------------------------------------------------------------------------------------------
// synthetic fill + bf16 reduce
// ------------------------------------------------------------------------------------------

__device__ __forceinline__ uint64_t kr_splitmix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__global__ void kr_fill_words_kernel(uint32_t* q, size_t n_words, uint64_t seed) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += (size_t)gridDim.x * blockDim.x)
        q[i] = (uint32_t)kr_splitmix(seed + i);
}
// bf16 scales 0.005 + u*0.045, truncated to bf16 (decode.rs:4386-4392), two per word
__global__ void kr_fill_scales_kernel(uint32_t* s, size_t n_words, uint64_t seed) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += (size_t)gridDim.x * blockDim.x) {
        const uint64_t r = kr_splitmix(seed ^ 0xABCDEF12345ull ^ (i << 1));
        const float f0 = 0.005f + ((float)(uint32_t)r / 4294967295.0f) * 0.045f;
        const float f1 = 0.005f + ((float)(uint32_t)(r >> 32) / 4294967295.0f) * 0.045f;
        s[i] = (__float_as_uint(f0) >> 16) | (__float_as_uint(f1) & 0xFFFF0000u);
    }
}

void kr_launch_fill_synth(void* q, size_t q_bytes, uint32_t* s, size_t s_words, uint64_t seed, hipStream_t st) {
    hipLaunchKernelGGL(kr_fill_words_kernel, dim3(2048), dim3(256), 0, st, (uint32_t*)q, q_bytes / 4, seed);
    hipLaunchKernelGGL(kr_fill_scales_kernel, dim3(512), dim3(256), 0, st, s, s_words, seed);
}

// uniform f32 in [-amp, amp] and random FP16 KV patterns (decode.rs:4371-4375, 4402-4411), counter-hash based
__global__ void kr_fill_uniform_f32_kernel(float* x, size_t n, float amp, uint64_t seed) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int64_t b = (int64_t)kr_splitmix(seed * 0x100000001B3ull + i);
        x[i] = (float)((double)b / 9223372036854775807.0) * amp;
    }
}
__global__ void kr_fill_fp16_kv_kernel(uint16_t* x, size_t n, uint64_t seed) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const uint64_t bits = kr_splitmix(seed * 0x100000001B3ull + i);
        const uint16_t sign = (uint16_t)((bits >> 15) & 1), ex = (uint16_t)(((bits >> 5) & 0xF) + 8), mant = (uint16_t)(bits & 0x3FF);
        x[i] = (uint16_t)((sign << 15) | (ex << 10) | mant);
    }
}
// E4M3 twin of the FP16 pattern (decode.rs:4402-4411 draws sign / exponent in [8,23] / mantissa for FP16 = magnitudes 2^-7 .. 2^8): sign,
// exponent field in [3,10] (2^-4 .. 2^3 with bias 7), 3 mantissa bits -- finite by construction (the only NaN code has exponent 15)
__global__ void kr_fill_e4m3_kv_kernel(uint8_t* x, size_t n, uint64_t seed) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const uint64_t bits = kr_splitmix(seed * 0x100000001B3ull + i);
        const uint8_t sign = (uint8_t)((bits >> 15) & 1), ex = (uint8_t)(((bits >> 5) & 0x7) + 3), mant = (uint8_t)(bits & 0x7);
        x[i] = (uint8_t)((sign << 7) | (ex << 3) | mant);
    }
}
void kr_launch_fill_e4m3_kv(uint8_t* x, size_t n, uint64_t seed, hipStream_t st) {
    hipLaunchKernelGGL(kr_fill_e4m3_kv_kernel, dim3(1024), dim3(256), 0, st, x, n, seed);
}
void kr_launch_fill_uniform_f32(float* x, size_t n, float amp, uint64_t seed, hipStream_t st) {
    hipLaunchKernelGGL(kr_fill_uniform_f32_kernel, dim3(2048), dim3(256), 0, st, x, n, amp, seed);
}
void kr_launch_fill_fp16_kv(uint16_t* x, size_t n, uint64_t seed, hipStream_t st) {
    hipLaunchKernelGGL(kr_fill_fp16_kv_kernel, dim3(1024), dim3(256), 0, st, x, n, seed);
}

// reduce_sum_bf16 (moe.rs:2505): f32 accumulate in input order, RNE to bf16
__global__ void kr_reduce_sum_bf16_kernel(const uint16_t* const* in, int n_in, uint16_t* out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        if (n_in == 1) { out[i] = in[0][i]; continue; }
        float s = 0.0f;
        for (int p = 0; p < n_in; p++) s = s + kr_bf16_to_f32(in[p][i]);
        out[i] = kr_f32_to_bf16(s);
    }
}
void kr_launch_reduce_sum_bf16(const uint16_t* const* tbl, int n_in, uint16_t* out, size_t n, hipStream_t st) {
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(kr_reduce_sum_bf16_kernel, dim3(blocks ? blocks : 1), dim3(256), 0, st, tbl, n_in, out, n);
}
