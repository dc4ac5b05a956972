// kr_multi_mla_split.hip -- "multi_mla_exact_split" (docs/design/31-multi-mla-exact-split.md): the attention of kr_multi_mla_attn_kernel (kr_multi.hip) as three
// launches behind the unchanged absorption and prep launch and ahead of the unchanged w_vc projection, bit for bit that kernel's result for every row.  MLA is
// GQA with one KV head shared by all nh heads: K row = [latent klr | rope rd], V row = the latent klr.
//   1  scores        grid (position tile, group of KR_MLS_HG heads, row): a score depends on its own (position, head) alone, so any split over positions and heads
//                    keeps it -- the 16-lane chains of that kernel, kr_mla_pair_hsum over klr, the same over rd, their sum, * sm_scale.  The rows come through LDS
//                    in 16-byte loads
//   2  softmax       one wave per (row, head): kr_m_wave_softmax as it stands
//   3  weighted sum  grid (latent slice, row): output (h, j) is one fma per position, ascending, from 0.0f; the split is over j and heads, never over positions.
//                    The latent rows come through LDS in 16-byte loads
// They read and write the score scratch a.scores[row][nh][sc_ld] exactly as that kernel does.  E4M3 -> f32 and f16 -> f32 are exact, so where a cache element is
// widened (on the way out of LDS, or into it) changes nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kr_device.h"
#include "kr_libm.h"
#include "kr_exact_dev.h"
#include "kr_multi.h"
#include "kr_multi_softmax_dev.h"
#include "kr_mla_dev.h"

#define KR_MLS_HG 4         // heads per scores workgroup (= KR_MM_HG of kr_multi_mla_attn_kernel: the same head groups)
#define KR_MLS_ROWS 32      // latent + rope rows per LDS stage of the scores kernel; never straddles a page (KR_PAGE_MIN_TOKENS)
#define KR_MLS_TILE 64      // positions per scores workgroup: position 4096 of 16 heads gives 65 x 4 workgroups, one per CU and more
#define KR_MLS_PT 64        // positions per stage of the weighted sum
#define KR_MLS_DS 32        // latent elements j per workgroup of the weighted sum
#define KR_MLS_VLD 68       // floats per staged latent column: KR_MLS_PT positions and four of padding (16-byte aligned columns, 16 lanes of a 16-byte read on 64 banks)
#define KR_MLS_TPD 8        // threads per output column of the weighted sum (256 / KR_MLS_DS)
#define KR_MLS_ACC 4        // heads per thread and pass of the weighted sum (32 heads a pass)
#define KR_MLS_HP (KR_MLS_ACC * KR_MLS_TPD)      // heads per pass
#define KR_MLS_NPR (KR_MLS_HP * KR_MLS_PT / 256) // probabilities of a stage per thread
static_assert(KR_PAGE_MIN_TOKENS % KR_MLS_ROWS == 0 && KR_MLS_TILE % KR_MLS_ROWS == 0, "a stage of the scores kernel lies in one page and in one tile");

// base of position s of the row's slot in a cache whose slot (PAGED: page) is `stride` bytes and whose rows are RB bytes.  PAGED: through the slot's table slice, one
// entry per call -- a workgroup reads only the entries of the positions it loads (every page of [0, seq) was mapped by the host before the pass: max(., 0) as in the
// unsplit kernel)
template <int RB, bool PAGED>
__device__ __forceinline__ const unsigned char* kr_mls_row(const KrMultiMlaArgs& a, const void* cache, size_t stride, int slot, int s) {
    if constexpr (PAGED) {
        const int pg = max(a.page_table[(size_t)slot * a.page_stride + (s >> a.page_shift)], 0);
        return reinterpret_cast<const unsigned char*>(cache) + (size_t)pg * stride + (size_t)(s & ((1 << a.page_shift) - 1)) * RB;
    } else return reinterpret_cast<const unsigned char*>(cache) + (size_t)slot * stride + (size_t)s * RB;
}
// element j of a 16-byte chunk held in registers (j a constant after unrolling: shifts, no addressing)
template <bool FP8> __device__ __forceinline__ float kr_mls_chunk_elem(const u32x4& r, int j) {
    if (FP8) return kr_e4m3_to_f32((uint8_t)(r[j >> 2] >> (8 * (j & 3))));
    return (float)__builtin_bit_cast(_Float16, (uint16_t)(r[j >> 1] >> (16 * (j & 1))));
}

// ---- 1: scores.  grid (ceil(sc_ld / KR_MLS_TILE), ceil(nh / KR_MLS_HG), rows), 512 threads; static LDS = the group's absorbed and rope query rows f32, lane by
// lane, + one stage of KR_MLS_ROWS raw [latent | rope] rows.  A stage is fetched by all 512 threads, 16 bytes each (NLD loads per thread), the next stage's loads
// issued before the current one is consumed.  16 lanes own one staged position: they widen their elements of the row once, into registers, and run the chains of
// every head of the group against them, the query elements read four at a time from LDS -- one staged row serves every head of the group.  Bounds: a row s is
// loaded only for s < min(seq, tile end), seq = pos + 1 <= the slot's capacity; the 16-byte chunks c < CPR_C tile the klr * esz bytes of the latent row exactly and
// c - CPR_C < CPR_R the rd * esz bytes of the rope row; scores are written for those s only, s < seq <= sc_ld.  Workgroups past the row's position, and the rows
// of the run kernels, leave ahead of every barrier
template <bool FP8, int NBC, bool PAGED>
__global__ void __launch_bounds__(512) kr_multi_mla_split_scores_kernel(const KrMultiMlaArgs a) {
    constexpr int klr = NBC * 8, NBR = 8, rd = NBR * 8, esz = FP8 ? 1 : 2, HG = KR_MLS_HG, ROWS = KR_MLS_ROWS;
    constexpr int CPR_C = klr * esz / 16, CPR_R = rd * esz / 16, CPR = CPR_C + CPR_R, pitch = (klr + rd) * esz + 16, NLD = (ROWS * CPR + 511) / 512;
    // lane c16 = (accumulator a2, AVX lane l) of kr_multi_mla_attn_kernel owns the 8-blocks i % 2 == a2, ascending: NQC of the latent row, NQR of the rope row.  Its
    // query elements stand side by side, [head][c16][QLD]: 16-byte reads, and QLD = 36 / 20 floats puts the 16 lanes' reads on distinct banks
    constexpr int NQC = NBC / 2, NQR = NBR / 2, QLD = NQC + NQR;
    static_assert(ROWS * 16 == 512 && NQC % 4 == 0 && NQR == 4 && QLD % 4 == 0, "work split: 16 lanes per staged row, query elements in groups of four");
    static_assert((size_t)HG * 16 * QLD * 4 + (size_t)ROWS * pitch <= 64 * 1024, "the scores kernel stays inside the default 64 KiB LDS window");
    __shared__ __attribute__((aligned(16))) float qs[HG * 16 * QLD];              // [HG][16][QLD]
    __shared__ __attribute__((aligned(16))) unsigned char stage[ROWS * pitch];    // [ROWS][pitch]
    const int row = blockIdx.z, hg0 = blockIdx.y * HG, nhg = min(HG, a.nh - hg0), t = threadIdx.x;
    if (kr_m_row_in_run(a, row)) return;      // the run kernels' row (workgroup-uniform, ahead of every barrier)
    const int seq = a.positions[row] + 1, t0 = blockIdx.x * KR_MLS_TILE;
    if (t0 >= seq) return;                    // (workgroup-uniform, ahead of every barrier)
    const int tend = min(seq, t0 + KR_MLS_TILE), slot = a.slots[row];
    u32x4 rg[NLD];
    auto issue = [&](int s0) {
#pragma unroll
        for (int i = 0; i < NLD; i++) {
            const int u = t + 512 * i, r = u / CPR, c = u % CPR;
            if (u < ROWS * CPR && s0 + r < tend) {
                const unsigned char* src = c < CPR_C ? kr_mls_row<klr * esz, PAGED>(a, a.ckv_cache, a.ckv_stride, slot, s0 + r) + c * 16
                                                     : kr_mls_row<rd * esz, PAGED>(a, a.kpe_cache, a.kpe_stride, slot, s0 + r) + (c - CPR_C) * 16;
                rg[i] = *reinterpret_cast<const u32x4*>(src);
            }
        }
    };
    auto commit = [&](int s0) {      // chunk c of a row lands at byte c * 16 of its staged row: the rope row stands behind the latent row's klr * esz bytes
#pragma unroll
        for (int i = 0; i < NLD; i++) {
            const int u = t + 512 * i, r = u / CPR, c = u % CPR;
            if (u < ROWS * CPR && s0 + r < tend) *reinterpret_cast<u32x4*>(stage + r * pitch + c * 16) = rg[i];
        }
    };
    issue(t0);
    // element e of a head's latent (rope) query row is 8-block e >> 3, AVX lane e & 7: lane ((e >> 3) & 1, e & 7), its element e >> 4 (NQC + (e >> 4)); index < HG * 16 * QLD
    for (int i = t; i < nhg * klr; i += 512) { const int h = i / klr, e = i % klr; qs[(h * 16 + ((e >> 3) & 1) * 8 + (e & 7)) * QLD + (e >> 4)] = a.q_abs[((size_t)row * a.nh + hg0) * klr + i]; }
    for (int i = t; i < nhg * rd; i += 512) { const int h = i / rd, e = i % rd; qs[(h * 16 + ((e >> 3) & 1) * 8 + (e & 7)) * QLD + NQC + (e >> 4)] = a.q_pe[((size_t)row * a.nh + hg0) * rd + i]; }
    const int c16 = t & 15, a2 = c16 >> 3, l = c16 & 7, r = t >> 4;      // this lane's role, and its 16 lanes' row of a stage
    float* out = a.scores + ((size_t)row * a.nh + hg0) * a.sc_ld;        // [nhg][sc_ld]
    for (int s0 = t0; s0 < tend; s0 += ROWS) {
        if (s0 != t0) __syncthreads();          // the stage before this one is consumed
        commit(s0);
        if (s0 + ROWS < tend) issue(s0 + ROWS);
        __syncthreads();                        // (first stage: also the query rows)
        if (s0 + r >= tend) continue;           // uniform over the 16 lanes of a position (and no barrier depends on it); a position at or past seq is skipped, never multiplied
        const unsigned char* srow = stage + r * pitch;
        float kc[NQC], kr[NQR];
#pragma unroll
        for (int u = 0; u < NQC; u++) kc[u] = kr_stage_val<FP8>(srow, (2 * u + a2) * 8 + l);
#pragma unroll
        for (int u = 0; u < NQR; u++) kr[u] = kr_stage_val<FP8>(srow + klr * esz, (2 * u + a2) * 8 + l);
#pragma unroll 1
        for (int h = 0; h < nhg; h++) {
            const float* qh = qs + (h * 16 + c16) * QLD;
            float acc = 0.0f;
#pragma unroll
            for (int u = 0; u < NQC; u += 4) {
                const float4 q4 = *reinterpret_cast<const float4*>(qh + u);
                acc = __builtin_fmaf(q4.x, kc[u], acc); acc = __builtin_fmaf(q4.y, kc[u + 1], acc);
                acc = __builtin_fmaf(q4.z, kc[u + 2], acc); acc = __builtin_fmaf(q4.w, kc[u + 3], acc);
            }
            float v = kr_mla_pair_hsum(acc, a2);
            acc = 0.0f;
            {
                const float4 q4 = *reinterpret_cast<const float4*>(qh + NQC);
                acc = __builtin_fmaf(q4.x, kr[0], acc); acc = __builtin_fmaf(q4.y, kr[1], acc);
                acc = __builtin_fmaf(q4.z, kr[2], acc); acc = __builtin_fmaf(q4.w, kr[3], acc);
            }
            v += kr_mla_pair_hsum(acc, a2);
            v *= a.sm_scale;
            if (c16 == 0) out[(size_t)h * a.sc_ld + s0 + r] = v;
        }
    }
}

// ---- 2: softmax.  grid (ceil(nh / 4), rows), 256 threads: wave w takes head 4 x + w of the row.  kr_m_wave_softmax holds workgroup barriers, as many as seq has
// tiles: the four waves of a workgroup belong to one row, so they share seq and pass the same barriers; a wave past the last head calls it with on = false on the
// row of head 0 (a valid pointer it never dereferences).  The run kernels' rows leave ahead of the call, the whole workgroup at once
__global__ void __launch_bounds__(256) kr_multi_mla_split_softmax_kernel(const KrMultiMlaArgs a) {
    __shared__ __attribute__((aligned(16))) float tile[4 * KR_MG_TILE];
    const int row = blockIdx.y, t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (kr_m_row_in_run(a, row)) return;
    const int seq = a.positions[row] + 1, h = blockIdx.x * 4 + w;
    const bool on = h < a.nh;
    kr_m_wave_softmax(a.scores + ((size_t)row * a.nh + (size_t)(on ? h : 0)) * a.sc_ld, seq, tile + w * KR_MG_TILE, on, lane);
}

// ---- 3: weighted sum.  grid (klr / KR_MLS_DS, rows), 256 threads: thread t owns latent element j0 + t % 32 of heads t / 32 + 8 k of a pass of 32 heads (more heads:
// further passes over the slot); one fma per position, ascending, from 0.0f; positions past the row's are skipped, not multiplied by zero -- the unsplit kernel's
// statements.  Static LDS: the stage's latent slice widened to f32 and transposed, [KR_MLS_DS][KR_MLS_VLD], and the pass's probabilities of the stage,
// [KR_MLS_HP][KR_MLS_PT] -- a thread reads four positions of its column, and four probabilities of a head, per 16-byte LDS read.  A stage is fetched 16 bytes per
// thread (at most one load each) and its probabilities KR_MLS_NPR per thread, the next stage's loads issued before the current one is consumed.  Bounds: a latent row
// s is loaded only for s < seq; the chunks c < CPS tile the 32 j of this slice exactly; probabilities are read for s < seq <= sc_ld and heads < nh only
// one stage of the chains of K heads (p0: the first one's probabilities, the others KR_MLS_TPD rows further each) over column vrow: n positions, ascending
template <int K>
__device__ __forceinline__ void kr_mls_pv_stage(float (&o)[KR_MLS_ACC], const float* p0, const float* vrow, int n) {
    int s1 = 0;
    for (; s1 + 8 <= n; s1 += 8) {
        const float4 va = *reinterpret_cast<const float4*>(vrow + s1), vb = *reinterpret_cast<const float4*>(vrow + s1 + 4);
#pragma unroll
        for (int k = 0; k < K; k++) {
            const float4 pa = *reinterpret_cast<const float4*>(p0 + k * KR_MLS_TPD * KR_MLS_PT + s1), pb = *reinterpret_cast<const float4*>(p0 + k * KR_MLS_TPD * KR_MLS_PT + s1 + 4);
            float x = o[k];
            x = __builtin_fmaf(pa.x, va.x, x); x = __builtin_fmaf(pa.y, va.y, x); x = __builtin_fmaf(pa.z, va.z, x); x = __builtin_fmaf(pa.w, va.w, x);
            x = __builtin_fmaf(pb.x, vb.x, x); x = __builtin_fmaf(pb.y, vb.y, x); x = __builtin_fmaf(pb.z, vb.z, x); x = __builtin_fmaf(pb.w, vb.w, x);
            o[k] = x;
        }
    }
    for (; s1 < n; s1++) {      // the last, partial group of the row (once per pass)
        const float v = vrow[s1];
#pragma unroll
        for (int k = 0; k < K; k++) o[k] = __builtin_fmaf(p0[k * KR_MLS_TPD * KR_MLS_PT + s1], v, o[k]);
    }
}
template <bool FP8, int NBC, bool PAGED>
__global__ void __launch_bounds__(256) kr_multi_mla_split_pv_kernel(const KrMultiMlaArgs a) {
    constexpr int klr = NBC * 8, esz = FP8 ? 1 : 2, CPS = KR_MLS_DS * esz / 16, EPC = 16 / esz;      // chunks per row slice, elements per chunk
    static_assert(klr % KR_MLS_DS == 0 && KR_MLS_PT * CPS <= 256 && KR_MLS_NPR * 256 == KR_MLS_HP * KR_MLS_PT, "work split");
    static_assert(sizeof(float) * (KR_MLS_DS * KR_MLS_VLD + KR_MLS_HP * KR_MLS_PT) <= 64 * 1024, "the weighted sum stays inside the default 64 KiB LDS window");
    __shared__ __attribute__((aligned(16))) float vs[KR_MLS_DS * KR_MLS_VLD];     // [j][position]
    __shared__ __attribute__((aligned(16))) float pt[KR_MLS_HP * KR_MLS_PT];      // [head of the pass][position]
    const int j0 = blockIdx.x * KR_MLS_DS, row = blockIdx.y, t = threadIdx.x;
    if (kr_m_row_in_run(a, row)) return;      // the run kernels' row (workgroup-uniform, ahead of every barrier)
    const int seq = a.positions[row] + 1, nh = a.nh, slot = a.slots[row];
    const float* sc = a.scores + (size_t)row * nh * a.sc_ld;      // [nh][sc_ld]
    const int lr = t / CPS, lc = t % CPS;      // this thread's row and chunk of a stage
    const bool loader = t < KR_MLS_PT * CPS;
    const int ps = t % KR_MLS_PT, pg = t / KR_MLS_PT;      // this thread's probabilities of a stage: position ps of the pass's heads pg + 4 k
    const int dl = t % KR_MLS_DS, hg = t / KR_MLS_DS;      // heads are dealt round-robin over the KR_MLS_TPD threads of an output column
    const float* vrow = vs + dl * KR_MLS_VLD;
    const float* p0 = pt + hg * KR_MLS_PT;
    for (int gp = 0; gp < nh; gp += KR_MLS_HP) {      // heads gp + hg + k * KR_MLS_TPD, k < KR_MLS_ACC
        const int ka = min(KR_MLS_ACC, max(0, (nh - gp - hg + KR_MLS_TPD - 1) / KR_MLS_TPD));      // this thread's heads in this pass
        u32x4 rg = {0, 0, 0, 0};
        float pr[KR_MLS_NPR];
#pragma unroll
        for (int k = 0; k < KR_MLS_NPR; k++) pr[k] = 0.0f;
        auto issue = [&](int s0) {
            if (loader && s0 + lr < seq) rg = *reinterpret_cast<const u32x4*>(kr_mls_row<klr * esz, PAGED>(a, a.ckv_cache, a.ckv_stride, slot, s0 + lr) + (size_t)j0 * esz + lc * 16);
            if (s0 + ps < seq) {
#pragma unroll
                for (int k = 0; k < KR_MLS_NPR; k++) { const int h = gp + pg + 4 * k; if (h < nh) pr[k] = sc[(size_t)h * a.sc_ld + s0 + ps]; }
            }
        };
        auto commit = [&](int s0, int n) {
            if (loader && s0 + lr < seq) {
                float* dst = vs + lc * EPC * KR_MLS_VLD + lr;
#pragma unroll
                for (int j = 0; j < EPC; j++) dst[j * KR_MLS_VLD] = kr_mls_chunk_elem<FP8>(rg, j);
            }
#pragma unroll
            for (int k = 0; k < KR_MLS_NPR; k++) pt[(pg + 4 * k) * KR_MLS_PT + ps] = (ps < n && gp + pg + 4 * k < nh) ? pr[k] : 0.0f;
        };
        float o[KR_MLS_ACC];
#pragma unroll
        for (int k = 0; k < KR_MLS_ACC; k++) o[k] = 0.0f;
        issue(0);
        for (int s0 = 0; s0 < seq; s0 += KR_MLS_PT) {
            const int n = min(KR_MLS_PT, seq - s0);
            __syncthreads();      // the stage before this one is consumed
            commit(s0, n);
            if (s0 + KR_MLS_PT < seq) issue(s0 + KR_MLS_PT);
            __syncthreads();
            if (ka == 1) kr_mls_pv_stage<1>(o, p0, vrow, n);
            else if (ka == 4) kr_mls_pv_stage<4>(o, p0, vrow, n);
            else if (ka == 2) kr_mls_pv_stage<2>(o, p0, vrow, n);
            else if (ka == 3) kr_mls_pv_stage<3>(o, p0, vrow, n);
        }
#pragma unroll
        for (int k = 0; k < KR_MLS_ACC; k++) {
            const int h = gp + hg + k * KR_MLS_TPD;
            if (h < nh) a.attn_lat[((size_t)row * nh + h) * klr + j0 + dl] = o[k];
        }
    }
}

// the three launches over `rows` rows of the pass (after the prep launch, ahead of the w_vc projection).  The caller has made kr_launch_multi_mla's checks
// (kr_multi_mla_ok, nh >= 1, sc_ld % 32 == 0, the page fields) -- a call refused with the option off is refused the same way with it on.  Every kernel's LDS is
// static and inside the default window, whatever the head count
int kr_launch_multi_mla_split(const KrMultiMlaArgs& a, int rows, hipStream_t st) {
    if (!kr_multi_mla_ok(a.klr, a.nd, a.rd) || a.nh < 1 || !a.scores || a.sc_ld < 32 || a.sc_ld % 32 || rows < 1) return 1;
    if (a.page_table && (a.page_stride < 1 || (1 << a.page_shift) < KR_MLS_ROWS)) return 1;      // a stage of the scores kernel must not straddle a page
    const dim3 gs((a.sc_ld + KR_MLS_TILE - 1) / KR_MLS_TILE, (a.nh + KR_MLS_HG - 1) / KR_MLS_HG, rows), gm((a.nh + 3) / 4, rows), gp(a.klr / KR_MLS_DS, rows);
#define KR_MLSL(F_, NBC_, P_) do { \
        hipLaunchKernelGGL((kr_multi_mla_split_scores_kernel<F_, NBC_, P_>), gs, dim3(512), 0, st, a); \
        hipLaunchKernelGGL(kr_multi_mla_split_softmax_kernel, gm, dim3(256), 0, st, a); \
        hipLaunchKernelGGL((kr_multi_mla_split_pv_kernel<F_, NBC_, P_>), gp, dim3(256), 0, st, a); } while (0)
#define KR_MLSL_KLR(F_, P_) do { if (a.klr == 512) KR_MLSL(F_, 64, P_); else KR_MLSL(F_, 32, P_); } while (0)
    if (a.page_table) { if (a.kv_fp8) KR_MLSL_KLR(true, true); else KR_MLSL_KLR(false, true); }
    else { if (a.kv_fp8) KR_MLSL_KLR(true, false); else KR_MLSL_KLR(false, false); }
#undef KR_MLSL_KLR
#undef KR_MLSL
    return 0;
}
