// kr_decode_prefill.cpp -- the whole-model prompt pass on the GPU.
//
// The reference runs the prompt through third-party GPU kernels (flashinfer attention, sglang fused_marlin_moe, torch matmuls:
// python/krasis/model.py forward_prefill_layer_grouped, layer.py:242-461, attention.py:496-687, linear_attention.py:695-845) and
// then hands KV / recurrent state to the CPU decoder (decode_setup.py:232-278).  Here the prompt pass is defined as "what the
// decode graph would have produced token by token": kr_decode_prefill(tokens[0..n)) leaves logits, FP16 KV caches, conv and
// recurrent state bit-identical to n successive kr_decode_step calls (src/decode.rs:2690-3520), so there is one numerics story for
// prefill and decode and no state hand-off.  GEMM-shaped work rides the int8-MFMA grouped GEMM (kr_prefill.hip); everything else
// is the batched form of the decode operators (kr_prefill_ops.hip).  Tokens are processed in chunks through all layers.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/krasis_hip.h"
#include "kr_multi_plan.h"
#include "kr_rows_plan.h"
#include "kr_decode_internal.h"
#include "kr_prefill.h"
#include "kr_prefill_ops.h"
#include "kr_router.h"

#define KR_PFM_CHUNK 1024     // tokens per chunk; with KR_PFM_DEPTH chunks in flight (round-1 sweep, docs/design/08-measurement.md: 1024 x 3 beats 2048 x 2 at 4k / 8k / 20k prompts)
#define KR_PFM_DEPTH 3

namespace {
struct Scratch {   // carved from one allocation per arena (grown on demand)
    float* lac;
    float *res, *hid, *normed, *pa, *pb, *pc, *q, *k, *v, *z, *gexp, *beta, *recur, *attn, *gate, *moe, *sh, *gv, *sgu, *logits;
    int8_t *xh, *xl, *yh, *yl; float *xs, *ys;
    uint16_t *xf, *yf; float *xfm, *yfm;     // KR_GEMM_FAST: the same two activation slots as f16 rows + row multipliers (kr_prefill_h.hip)
    uint16_t* xb; int32_t* ids; float* w;
    float* cv;                               // multi-sequence step: conv + SiLU outputs [rows][conv_dim] of a linear-attention layer
    // "pass_few_rows" (set per pass, kr_rows_plan.h): the projections read their f32 source rows themselves (kr_rows_matvec.hip) -- slot x is B.normed [rows][H],
    // slot y what pf_rows / pf_act were last given (they launch nothing then)
    bool few; int few_group, H; const float* ysrc; int yld, yact;
};
struct Act {      // one GEMM input: INT16 digits or f16 rows; few: its f32 source rows (ld floats apart; act >= 0: rows of [gate | up], that activation first)
    const int8_t* h; const int8_t* l; const float* s; const uint16_t* f; const float* fm;
    bool few; int few_group; const float* x; int ld, act;
};
Act X(const Scratch& B) { return Act{B.xh, B.xl, B.xs, B.xf, B.xfm, B.few, B.few_group, B.normed, B.H, -1}; }
Act Y(const Scratch& B) { return Act{B.yh, B.yl, B.ys, B.yf, B.yfm, B.few, B.few_group, B.ysrc, B.yld, B.yact}; }
struct MultiPass {      // the batched pass over device slots: row b = slot slots[b] at pos[b]; nruns x [slot, off, cnt], the runs of token rows per slot (kr_multi.h)
    const KrMultiPlan& plan;      // what the pass decided (kr_multi_plan.h); its spans are relative to `tables`
    const int32_t* tables; float* lc_scratch; float *xm_inv, *xm_tmax;      // device
    const int32_t *slots, *pos, *runs; int nruns;                           // device
    bool verify;      // kr_decode_verify_multi's pass: linear-attention layers record instead of storing state (docs/design/18-multi-verify.md)
    const int32_t* table(KrMpSpan sp) const { return sp.off < 0 ? nullptr : tables + sp.off; }
};
struct Chunk {      // one chunk of the prompt in flight: its arena, stream and running flags
    Scratch B; float* scores; const int* tok; int Cc, pos0, set; bool first, add_is_emb; hipStream_t st;
    KrPfSync sy;      // this (chunk, layer)'s hand-overs with the previous / next chunk (set by the scheduler before every run_layer)
    bool verify = false;      // kr_decode_verify's pass: linear-attention layers write their recurrence inputs into the store's verify buffers (kr_spec.h)
    const MultiPass* mp = nullptr;      // the batched pass over device slots (kr_multi_pass): what its per-slot sections read; null: a prompt pass
};
size_t al(size_t n) { return (n + 255) & ~(size_t)255; }
}  // namespace

// "pass_few_rows": the projections of a pass of at most 16 token rows on the few-row streaming matvec, every row with the decode step's bits
static int pf_few(const KrMatDev* mats, float* const* outs, const int* lds, int n, const Act& A, int C, hipStream_t st) {
    if (kr_launch_rows_matvec(mats, outs, lds, n, A.x, A.ld, C, A.act, A.few_group, st)) return kr_fail(KR_ERR_HIP, "pass_few_rows: the few-row matvec launch was refused (%d rows, K %d)", C, mats[0].K);
    return KR_OK;
}
static int pf_gemm(kr_decode_store* s, int wid, const Act& A, int C, float* out, int ld, hipStream_t st) {
    DWeight& W = *s->weights[wid];
    if (A.few) { const KrMatDev m = W.ms.view(); return pf_few(&m, &out, &ld, 1, A, C, st); }
    if (s->gemm_fast) { kr_launch_pfh_gemm(W.ms.view(), A.f, A.fm, nullptr, 1, 0, 0, C, out, ld, st); return KR_OK; }
    if (!W.ms.wsum.p) return kr_fail(KR_ERR_STATE, "internal: nibble sums of weight %d were not prepared", wid);
    kr_launch_pf_gemm(W.ms.view(), (const uint32_t*)W.ms.wsum.p, A.h, A.l, A.s, nullptr, 1, 0, 0, C, out, ld, st);
    return KR_OK;
}
// up to three projections of the same input in ONE launch (q | k | v, qkvz | ba, shared gate_up | shared gate); falls back to one launch each
// when the weight widths or K differ
static int pf_gemm_multi(kr_decode_store* s, const int* wids, float* const* outs, const int* lds, int n, const Act& A, int C, hipStream_t st) {
    KrMatDev mats[3]; const uint32_t* ws[3];
    if (A.few && n <= 3) {      // one launch for matrices of one width and K, one each otherwise (the launcher's rule)
        for (int i = 0; i < n; i++) mats[i] = s->weights[wids[i]]->ms.view();
        return pf_few(mats, outs, lds, n, A, C, st);
    }
    bool same = n <= 3;
    for (int i = 0; i < n; i++) {
        DWeight& W = *s->weights[wids[i]];
        if (!s->gemm_fast && !W.ms.wsum.p) return kr_fail(KR_ERR_STATE, "internal: nibble sums of weight %d were not prepared", wids[i]);
        if (i < 3) { mats[i] = W.ms.view(); ws[i] = (const uint32_t*)W.ms.wsum.p; same = same && mats[i].bits == mats[0].bits && mats[i].ng == mats[0].ng; }
    }
    if (same && n > 1) {
        if (s->gemm_fast) kr_launch_pfh_gemm_multi(mats, outs, lds, n, A.f, A.fm, C, st);
        else kr_launch_pf_gemm_multi(mats, ws, outs, lds, n, A.h, A.l, A.s, C, st);
        return KR_OK;
    }
    for (int i = 0; i < n; i++) if (int rc = pf_gemm(s, wids[i], A, C, outs[i], lds[i], st)) return rc;
    return KR_OK;
}
// the producers of a GEMM input: INT16 digits (exact) or f16 rows (KR_GEMM_FAST)
static void pf_rows(kr_decode_store* s, const float* x, int C, int ld, int K, Scratch& B, bool slot_y, hipStream_t st) {
    if (B.few && slot_y) { B.ysrc = x; B.yld = ld; B.yact = -1; return; }      // the few-row kernel quantises the rows in its prologue
    if (s->gemm_fast) kr_launch_pfh_rows_f32(x, C, ld, K, slot_y ? B.yf : B.xf, slot_y ? B.yfm : B.xfm, st);
    else kr_launch_pfm_quant_f32(x, C, ld, K, slot_y ? B.yh : B.xh, slot_y ? B.yl : B.xl, slot_y ? B.ys : B.xs, st);
}
static void pf_act(kr_decode_store* s, const float* gu, int C, int n, int gu_ld, Scratch& B, hipStream_t st) {
    if (B.few) { B.ysrc = gu; B.yld = gu_ld; B.yact = KR_ACT_SILU_MUL; return; }      // ... and applies the activation there
    if (s->gemm_fast) kr_launch_pfh_act(gu, C, n, gu_ld, KR_ACT_SILU_MUL, 0.0f, 0.0f, B.yf, B.yfm, st);
    else kr_launch_pf_act(gu, C, n, gu_ld, KR_ACT_SILU_MUL, 0.0f, 0.0f, B.yh, B.yl, B.ys, st);
}

// "gguf_exact_pass": native-GGUF MoE layers of every multi-row pass take the exact forms (B.xb holds bf16_rne(normed), kr_pfm_norm_kernel: the row
// gg_prologue_f32_as_bf16 forms from the decode step's f32 hidden, so the activation images are the step's)
// "pass_few_rows": a pass of T token rows (n_tokens of prefill / verify, the sum of the counts of a slot entry point) takes the few-row kernels (kr_rows_plan.h)
static bool pass_few_rows(const kr_decode_store* s, int T) {
    return kr_rows_use(s->opt_pass_few_rows, s->opt_pass_few_rows_max, T, s->gemm_fast ? KR_ROWS_MODE_GEMM_FAST : 0);
}
static int gguf_exact_bits(const kr_decode_store* s) {
    return s->opt_gguf_exact_pass ? KR_PF_SET_GGUF_EXACT | (s->opt_gguf_exact_grouped ? 0 : KR_PF_SET_GGUF_STREAM) : 0;
}
static bool has_gguf_moe(const kr_decode_store* s) {
    const kr_engine* e = s->eng;
    if (!e || s->own_eng) return false;
    for (const DLayer& L : s->layers) if (L.mlp == MLP_MOE && L.moe_layer >= 0 && L.moe_layer < (int)e->layers.size() && e->layers[L.moe_layer].gguf) return true;
    return false;
}

// ---- the batched pass over device slots: a layer's arguments for the per-slot kernels (kr_multi.hip), from the layer, the chunk's arena and the pass
static KrMultiLaArgs multi_la_args(kr_decode_store* s, size_t li, const Scratch& B, const MultiPass& P, float* qkvz) {
    const kr_multi_state& M = *s->multi; const DLayer& L = s->layers[li]; const KrMultiPlan& pl = P.plan;
    KrMultiLaArgs m{};
    m.qkvz = qkvz; m.ld_qkvz = s->weights[L.qkvz_wid]->rows; m.ba = B.pb; m.ld_ba = s->weights[L.ba_wid]->rows;
    m.conv_w = (const float*)L.conv_w.p; m.a_log = (const float*)L.a_log.p; m.dt_bias = (const float*)L.dt_bias.p; m.norm_w = (const float*)L.la_norm_w.p;
    m.conv_state = (float*)M.a[li].p; m.conv_stride = M.a_stride[li] / 4; m.recur = (float*)M.b[li].p; m.recur_stride = M.b_stride[li] / 4;
    m.conv_out = B.cv; m.out = B.attn; m.ld_out = s->weights[L.out_wid]->cols; m.nk = L.nk; m.nv = L.nv; m.dk = L.dk; m.dv = L.dv; m.hr = L.nv / L.nk; m.scale = L.la_scale; m.eps = s->eps;
    if (P.verify) {
        const KrMultiLaCommit& R = M.v_host[(size_t)M.v_la_of[li]];
        m.rec_x = (float*)R.rec_x; m.rec_k = (float*)R.rec_k; m.rec_v = (float*)R.rec_v; m.rec_ge = (float*)R.rec_ge; m.rec_be = (float*)R.rec_be;
    }
    if (pl.lx_nruns) m.lx_min = s->mopt.extend_la_exact_min;      // "multi_extend_la_exact": the run kernels leave the staged runs (multi_lx_args)
    if (pl.lc_nruns) {      // "multi_extend_la_chunk": the runs of >= 64 tokens take the chunked rule, its output rows in B.recur ahead of the gated norm
        m.lc_runs = P.table(pl.lc_runs); m.lc_tiles = P.table(pl.lc_tiles); m.lc_nruns = pl.lc_nruns; m.lc_ntiles = pl.lc_ntiles; m.lc_short = pl.lc_short;
        m.lc_scratch = P.lc_scratch; m.lc_o = B.recur;
    }
    return m;
}
// "multi_extend_la_exact": the staged runs' tables and the arena rows their four launches write and read (the same for every linear-attention layer)
static KrMultiLxArgs multi_lx_args(const Scratch& B, const MultiPass& P) {
    const KrMultiPlan& pl = P.plan;
    return KrMultiLxArgs{P.table(pl.lx_runs), P.table(pl.lx_t16), P.table(pl.lx_t8), pl.lx_nruns, pl.lx_t16.n, pl.lx_t8.n, pl.lx_short, B.q, B.k, B.v, B.z, B.gexp, B.beta, B.recur};
}
static KrMultiGqaArgs multi_gqa_args(kr_decode_store* s, size_t li, const Scratch& B, const MultiPass& P) {
    const kr_multi_state& M = *s->multi; const DLayer& L = s->layers[li]; const KrMultiPlan& pl = P.plan;
    KrMultiGqaArgs m{};
    m.slots = P.slots; m.positions = P.pos; m.q_in = B.pa; m.k_in = B.pb; m.v_in = B.pc;
    m.ld_q = s->weights[L.q_wid]->rows; m.ld_k = s->weights[L.k_wid]->rows; m.ld_v = s->weights[L.v_wid]->rows;
    m.q_norm = L.q_norm_len ? (const float*)L.q_norm.p : nullptr; m.k_norm = L.k_norm_len ? (const float*)L.k_norm.p : nullptr;
    m.q_norm_per_head = L.q_norm_len == L.nh * L.hd; m.k_norm_per_head = L.k_norm_len == L.nkv * L.hd;
    m.rope_cos = (const float*)s->rope_cos.p; m.rope_sin = (const float*)s->rope_sin.p; m.rope_half = s->rope_half;
    m.k_cache = M.a[li].p; m.v_cache = M.b[li].p; m.slot_elems = M.a_row[li] ? M.a_stride[li] / M.a_row[li] * L.nkv * L.hd : 0; m.kv_fp8 = M.kv_fp8;
    m.q_out = B.q; m.gate = B.gate; m.attn_out = B.attn; m.scores = (float*)M.scores.p; m.sc_ld = pl.sc_ld;
    if (M.pg.paged()) { m.page_table = (const int*)M.pg_table.p; m.page_stride = M.pg.stride; m.page_shift = M.pg.shift; }      // paged slots: a / b are pools
    m.gated = L.gated; m.nh = L.nh; m.nkv = L.nkv; m.hd = L.hd; m.eps = s->eps; m.sm_scale = L.sm_scale;
    m.xs_split = pl.xs_split;      // "multi_attn_exact_split": the exact per-slot attention as three launches
    if (pl.fd_chunks) { m.fd_o = (float*)M.fd_o.p; m.fd_ml = (float*)M.fd_ml.p; m.fd_chunk = pl.fd_chunk; m.fd_chunks = pl.fd_chunks; }      // "multi_attn_fast", long slots
    if (pl.gqa_runs == KR_MP_RUNS_FLASH) {      // "multi_extend_flash": the runs of >= 2 tokens take the run kernels, the per-row kernels the first nruns rows
        const KrMpSpan t = kr_mp_pf(pl, L.nh, L.nkv);
        m.pf_runs = P.runs; m.pf_nruns = P.nruns; m.pf_tiles = P.table(t); m.pf_ntiles = t.n; m.pf_units = pl.n_unit;
    }
    return m;
}
static KrMultiMlaArgs multi_mla_args(kr_decode_store* s, size_t li, const Scratch& B, const MultiPass& P) {
    const kr_multi_state& M = *s->multi; const DLayer& L = s->layers[li]; const KrMultiPlan& pl = P.plan;
    KrMultiMlaArgs m{};
    m.slots = P.slots; m.positions = P.pos; m.kv_out = B.pb; m.ld_kv = s->weights[L.kva_wid]->rows; m.q_full = B.pa; m.ld_q = L.nh * (L.nd + L.rd);
    m.kv_a_norm = (const float*)L.kv_a_norm.p; m.w_kc = (const float*)L.w_kc.p; m.w_vc = (const float*)L.w_vc.p;
    m.rope_cos = (const float*)L.mla_cos.p; m.rope_sin = (const float*)L.mla_sin.p;
    m.ckv_cache = M.a[li].p; m.kpe_cache = M.b[li].p; m.ckv_stride = M.a_stride[li]; m.kpe_stride = M.b_stride[li]; m.kv_fp8 = M.kv_fp8;
    m.q_abs = B.q; m.q_pe = B.z; m.attn_lat = B.recur; m.v_proj = B.attn; m.scores = (float*)M.scores.p; m.sc_ld = pl.sc_ld;
    m.nh = L.nh; m.klr = L.klr; m.nd = L.nd; m.rd = L.rd; m.vhd = L.vhd; m.eps = s->eps; m.sm_scale = L.sm_scale;
    if (M.pg.paged()) { m.page_table = (const int*)M.pg_table.p; m.page_stride = M.pg.stride; m.page_shift = M.pg.shift; }      // paged slots: the strides are a page's bytes
    m.xs_split = pl.mla_xs_split;      // "multi_mla_exact_split": the exact per-slot attention as three launches
    if (pl.mla_chunks) { m.fd_o = (float*)M.fd_o.p; m.fd_ml = (float*)M.fd_ml.p; m.fd_chunk = pl.mla_chunk; m.fd_chunks = pl.mla_chunks; }      // "multi_mla_fast", long slots
    if (pl.mla_runs == KR_MP_RUNS_FLASH) {      // "multi_extend_mla_flash": the runs of >= 2 tokens take the run kernel, the per-row kernels the first nruns rows
        const KrMpSpan t = kr_mp_mf(pl, L.nh);
        m.mf_runs = P.runs; m.mf_nruns = P.nruns; m.mf_tiles = P.table(t); m.mf_ntiles = t.n; m.mf_units = pl.n_unit;
    }
    return m;
}
// the matrix-core passes' tables of a layer of nh heads over nkv rows (MLA: 1), the score rows' 1 / sum and maxima, one past the largest position a run reads
static KrMultiXmArgs multi_xm_args(const MultiPass& P, int nh, int nkv) {
    const KrMpSpan a = kr_mp_xa(P.plan, nh, nkv), c = kr_mp_xc(P.plan, nh, nkv);
    return KrMultiXmArgs{P.table(a), P.table(c), a.n, c.n, P.xm_inv, P.xm_tmax, P.plan.kv_end};
}

// everything a layer launches, for one chunk, on the chunk's stream
static int run_layer(kr_decode_store* s, Chunk& cx, size_t li) {
    kr_engine* e = s->eng;
    const int H = s->hidden, k = s->topk, Cc = cx.Cc, pos0 = cx.pos0;
    Scratch& B = cx.B; hipStream_t st = cx.st;
    DLayer& L = s->layers[li];
    // ---- input norm (+ digits for the projections)
    KrPfmNormArgs na{};
    na.mode = cx.add_is_emb ? 1 : 0; na.add_in = B.hid; na.emb = (const float*)s->embedding.p; na.tokens = cx.tok; na.res = B.res;
    na.w = (const float*)s->norms[L.input_norm]->p; na.out = B.normed; na.xh = B.xh; na.xl = B.xl; na.xs = B.xs; na.H = H; na.first = cx.first ? 1 : 0;
    na.bias_one = s->norm_bias_one; na.eps = s->eps;
    if (s->gemm_fast || B.few) { na.xh = nullptr; na.xl = nullptr; na.xs = nullptr; }      // tolerance GEMMs take f16 rows of the normalised value instead of the digits; the few-row kernels the f32 rows
    if (s->gemm_fast && s->opt_norm_rows) { na.xf = B.xf; na.xfm = B.xfm; }      // ... and the norm launch writes that row image itself (round 6: one launch per norm less)
    kr_launch_pfm_norm(na, Cc, st);
    if (s->gemm_fast && !s->opt_norm_rows) kr_launch_pfh_rows_f32(B.normed, Cc, H, H, B.xf, B.xfm, st);
    cx.first = false; cx.add_is_emb = false;
    if (L.attn == ATTN_LA) {
        const int nq = s->weights[L.qkvz_wid]->rows, nb = s->weights[L.ba_wid]->rows, oc = s->weights[L.out_wid]->cols;
        // verify pass: the in-projection rows (the conv inputs) and k / v / e^g / beta land in this layer's slice of the verify buffers -- what a rollback replays
        const KrSpecLa* vc = cx.verify ? &s->spec_host[(size_t)s->spec_la_of[li]] : nullptr;
        float* qkvz = vc ? (float*)vc->qkvz : B.pa;
        { const int wids[2] = {L.qkvz_wid, L.ba_wid}; float* outs[2] = {qkvz, B.pb}; const int lds[2] = {nq, nb};
          if (int rc = pf_gemm_multi(s, wids, outs, lds, 2, X(B), Cc, st)) return rc; }
        if (cx.mp) {      // multi-sequence step: every row advances its own slot's conv / recurrent state (kr_multi.hip)
            if (oc != L.nv * L.dv) return kr_fail(KR_ERR_VALUE, "out_proj cols %d != nv*dv", oc);
            const KrMultiLaArgs m = multi_la_args(s, li, B, *cx.mp, qkvz);
            const KrMultiLxArgs x = multi_lx_args(B, *cx.mp);
            if (kr_launch_multi_la(m, cx.mp->runs, cx.mp->nruns, Cc, st, cx.mp->plan.lx_nruns ? &x : nullptr)) return kr_fail(KR_ERR_VALUE, "unsupported linear-attention geometry for the multi-sequence step");
        } else {
            KrPfmLaArgs a{};
            a.qkvz = qkvz; a.ld_qkvz = nq; a.ba = B.pb; a.ld_ba = nb; a.conv_state = (float*)L.conv_state.p; a.conv_w = (const float*)L.conv_w.p;
            a.a_log = (const float*)L.a_log.p; a.dt_bias = (const float*)L.dt_bias.p; a.scale = L.la_scale; a.q = B.q; a.k = B.k; a.v = B.v; a.z = B.z;
            a.gexp = B.gexp; a.beta = B.beta; a.nk = L.nk; a.nv = L.nv; a.dk = L.dk; a.dv = L.dv; a.hr = L.nv / L.nk;
            if (vc) { a.k = (float*)vc->k; a.v = (float*)vc->v; a.gexp = (float*)vc->gexp; a.beta = (float*)vc->beta; }
            a.lac = B.lac; a.fast = s->attn_fast; a.conv_fused = s->opt_la_conv_fused;
            if (kr_launch_pfm_la(a, (float*)L.recur_state.p, B.recur, (const float*)L.la_norm_w.p, B.attn, Cc, s->eps, st, &cx.sy))
                return kr_fail(KR_ERR_VALUE, "unsupported linear-attention geometry");
        }
        if (oc != L.nv * L.dv) return kr_fail(KR_ERR_VALUE, "out_proj cols %d != nv*dv", oc);
        pf_rows(s, B.attn, Cc, oc, oc, B, true, st);
        if (int rc = pf_gemm(s, L.out_wid, Y(B), Cc, B.hid, H, st)) return rc;
    } else if (L.attn == ATTN_GQA) {
        if (!L.kv_k.p && !cx.mp) return kr_fail(KR_ERR_STATE, "set_decode_state was not called (no KV cache for layer %zu)", li);
        const int nq = s->weights[L.q_wid]->rows, nk_ = s->weights[L.k_wid]->rows, nv_ = s->weights[L.v_wid]->rows, oc = s->weights[L.o_wid]->cols;
        { const int wids[3] = {L.q_wid, L.k_wid, L.v_wid}; float* outs[3] = {B.pa, B.pb, B.pc}; const int lds[3] = {nq, nk_, nv_};
          if (int rc = pf_gemm_multi(s, wids, outs, lds, 3, X(B), Cc, st)) return rc; }
        if (cx.mp) {      // multi-sequence step: each row appends to and attends over its own slot at its own position (kr_multi.hip)
            const MultiPass& P = *cx.mp;
            if (oc != L.nh * L.hd) return kr_fail(KR_ERR_VALUE, "o_proj cols %d != nh*hd", oc);
            const KrMultiGqaArgs m = multi_gqa_args(s, li, B, P);
            if (P.plan.gqa_runs == KR_MP_RUNS_XM) {      // "multi_extend_exact_mfma": the runs of >= 2 tokens take the three exact matrix-core passes, the per-row kernels the first nruns rows
                if (kr_launch_multi_gqa_xm(m, multi_xm_args(P, L.nh, L.nkv), P.runs, P.nruns, P.plan.n_unit, Cc, st))
                    return kr_fail(KR_ERR_VALUE, "multi_extend_exact_mfma: unsupported GQA geometry for the multi-sequence step (nh %d nkv %d head_dim %d)", L.nh, L.nkv, L.hd);
            } else if (kr_launch_multi_gqa(m, Cc, st)) return kr_fail(KR_ERR_VALUE, "unsupported GQA geometry for the multi-sequence step");
        } else {
            KrPfmGqaArgs a{};
            a.q_in = B.pa; a.k_in = B.pb; a.v_in = B.pc; a.ld_q = nq; a.ld_k = nk_; a.ld_v = nv_;
            a.q_norm = L.q_norm_len ? (const float*)L.q_norm.p : nullptr; a.k_norm = L.k_norm_len ? (const float*)L.k_norm.p : nullptr;
            a.q_norm_per_head = L.q_norm_len == L.nh * L.hd; a.k_norm_per_head = L.k_norm_len == L.nkv * L.hd;
            a.rope_cos = (const float*)s->rope_cos.p; a.rope_sin = (const float*)s->rope_sin.p; a.rope_half = s->rope_half;
            a.k_cache = L.kv_k.p; a.v_cache = L.kv_v.p; a.kv_fp8 = s->kv_fp8; a.q_out = B.q; a.gate = B.gate; a.attn_out = B.attn;
            a.gated = L.gated; a.nh = L.nh; a.nkv = L.nkv; a.hd = L.hd; a.pos0 = pos0; a.eps = s->eps; a.sm_scale = L.sm_scale;
            if (s->max_rope_seq > 0 && pos0 + Cc > s->max_rope_seq) return kr_fail(KR_ERR_VALUE, "prompt exceeds the rope table (%d)", s->max_rope_seq);
            bool flash = false, flash_tried = false;
            if (s->attn_fast && kr_pfm_gqa_flash_ok(L.nh, L.nkv, L.hd)) {      // tolerance mode: flash attention on the matrix cores (same prep launch)
                kr_launch_pfm_gqa_prep(a, Cc, st);
                kr_pf_wait(st, cx.sy.wait_b); kr_pf_rec(st, cx.sy.rec_b);      // own rows appended; the previous chunks' rows are read from here on
                flash = 0 == kr_launch_pfm_gqa_flash(a, Cc, st);
                flash_tried = true;
            }
            if (!flash) {
                if (flash_tried) return kr_fail(KR_ERR_HIP, "KR_ATTN_FAST: the flash-attention launch was refused (LDS window of head_dim %d)", L.hd);
                if (!cx.scores) return kr_fail(KR_ERR_STATE, "internal: no score scratch for the exact attention passes");
                const int sc_ld = (pos0 + Cc + 63) & ~63;
                float* scp = cx.scores;   // this chunk's arena (chunks in flight on other streams have their own)
                if (kr_launch_pfm_gqa(a, Cc, scp, sc_ld, scp + (size_t)Cc * L.nh * sc_ld, st, &cx.sy)) return kr_fail(KR_ERR_VALUE, "unsupported GQA geometry for the prompt pass");
            }
        }
        if (oc != L.nh * L.hd) return kr_fail(KR_ERR_VALUE, "o_proj cols %d != nh*hd", oc);
        pf_rows(s, B.attn, Cc, oc, oc, B, true, st);
        if (int rc = pf_gemm(s, L.o_wid, Y(B), Cc, B.hid, H, st)) return rc;
    } else if (L.attn == ATTN_MLA) {
        // MLA (decode.rs:2993-3252): batched projections on the GEMM, then the three decode launches with a token dimension.  The
        // prep launch appends every token's latent / rope rows before the attention launch reads them, so token t of the chunk
        // sees exactly the cache decode_step would have built.
        if (!L.kv_k.p && !cx.mp) return kr_fail(KR_ERR_STATE, "set_decode_state was not called (no MLA cache for layer %zu)", li);
        if (!cx.mp && L.mla_rope_seq < pos0 + Cc) return kr_fail(KR_ERR_VALUE, "prompt exceeds the MLA rope table (%d)", L.mla_rope_seq);
        const int nkv = s->weights[L.kva_wid]->rows, nq = L.nh * (L.nd + L.rd), oc = s->weights[L.o_wid]->cols;
        if (int rc = pf_gemm(s, L.kva_wid, X(B), Cc, B.pb, nkv, st)) return rc;
        if (L.mq_wid >= 0) {
            if (int rc = pf_gemm(s, L.mq_wid, X(B), Cc, B.pa, nq, st)) return rc;
        } else {   // LoRA query path: q_a_proj -> sequential RMSNorm -> q_b_proj (decode.rs:3036-3079)
            const int qlr = s->weights[L.mqa_wid]->rows, qc = s->weights[L.mqb_wid]->cols;
            if (qc != qlr || qlr % 128) return kr_fail(KR_ERR_VALUE, "q_b_proj cols %d != q_a_proj rows %d (multiple of 128)", qc, qlr);
            if (int rc = pf_gemm(s, L.mqa_wid, X(B), Cc, B.pc, qlr, st)) return rc;
            if (L.q_a_norm_len) kr_launch_rmsnorm_seq(B.pc, (const float*)L.q_a_norm.p, qlr, s->eps, st, Cc, qlr);
            pf_rows(s, B.pc, Cc, qlr, qlr, B, true, st);
            if (int rc = pf_gemm(s, L.mqb_wid, Y(B), Cc, B.pa, nq, st)) return rc;
        }
        if (cx.mp) {      // multi-sequence step: each row appends to and attends over its own slot at its own position (kr_multi.hip); row positions
                          // were bounded by the shortest MLA rope table before the pass (check_args, kr_decode_multi.cpp)
            const MultiPass& P = *cx.mp;
            const KrMultiMlaArgs m = multi_mla_args(s, li, B, P);
            if (P.plan.mla_runs == KR_MP_RUNS_FLASH && (!m.mf_tiles || !kr_multi_mla_pf_args_ok(m)))
                return kr_fail(KR_ERR_VALUE, "multi_extend_mla_flash: MLA geometry of layer %zu not covered by the run kernel", li);
            if (nkv < L.klr + L.rd) return kr_fail(KR_ERR_VALUE, "kv_a_proj rows %d < kv_lora_rank + rope dim", nkv);
            if (oc != L.nh * L.vhd) return kr_fail(KR_ERR_VALUE, "o_proj cols %d != nh*v_head_dim", oc);
            if (P.plan.mla_runs == KR_MP_RUNS_XM) {      // "multi_extend_mla_exact_mfma": the runs of >= 2 tokens take the three exact matrix-core passes, the per-row kernels the first nruns rows
                if (kr_launch_multi_mla_xm(m, multi_xm_args(P, L.nh, 1), P.runs, P.nruns, P.plan.n_unit, Cc, st))
                    return kr_fail(KR_ERR_VALUE, "multi_extend_mla_exact_mfma: unsupported MLA geometry for the multi-sequence step (heads %d kv_lora_rank %d rope %d)", L.nh, L.klr, L.rd);
            } else if (kr_launch_multi_mla(m, Cc, st)) return kr_fail(KR_ERR_VALUE, "unsupported MLA geometry for the multi-sequence step");
        } else {
            KrMlaArgs a{};
            a.step = nullptr; a.pos0 = pos0; a.kv_out = B.pb; a.ld_kv = nkv; a.q_full = B.pa; a.ld_q = nq;
            a.kv_a_norm = (const float*)L.kv_a_norm.p; a.w_kc = (const float*)L.w_kc.p; a.w_vc = (const float*)L.w_vc.p;
            a.rope_cos = (const float*)L.mla_cos.p; a.rope_sin = (const float*)L.mla_sin.p;
            a.ckv_cache = L.kv_k.p; a.kpe_cache = L.kv_v.p; a.kv_fp8 = s->kv_fp8; a.q_abs = B.q; a.q_pe = B.z; a.attn_lat = B.recur; a.v_proj = B.attn;
            a.nh = L.nh; a.klr = L.klr; a.nd = L.nd; a.rd = L.rd; a.vhd = L.vhd; a.eps = s->eps; a.sm_scale = L.sm_scale; a.fast = s->attn_fast;
            if (!s->attn_fast && cx.scores) { a.pf_sc = cx.scores; a.pf_sc_ld = (pos0 + Cc + 63) & ~63; }      // exact mode: this chunk's score scratch for the matrix-core passes
            kr_pf_wait(st, cx.sy.wait_b);            // the latent / rope rows of the earlier chunks (the three MLA launches append and read in one go)
            kr_launch_mla(a, s->kv_max_seq, st, Cc);
            kr_pf_rec(st, cx.sy.rec_b);
        }
        if (oc != L.nh * L.vhd) return kr_fail(KR_ERR_VALUE, "o_proj cols %d != nh*v_head_dim", oc);
        pf_rows(s, B.attn, Cc, oc, oc, B, true, st);
        if (int rc = pf_gemm(s, L.o_wid, Y(B), Cc, B.hid, H, st)) return rc;
    }
    // ---- post-attention norm: f32 hidden, digits (shared expert / dense MLP), bf16 copy (routed experts)
    na.mode = 0; na.add_in = B.hid; na.first = 0; na.w = (const float*)s->norms[L.post_norm]->p; na.out_bf16 = L.mlp == MLP_MOE ? B.xb : nullptr;
    const bool post_rows = s->gemm_fast && (L.mlp == MLP_DENSE || (L.mlp == MLP_MOE && L.sgu_wid >= 0));      // the shared expert / dense MLP take the f16 rows of the normalised value
    na.xf = post_rows && s->opt_norm_rows ? B.xf : nullptr; na.xfm = post_rows && s->opt_norm_rows ? B.xfm : nullptr;
    kr_launch_pfm_norm(na, Cc, st);
    if (post_rows && !s->opt_norm_rows) kr_launch_pfh_rows_f32(B.normed, Cc, H, H, B.xf, B.xfm, st);
    if (L.mlp == MLP_MOE) {
        Layer& EL = e->layers[L.moe_layer];
        if (!EL.routing_present) return kr_fail(KR_ERR_STATE, "Routing weights not set for layer %d", L.moe_layer);
        if (!EL.w13.allocated() && !EL.gguf) return kr_fail(KR_ERR_STATE, "Model not loaded (MoE layer %d has no experts)", L.moe_layer);   // native GGUF layers: kr_moe_prefill_set walks the block kernels
        const int E = e->r_ne;
        const float* rbias = EL.has_bias ? (const float*)EL.bias.p : nullptr;
        // KR_GEMM_FAST: the router's logits in the tolerance form too (bf16 MFMA on x = hi + lo; its input already carries the mode's f16 operand rounding)
        if (!(s->gemm_fast && Cc >= 32 && EL.gate_row.p && 0 == kr_launch_route_logits_fast(EL.gate_row.p, EL.gate_bf16_exact, B.normed, rbias, B.logits, Cc, E, H, st)))
        if (!(Cc >= 32 && EL.gate_row.p && 0 == kr_launch_route_logits_mfma(EL.gate_row.p, EL.gate_bf16_exact, B.normed, rbias, B.logits, Cc, E, H, st)))
            kr_launch_route_logits_decode(EL.gate_cm.p, EL.gate_bf16_exact, B.normed, rbias, B.logits, Cc, E, H, st);
        kr_launch_route_select(B.logits, EL.has_esc ? (const float*)EL.esc.p : nullptr, B.ids, B.w, Cc, E, k, s->scoring, s->norm_topk, KR_ROUTE_RULE_DECODE, 0, st);
        // routed experts: exact CPU-engine arithmetic on the matrix cores, f32 weighted sum in routing order
        // expert parallelism (kr_ep_init on the engine): this rank's chunk exchanges its (token, slot) rows with the owners over RCCL.  A collective:
        // prefill_impl pads ranks that have fewer chunks with empty-shard calls.  Every chunk in flight has its own exchange-buffer set (cx.set) and stream; the
        // collectives of all chunks are ISSUED in one host order that is the same on every rank (the loop structure below depends only on the agreed chunk count).
        if (e->ep) { if (int rc = kr_moe_prefill_ep_set(e, L.moe_layer, B.xb, B.ids, B.w, B.moe, Cc, k, KR_OUT_F32, 1, cx.set, st ? (void*)st : (void*)1)) return rc; }
        else if (int rc = kr_moe_prefill_set(e, L.moe_layer, B.xb, B.ids, B.w, B.moe, Cc, k, KR_OUT_F32, 1, cx.set | (s->gemm_fast ? KR_PF_SET_FAST : 0) | gguf_exact_bits(s) | (B.few ? KR_PF_SET_ROWS : 0), st)) return rc;
        const bool has_shared = L.sgu_wid >= 0, has_gate = has_shared && L.sg_wid >= 0;
        if (has_shared) {   // decode-store numerics: f32 input digits, fast_silu_mul + f32::round digits (decode.rs:3356-3378)
            const int si2 = s->weights[L.sgu_wid]->rows, SI = si2 / 2;
            if (SI % 128) return kr_fail(KR_ERR_VALUE, "shared expert intermediate %d not a multiple of 128", SI);
            { const int wids[2] = {L.sgu_wid, L.sg_wid}; float* outs[2] = {B.sgu, B.gv}; const int lds[2] = {si2, 1};       // gate_up (| the 1-column gate)
              if (int rc = pf_gemm_multi(s, wids, outs, lds, has_gate ? 2 : 1, X(B), Cc, st)) return rc; }
            pf_act(s, B.sgu, Cc, SI, si2, B, st);
            if (int rc = pf_gemm(s, L.sd_wid, Y(B), Cc, B.sh, H, st)) return rc;
        }
        kr_launch_pfm_moe_epilogue(B.moe, has_shared ? B.sh : nullptr, has_gate ? B.gv : nullptr, 1, s->rsf, B.hid, Cc, H, st);
    } else if (L.mlp == MLP_DENSE) {
        const int K = s->weights[L.down_wid]->cols, ng = s->weights[L.gate_wid]->rows, nu = s->weights[L.up_wid]->rows;
        if (K % 128) return kr_fail(KR_ERR_VALUE, "dense MLP intermediate %d not a multiple of 128", K);
        KR_HIP(hipMemsetAsync(B.sgu, 0, (size_t)Cc * 2 * K * 4, st));   // padding of gate | up stays 0 (decode.rs dense path)
        {   // gate -> [0,K), up -> [K,2K) of each row
            DWeight& Wg = *s->weights[L.gate_wid]; DWeight& Wu = *s->weights[L.up_wid];
            if (int rc = kr_ensure_wsum(e, Wg.ms, st)) return rc;
            if (int rc = kr_ensure_wsum(e, Wu.ms, st)) return rc;
            if (int rc = pf_gemm(s, L.gate_wid, X(B), Cc, B.sgu, 2 * K, st)) return rc;
            if (int rc = pf_gemm(s, L.up_wid, X(B), Cc, B.sgu + K, 2 * K, st)) return rc;
            (void)ng; (void)nu;
        }
        pf_act(s, B.sgu, Cc, K, 2 * K, B, st);
        if (int rc = pf_gemm(s, L.down_wid, Y(B), Cc, B.hid, H, st)) return rc;
    } else {
        KR_HIP(hipMemcpyAsync(B.hid, B.normed, (size_t)Cc * H * 4, hipMemcpyDeviceToDevice, st));   // no MLP: hidden stays the normalised value
    }
    return KR_OK;
}

// final norm + lm_head + greedy sample for the LAST token only (the other positions' logits are never consumed)
static void run_final(kr_decode_store* s, Chunk& cx) {
    Scratch& B = cx.B; const int H = s->hidden;
    KrPfmNormArgs na{};
    na.mode = cx.add_is_emb ? 1 : 0; na.add_in = B.hid; na.emb = (const float*)s->embedding.p; na.tokens = cx.tok; na.res = B.res;
    na.w = (const float*)s->norms[s->final_norm]->p; na.out = B.normed; na.H = H; na.first = cx.first ? 1 : 0; na.bias_one = s->norm_bias_one; na.eps = s->eps;
    kr_launch_pfm_norm(na, cx.Cc, cx.st);
    kr_launch_matvec(mv(s, s->lm_head), B.normed + (size_t)(cx.Cc - 1) * H, 1, (float*)s->logits.p, cx.st);
    kr_launch_argmax((const float*)s->logits.p, s->vocab, (int*)s->tok.p, (float*)s->argmax_scratch.p, cx.st);
}

// final norm + lm_head GEMM for EVERY token of the chunk into vlogits [Cc][V] (the decode step's logits bit for bit)
static int final_rows(kr_decode_store* s, Chunk& cx, float* vlogits) {
    Scratch& B = cx.B; const int H = s->hidden; const size_t V = (size_t)s->vocab;
    KrPfmNormArgs na{};
    na.mode = cx.add_is_emb ? 1 : 0; na.add_in = B.hid; na.emb = (const float*)s->embedding.p; na.tokens = cx.tok; na.res = B.res;
    na.w = (const float*)s->norms[s->final_norm]->p; na.out = B.normed; na.xh = B.xh; na.xl = B.xl; na.xs = B.xs; na.H = H; na.first = cx.first ? 1 : 0;
    na.bias_one = s->norm_bias_one; na.eps = s->eps;
    if (s->gemm_fast || B.few) { na.xh = nullptr; na.xl = nullptr; na.xs = nullptr; }
    if (s->gemm_fast && s->opt_norm_rows) { na.xf = B.xf; na.xfm = B.xfm; }
    kr_launch_pfm_norm(na, cx.Cc, cx.st);
    if (s->gemm_fast && !s->opt_norm_rows) kr_launch_pfh_rows_f32(B.normed, cx.Cc, H, H, B.xf, B.xfm, cx.st);
    return pf_gemm(s, s->lm_head, X(B), cx.Cc, vlogits, (int)V, cx.st);
}

// scoring mode (kr_decode_prefill_nll): all-row logits, then the next-token negative log-likelihood per row; the last chunk also leaves the last
// row's logits and greedy sample where run_final would
static int run_final_all(kr_decode_store* s, Chunk& cx, float* vlogits, int first_tok, int n_tokens, bool last) {
    const size_t V = (size_t)s->vocab;
    if (int rc = final_rows(s, cx, vlogits)) return rc;
    const int scored = std::min(cx.Cc, n_tokens - 1 - first_tok);      // the last prompt token has no label
    kr_launch_pfm_nll(vlogits, V, cx.tok + 1, (float*)s->pf_nll.p + first_tok, scored, (int)V, cx.st);
    if (last) {
        KR_HIP(hipMemcpyAsync(s->logits.p, vlogits + (size_t)(cx.Cc - 1) * V, V * 4, hipMemcpyDeviceToDevice, cx.st));
        kr_launch_argmax((const float*)s->logits.p, s->vocab, (int*)s->tok.p, (float*)s->argmax_scratch.p, cx.st);
    }
    return KR_OK;
}

// verify mode (kr_decode_verify): all-row logits into spec_logits, then the accept kernel -> spec_out = [greedy ids, n_match]; s->logits / s->tok are
// left to kr_decode_commit
static int run_final_verify(kr_decode_store* s, Chunk& cx) {
    if (int rc = final_rows(s, cx, (float*)s->spec_logits.p)) return rc;
    kr_launch_spec_accept((const float*)s->spec_logits.p, (size_t)s->vocab, s->vocab, cx.Cc, cx.tok, (int*)s->spec_out.p, (float*)s->spec_part.p,
                          (unsigned*)((float*)s->spec_part.p + 2 * KR_VERIFY_MAX), cx.st);
    return KR_OK;
}

struct PfLayout {   // one arena: byte offsets of the Scratch buffers, total bytes; score-scratch rows (exact attention) and chunked-LA floats
    size_t total = 0, sc_rows = 0, lac_floats = 0;
    size_t o_res, o_hid, o_nrm, o_pa, o_pb, o_pc, o_q, o_k, o_v, o_z, o_ge, o_be, o_rec, o_att, o_gate, o_moe, o_sh, o_gv, o_sgu, o_xh, o_xl, o_xs, o_yh,
           o_yl, o_ys, o_xb, o_ids, o_w, o_lg, o_lac, o_xf, o_xfm, o_yf, o_yfm, o_cv;
};
// geometry of the widest layer -> the arena of a chunk of C rows; nibble sums of every weight the GEMMs will touch (lm_rows: the all-row lm_head GEMM
// too); multi: the conv-output rows of the multi-sequence step
static int pf_layout(kr_decode_store* s, size_t C, bool lm_rows, bool multi, hipStream_t st, PfLayout& Lo) {
    kr_engine* e = s->eng;
    const size_t H = (size_t)s->hidden;
    size_t cvd = 0, pa = H, pb = 64, pc = 64, qd = 64, kd = 64, vd = 64, zd = 64, nvmax = 1, ad = H, sid = 0, kmax = H, sc_rows = 0;
    std::vector<int> wids;
    for (auto& Ly : s->layers) {
        if (Ly.attn == ATTN_LA) {
            if (multi) cvd = std::max(cvd, (size_t)(2 * Ly.nk * Ly.dk + Ly.nv * Ly.dv));
            pa = std::max(pa, (size_t)s->weights[Ly.qkvz_wid]->rows); pb = std::max(pb, (size_t)s->weights[Ly.ba_wid]->rows);
            qd = std::max(qd, (size_t)Ly.nv * Ly.dk); kd = std::max(kd, (size_t)Ly.nv * Ly.dk); vd = std::max(vd, (size_t)Ly.nv * Ly.dv); zd = std::max(zd, (size_t)Ly.nv * Ly.dv);
            nvmax = std::max(nvmax, (size_t)Ly.nv); ad = std::max(ad, (size_t)s->weights[Ly.out_wid]->cols);
            for (int w : {Ly.qkvz_wid, Ly.ba_wid, Ly.out_wid}) wids.push_back(w);
        } else if (Ly.attn == ATTN_GQA) {
            pa = std::max(pa, (size_t)s->weights[Ly.q_wid]->rows); pb = std::max(pb, (size_t)s->weights[Ly.k_wid]->rows); pc = std::max(pc, (size_t)s->weights[Ly.v_wid]->rows);
            qd = std::max(qd, (size_t)Ly.nh * Ly.hd); zd = std::max(zd, (size_t)Ly.nh * Ly.hd); ad = std::max(ad, (size_t)s->weights[Ly.o_wid]->cols);
            // the score scratch (rows x context f32, per arena) serves the EXACT attention passes only: under KR_ATTN_FAST the flash kernel has none.  Sizing it
            // regardless made a 49 863-token tolerance pass allocate 3 x 13.5 GB it never touched (16.7 k instead of ~45 k tok/s)
            if (!(s->attn_fast && kr_pfm_gqa_flash_ok(Ly.nh, Ly.nkv, Ly.hd))) sc_rows = std::max(sc_rows, (size_t)Ly.nh);
            for (int w : {Ly.q_wid, Ly.k_wid, Ly.v_wid, Ly.o_wid}) wids.push_back(w);
        } else if (Ly.attn == ATTN_MLA) {
            const size_t nq = (size_t)Ly.nh * (Ly.nd + Ly.rd);
            pa = std::max(pa, nq); pb = std::max(pb, (size_t)s->weights[Ly.kva_wid]->rows);
            qd = std::max(qd, (size_t)Ly.nh * Ly.klr); vd = std::max(vd, (size_t)Ly.nh * Ly.klr); zd = std::max(zd, (size_t)Ly.nh * Ly.rd);
            ad = std::max(ad, (size_t)s->weights[Ly.o_wid]->cols);
            if (!s->attn_fast && kr_mla_exact_mfma_ok(Ly.nh, Ly.klr, Ly.rd)) sc_rows = std::max(sc_rows, (size_t)Ly.nh);     // score scratch of the exact matrix-core passes
            wids.push_back(Ly.kva_wid); wids.push_back(Ly.o_wid);
            if (Ly.mq_wid >= 0) wids.push_back(Ly.mq_wid);
            else { pc = std::max(pc, (size_t)s->weights[Ly.mqa_wid]->rows); kmax = std::max(kmax, (size_t)s->weights[Ly.mqa_wid]->rows); wids.push_back(Ly.mqa_wid); wids.push_back(Ly.mqb_wid); }
        }
        if (Ly.mlp == MLP_MOE) {
            if (Ly.sgu_wid >= 0) { sid = std::max(sid, (size_t)s->weights[Ly.sgu_wid]->rows); kmax = std::max(kmax, (size_t)s->weights[Ly.sd_wid]->cols); wids.push_back(Ly.sgu_wid); wids.push_back(Ly.sd_wid); }
            if (Ly.sgu_wid >= 0 && Ly.sg_wid >= 0) wids.push_back(Ly.sg_wid);
            if (s->own_eng || Ly.moe_layer >= (int)e->layers.size()) return kr_fail(KR_ERR_STATE, "set_moe_store was not called (MoE layer %d has no engine)", Ly.moe_layer);
            Layer& EL = e->layers[Ly.moe_layer];
            if (int rc = kr_ensure_gate_row(e, Ly.moe_layer)) return rc;
            if (int rc = kr_ensure_wsum(e, EL.w13, st)) return rc;
            if (int rc = kr_ensure_wsum(e, EL.w2, st)) return rc;
            if (int rc = kr_moe_prefill_prepare(e, Ly.moe_layer, s->gemm_fast ? 1 : 0, 1, st, s->opt_gguf_exact_pass)) return rc;     // native-GGUF layers: block sums / tolerance copies, before any chunk stream runs
        } else if (Ly.mlp == MLP_DENSE) {
            sid = std::max(sid, 2 * (size_t)s->weights[Ly.down_wid]->cols); kmax = std::max(kmax, (size_t)s->weights[Ly.down_wid]->cols);
            for (int w : {Ly.gate_wid, Ly.up_wid, Ly.down_wid}) wids.push_back(w);
        }
    }
    if (lm_rows) wids.push_back(s->lm_head);
    for (int w : wids) {
        DWeight& W = *s->weights[w];
        if (int rc = kr_ensure_wsum(e, W.ms, st)) return rc;
    }
    kmax = std::max(kmax, ad);
    if (s->gemm_fast && C * std::max(kmax, (size_t)H) * 2 >= (1ull << 32)) return kr_fail(KR_ERR_VALUE, "KR_GEMM_FAST: chunk of %zu tokens x %zu values exceeds 4 GiB of f16 activations; lower the chunk", C, std::max(kmax, (size_t)H));
    size_t& total = Lo.total; size_t& lac_floats = Lo.lac_floats; Lo.sc_rows = sc_rows;
    if (s->attn_fast)
        for (auto& Ly : s->layers) if (Ly.attn == ATTN_LA && kr_pfm_la_chunk_ok(Ly.dk, Ly.dv, (int)C)) lac_floats = std::max(lac_floats, kr_pfm_la_chunk_scratch_floats((int)C, Ly.nv));
    auto take = [&](size_t bytes) { const size_t o = total; total += al(bytes); return o; };
    Lo.o_res = take(C * H * 4); Lo.o_hid = take(C * H * 4); Lo.o_nrm = take(C * H * 4); Lo.o_pa = take(C * pa * 4); Lo.o_pb = take(C * pb * 4); Lo.o_pc = take(C * pc * 4);
    Lo.o_q = take(C * qd * 4); Lo.o_k = take(C * kd * 4); Lo.o_v = take(C * vd * 4); Lo.o_z = take(C * zd * 4); Lo.o_ge = take(C * nvmax * 4); Lo.o_be = take(C * nvmax * 4);
    Lo.o_rec = take(C * vd * 4); Lo.o_att = take(C * ad * 4); Lo.o_gate = take(C * zd * 4); Lo.o_moe = take(C * H * 4); Lo.o_sh = take(C * H * 4); Lo.o_gv = take(C * 4);
    Lo.o_sgu = take(C * std::max(sid, (size_t)64) * 4); Lo.o_xh = take(C * H); Lo.o_xl = take(C * H); Lo.o_xs = take(C * (H / 128) * 4); Lo.o_yh = take(C * kmax);
    Lo.o_yl = take(C * kmax); Lo.o_ys = take(C * (kmax / 128 + 1) * 4); Lo.o_xb = take(C * H * 2); Lo.o_ids = take(C * 32 * 4); Lo.o_w = take(C * 32 * 4);
    Lo.o_lg = take(C * (size_t)std::max(e->r_ne, 64) * 4); Lo.o_lac = take(lac_floats * 4);
    Lo.o_xf = take(C * H * 2); Lo.o_xfm = take(C * 4); Lo.o_yf = take(C * kmax * 2); Lo.o_yfm = take(C * 4);
    Lo.o_cv = take(C * cvd * 4);      // multi-sequence step: conv outputs of every linear-attention channel (0 bytes in the prompt pass)
    return KR_OK;
}
static Scratch pf_carve(const PfLayout& Lo, char* base) {
    Scratch B{};
    B.res = (float*)(base + Lo.o_res); B.hid = (float*)(base + Lo.o_hid); B.normed = (float*)(base + Lo.o_nrm); B.pa = (float*)(base + Lo.o_pa); B.pb = (float*)(base + Lo.o_pb);
    B.pc = (float*)(base + Lo.o_pc); B.q = (float*)(base + Lo.o_q); B.k = (float*)(base + Lo.o_k); B.v = (float*)(base + Lo.o_v); B.z = (float*)(base + Lo.o_z);
    B.gexp = (float*)(base + Lo.o_ge); B.beta = (float*)(base + Lo.o_be); B.recur = (float*)(base + Lo.o_rec); B.attn = (float*)(base + Lo.o_att); B.gate = (float*)(base + Lo.o_gate);
    B.moe = (float*)(base + Lo.o_moe); B.sh = (float*)(base + Lo.o_sh); B.gv = (float*)(base + Lo.o_gv); B.sgu = (float*)(base + Lo.o_sgu); B.xh = (int8_t*)(base + Lo.o_xh);
    B.xl = (int8_t*)(base + Lo.o_xl); B.xs = (float*)(base + Lo.o_xs); B.yh = (int8_t*)(base + Lo.o_yh); B.yl = (int8_t*)(base + Lo.o_yl); B.ys = (float*)(base + Lo.o_ys);
    B.xb = (uint16_t*)(base + Lo.o_xb); B.ids = (int32_t*)(base + Lo.o_ids); B.w = (float*)(base + Lo.o_w); B.logits = (float*)(base + Lo.o_lg);
    B.lac = Lo.lac_floats ? (float*)(base + Lo.o_lac) : nullptr;
    B.xf = (uint16_t*)(base + Lo.o_xf); B.xfm = (float*)(base + Lo.o_xfm); B.yf = (uint16_t*)(base + Lo.o_yf); B.yfm = (float*)(base + Lo.o_yfm);
    B.cv = (float*)(base + Lo.o_cv);
    return B;
}

static int prefill_impl(kr_decode_store* s, const int32_t* tokens, int n_tokens, int start_pos, float* logits_out, float* nll_out, void* stream, bool verify = false) {
    if (!s) return kr_fail(KR_ERR_VALUE, "null decode store");
    if (!s->configured) return kr_fail(KR_ERR_STATE, "Call configure_decode first");
    if (!verify) if (int rc = kr_spec_pending_fail(s)) return rc;
    if (!tokens || n_tokens <= 0) return kr_fail(KR_ERR_VALUE, "kr_decode_prefill: empty prompt");
    if ((int)s->layers.size() != s->n_layers) return kr_fail(KR_ERR_STATE, "finalize_decode was not called");
    if (s->opt_gguf_exact_pass && s->gemm_fast && has_gguf_moe(s))
        return kr_fail(KR_ERR_STATE, "the \"gguf_exact_pass\" option and KR_GEMM_FAST exclude each other on a store with native GGUF experts: the exact pass has no tolerance GEMM (clear one of them)");
    if (start_pos < 0 || (s->kv_max_seq > 0 && start_pos + n_tokens > s->kv_max_seq))
        return kr_fail(KR_ERR_VALUE, "prompt [%d, %d) does not fit kv_max_seq %d", start_pos, start_pos + n_tokens, s->kv_max_seq);
    for (int i = 0; i < n_tokens; i++) if (tokens[i] < 0 || tokens[i] >= s->vocab) return kr_fail(KR_ERR_VALUE, "token id %d out of range (vocab %d)", tokens[i], s->vocab);
    kr_engine* e = s->eng;
    KR_HIP(hipSetDevice(e->device));
    hipStream_t st = kr_pick_stream(e, stream);
    const int H = s->hidden;
    if (H % 128) return kr_fail(KR_ERR_VALUE, "kr_decode_prefill needs hidden %% 128 == 0");
    // defaults: 1024 tokens x 3 chunks in flight for the exact pass (its serial per-token kernels need the overlap); with both tolerance bits set the
    // kernels are chunk-parallel and fatter chunks feed the expert GEMMs better (rows per expert grow with the chunk): 4096 x 2 measured best at
    // 8192 tokens (tools/probes/prefill_sweep.py: 1024 x 3 171 ms, 2048 x 2 168, 4096 x 2 164, 8192 x 1 193)
    // (second sweep: three chunks in flight beat two once the prompt has three chunks to give -- 8192 tokens: 2752 x 3 148.6 ms vs 4096 x 2 151.4;
    // 20 434 tokens: 4096 x 3 407 ms vs 4096 x 2 423 -- so: a third of the prompt per chunk, between 1024 and 4096 tokens, three in flight; 3000 tokens: 1024 x 3 56.8 ms vs 2048 + 952 60.9)
    const int third = ((n_tokens + 2) / 3 + 63) / 64 * 64;
    const int tol_chunk = std::min(4096, std::max(KR_PFM_CHUNK, third));
    // (round 6: the same rule with KR_ATTN_FAST alone -- its attention / delta-rule kernels are chunk-parallel too and the exact expert GEMM likes the fatter chunks:
    // 8192 tokens 173.8 -> 162.0 ms, 20 434: 448.5 -> 428.1, 49 863: 1221.6 -> 1185.4; the exact pass keeps 1024 x 3: its per-token recurrences need the overlap)
    const int depth = s->pf_depth >= 1 && s->pf_depth <= KR_PF_MAX_DEPTH ? s->pf_depth : KR_PFM_DEPTH;   // chunks in flight (streams / arenas)
    // exact pass: chunks of ~1024 tokens, their COUNT a multiple of the depth when the prompt has that many -- the last round of chunks then fills every stream
    // (8192 tokens: 8 x 1024 = 3 + 3 + 2 chunks 382.9 ms, 6 x 1366 355.8; 20 434: 20 x 1024 1207.9, 18 x 1136 1180.1; 49 863: unchanged, attention-bound)
    const int q1k = (n_tokens + KR_PFM_CHUNK - 1) / KR_PFM_CHUNK, nc_exact = q1k >= depth ? (q1k / depth) * depth : q1k;
    const int exact_chunk = (n_tokens + nc_exact - 1) / nc_exact;
    const int CH = verify ? n_tokens : std::min(n_tokens, s->pf_chunk > 0 ? s->pf_chunk : (s->attn_fast ? tol_chunk : exact_chunk));     // verify: one chunk
    // expert parallelism: every rank must walk the SAME (chunk, layer) schedule -- the exchanges are collectives -- so the schedule is built from the chunk
    // count of the longest prompt shard (agreed below, before the first exchange); chunks a rank does not have run as empty shards
    int n_chunks_max = (n_tokens + CH - 1) / CH;
    if (e->ep) if (int rc = kr_ep_max_int(e, n_chunks_max, &n_chunks_max, st ? (void*)st : (void*)1)) return rc;
    const int n_chunks = (n_tokens + CH - 1) / CH, n_arenas = std::min(e->ep ? n_chunks_max : n_chunks, depth), D = n_arenas;
    const int L = (int)s->layers.size();

    const size_t C = CH;
    PfLayout Lo;
    if (int rc = pf_layout(s, C, nll_out || verify, false, st, Lo)) return rc;
    const size_t total = Lo.total, sc_rows = Lo.sc_rows;
    const size_t sc_ld_max = (size_t)((start_pos + n_tokens + 63) & ~63), sc_bytes = al(C * sc_rows * (sc_ld_max + 1 + sc_ld_max / 32) * 4);     // scores + 1 / sum per row + row maxima per 32 positions
    if (s->pf_scratch.ensure(total * n_arenas) || s->pf_tokens.ensure((size_t)n_tokens * 4) || (sc_rows && s->pf_scores.ensure(sc_bytes * n_arenas)))
        return kr_fail(KR_ERR_HIP, "hipMalloc of prefill scratch (%zu MiB) failed", (total * n_arenas + sc_bytes * n_arenas) >> 20);
    const size_t vl_bytes = al(C * (size_t)s->vocab * 4);                 // scoring mode: logits of a whole chunk, one buffer per arena
    if (nll_out && (s->pf_vlogits.ensure(vl_bytes * n_arenas) || s->pf_nll.ensure((size_t)n_tokens * 4)))
        return kr_fail(KR_ERR_HIP, "hipMalloc of the all-position logits (%zu MiB) failed", (vl_bytes * n_arenas) >> 20);
    KR_HIP(hipMemcpyAsync(s->pf_tokens.p, tokens, (size_t)n_tokens * 4, hipMemcpyHostToDevice, st));
    auto carve = [&](int arena) { return pf_carve(Lo, (char*)s->pf_scratch.p + (size_t)arena * total); };

    // ---- streams: chunk c runs on stream c % D with arena c % D.  Cell (chunk c, layer l) needs (c, l-1) [same stream] and, from (c-1, l) on another
    // stream, exactly two things: the carried conv slots before its conv launch, and the recurrent state before its scan (linear attention) or the
    // appended KV / latent rows before its attention launch -> two events per (arena, layer), waited for AT THOSE LAUNCHES (KrPfSync), not at the top of the
    // layer.  (Round 3 recorded one event at the END of a layer and waited for it at the start of the next chunk's layer: the kernel trace showed the state
    // scan of a chunk running alone for 62 % of its time -- 8.5 % of the wall clock -- with both neighbours parked behind whole-layer waits, and two kernels
    // in flight 78 % of the time at a depth of three.)  The serial, low-occupancy kernels of one chunk (delta-rule scan, softmax sums, router top-k) overlap
    // with the GEMMs and attention passes of its neighbours.
    hipStream_t streams[KR_PF_MAX_DEPTH];
    for (auto& x : streams) x = st;
    const size_t ev_start = (size_t)2 * D * L, ev_end = ev_start + 1;     // [arena][layer][a | b], + one start event, + one end event per side stream
    if (D > 1) {
        while ((int)s->pf_side.size() < D - 1) { hipStream_t ns; KR_HIP(hipStreamCreateWithFlags(&ns, hipStreamNonBlocking)); s->pf_side.push_back(ns); }
        for (int i = 1; i < D; i++) streams[i] = s->pf_side[i - 1];
        while (s->pf_events.size() < ev_end + D) { hipEvent_t ev; KR_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming)); s->pf_events.push_back(ev); }
        KR_HIP(hipEventRecord(s->pf_events[ev_start], st));               // side streams start after everything already queued on the main one
        for (int i = 1; i < D; i++) KR_HIP(hipStreamWaitEvent(streams[i], s->pf_events[ev_start], 0));
    }
    const auto t_enqueue = std::chrono::steady_clock::now();
    const bool few = pass_few_rows(s, n_tokens);      // decided for the pass, never per chunk
    s->path_counts[KR_MPC_SEQ_PASSES]++; s->path_counts[KR_MPC_SEQ_FEW] += few;      // kr_decode_multi_path_counts (host-side test aid)
    std::vector<Chunk> chunks(n_chunks);
    for (int c = 0; c < n_chunks; c++) {
        Chunk& cx = chunks[c];
        cx.set = c % D; cx.B = carve(cx.set); cx.B.H = H; cx.B.few = few; cx.B.few_group = s->opt_pass_few_rows_group; cx.scores = sc_rows ? (float*)((char*)s->pf_scores.p + (size_t)cx.set * sc_bytes) : nullptr;
        cx.Cc = std::min(CH, n_tokens - c * CH); cx.pos0 = start_pos + c * CH; cx.tok = (const int*)s->pf_tokens.p + (size_t)c * CH;
        cx.first = true; cx.add_is_emb = true; cx.st = streams[cx.set]; cx.verify = verify;
    }
    // D chunks in flight (one per stream / arena): groups of D chunks are enqueued layer-interleaved; chunk c + D follows chunk c on the same
    // stream, so its arena is free, and it waits layer by layer for chunk c + D - 1 -- the pipeline never drains between groups
    const int n_sched = e->ep ? n_chunks_max : n_chunks;      // expert parallelism: the schedule of the longest shard; this rank's missing chunks are phantoms
    for (int p0 = 0; p0 < n_sched; p0 += D) {
        const int nb = std::min(D, n_sched - p0);
        for (int d = 0; d < L + nb - 1; d++) {
            for (int j = 0; j < nb; j++) {
                const int l = d - j, c = p0 + j;
                if (l < 0 || l >= L) continue;
                if (c >= n_chunks) {
                    // phantom chunk: kr_moe_prefill_ep is a collective, one call per (chunk, MoE layer) on every rank IN THE SAME ORDER.  A rank whose prompt
                    // shard has fewer chunks answers with an empty shard at the position the chunk would have had (its experts still serve the peers' rows).
                    const DLayer& Ly = s->layers[(size_t)l];
                    if (Ly.mlp == MLP_MOE) {
                        hipStream_t ps = streams[c % D];
                        if (int rc = kr_moe_prefill_ep_set(e, Ly.moe_layer, nullptr, nullptr, nullptr, nullptr, 0, s->topk, KR_OUT_F32, 1, c % D, ps ? (void*)ps : (void*)1)) return rc;
                    }
                    continue;
                }
                Chunk& cx = chunks[c];
                cx.sy = KrPfSync{};
                if (D > 1) {
                    hipEvent_t* own = &s->pf_events[((size_t)(c % D) * L + l) * 2];
                    cx.sy.rec_a = own[0]; cx.sy.rec_b = own[1];
                    if (c > 0) { hipEvent_t* prev = &s->pf_events[((size_t)((c - 1) % D) * L + l) * 2]; cx.sy.wait_a = prev[0]; cx.sy.wait_b = prev[1]; }
                }
                if (int rc = run_layer(s, cx, (size_t)l)) return rc;
                if (nll_out && l == L - 1)
                    if (int rc = run_final_all(s, cx, (float*)((char*)s->pf_vlogits.p + (size_t)cx.set * vl_bytes), c * CH, n_tokens, c == n_chunks - 1)) return rc;
                if (verify && l == L - 1)
                    if (int rc = run_final_verify(s, cx)) return rc;
            }
        }
    }
    Chunk& last = chunks[n_chunks - 1];
    if (!nll_out && !verify) run_final(s, last);
    for (int i = 1; i < D; i++) {                                          // results become visible on the caller's stream
        KR_HIP(hipEventRecord(s->pf_events[ev_end + i], streams[i]));
        KR_HIP(hipStreamWaitEvent(st, s->pf_events[ev_end + i], 0));
    }
    KR_HIP(hipGetLastError());
    s->last_stream = st;
    if (s->opt_pfm_timing) {      // tuning aid: how long the host took to enqueue the pass vs how long the GPU needs to drain it
        const double enq = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_enqueue).count();
        (void)hipStreamSynchronize(st);
        const double tot = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_enqueue).count();
        fprintf(stderr, "[kr_decode_prefill] %d tokens: host enqueue %.1f ms, GPU drained after %.1f ms\n", n_tokens, enq, tot);
    }
    if (logits_out) {
        if (is_device_ptr(logits_out)) KR_HIP(hipMemcpyAsync(logits_out, s->logits.p, (size_t)s->vocab * 4, hipMemcpyDeviceToDevice, st));
        else { KR_HIP(hipMemcpyAsync(logits_out, s->logits.p, (size_t)s->vocab * 4, hipMemcpyDeviceToHost, st)); KR_HIP(hipStreamSynchronize(st)); }
    }
    if (nll_out && n_tokens > 1) {
        if (is_device_ptr(nll_out)) KR_HIP(hipMemcpyAsync(nll_out, s->pf_nll.p, (size_t)(n_tokens - 1) * 4, hipMemcpyDeviceToDevice, st));
        else { KR_HIP(hipMemcpyAsync(nll_out, s->pf_nll.p, (size_t)(n_tokens - 1) * 4, hipMemcpyDeviceToHost, st)); KR_HIP(hipStreamSynchronize(st)); }
    }
    return KR_OK;
}

extern "C" int kr_decode_prefill(kr_decode_store* s, const int32_t* tokens, int n_tokens, int start_pos, float* logits_out, void* stream) {
    return prefill_impl(s, tokens, n_tokens, start_pos, logits_out, nullptr, stream);
}
// prompt pass that also scores the prompt: nll_out[i] = -log softmax(logits at position i)[tokens[i + 1]], i in [0, n_tokens - 1)
extern "C" int kr_decode_prefill_nll(kr_decode_store* s, const int32_t* tokens, int n_tokens, int start_pos, float* nll_out, float* logits_out, void* stream) {
    if (!nll_out) return kr_fail(KR_ERR_VALUE, "kr_decode_prefill_nll: null nll_out");
    if (n_tokens < 2) return kr_fail(KR_ERR_VALUE, "Need at least 2 tokens, got %d", n_tokens);
    return prefill_impl(s, tokens, n_tokens, start_pos, logits_out, nll_out, stream);
}

// tuning hook: chunks in flight (1..8, 0 = default 3)
extern "C" int kr_decode_set_prefill_depth(kr_decode_store* s, int depth) {
    if (!s) return kr_fail(KR_ERR_VALUE, "null decode store");
    if (depth < 0 || depth > KR_PF_MAX_DEPTH) return kr_fail(KR_ERR_VALUE, "prefill depth %d out of range [0, %d]", depth, KR_PF_MAX_DEPTH);
    s->pf_depth = depth;
    return KR_OK;
}

// test / tuning hook: tokens per chunk of the prompt pass (0 = default 1024)
extern "C" int kr_decode_set_prefill_chunk(kr_decode_store* s, int chunk) {
    if (!s) return kr_fail(KR_ERR_VALUE, "null decode store");
    if (chunk < 0 || chunk > 8192) return kr_fail(KR_ERR_VALUE, "prefill chunk %d out of range [0, 8192]", chunk);
    s->pf_chunk = chunk;
    return KR_OK;
}

// ------------------------------------------------------------------------------------------------
// exact speculative greedy decoding: verify / commit (docs/design/12-speculative.md)
// ------------------------------------------------------------------------------------------------
int kr_spec_pending_fail(kr_decode_store* s) {
    return s && s->spec_pending ? kr_fail(KR_ERR_STATE, "a kr_decode_verify is pending: kr_decode_commit must come first") : KR_OK;
}

// paged slots under "multi_attn_fast" alone: the entry point refuses the call with the words it always had (paged_refuse, kr_decode_multi.cpp), unless its
// argument check does first; every refusal of a later option stands back there, so that one stays ahead of theirs
bool paged_refused(const kr_decode_store* s) { return s->multi && s->multi->pg.paged() && s->mopt.attn_fast && !s->mopt.attn_fast_paged; }
// the store has a layer of this attention kind (ATTN_*)
bool has_attn(const kr_decode_store* s, int kind) {
    for (const DLayer& L : s->layers) if (L.attn == kind) return true;
    return false;
}

// what no exact pass over this store runs: tolerance modes, expert parallelism, MoE layers without an engine or with native-GGUF experts (unless the
// "gguf_exact_pass" option gives those an exact pass, docs/design/20-gguf-exact-pass.md), geometries the
// verify-form kernels do not cover.  slots: the pass over device slots (multi_refuse, kr_decode_multi.cpp), whose messages start with another noun and whose
// per-slot kernels refuse more; its base clauses sit here, each in its place, because the order of the refusals is part of both contracts; the slot options' own
// rules follow in kr_option_rules below (the "multi_attn_fast" MLA clause apart: its place ahead of the expert-parallelism clause can be seen)
int kr_exact_refuse(kr_decode_store* s, bool slots) {
    const char *the = slots ? "the " : "", *what = slots ? "multi-sequence step" : "speculative decoding";
    if (s->attn_fast || s->gemm_fast || s->decode_fast)
        return kr_fail(KR_ERR_STATE, "%s%s is exact-mode only: the attention mode has tolerance bits set (%d)", the, what, s->attn_fast | s->gemm_fast << 1 | s->decode_fast << 2);
    if (slots && (s->mopt.attn_fast || s->mopt.attn_fast_paged))
        for (size_t i = 0; i < s->layers.size(); i++)
            if (s->layers[i].attn == ATTN_MLA)
                return kr_fail(KR_ERR_STATE, "the \"%s\" option covers GQA layers only: layer %zu is MLA (set the option to 0 for the exact step)",
                               s->mopt.attn_fast_paged ? "multi_attn_fast_paged" : "multi_attn_fast", i);
    kr_engine* e = s->eng;
    if (e->ep) return kr_fail(KR_ERR_STATE, "%s%s does not run under expert parallelism", the, what);
    for (const DLayer& L : s->layers) {
        if (slots && L.attn == ATTN_MLA && !kr_multi_mla_ok(L.klr, L.nd, L.rd))
            return kr_fail(KR_ERR_VALUE, "%s: MLA geometry kv_lora_rank %d nope %d rope %d not covered (kv_lora_rank 512 / 256, rope 64)", what, L.klr, L.nd, L.rd);
        if (L.mlp == MLP_MOE) {
            if (s->own_eng || L.moe_layer >= (int)e->layers.size()) return kr_fail(KR_ERR_STATE, "set_moe_store was not called (MoE layer %d has no engine)", L.moe_layer);
            if (e->layers[L.moe_layer].gguf && !s->opt_gguf_exact_pass)
                return kr_fail(KR_ERR_STATE, "%s%s is exact-mode only: MoE layer %d holds native GGUF experts (their prompt pass is tolerance-only); the \"gguf_exact_pass\" option gives them an exact pass",
                               the, what, L.moe_layer);
        }
        // the slots' kernels also need whole value-head groups per key head
        if (L.attn == ATTN_LA && (L.kd != 4 || (L.dk != 64 && L.dk != 128) || L.dv > 256 || L.dv % 8 || (slots && L.nv != L.nk * (L.nv / L.nk))))
            return kr_fail(KR_ERR_VALUE, "%s: linear-attention geometry kd %d dk %d dv %d not covered (kd 4, dk 64 / 128, dv <= 256)", what, L.kd, L.dk, L.dv);
        if (slots && L.attn == ATTN_GQA && ((L.hd != 64 && L.hd != 128 && L.hd != 256) || L.nkv < 1 || L.nh % L.nkv || (L.nh / L.nkv) * (L.hd + 64) > 12288))
            return kr_fail(KR_ERR_VALUE, "%s: GQA geometry nh %d nkv %d head_dim %d not covered (head_dim 64 / 128 / 256)", what, L.nh, L.nkv, L.hd);
    }
    return KR_OK;
}
int kr_spec_refuse(kr_decode_store* s) { return kr_exact_refuse(s, false); }

// The slot options' refusals as ONE ordered list (docs/design/39-slot-option-rules.md), walked behind kr_exact_refuse(s, true), so everything refused before
// an option existed is refused first and with the same words.  The order of the rules, and of the steps within a rule, is what a caller sees when two
// options refuse one store: it is part of the contract (tests/test_multi_option_refusals_gpu.py).  A rule that is asked refuses, in this order: its rival
// option being set too (two options claim the same rows); [geo_first: its geometry rule]; [mla_at 1: an MLA layer -- its runs would stay exact beside the
// tolerance form, and no single-sequence pass is like that]; a store without a layer of its kind (an option that silently does nothing is a trap); [mla_at
// 2: an MLA layer]; a layer of its kind outside its kernels' geometry (an error, never a fall-back).  stand_back: the rule is not asked where paged_refused
// holds, so the entry point's paged refusal stays ahead of it.  tail: how the message ends its advice.  prepare / ready: the LDS windows of its run kernels,
// raised once per slot set -- never by the refusing walk
struct KrOptRule {
    const char* name; int KrMultiOpts::*flag; int kind; bool stand_back;
    const char* rival_name; int KrMultiOpts::*rival; const char* claim;
    int mla_at; bool geo_first; const char* tail;
    int (*geo)(const kr_decode_store* s, const DLayer& L);      // KR_OK, or the refusal of this layer
    int (*prepare)(kr_decode_store* s); bool kr_multi_state::*ready;
};
static const char* const kr_kind_words[] = {"", "linear-attention", "GQA", "MLA"};      // by ATTN_*
static const KrOptRule kr_opt_rules[] = {
    // more than 64 heads, or a geometry outside the flash kernel's: the single-sequence launcher falls back to the exact kernels there (kr_launch_mla_flash_decode), so there would be no fast step to be identical to
    {"multi_mla_fast", &KrMultiOpts::mla_fast, ATTN_MLA, false, nullptr, nullptr, nullptr, 0, true, " for the exact step",
     [](const kr_decode_store*, const DLayer& L) { return kr_multi_mla_fd_ok(L.nh, L.klr, L.rd) ? KR_OK : kr_fail(KR_ERR_VALUE, "multi_mla_fast: MLA geometry heads %d kv_lora_rank %d rope %d not covered (at most 64 heads, kv_lora_rank 512 / 256, rope 64)", L.nh, L.klr, L.rd); },
     nullptr, nullptr},
    // the run kernel's geometry rule (kr_launch_mla_flash's: any head count) is kr_multi_mla_ok's, which kr_exact_refuse has asked of every MLA layer
    {"multi_extend_mla_flash", &KrMultiOpts::extend_mla_flash, ATTN_MLA, true, nullptr, nullptr, nullptr, 0, false, " for the exact pass", nullptr,
     [](kr_decode_store* s) {
         for (const DLayer& L : s->layers)
             if (L.attn == ATTN_MLA && kr_multi_mla_pf_prepare(L.klr, s->multi->kv_fp8, s->multi->pg.paged()))
                 return kr_fail(KR_ERR_HIP, "multi_extend_mla_flash: LDS window of the run kernel refused (kv_lora_rank %d)", L.klr);
         return (int)KR_OK;
     }, &kr_multi_state::mf_ready},
    {"multi_extend_flash", &KrMultiOpts::extend_flash, ATTN_GQA, true, nullptr, nullptr, nullptr, 1, false, " for the exact pass",
     [](const kr_decode_store*, const DLayer& L) { return kr_pfm_gqa_flash_ok(L.nh, L.nkv, L.hd) ? KR_OK : kr_fail(KR_ERR_VALUE, "multi_extend_flash: GQA geometry nh %d nkv %d head_dim %d not covered (heads per KV head must divide 128, head_dim 64 / 128 / 256)", L.nh, L.nkv, L.hd); },
     [](kr_decode_store* s) {
         for (const DLayer& L : s->layers)
             if (L.attn == ATTN_GQA && kr_multi_pf_prepare(L.hd, s->multi->kv_fp8, s->multi->pg.paged()))
                 return kr_fail(KR_ERR_HIP, "multi_extend_flash: LDS window of the run kernel refused (head_dim %d)", L.hd);
         return (int)KR_OK;
     }, &kr_multi_state::pf_ready},
    {"multi_extend_la_chunk", &KrMultiOpts::extend_la_chunk, ATTN_LA, true, nullptr, nullptr, nullptr, 2, false, " for the exact pass",
     [](const kr_decode_store* s, const DLayer& L) { return kr_multi_lc_ok(L.dk, L.dv, L.nk, L.nv, s->weights[L.qkvz_wid]->rows) ? KR_OK : kr_fail(KR_ERR_VALUE, "multi_extend_la_chunk: linear-attention geometry nk %d nv %d dk %d dv %d not covered (dk = dv = 128, whole value-head groups per key head)", L.nk, L.nv, L.dk, L.dv); },
     [](kr_decode_store*) { return kr_multi_lc_prepare() ? kr_fail(KR_ERR_HIP, "multi_extend_la_chunk: LDS window of the chunked delta rule's kernels refused") : (int)KR_OK; }, &kr_multi_state::lc_ready},
    // the exact forms below have nothing to prepare: their kernels' LDS is below the default window
    {"multi_extend_exact_mfma", &KrMultiOpts::extend_exact_mfma, ATTN_GQA, true, "multi_extend_flash", &KrMultiOpts::extend_flash, "the runs of >= 2 tokens of the GQA layers", 0, false, "",
     [](const kr_decode_store*, const DLayer& L) {
         KrPfmGqaArgs g{};
         g.nh = L.nh; g.nkv = L.nkv; g.hd = L.hd;
         return kr_pfm_gqa_exact_mfma_ok(g) ? KR_OK : kr_fail(KR_ERR_VALUE, "multi_extend_exact_mfma: GQA geometry nh %d nkv %d head_dim %d not covered (heads per KV head must divide 32, head_dim 64 / 128 / 256; set the option to 0 for the per-row kernel)", L.nh, L.nkv, L.hd);
     }, nullptr, nullptr},
    {"multi_extend_mla_exact_mfma", &KrMultiOpts::extend_mla_exact_mfma, ATTN_MLA, true, "multi_extend_mla_flash", &KrMultiOpts::extend_mla_flash, "the runs of >= 2 tokens of the MLA layers", 0, false, "",
     [](const kr_decode_store*, const DLayer& L) { return kr_mla_exact_mfma_ok(L.nh, L.klr, L.rd) ? KR_OK : kr_fail(KR_ERR_VALUE, "multi_extend_mla_exact_mfma: MLA geometry heads %d kv_lora_rank %d rope %d not covered (the head count must divide 32, kv_lora_rank 512 / 256, rope 64; set the option to 0 for the per-row kernel)", L.nh, L.klr, L.rd); },
     nullptr, nullptr},
    // the two splits cover every geometry the one kernel covers, and the pass makes that kernel's checks either way
    {"multi_attn_exact_split", &KrMultiOpts::attn_exact_split, ATTN_GQA, true, nullptr, nullptr, nullptr, 0, false, "", nullptr, nullptr, nullptr},
    {"multi_mla_exact_split", &KrMultiOpts::mla_exact_split, ATTN_MLA, true, nullptr, nullptr, nullptr, 0, false, "", nullptr, nullptr, nullptr},
    {"multi_extend_la_exact", &KrMultiOpts::extend_la_exact, ATTN_LA, true, "multi_extend_la_chunk", &KrMultiOpts::extend_la_chunk, "the long runs of the linear-attention layers", 0, false, "",
     [](const kr_decode_store* s, const DLayer& L) { return kr_multi_lx_ok(L.dk, L.dv, L.nk, L.nv, s->weights[L.qkvz_wid]->rows) ? KR_OK : kr_fail(KR_ERR_VALUE, "multi_extend_la_exact: linear-attention geometry nk %d nv %d dk %d dv %d not covered (dk 64 / 128, dk <= dv <= 256, dv a multiple of 8, 16-byte in-projection rows, whole value-head groups per key head; set the option to 0 for the run kernels)", L.nk, L.nv, L.dk, L.dv); },
     nullptr, nullptr},
};
// the one walk of the list.  prepare false: the refusals (multi_refuse).  prepare true: every refusal of the call has passed (multi_begin) and the rules that
// are set and asked raise their LDS windows, once per slot set and outside kr_multi_pass.  Allocates nothing
int kr_option_rules(kr_decode_store* s, bool prepare) {
    const bool back = paged_refused(s);
    for (const KrOptRule& r : kr_opt_rules) {
        if (!(s->mopt.*r.flag) || (r.stand_back && back)) continue;
        if (prepare) {
            if (!r.prepare || !s->multi || s->multi.get()->*r.ready) continue;
            KR_HIP(hipSetDevice(s->eng->device));
            if (int rc = r.prepare(s)) return rc;
            s->multi.get()->*r.ready = true;
            continue;
        }
        const char* kind = kr_kind_words[r.kind];
        auto geo = [&]() { for (const DLayer& L : s->layers) if (L.attn == r.kind) if (int rc = r.geo(s, L)) return rc; return (int)KR_OK; };
        auto mla = [&]() {
            for (size_t i = 0; i < s->layers.size(); i++)
                if (s->layers[i].attn == ATTN_MLA) return kr_fail(KR_ERR_STATE, "the \"%s\" option covers %s layers only: layer %zu is MLA (set the option to 0%s)", r.name, kind, i, r.tail);
            return (int)KR_OK;
        };
        if (r.rival && s->mopt.*r.rival) return kr_fail(KR_ERR_STATE, "the \"%s\" and \"%s\" options both claim %s: set one of them to 0", r.name, r.rival_name, r.claim);
        if (r.geo && r.geo_first) if (int rc = geo()) return rc;
        if (r.mla_at == 1) if (int rc = mla()) return rc;
        if (!has_attn(s, r.kind)) return kr_fail(KR_ERR_STATE, "the \"%s\" option covers %s layers only: this store has none (set the option to 0%s)", r.name, kind, r.tail);
        if (r.mla_at == 2) if (int rc = mla()) return rc;
        if (r.geo && !r.geo_first) if (int rc = geo()) return rc;
    }
    return KR_OK;
}

// verify buffers of every linear-attention layer (KR_VERIFY_MAX rows) + the device table the snapshot / rollback kernels walk
static int spec_prepare(kr_decode_store* s, hipStream_t st) {
    s->spec_la.clear(); s->spec_la_of.assign(s->layers.size(), -1);
    size_t total = 0, max_floats = 0;
    auto take = [&](size_t floats) { const size_t o = total; total += (floats + 63) & ~(size_t)63; return o; };
    struct Off { size_t qkvz, k, v, ge, be, sr, sc; };
    std::vector<Off> offs;
    s->spec_nv_max = 0; s->spec_dv_max = 0; s->spec_has64 = false; s->spec_has128 = false;
    for (size_t li = 0; li < s->layers.size(); li++) {
        const DLayer& L = s->layers[li];
        if (L.attn != ATTN_LA) continue;
        s->spec_la_of[li] = (int)s->spec_la.size(); s->spec_la.push_back((int)li);
        const size_t R = KR_VERIFY_MAX, nq = (size_t)s->weights[L.qkvz_wid]->rows, rec = (size_t)L.nv * L.dk * L.dv, conv = (size_t)(2 * L.nk * L.dk + L.nv * L.dv) * 4;
        Off o;
        o.qkvz = take(R * nq); o.k = take(R * L.nv * L.dk); o.v = take(R * L.nv * L.dv); o.ge = take(R * L.nv); o.be = take(R * L.nv); o.sr = take(rec); o.sc = take(conv);
        offs.push_back(o);
        max_floats = std::max(max_floats, rec + conv);
        s->spec_nv_max = std::max(s->spec_nv_max, L.nv); s->spec_dv_max = std::max(s->spec_dv_max, L.dv);
        (L.dk == 64 ? s->spec_has64 : s->spec_has128) = true;
    }
    const bool fresh_part = s->spec_part.bytes == 0;
    if (s->spec_buf.ensure(std::max(total, (size_t)64) * 4) || s->spec_logits.ensure((size_t)KR_VERIFY_MAX * s->vocab * 4) || s->spec_out.ensure(64 * 4) ||
        s->spec_part.ensure(64 * 4) || s->spec_tab.ensure(std::max(offs.size(), (size_t)1) * sizeof(KrSpecLa)))
        return kr_fail(KR_ERR_HIP, "hipMalloc of the verify buffers (%zu MiB) failed", (total * 4 + (size_t)KR_VERIFY_MAX * s->vocab * 4) >> 20);
    if (fresh_part) KR_HIP(hipMemsetAsync(s->spec_part.p, 0, s->spec_part.bytes, st));     // the accept kernel's counter starts at 0 and resets itself
    std::vector<KrSpecLa> tab(offs.size());
    float* base = (float*)s->spec_buf.p;
    for (size_t i = 0; i < offs.size(); i++) {
        DLayer& L = s->layers[(size_t)s->spec_la[i]];
        KrSpecLa& E = tab[i];
        E.recur = (float*)L.recur_state.p; E.conv = (float*)L.conv_state.p; E.snap_recur = base + offs[i].sr; E.snap_conv = base + offs[i].sc;
        E.qkvz = base + offs[i].qkvz; E.k = base + offs[i].k; E.v = base + offs[i].v; E.gexp = base + offs[i].ge; E.beta = base + offs[i].be;
        E.nk = L.nk; E.nv = L.nv; E.dk = L.dk; E.dv = L.dv; E.hr = L.nv / L.nk; E.ld_qkvz = s->weights[L.qkvz_wid]->rows;
    }
    if (tab.size() != s->spec_host.size() || (!tab.empty() && memcmp(tab.data(), s->spec_host.data(), tab.size() * sizeof(KrSpecLa)))) {
        KR_HIP(hipStreamSynchronize(st));            // an earlier pass may still read the old table
        if (!tab.empty()) KR_HIP(hipMemcpy(s->spec_tab.p, tab.data(), tab.size() * sizeof(KrSpecLa), hipMemcpyHostToDevice));
        s->spec_host = tab;
    }
    s->spec_floats = max_floats;
    return KR_OK;
}

extern "C" int kr_decode_verify(kr_decode_store* s, const int32_t* tokens, int n_tokens, int start_pos, int32_t* greedy_out, int* n_match_out, void* stream) {
    if (!s) return kr_fail(KR_ERR_VALUE, "null decode store");
    if (!s->configured) return kr_fail(KR_ERR_STATE, "Call configure_decode first");
    if ((int)s->layers.size() != s->n_layers) return kr_fail(KR_ERR_STATE, "finalize_decode was not called");
    if (int rc = kr_spec_pending_fail(s)) return rc;
    if (int rc = kr_spec_refuse(s)) return rc;
    if (!tokens || !greedy_out || !n_match_out) return kr_fail(KR_ERR_VALUE, "kr_decode_verify: null pointer");
    if (n_tokens < 1 || n_tokens > KR_VERIFY_MAX) return kr_fail(KR_ERR_VALUE, "kr_decode_verify: %d tokens, must be in [1, %d]", n_tokens, KR_VERIFY_MAX);
    for (int i = 0; i < n_tokens; i++) if (tokens[i] < 0 || tokens[i] >= s->vocab) return kr_fail(KR_ERR_VALUE, "token id %d out of range (vocab %d)", tokens[i], s->vocab);
    const int end = start_pos + n_tokens;
    if (start_pos < 0 || (s->kv_max_seq > 0 && end > s->kv_max_seq)) return kr_fail(KR_ERR_VALUE, "verify [%d, %d) does not fit kv_max_seq %d", start_pos, end, s->kv_max_seq);
    if (s->max_rope_seq > 0 && end > s->max_rope_seq) return kr_fail(KR_ERR_VALUE, "verify [%d, %d) exceeds the rope table (%d)", start_pos, end, s->max_rope_seq);
    for (const DLayer& L : s->layers)
        if (L.attn == ATTN_MLA && L.mla_rope_seq < end) return kr_fail(KR_ERR_VALUE, "verify [%d, %d) exceeds the MLA rope table (%d)", start_pos, end, L.mla_rope_seq);
    KR_HIP(hipSetDevice(s->eng->device));
    hipStream_t st = kr_pick_stream(s->eng, stream);
    if (int rc = spec_prepare(s, st)) return rc;
    const int n_la = (int)s->spec_la.size();
    const KrSpecLa* tab = (const KrSpecLa*)s->spec_tab.p;
    if (n_la) kr_launch_spec_snapshot(tab, n_la, (int)s->spec_floats, st);
    if (int rc = prefill_impl(s, tokens, n_tokens, start_pos, nullptr, nullptr, stream, true)) {
        if (n_la) kr_launch_spec_rollback(tab, n_la, s->spec_has64, s->spec_has128, s->spec_nv_max, s->spec_dv_max, 0, st);     // back to the snapshot
        return rc;
    }
    int32_t res[KR_VERIFY_MAX + 1];
    KR_HIP(hipMemcpyAsync(res, s->spec_out.p, (size_t)(n_tokens + 1) * 4, hipMemcpyDeviceToHost, st));
    KR_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < n_tokens; i++) greedy_out[i] = res[i];
    *n_match_out = res[n_tokens];
    s->spec_pending = true; s->spec_n = n_tokens; s->spec_match = res[n_tokens]; s->spec_st = st; s->last_stream = st;
    return KR_OK;
}

extern "C" int kr_decode_commit(kr_decode_store* s, int n_keep) {
    if (!s) return kr_fail(KR_ERR_VALUE, "null decode store");
    if (!s->spec_pending) return kr_fail(KR_ERR_STATE, "kr_decode_commit without a pending kr_decode_verify");
    if (n_keep < 1 || n_keep > s->spec_match + 1) return kr_fail(KR_ERR_VALUE, "n_keep %d out of range [1, %d] (n_match %d)", n_keep, s->spec_match + 1, s->spec_match);
    KR_HIP(hipSetDevice(s->eng->device));
    hipStream_t st = s->spec_st;
    const int n_la = (int)s->spec_la.size();
    if (n_keep < s->spec_n && n_la)
        kr_launch_spec_rollback((const KrSpecLa*)s->spec_tab.p, n_la, s->spec_has64, s->spec_has128, s->spec_nv_max, s->spec_dv_max, n_keep, st);
    const size_t V = (size_t)s->vocab;
    KR_HIP(hipMemcpyAsync(s->logits.p, (const float*)s->spec_logits.p + (size_t)(n_keep - 1) * V, V * 4, hipMemcpyDeviceToDevice, st));
    KR_HIP(hipMemcpyAsync(s->tok.p, (const int*)s->spec_out.p + (n_keep - 1), 4, hipMemcpyDeviceToDevice, st));
    KR_HIP(hipGetLastError());
    s->spec_pending = false; s->last_stream = st;
    return KR_OK;
}

// ------------------------------------------------------------------------------------------------
// the multi-sequence pass (kr_decode_multi.cpp, docs/design/13-multi-sequence.md, 17-multi-extend.md): one chunk of n token rows in n_final runs of
// consecutive tokens per slot, row b = a token of slot slots[b] at positions[b]; d_runs = n_final x [slot, off, cnt] after kr_multi.h (a step: runs of one).
// Every row-wise section of run_layer runs unchanged; the linear-attention, GQA and MLA sections take the per-slot kernels (kr_multi.hip).  The last
// token of run i is row i, so the final norm, lm_head GEMM and M.logits cover the first n_final rows only (verify: all n rows, and the linear-attention
// sections leave records instead of state, docs/design/18-multi-verify.md).  Engine buffer set KR_PF_MAX_DEPTH - 1; the
// caller has ordered this pass after everything the store queued.
// ------------------------------------------------------------------------------------------------
// kr_decode_multi_path_counts: one batched pass that was queued, by the values the sections of run_layer branch on -- the plan, the pass's few-row flag, the
// GGUF bits of the store.  The position split is counted where its three launches exist: the launchers (kr_multi.hip) give flash-decode rows the flash-decode
// kernels whatever the flag says, and under the flash or matrix-core run forms they launch the per-row attention for the unit rows only.  Host only
static void multi_path_count(kr_decode_store* s, const KrMultiPlan& pl, bool verify, bool few) {
    int64_t* c = s->path_counts;
    c[KR_MPC_PASSES]++; c[KR_MPC_VERIFY] += verify; c[KR_MPC_FEW] += few;
    c[KR_MPC_XS_SPLIT] += pl.xs_split && !pl.fd_chunks && (pl.gqa_runs == KR_MP_RUNS_ROWS || pl.n_unit > 0);
    c[KR_MPC_MLA_XS_SPLIT] += pl.mla_xs_split && !pl.mla_chunks && (pl.mla_runs == KR_MP_RUNS_ROWS || pl.n_unit > 0);
    c[KR_MPC_GQA_XM] += pl.gqa_runs == KR_MP_RUNS_XM; c[KR_MPC_MLA_XM] += pl.mla_runs == KR_MP_RUNS_XM;
    c[KR_MPC_LX] += pl.lx_nruns > 0; c[KR_MPC_LX_RUNS] += pl.lx_nruns; c[KR_MPC_LX_SHORT] += pl.lx_short;
    c[KR_MPC_FD] += pl.fd_chunks > 0; c[KR_MPC_MLA_FD] += pl.mla_chunks > 0;
    c[KR_MPC_GQA_FLASH] += pl.gqa_runs == KR_MP_RUNS_FLASH; c[KR_MPC_MLA_FLASH] += pl.mla_runs == KR_MP_RUNS_FLASH; c[KR_MPC_LC] += pl.lc_nruns > 0;
    c[KR_MPC_RUNS] += pl.any_run;
    if (has_gguf_moe(s) && (gguf_exact_bits(s) & KR_PF_SET_GGUF_EXACT)) { c[KR_MPC_GGUF_EXACT]++; c[KR_MPC_GGUF_GROUPED] += !(gguf_exact_bits(s) & KR_PF_SET_GGUF_STREAM); }
}
extern "C" int kr_decode_multi_path_counts(kr_decode_store* s, int64_t* out, int n, int reset) {
    if (!s || n < 0 || n > KR_MPC_COUNT || (n > 0 && !out)) return kr_fail(KR_ERR_VALUE, "kr_decode_multi_path_counts: null store, null out or n %d outside [0, %d]", n, (int)KR_MPC_COUNT);
    for (int i = 0; i < n; i++) out[i] = s->path_counts[i];
    if (reset) for (int64_t& c : s->path_counts) c = 0;
    return KR_OK;
}

int kr_multi_pass(kr_decode_store* s, int n, int n_final, const int32_t* d_rows, const int32_t* d_runs, int max_pos, hipStream_t st, bool verify,
                  const int32_t* h_counts, const int32_t* h_positions) {
    kr_multi_state& M = *s->multi;
    PfLayout Lo;
    if (int rc = pf_layout(s, (size_t)n, true, true, st, Lo)) return rc;
    // everything the pass decides, from plain values (kr_multi_plan.h, docs/design/32-multi-pass-plan.md); here: allocation, upload and launch
    KrMultiPlanOpts o{};
    o.opt = s->mopt; o.attn_fast = s->mopt.attn_fast || s->mopt.attn_fast_paged; o.gqa_split_min = s->gqa_split_min; o.mla_split_min = s->mla_split_min;
    o.max_seq = M.max_seq; o.fd_chunk = kr_fd_flash_chunk(M.max_seq); o.mla_chunk = kr_mla_flash_decode_chunk(M.max_seq);
    std::vector<KrMultiPlanLayer> pl_layers;
    for (const DLayer& L : s->layers) pl_layers.push_back(KrMultiPlanLayer{L.attn, L.nh, L.nkv, L.hd, L.klr, L.nv});      // ATTN_* are KR_MP_*
    static_assert(ATTN_NONE == KR_MP_OTHER && ATTN_LA == KR_MP_LA && ATTN_GQA == KR_MP_GQA && ATTN_MLA == KR_MP_MLA, "the plan's layer kinds are the store's");
    KrMultiPlan plan;
    switch (kr_multi_plan(o, pl_layers.data(), (int)pl_layers.size(), KrMultiPlanRows{n, n_final, max_pos, verify, h_counts, h_positions}, plan)) {
    case KR_MP_GQA_CHUNKS: return kr_fail(KR_ERR_VALUE, "multi_attn_fast: position %d needs %d chunks of %d positions (at most 1024)", plan.attn_pos, plan.fd_chunks, plan.fd_chunk);
    case KR_MP_MLA_CHUNKS: return kr_fail(KR_ERR_VALUE, "multi_mla_fast: position %d needs %d chunks of %d positions (at most 1024)", plan.mla_pos, plan.mla_chunks, plan.mla_chunk);
    }
    // the LDS windows of the flash-decode kernels, on the first pass that needs them
    if (plan.fd_chunks && !M.fd_ready) {
        for (const DLayer& L : s->layers) {
            if (L.attn != ATTN_GQA) continue;
            if (!kr_multi_fd_ok(L.nh, L.nkv, L.hd)) return kr_fail(KR_ERR_VALUE, "multi_attn_fast: GQA geometry nh %d nkv %d head_dim %d not covered (head_dim 64 / 128 / 256, at most 32 heads per KV head)", L.nh, L.nkv, L.hd);
            if (kr_multi_fd_prepare(L.hd, M.kv_fp8, M.pg.paged())) return kr_fail(KR_ERR_HIP, "multi_attn_fast: LDS window of the flash-decode kernel refused (head_dim %d)", L.hd);
        }
        M.fd_ready = true;
    }
    if (plan.mla_chunks && !M.mla_fd_ready) {
        for (const DLayer& L : s->layers)
            if (L.attn == ATTN_MLA && kr_multi_mla_fd_prepare(L.klr, M.kv_fp8, M.pg.paged()))
                return kr_fail(KR_ERR_HIP, "multi_mla_fast: LDS window of the flash-decode kernel refused (kv_lora_rank %d)", L.klr);
        M.mla_fd_ready = true;
    }
    if ((plan.fd_chunks || plan.mla_chunks) && (M.fd_o.ensure(plan.fd_o_bytes) || M.fd_ml.ensure(plan.fd_ml_bytes)))
        return kr_fail(KR_ERR_HIP, "hipMalloc of the multi-sequence step's split-KV partials (%zu MiB) failed", (plan.fd_o_bytes + plan.fd_ml_bytes) >> 20);
    if (M.scratch.ensure(Lo.total) || (plan.need_scores && M.scores.ensure(plan.score_bytes)) || M.logits.ensure((size_t)plan.n_logits * s->vocab * 4))
        return kr_fail(KR_ERR_HIP, "hipMalloc of the multi-sequence step's scratch (%zu MiB) failed", (Lo.total + plan.score_bytes + (size_t)plan.n_logits * s->vocab * 4) >> 20);
    if (plan.xm_inv_bytes && M.xm_rows.ensure(plan.xm_inv_bytes + plan.xm_tmax_bytes))
        return kr_fail(KR_ERR_HIP, "hipMalloc of the multi-sequence pass's exact matrix-core attention tables failed");
    if (plan.lc_nruns && M.lc_scratch.ensure(plan.lc_scratch_floats * 4))
        return kr_fail(KR_ERR_HIP, "hipMalloc of the multi-sequence pass's chunked delta-rule scratch (%zu MiB) failed", plan.lc_scratch_floats * 4 >> 20);
    if (!plan.tables.empty()) {      // every table of the pass in one upload
        if (M.tiles.ensure(std::max(plan.tables.size() * 4, (size_t)65536))) return kr_fail(KR_ERR_HIP, "hipMalloc of the multi-sequence pass's query tiles failed");
        KR_HIP(hipMemcpyAsync(M.tiles.p, plan.tables.data(), plan.tables.size() * 4, hipMemcpyHostToDevice, st));      // pageable source: staged before the call returns
    }
    const MultiPass mp{plan, (const int32_t*)M.tiles.p, (float*)M.lc_scratch.p, (float*)M.xm_rows.p, (float*)((char*)M.xm_rows.p + plan.xm_inv_bytes),
                       d_rows, d_rows + 2 * n, d_runs, n_final, verify};
    Chunk cx{};
    const bool few = pass_few_rows(s, n);
    cx.B = pf_carve(Lo, (char*)M.scratch.p); cx.B.H = s->hidden; cx.B.few = few; cx.B.few_group = s->opt_pass_few_rows_group; cx.scores = nullptr; cx.tok = d_rows + n; cx.Cc = n; cx.pos0 = 0; cx.set = KR_PF_MAX_DEPTH - 1;
    cx.first = true; cx.add_is_emb = true; cx.st = st; cx.mp = &mp;
    for (size_t l = 0; l < s->layers.size(); l++)
        if (int rc = run_layer(s, cx, l)) return rc;
    cx.Cc = plan.n_logits;
    if (int rc = final_rows(s, cx, (float*)M.logits.p)) return rc;
    multi_path_count(s, plan, mp.verify, few);
    return KR_OK;
}
