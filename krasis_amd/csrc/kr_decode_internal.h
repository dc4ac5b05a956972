// kr_decode_internal.h -- the decode store's state, shared by kr_decode.cpp (single-token graph) and kr_decode_prefill.cpp (batched prompt)
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <vector>

#include "kr_decode_ops.h"
#include "kr_engine_internal.h"
#include "kr_multi.h"
#include "kr_multi_opts.h"
#include "kr_page_pool.h"
#include "kr_spec.h"

struct DWeight { MatSet ms; int rows = 0, cols = 0; };

enum { ATTN_NONE = 0, ATTN_LA = 1, ATTN_GQA = 2, ATTN_MLA = 3 };
enum { MLP_NONE = 0, MLP_MOE = 1, MLP_DENSE = 2 };

struct DLayer {
    int input_norm = -1, post_norm = -1;
    int attn = ATTN_NONE, mlp = MLP_NONE;
    // LA
    int qkvz_wid = -1, ba_wid = -1, out_wid = -1, nk = 0, nv = 0, dk = 0, dv = 0, kd = 4; float la_scale = 1.0f;
    DevBuf conv_w, a_log, dt_bias, la_norm_w, conv_state, recur_state;
    // GQA
    int q_wid = -1, k_wid = -1, v_wid = -1, o_wid = -1, gated = 0, nh = 0, nkv = 0, hd = 0; float sm_scale = 1.0f;
    DevBuf q_norm, k_norm, kv_k, kv_v; int q_norm_len = 0, k_norm_len = 0;
    // MLA (kv_k = compressed-KV cache [max_seq, klr], kv_v = k_pe cache [max_seq, rd], both FP16)
    int kva_wid = -1, mq_wid = -1, mqa_wid = -1, mqb_wid = -1, klr = 0, nd = 0, rd = 0, vhd = 0, q_a_norm_len = 0;
    DevBuf w_kc, w_vc, kv_a_norm, q_a_norm, mla_cos, mla_sin; int mla_rope_seq = 0;
    // MLP
    int moe_layer = -1, sgu_wid = -1, sd_wid = -1, sg_wid = -1;
    int gate_wid = -1, up_wid = -1, down_wid = -1;
};

// sequence slots of the multi-sequence step (kr_decode_multi.cpp, docs/design/13-multi-sequence.md): per store layer one buffer of n slots --
// linear attention: conv state [n][conv_dim][4] (conv) and recurrent state [n][nv][dk][dv] (recur); GQA: K / V caches [n][max_seq][nkv][hd];
// MLA: compressed-KV rows [n][max_seq][klr] and rope-key rows [n][max_seq][rd] (docs/design/15-multi-mla.md)
struct kr_multi_state {
    int n_slots = 0, max_seq = 0, kv_fp8 = 0;
    std::vector<DevBuf> a, b;                  // per layer: LA conv / recurrent state, GQA K / V, MLA latent / rope-key rows
    std::vector<size_t> a_stride, b_stride;    // per layer: bytes per slot
    std::vector<size_t> a_row, b_row;          // per GQA / MLA layer: bytes of one cache row of a / b (one position; a slot is max_seq of them, a page page_tokens)
    // paged slots (kr_decode_slots_create_paged, docs/design/21-paged-slots.md): a / b of a GQA or MLA layer are then pools [n_pages][page_tokens][row] shared by
    // all slots and a_stride / b_stride the bytes of one page.  pg: the free list, the page table and the queue of mappings the device has not seen yet, all on
    // the host: the pool owns the queue and prunes it whenever entries are given back; pg_flush only carries out its plan.  pg_table: the table's device copy;
    // pg_pools: KrPagePoolDev of every pool; pg_new: the ids of the pages a pass has to zero
    KrPagePool pg; DevBuf pg_table, pg_pools, pg_new; int pg_npools = 0;
    // shared pages (kr_decode_slot_fork, docs/design/22-slot-fork.md): pg_new holds, behind the n_pages ids to zero, [dst | src | rows] of the page copies a pass
    // opens with.  la_pools: KrPagePoolDev of every linear-attention state buffer, a "page" being a slot (flat and paged slots); fk_ids: [dst | src | rows] slots of a fork
    DevBuf la_pools, fk_ids; int la_npools = 0;
    DevBuf rows, ids, logits, scores, scratch; // step: [slots | tokens | positions] (device), greedy ids, [n][vocab] logits, attention scores, the arena
    DevBuf fd_o, fd_ml; bool fd_ready = false; // "multi_attn_fast": split-KV partials [n][nkv][chunks][G][hd] and (max, sum) [n][nh][chunks][2] of one GQA layer, sized by the step's longest row; the kernels' LDS windows are raised
    DevBuf tiles;                              // every tile table of a pass, one upload (kr_multi_plan.h: the plan's vector; its spans are relative to this buffer)
    bool pf_ready = false, mf_ready = false, lc_ready = false;   // "multi_extend_flash" / "multi_extend_mla_flash" / "multi_extend_la_chunk": the LDS windows of the run kernels are raised (kr_option_rules, once per slot set)
    DevBuf lc_scratch;                         // "multi_extend_la_chunk": the rule's scratch of one layer, sized by the pass's sub-chunks
    DevBuf xm_rows;                            // "multi_extend_exact_mfma" / "multi_extend_mla_exact_mfma": 1 / sum [n * nh] and the row maxima per 32 positions [n * nh][sc_ld / 32] of the pass's score rows
    bool mla_fd_ready = false;               // "multi_mla_fast": the partials of one MLA layer, [n][chunks][nh][klr] and [n][nh][chunks][2], share fd_o / fd_ml (sized for the larger need); the kernels' LDS windows are raised
    // per-slot samplers (kr_decode_slot_sampler, docs/design/14-multi-sampling.md): allocated for every slot on the first call; empty = every slot greedy
    struct Sampler { float temperature = 0.0f, top_p = 1.0f, penalty = 0.0f; int top_k = 0; };
    std::vector<Sampler> smp; size_t smp_words = 0;   // host: parameters per slot; seen-bitmap words per slot
    DevBuf smp_seen, smp_rng;                  // [n_slots][smp_words] seen-token bitmaps, [n_slots] xorshift64 states
    DevBuf smp_rows, smp_work, smp_sorted, smp_keys, smp_temp, smp_probs; size_t smp_temp_bytes = 0;   // a sampled step: KrMsRow [n] (a sampled verify: then KrMsAt [n]), prepared rows, top-k keys, per-row path scratch
    DevBuf smp_hyp;                            // a sampled verify's per-row path: one staged seen bitmap [smp_words] + xorshift64 state (docs/design/19-multi-verify-sample.md)
    // verify over slots (kr_decode_verify_multi / kr_decode_commit_multi, docs/design/18-multi-verify.md): what the verify-form linear-attention launches
    // recorded (one allocation, a slice per layer, sized by the call's token rows), the table of those layers on the host and the device (v_la_of[store layer] =
    // its entry), [greedy ids in caller order | n_match], the commit's n_keep.  v_pending: the rows of the last verify wait for their commit -- the run table
    // in `rows` and the records are theirs until then; v_sampled: it drew with the slots' samplers (smp_rows and ids are its too: the commit applies the kept draws)
    DevBuf v_rec, v_tab, v_out, v_keep; std::vector<KrMultiLaCommit> v_host; std::vector<int> v_la_of;
    bool v_pending = false, v_sampled = false, v_has64 = false, v_has128 = false; int v_nv_max = 0, v_dv_max = 0; size_t v_rows = 0;
    std::vector<int32_t> v_match; hipStream_t v_st = nullptr;
    hipEvent_t ev = nullptr;
    // slot export / import (kr_decode_slots_export / _import, docs/design/38-slot-swap.md), allocated on the first call: sw_stage = the device staging buffer and
    // sw_pinned the pinned host buffer, two halves of sw_half bytes each; sw_stream carries the copies between them while the call's stream packs or unpacks the
    // other half; sw_ev[h] = half h has been packed / unpacked, sw_ev[2 + h] = half h has been copied; sw_pools = KrPagePoolDev of every buffer a piece names
    // (kr_slot_image.h: 2 per store layer, then the samplers' states and seen bitmaps), sw_pieces = the pieces of one call
    DevBuf sw_stage, sw_pools, sw_pieces; void* sw_pinned = nullptr; size_t sw_half = 0; hipStream_t sw_stream = nullptr; hipEvent_t sw_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    ~kr_multi_state() {
        if (ev) (void)hipEventDestroy(ev);
        for (hipEvent_t e : sw_ev) if (e) (void)hipEventDestroy(e);
        if (sw_stream) (void)hipStreamDestroy(sw_stream);
        if (sw_pinned) (void)hipHostFree(sw_pinned);
    }
};

struct kr_standalone_state;   // kr_decode_standalone.cpp: staging buffers, stand-alone router gates, cancel flag, elapsed time
struct kr_decode_store {
    kr_standalone_state* standalone = nullptr;
    kr_engine* eng = nullptr; int device = 0; bool own_eng = false;   // own_eng: a bare engine made by kr_decode_create(NULL, ...), replaced by kr_decode_set_moe_store
    int group_size = 128; bool norm_bias_one = false;
    std::vector<std::unique_ptr<DWeight>> weights;
    std::vector<std::unique_ptr<DevBuf>> norms; std::vector<int> norm_len;
    bool configured = false;
    int hidden = 0, n_layers = 0, vocab = 0, topk = 0, scoring = 1, norm_topk = 1, final_norm = -1, lm_head = -1;
    float eps = 1e-6f, rsf = 1.0f;
    DevBuf embedding;
    std::vector<DLayer> layers;
    DevBuf rope_cos, rope_sin; int rope_half = 0, max_rope_seq = 0;
    int kv_max_seq = 0;
    // scratch
    DevBuf hid, res, proj_a, proj_b, qbuf, kbuf, vbuf, zbuf, gbuf, betabuf, gatebuf, latbuf, recur_out, attn_out, logits, gate_val, tok;
    DevBuf dense_gu;  // [gate(K) | up(K)] of the dense MLP; only [0,inter) of each half is ever written, the padding stays 0
    DevBuf hid2, res2, r_counter, argmax_scratch;
    int kv_fp8 = 0;            // GQA KV element type: 0 FP16 (reference CPU decode), 1 FP8-E4M3 (reference GPU cache dtype)
    DevBuf img_in, img_post, img_post_bf16, img_attn;   // pre-built INT16 activation images (input norm, post-attention norm f32 / bf16, attention output)
    int opt_gqa_stream = 0, opt_pfm_timing = 0, opt_norm_rows = 1, opt_la_conv_fused = 1, opt_gqa_fused = 1, opt_lm_fused = 1, opt_la_heads = 1, opt_w2_combine = 1, opt_dense_fast = 1, opt_slot_select = 1, opt_slot_rows_late_first = 1;   // kr_decode_set_option: test / tuning hooks (no environment lookups on launch paths)
    int opt_multi_sample_loop = 0;               // kr_decode_set_option("multi_sample_loop"): every sampled row of a multi-sequence step takes the single-row sampler, one row after another (A/B and test hook; same tokens)
    int opt_gguf_exact_pass = 0;                 // kr_decode_set_option("gguf_exact_pass"): every multi-row pass runs native-GGUF MoE layers through the exact forms (KR_PF_SET_GGUF_EXACT, docs/design/20-gguf-exact-pass.md): a row carries the bits of kr_decode_step, and the slot / speculation entry points accept such a store
    int opt_gguf_exact_grouped = 1;              // ... 0 = through the streaming kernels for every block type (A/B and test hook; same bits)
    KrMultiOpts mopt;                            // kr_decode_set_option("multi_..."): the opt-in forms of the batched pass over device slots, each described on its field (kr_multi_opts.h)
    int opt_pass_few_rows = 0;                   // kr_decode_set_option("pass_few_rows"): a multi-row pass of at most opt_pass_few_rows_max token rows (prefill / verify: n_tokens; slot entry points: the sum of the counts) runs its projections on the few-row streaming matvec (kr_rows_matvec.hip) and its INT4 / INT8 routed experts as the decode step's three launches -- bit for bit what it gives without the option (docs/design/34-pass-few-rows.md); KR_GEMM_FAST passes and larger passes keep their GEMMs
    int opt_pass_few_rows_max = 16;              // kr_decode_set_option("pass_few_rows_max"), 1 .. 16: the most token rows of a pass that takes the few-row kernels (a measured default: profiles/pass_few_rows.txt)
    int opt_pass_few_rows_group = 0;             // kr_decode_set_option("pass_few_rows_group"), 0 .. 16: the most rows a workgroup of the few-row matvec holds, 0 = chosen per launch (kr_rows_plan.h; A/B and test hook, same bits)
    int opt_slot_swap_chunk_bytes = KR_SLOT_CHUNK_DEFAULT;   // kr_decode_set_option("slot_swap_chunk_bytes"), a multiple of 16 and at least 1024: the bytes of one staging half of slot export / import (docs/design/38-slot-swap.md; a measured default: profiles/slot_swap.txt)
    int64_t path_counts[KR_MPC_COUNT] = {};     // kr_decode_multi_path_counts: which forms the multi-row passes took (host-side test aid; written where a pass has been queued, read by nothing)
    int opt_gen_lookahead = 0;                  // kr_decode_set_option("generate_lookahead"): generate_batch feeds the sampled token back ON THE DEVICE and queues step i + 1 before the host has read token i
    int opt_ep_graph = 0;                         // kr_decode_set_option("ep_graph"): expert-parallel decode over RCCL replays a captured graph (the all-reduce is captured with the kernels)
    uint64_t ep_generation_seen = 0;               // kr_engine::ep_generation at the last step: a new / destroyed communicator invalidates the graph and restarts the warm-up
    int ep_eager_steps = 0;                        // expert-parallel decode: steps enqueued eagerly so far (RCCL warms up outside any capture)
    int* gen_ring = nullptr; int gen_ring_n = 0; hipEvent_t gen_ev[2] = {nullptr, nullptr};   // pinned token ring + events of the look-ahead loop
    int decode_fast = 0; DevBuf f_qk;         // KR_DECODE_FAST: decode steps on the tolerance-mode kernels (kr_decode_fast.hip); f_qk = conv outputs [nk][q(dk) | k(dk)]
    int gemm_fast = 0;                        // KR_GEMM_FAST: prompt-pass GEMMs in the tolerance form (kr_prefill_h.hip)
    int attn_fast = 0; DevBuf fd_o, fd_ml;   // KR_ATTN_FAST: split-KV softmax + p.v with a log-sum-exp merge for long caches (tolerance mode)
    DevBuf gqa_scores; int gqa_split_min = 1024, mla_split_min = 512;   // caches longer than this split decode attention into a scores launch + softmax / p.v launch
    DevBuf smp_seen, smp_keys, smp_temp, smp_probs, smp_rng; size_t smp_temp_bytes = 0;   // sampler: seen bitmap, sort keys / scratch, probabilities, xorshift64 state
    DevBuf pf_scores;          // kr_decode_prefill: attention scores [chunk*nh rows][context] f32
    DevBuf pf_vlogits, pf_nll; // kr_decode_prefill_nll: [chunk, vocab] logits per arena; per-position negative log-likelihoods
    DevBuf pf_tokens; int pf_chunk = 0; int pf_depth = 0; std::vector<hipStream_t> pf_side; std::vector<hipEvent_t> pf_events;   // prompt pass: token ids, chunk size, second stream
    DevBuf pf_scratch;         // kr_decode_prefill: one arena for the chunk buffers
    DevBuf moe_gu, moe_eo, r_logits, r_ids, r_w;  // store-owned so a captured graph never sees them reallocated
    DevBuf step_dev; hipStream_t last_stream = nullptr;   // stream of the most recent step / prompt pass (kr_decode_last_token waits on it)
    size_t weight_bytes = 0;
    // exact speculative decoding (kr_decode_verify / kr_decode_commit, kr_decode_prefill.cpp): per linear-attention layer the snapshot of its states and
    // what a verify pass fed the recurrence (spec_la[i] = the store layer of table entry i), the all-row logits, [greedy ids, n_match], accept partials
    std::vector<int> spec_la, spec_la_of; std::vector<KrSpecLa> spec_host; DevBuf spec_buf, spec_tab, spec_logits, spec_out, spec_part;
    std::unique_ptr<kr_multi_state> multi;       // sequence slots + the multi-sequence step's buffers (kr_decode_slots_create)
    bool spec_pending = false; int spec_n = 0, spec_match = 0, spec_nv_max = 0, spec_dv_max = 0; bool spec_has64 = false, spec_has128 = false; size_t spec_floats = 0; hipStream_t spec_st = nullptr;
    // captured graph of one decode step
    hipGraphExec_t graph_exec = nullptr; bool graph_ok = false; bool use_graph = true;
    // profiling pass (kr_decode_profile_step): HIP events around every launch, accumulated per kernel kind
    bool prof = false; std::vector<hipEvent_t> ev_pool; size_t ev_used = 0; std::vector<int> ev_kind;
};

enum { PK_EMBED = 0, PK_RMSNORM, PK_MATVEC, PK_LA_CONV, PK_LA_RECUR, PK_GATED_NORM, PK_GQA, PK_ROUTE_LOGITS, PK_ROUTE_SELECT, PK_MOE_W13,
       PK_MOE_W2, PK_MOE_COMBINE, PK_LM_HEAD, PK_ARGMAX, PK_SHARED_GATE, PK_OUT_PROJ /* KR_DECODE_FAST: the out / o projection from the attention image (its own kernel instantiation) */, PK_COUNT };


static inline KrMatDev mv(kr_decode_store* s, int wid) { return s->weights[wid]->ms.view(); }
int kr_ensure_wsum(kr_engine* e, MatSet& ms, hipStream_t st);
int kr_moe_prefill_prepare(kr_engine* e, int layer, int fast, int routed_only, hipStream_t st, int gguf_exact = 0);   // kr_engine.cpp: the lazily derived data of a native-GGUF layer, built on `st` now
void kr_standalone_release(kr_decode_store* s);
int kr_exact_refuse(kr_decode_store* s, bool slots);   // kr_decode_prefill.cpp: KR_OK when an exact pass can run on this store -- speculative decoding on its own sequence, or (slots) the multi-sequence step
int kr_spec_refuse(kr_decode_store* s);          // kr_exact_refuse(s, false)
bool paged_refused(const kr_decode_store* s);    // kr_decode_prefill.cpp: paged slots under "multi_attn_fast" alone -- what paged_refuse (kr_decode_multi.cpp) refuses and the rules of kr_option_rules stand back for
int kr_option_rules(kr_decode_store* s, bool prepare);   // kr_decode_prefill.cpp: the one walk of the slot options' ordered rule list, behind kr_exact_refuse(s, true) -- its refusals, or (prepare, once they have all passed) the LDS windows of the options that are set
bool has_attn(const kr_decode_store* s, int kind);   // kr_decode_prefill.cpp: the store has a layer of this attention kind (ATTN_*)
int kr_spec_pending_fail(kr_decode_store* s);    // KR_ERR_STATE while a verify waits for its commit
int kr_standalone_cancelled(kr_decode_store* s);
// kr_decode_prefill.cpp: the layers + final norm + lm_head GEMM of the multi-sequence pass on `st` in s->multi's arena: n_rows token rows in n_runs runs of
// consecutive tokens per slot (a step: runs of one).  d_rows = [slots | tokens | positions] of n_rows each on the device, the last token of run i in row i;
// d_runs = n_runs x [slot, off, cnt] (kr_multi.h); logits of the first n_runs rows -> s->multi->logits [n_runs][vocab].  verify: the linear-attention layers
// take the verify form (no state stored; records into the layers of s->multi->v_host), and the logits of all n_rows rows -> s->multi->logits [n_rows][vocab]
// h_counts / h_positions (host, optional): the n_runs run lengths and first positions as the caller gave them -- what the plan (kr_multi_plan.h) builds the
// tables of the run options from and sizes the per-row kernels' scratch by; null counts: every run has one token
int kr_multi_pass(kr_decode_store* s, int n_rows, int n_runs, const int32_t* d_rows, const int32_t* d_runs, int max_pos, hipStream_t st, bool verify = false,
                  const int32_t* h_counts = nullptr, const int32_t* h_positions = nullptr);
void kr_standalone_set_elapsed(kr_decode_store* s, double sec);   // kr_engine.cpp: per (group, column) nibble sums for the int8-MFMA GEMM
