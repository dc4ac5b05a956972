/*
 * krasis_hip.h -- C ABI of libkrasis_hip.so: the MI355X (gfx950) quantized-MoE hot path.
 *
 * This is the drop-in boundary.  Each entry point names the reference
 * interface it replaces (paths relative to the brontoguana/krasis checkout).  The reference's
 * own FFI for this path is PyO3 (Rust <-> Python, raw `usize` pointers); a maintainer binds
 * these symbols from Rust with a plain `extern "C"` block (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; kr_last_error() gives the text.
 *     The Python mirror maps codes to the reference's exception classes
 *     (KR_ERR_STATE -> RuntimeError, KR_ERR_VALUE -> ValueError, KR_ERR_IO -> IOError).
 *   - "dev" pointers are HBM addresses on the engine's device, "host" pointers are CPU addresses.
 *     Entry points that take activations accept either: host pointers are staged through the
 *     engine's pinned bounce buffers (the reference passes host addresses, moe.rs:2843-2853).
 *   - `stream` is a hipStream_t cast to void*; NULL = the engine's own (non-blocking) stream, (void*)1 = the legacy default
 *     stream (what a framework reports as stream 0).  Device-pointer outputs are ready when that stream reaches the call.
 *   - no torch types, no Python callbacks; every entry point may be called without the GIL.
 */
#ifndef KRASIS_HIP_H
#define KRASIS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KR_OK 0
#define KR_ERR_STATE 1 /* PyRuntimeError in the reference ("Model not loaded -- call load() first", moe.rs:1783) */
#define KR_ERR_VALUE 2 /* PyValueError (shape/size errors, moe.rs:1790-1803) */
#define KR_ERR_IO 3    /* PyIOError */
#define KR_ERR_HIP 4   /* HIP runtime failure */

/* expert weight formats (SURVEY §8 path matrix) */
#define KR_FMT_INT4_G128 4   /* quantize_int4, marlin.rs:145; CPU transposed layout weights/mod.rs:329 */
#define KR_FMT_INT8_G128 8   /* quantize_int8, marlin.rs:65 */
/* raw GGUF block types use the GGML ids (gguf.rs:15-31): Q4_0=2 Q5_0=6 Q8_0=8 Q4_K=12 Q6_K=14 */
#define KR_GGML_Q4_0 2
#define KR_GGML_Q5_0 6
#define KR_GGML_Q8_0 8
#define KR_GGML_Q4_K 12
#define KR_GGML_Q6_K 14

#define KR_MAX_TOPK 32 /* moe.rs:2899 */

/* output dtype of kr_moe_forward */
#define KR_OUT_F32 0  /* KrasisEngine.moe_forward returns f32 bytes (moe.rs:1863) */
#define KR_OUT_BF16 1 /* forward_moe_direct / sync_forward return bf16 RNE (moe.rs:2947) */

typedef struct kr_engine kr_engine;

const char* kr_last_error(void);
int kr_version(void);
/* measurement aid (no reference counterpart): device allocations the library has made so far, process-wide.  bench.py reads it on both sides of
   every timed region and refuses a measurement that allocated (an allocation synchronises the device). */
long kr_alloc_count_total(void);

/* ---- engine lifetime: KrasisEngine::new / load (moe.rs:1435-1760) ---- */
typedef struct {
    int hidden_size;            /* ModelConfig, weights/mod.rs:51-70 */
    int moe_intermediate_size;
    int n_routed_experts;
    int num_experts_per_tok;
    int num_moe_layers;
    int n_shared_experts;       /* shared intermediate = n_shared * moe_intermediate */
    int group_size;             /* 128 (marlin.rs:12) */
    float routed_scaling_factor;
    float swiglu_limit;         /* 0 = SiLU; 7.0 = GPT-OSS (weights/mod.rs:159-166) */
    float activation_alpha;
} kr_model_config;

int kr_engine_create(int device_ordinal, const kr_model_config* cfg, kr_engine** out);
void kr_engine_destroy(kr_engine* e);
int kr_engine_get_config(const kr_engine* e, kr_model_config* out);
size_t kr_engine_device_bytes(const kr_engine* e);

/* ---- weight upload.  Host arrays are in the REFERENCE layouts; the library re-tiles them into its
 *      own HBM layout.  expert = -1 uploads the layer's shared expert. ---- */
/* UnifiedExpertWeights CPU transposed format (weights/mod.rs:287-322):
 *   bits 4: w13 u32 [H/8, 2I], w2 u32 [I/8, H];  bits 8: w13 i8 [H, 2I], w2 i8 [I, H]
 *   scales bf16 [H/gs, 2I] and [I/gs, H].  `inter` is this expert's intermediate size. */
int kr_upload_expert_unified(kr_engine* e, int layer, int expert, int inter,
                             const void* w13, const uint16_t* w13_scales, int w13_bits,
                             const void* w2, const uint16_t* w2_scales, int w2_bits);
/* GgufExpertWeights (weights/mod.rs:252-266): raw blocks, gate/up [inter, hidden], down [hidden, inter] */
int kr_upload_expert_gguf(kr_engine* e, int layer, int expert, int inter,
                          const uint8_t* gate, const uint8_t* up, int gate_up_type,
                          const uint8_t* down, int down_type);
/* load_from_hf (weights/mod.rs:1181 -> load_and_quantize_expert -> weights/marlin.rs:65,145): BF16 tensors of one expert in the HF
 * checkpoint layout -- gate, up [inter, hidden], down [hidden, inter], row-major, host or device pointers -- quantized on the GPU with
 * the reference's rule (scale = bf16(amax/7 | amax/127), q = clamp(round(v * (1/scale)))) and stored in the resident layout.
 * expert = -1: the shared expert (inter = n_shared_experts * moe_intermediate_size). */
int kr_upload_expert_bf16(kr_engine* e, int layer, int expert, int inter, const uint16_t* gate, const uint16_t* up, const uint16_t* down,
                          int w13_bits, int w2_bits);
/* Fill a layer's routed experts (and shared, if configured) with device-generated pseudo-random INT4/INT8
 * words and bf16 scales in [0.005,0.05] -- the distribution of bench_decode_synthetic (decode.rs:4379-4392),
 * generated by a counter hash on the GPU instead of one serial xorshift stream. */
int kr_fill_layer_synthetic(kr_engine* e, int layer, int bits, uint64_t seed);
/* the native-GGUF twin: every routed expert of the layer as Q4_K (12) / Q8_0 (8) blocks with the block distribution SURVEY 8d defines
 * (raw quant / scale bytes, d = f16((0.005 + u * 0.045) / 63), dmin = f16(8 d); Q8_0: d = f16((0.005 + u * 0.045) / 127)) */
int kr_fill_layer_synthetic_gguf(kr_engine* e, int layer, int gate_up_type, int down_type, uint64_t seed);
/* Read one expert back in the reference layout (inverse re-tiling); used by parity tests at full size. */
int kr_download_expert_unified(kr_engine* e, int layer, int expert, void* w13, uint16_t* w13_scales,
                               void* w2, uint16_t* w2_scales);

/* ---- the reference's Marlin GPU layout: marlin_repack / marlin_repack_int8 (src/weights/marlin.rs:256-491, :587-758), undone
 *      in the reference by inverse_marlin_repack / inverse_scale_permute (python/krasis/triton_moe.py:71-170).  Host-side conversions only -- no
 *      CDNA kernel consumes this layout.  row-major: packed [N, K/8] u32 (INT4, nibble = q + 8, LSB = lowest k) or [N, K] i8 (INT8), scales bf16
 *      [N, K/gs];  Marlin: packed [K/16, 2N] (INT4) / [K/16, 4N] (INT8) u32, scales bf16 [K/gs, N] permuted.  N % 64 == 0, K % 16 == 0. ---- */
int kr_marlin_repack(const void* rowmajor, const uint16_t* scales, int N, int K, int group_size, int bits, uint32_t* out_packed, uint16_t* out_scales);
int kr_marlin_unpack(const uint32_t* marlin_packed, const uint16_t* marlin_scales, int N, int K, int group_size, int bits, void* out_rowmajor, uint16_t* out_scales);
/* one expert in the Marlin GPU format of UnifiedExpertWeights::from_expert_weights_marlin_* (weights/mod.rs:506-640): w13 = repack(gate rows || up
 * rows), w2 = repack(down) with N padded per marlin_w2_padded_n (weights/mod.rs:942-949); what the reference's disk cache holds (:856-934) and
 * what KrasisEngine.get_expert_w13_packed / _scales / get_expert_w2_packed / _scales return (moe.rs:1972-2090) */
int kr_upload_expert_marlin(kr_engine* e, int layer, int expert, int inter, const uint32_t* w13_packed, const uint16_t* w13_scales,
                            const uint32_t* w2_packed, const uint16_t* w2_scales, int bits);
int kr_download_expert_marlin(kr_engine* e, int layer, int expert, uint32_t* w13_packed, uint16_t* w13_scales, uint32_t* w2_packed, uint16_t* w2_scales);

/* ---- MoE forward: moe_forward_unified / moe_forward_gguf (moe.rs:572, 990) behind
 *      KrasisEngine.moe_forward (moe.rs:1775), forward_moe_direct (moe.rs:2843), submit/sync_forward (:2723).
 *   act  bf16 [batch, hidden]; ids i32 [batch, topk] (-1 = skip, moe.rs:2904); w f32 [batch, topk]
 *   out  f32 or bf16 [batch, hidden].  routed_only != 0 omits shared expert and rsf (gpu_prefill.py:4467). */
int kr_moe_forward(kr_engine* e, int layer, const void* act_bf16, const int32_t* ids, const float* weights,
                   void* out, int batch, int topk, int out_dtype, int routed_only, void* stream);

/* ---- prefill: GpuPrefillManager.forward(moe_layer_idx, hidden[M,H] bf16, topk_ids[M,k] i32, topk_weights[M,k] f32, routed_only)
 *      (python/krasis/gpu_prefill.py:4374-4394).  All pointers are device pointers.  Token sort + int8-MFMA grouped GEMM; every row
 *      carries the arithmetic of expert_forward_unified (moe.rs:184), so the result equals kr_moe_forward on the same batch bit for bit.
 *      out = rsf*routed + shared unless routed_only (gpu_prefill.py:4467-4484).
 *      Native-GGUF layers (kr_upload_expert_gguf): Q4_K / Q8_0 blocks run on the same matrix cores -- raw super-blocks staged in LDS, one
 *      int8 MFMA per 32-wide sub-block and activation digit, the per-sub-block scale / min epilogue of gguf_kernels.rs:271-432 -- with ONE
 *      f32 chain per output instead of the AVX2 kernel's eight lane chains: equal to kr_moe_forward within ~1e-6 relative (stated in
 *      tests/test_gguf_gpu.py), not bit for bit; Q4_0 / Q5_0 / Q6_K layers walk the batch through the bit-exact streaming kernels. ---- */
int kr_moe_prefill(kr_engine* e, int layer, const void* x_bf16, const int32_t* ids, const float* weights, void* out, int M, int topk,
                   int out_dtype, int routed_only, void* stream);

/* ---- routing: set_routing_config / set_routing_weights / forward_moe_routed (moe.rs:2959-3246) ---- */
#define KR_SCORE_SIGMOID 0 /* decode.rs scoring_func codes (decode.rs:1955-1969) */
#define KR_SCORE_SOFTMAX 1
#define KR_SCORE_TOPK_SOFTMAX 2
#define KR_ROUTE_RULE_ENGINE 0 /* bf16 gate x bf16 act, sequential f32, iterative argmax (moe.rs:3088-3236) */
#define KR_ROUTE_RULE_DECODE 1 /* f32 gate x f32 hidden, 2x8-lane fma, heap top-k (decode.rs:1385-1535,4088) */
int kr_set_routing_config(kr_engine* e, int scoring, int norm_topk_prob, int topk, int n_experts, int hidden);
/* gate: bf16 [E,H] when gate_is_f32 == 0 else f32 [E,H]; bias / e_score_corr f32 [E] or NULL (host pointers) */
int kr_set_routing_weights(kr_engine* e, int layer, const void* gate, int gate_is_f32, const float* bias,
                           const float* e_score_corr);
/* bench_decode_synthetic's router gate (decode.rs:5181: fill_random_f32(route_data, rng, 0.02) over Xorshift64, decode.rs:4356-4376), generated
 * by the library's host side; round_bf16 != 0 truncates each value to bf16 like a checkpoint's gate tensor (stored as bf16 in HBM) */
int kr_set_routing_weights_synthetic(kr_engine* e, int layer, uint64_t seed, float amp, int round_bf16);
/* x: bf16 [m,H] (rule ENGINE) or f32 [m,H] (rule DECODE); ids_out i32 [m,topk]; w_out f32 [m,topk] */
int kr_route_topk(kr_engine* e, int layer, const void* x, int m, int rule, int32_t* ids_out, float* w_out,
                  float* logits_out /* optional f32 [m,E] */, void* stream);
/* forward_moe_routed (moe.rs:3050): act bf16 [1,H] -> out bf16 [1,H], router + experts */
int kr_forward_moe_routed(kr_engine* e, int layer, const void* act_bf16, void* out_bf16, void* stream);

/* ---- reduce_sum_bf16 (moe.rs:2505): N-way bf16 sum, f32 accumulate in input order, RNE ---- */
int kr_reduce_sum_bf16(kr_engine* e, const void* const* inputs, int n_inputs, void* out, size_t n, void* stream);

/* test / tuning hook: (token, slot) pairs per pass of kr_moe_prefill (0 = default 81 920: 8192 tokens of a top-10 model, 81 920 top-1 rows
 * of the expert-parallel dispatch); larger batches are walked in passes of pairs / topk tokens */
int kr_moe_set_prefill_pairs(kr_engine* e, int pairs);
/* numerics of the prompt-pass expert GEMMs of kr_moe_prefill: 0 (default) = the CPU engine's arithmetic (INT16 activation digits, one f32 fma per
 * 128-group: bit-identical to kr_moe_forward, moe.rs:184); 1 = tolerance form: f16 activations x weights de-quantized in registers, f32 accumulation
 * over the whole k range -- the dataflow of the reference's GPU prompt pass (gpu_prefill.py:64-239, Marlin).  Native GGUF layers stay exact.
 * 3 = the tolerance form on the register-staged kernels only (the LDS-ring kernel of kr_prefill_ring.hip off, process-wide): A/B and test hook,
 * results are bit-identical to mode 1; 5 = the ring kernel for every shape it takes, not only problems that fill the chip (test hook, same bits). */
int kr_moe_set_gemm_mode(kr_engine* e, int fast);
/* expert-parallel combine: out[t] = sum_s w[t][s] * eo_rows[pair_row[t][s]] in routing order (moe.rs:661-667); pair_row -1 = skip */
int kr_combine_rows(kr_engine* e, const float* eo_rows, const int32_t* pair_row, const float* weights, void* out, int M, int topk,
                    int out_dtype, void* stream);

/* ---- expert parallelism over RCCL inside the library (reference dataflow python/krasis/gpu_prefill.py:353-359,4140-4148 +
 *      python/krasis/model.py:3131-3241).  One process per GPU; rank r's engine is configured with ITS experts only (contiguous slice
 *      [r * floor(E/R), ...), the last rank takes the remainder) as local experts 0..n_local-1.  kr_moe_prefill_ep takes this rank's SHARD of
 *      the tokens with GLOBAL expert ids: every (token, slot) row travels once to the rank that owns its expert (ncclSend / ncclRecv groups
 *      -- xGMI is a full mesh, no ring), runs through that rank's expert GEMMs and returns; the source rank combines its rows in routing
 *      order.  With f32 return rows the result equals single-GPU kr_moe_prefill bit for bit; return_bf16 halves the return bytes for one
 *      extra rounding per row.  Bootstrap: rank 0 calls kr_ep_unique_id, the host carries the 128 bytes to the other ranks. ---- */
int kr_ep_unique_id(void* id_out128);
int kr_ep_init(kr_engine* e, int world, int rank, int n_experts_total, const void* id128 /* NULL when world == 1 */, int return_bf16);
int kr_ep_destroy(kr_engine* e);
int kr_moe_prefill_ep(kr_engine* e, int layer, const void* x_bf16, const int32_t* ids_global, const float* weights, void* out, int M, int topk,
                      int out_dtype, int routed_only, void* stream);   /* COLLECTIVE: every rank calls, same layer order; M == 0 (empty shard, NULL pointers) is valid and still takes part */
int kr_ep_comm_ranks(kr_engine* e, int* n_out);                        /* ranks of this engine's communicator as RCCL counts them (ncclCommCount) */
int kr_ep_max_int(kr_engine* e, int value, int* max_out, void* stream);                /* collective: max of `value` over the ranks (kr_decode_prefill pads ranks with fewer chunks) */
int kr_ep_allreduce_f32(kr_engine* e, float* buf_dev, size_t n, void* stream);         /* collective: in-place f32 sum over the ranks (expert-parallel decode step) */
/* Expert-parallel DECODE: a decode store whose engine has expert parallelism initialised (world > 1) runs kr_decode_step as a collective -- router,
 * attention, norms and the shared expert replicated on every rank, the routed experts of the rank's slice only, one f32 all-reduce of the k expert rows
 * ([k, hidden]; each row is non-zero on exactly one rank, so the result equals single-engine decode bit for bit) per MoE layer before the combine in
 * routing order.  The steps are enqueued eagerly (no hipGraph replay) and KR_DECODE_FAST is ignored on such stores. */
/* loopback transport: W virtual ranks = W engines of ONE process (normally on one device), every rank driven by its own host thread while a
 * collective call is in flight; the exchanges are hipMemcpyAsync pulls between the engines' buffers bracketed by host barriers.  It runs the
 * SAME split-size / offset / scatter code as the RCCL transport, so a single-GPU box can check world sizes 2, 3 (remainder slice), 8
 * against single-engine execution (tests/test_ep_gpu.py).  Not a performance path. */
typedef struct kr_ep_loop_group kr_ep_loop_group;
int kr_ep_loopback_create(int world, kr_ep_loop_group** out);
int kr_ep_loopback_destroy(kr_ep_loop_group* g);   /* refused (non-zero, group intact) while engines initialised on it have not been through kr_ep_destroy */
int kr_ep_init_loopback(kr_engine* e, kr_ep_loop_group* group, int rank, int n_experts_total, int return_bf16);

int kr_synchronize(kr_engine* e);

/* ================================================================================================
 * Decode graph: CpuDecodeStore (src/decode.rs:193-3602) with every weight, KV page and recurrent state in HBM.
 * Construction mirrors the reference's builder methods; pointer arguments keep their meaning (HOST f32/u16 buffers,
 * copied to the device).  decode_step is a fixed launch sequence replayed as a hipGraph.
 * ================================================================================================ */
typedef struct kr_decode_store kr_decode_store;
/* CpuDecodeStore(group_size=128, parallel=True, norm_bias_one=False)  decode.rs:229.  e may be NULL: the reference constructs the store first
 * and binds the engine LAST (set_moe_store, decode.rs:2250; decode_setup.py:1010); the store then runs on the current HIP device until
 * kr_decode_set_moe_store hands it the engine that owns the routed experts and routers (same device). */
int kr_decode_create(kr_engine* e, int group_size, int norm_bias_one, kr_decode_store** out);
int kr_decode_create_on(int device_ordinal, int group_size, int norm_bias_one, kr_decode_store** out);   /* the same, bare engine on the NAMED device (multi-GPU hosts) */
int kr_decode_set_moe_store(kr_decode_store* s, kr_engine* e);
void kr_decode_destroy(kr_decode_store* s);
/* store_weight_f32(ptr, rows, cols, bits) -> id (decode.rs:280): f32 [rows, cols] -> quantize_f32_to_transposed_int4/8
 * (decode.rs:46,115; scale = amax/7, q = round(v * 7/amax)) -> HBM */
int kr_decode_store_weight_f32(kr_decode_store* s, const float* w, int rows, int cols, int bits, int* id_out);
/* fake_transposed_weight (decode.rs:4480): random packed words + bf16 scales in [0.005,0.05], generated on the GPU */
int kr_decode_store_weight_synthetic(kr_decode_store* s, int rows, int cols, int bits, uint64_t seed, int* id_out);
/* read a stored weight back in the reference layout: packed [cols/8, rows] u32 (or [cols, rows] i8), scales [cols/128, rows] */
int kr_decode_download_weight(kr_decode_store* s, int wid, void* packed_t, uint16_t* scales_t);
int kr_decode_store_norm_weight(kr_decode_store* s, const float* w, int n, int* id_out);            /* decode.rs:430 */
/* configure_decode (decode.rs:1955): scoring 0 sigmoid / 1 softmax / 2 topk-softmax; embedding f32 [vocab, hidden] on the
 * host, or NULL for a GPU-generated +-0.1 table (decode.rs:5364) from synth_seed */
int kr_decode_configure(kr_decode_store* s, int hidden, int n_layers, float eps, int final_norm_id, int lm_head_wid, int vocab,
                        int topk, int scoring, int norm_topk_prob, float routed_scaling_factor, const float* embedding,
                        uint64_t synth_seed);
int kr_decode_add_la_layer(kr_decode_store* s, int input_norm_id, int post_attn_norm_id, int in_proj_qkvz_wid, int in_proj_ba_wid,
                           int out_proj_wid, const float* conv_weight, const float* a_log, const float* dt_bias,
                           const float* norm_weight, int nk, int nv, int dk, int dv, int kernel_dim, float scale); /* decode.rs:2036 */
int kr_decode_add_gqa_layer(kr_decode_store* s, int input_norm_id, int post_attn_norm_id, int q_wid, int k_wid, int v_wid, int o_wid,
                            const float* q_norm, int q_norm_len, const float* k_norm, int k_norm_len, int gated, int num_heads,
                            int num_kv_heads, int head_dim, float sm_scale);                                       /* decode.rs:2082 */
/* add_decode_mla_layer (decode.rs:2131): w_kc / w_vc are bf16 [nh, nope, klr] / [nh, vhd, klr] on the host (widened to f32 on upload,
 * decode.rs:2157-2160); q_proj_wid < 0 selects the LoRA query path (q_a_proj -> q_a_norm -> q_b_proj); rope tables f32
 * [rope_max_seq, qk_rope_dim/2].  The layer's caches are FP16 [kv_max_seq, kv_lora_rank] (compressed KV) and [kv_max_seq, qk_rope_dim]
 * (k_pe); kr_decode_set_state / kr_decode_get_state address them through the kv_k / kv_v slots of the layer. */
int kr_decode_add_mla_layer(kr_decode_store* s, int input_norm_id, int post_attn_norm_id, int kv_a_proj_wid, int o_proj_wid,
                            int q_proj_wid, int q_a_proj_wid, int q_b_proj_wid, const uint16_t* w_kc_bf16, size_t w_kc_len,
                            const uint16_t* w_vc_bf16, size_t w_vc_len, const float* kv_a_norm, int kv_a_norm_len,
                            const float* q_a_norm, int q_a_norm_len, const float* rope_cos, const float* rope_sin, int rope_max_seq,
                            int num_heads, int kv_lora_rank, int qk_nope_dim, int qk_rope_dim, int v_head_dim, float sm_scale);
/* set_decode_layer_moe (decode.rs:2195): routed experts + router of engine MoE layer `moe_layer_idx`; shared expert weights
 * are decode-store weights (ids, -1 = none) */
int kr_decode_set_layer_moe(kr_decode_store* s, int layer, int moe_layer_idx, int shared_gate_up_wid, int shared_down_wid,
                            int shared_gate_wid);
int kr_decode_set_layer_dense(kr_decode_store* s, int layer, int gate_wid, int up_wid, int down_wid);              /* decode.rs:2215 */
int kr_decode_set_rope(kr_decode_store* s, const float* cos_table, const float* sin_table, int half_dim, int max_seq);
int kr_decode_finalize(kr_decode_store* s);
/* element type of the GQA KV caches and of the MLA compressed-KV / rope caches: KR_KV_FP16 = the reference's CPU-decode cache (decode.rs:4423-4478, default), KR_KV_FP8_E4M3 = the
 * reference's GPU cache dtype (python/krasis/kv_cache.py:38-135, torch.float8_e4m3fn: RNE, no saturation).  Call before set_decode_state;
 * kv_k / kv_v buffers of kr_decode_set_state / kr_decode_get_state then hold 1-byte elements. */
#define KR_KV_FP16 0
#define KR_KV_FP8_E4M3 1
int kr_decode_set_kv_dtype(kr_decode_store* s, int kv_dtype);
/* numerics of attention over LONG caches / long prompts (north_star: fp tolerance outside the router ids).  KR_ATTN_EXACT (default): the
 * reference's sequential softmax sum and p.v order, bit-identical to decode.rs:4194-4281.  KR_ATTN_FAST: decode caches longer than 1024
 * positions are split over (256-position chunk x KV head) workgroups and merged by log-sum-exp (same products and exponentials, another
 * summation order: logits within ~1e-4 relative, tests state 5e-4).  Call before the first step (a captured graph is rebuilt). */
#define KR_ATTN_EXACT 0
#define KR_ATTN_FAST 1
#define KR_GEMM_FAST 2   /* or-ed into the mode: every GEMM of kr_decode_prefill (projections, shared expert, routed experts, lm_head of the scoring pass) in the tolerance form of kr_moe_set_gemm_mode; decode steps are unaffected */
#define KR_DECODE_FAST 4 /* or-ed into the mode: decode steps run the tolerance-mode kernels of kr_decode_fast.hip -- the reference's products (INT16 activation digits, exact integer group sums, its sigmoid / libm functions), but every f32 reduction as a lane / wave / workgroup TREE instead of the reference's sequential chain, the norms folded into the launches that consume them, top-k + silu*up + the expert combine inside the expert launches (6 launches per linear-attention MoE layer).  Router ids are those of the exact kernels for identical logits, with one stated exception: exact ties fall back to the reference's heap order, but with plain softmax scoring + renormalised weights the selection runs on the LOGITS, so two distinct logits among the leading k + 1 whose f32 softmax scores round to the same value (a few ulp apart) are ordered by value here and by the heap's tie rule in the exact kernel; logits agree with the exact mode to the tolerance stated in tests/test_decode_fast_gpu.py.  MLA layers: projections, absorption, latent norm and w_vc in this form, the attention launch itself in the exact order.  Native-GGUF MoE layers (Q4_K / Q8_0 / Q4_0): the routed slots of the two expert launches walk the GGUF blocks (the block kernels' products, a row's blocks split over two waves).  Geometries the kernels do not cover (the down projection of a dense MLP, GPT-OSS activation, E > 512, hidden > 4096, Q5_0 / Q6_K blocks) keep the exact kernels for that layer -- never a CPU path.  The prompt pass is unaffected. */
int kr_decode_set_attention_mode(kr_decode_store* s, int mode);
/* Options by name.  Test / tuning hooks: "gqa_stream", "pfm_timing", ... (see kr_decode.cpp); "multi_attn_fast": see kr_decode_step_multi;
 * "multi_attn_fast_paged" (default 0; docs/design/23-multi-attn-fast-paged.md): "multi_attn_fast" for flat and paged slots alike, see kr_decode_step_multi.
 * "multi_mla_fast" (default 0; docs/design/24-multi-mla-fast.md): the MLA layers of every batched entry point run split-KV flash-decode over slots of
 * max_seq > 512, flat or paged: row i carries the bits of kr_decode_step under KR_ATTN_FAST on that sequence alone; shorter slots keep the exact step.
 * Refused on a store without MLA layers (KR_ERR_STATE) and on MLA layers of more than 64 heads (KR_ERR_VALUE); see kr_decode_step_multi.
 * "multi_extend_flash" (default 0; docs/design/25-multi-extend-flash.md): in a non-verify batched pass (kr_decode_extend_multi) the GQA layers give every run of
 * counts[i] >= 2 tokens causal flash attention over its slot, flat or paged, on the f16 matrix cores: run i carries the bits of kr_decode_prefill(tokens,
 * positions[i]) under KR_ATTN_FAST on a store whose attention layers are all GQA and whose own sequence holds the same prefix -- the last token's logits and id
 * and every K / V row the run appends -- whatever other rows share the pass; the slot's cache is streamed once per query tile of 128 / (heads per KV head)
 * tokens instead of once per token, and no score scratch is needed for those rows.  Runs of one token (kr_decode_step_multi*, kr_decode_generate_multi*, decode
 * rows of a mixed pass) keep exactly what they had, verify passes are untouched, linear-attention layers stay exact (a hybrid store: within 3e-3 of the exact
 * run, docs/design/02-numerics.md 2b).  Consequence: under the option a token's bits depend on whether it entered in a run of >= 2 tokens or alone -- as the
 * store's KR_ATTN_FAST prompt pass differs from its decode step; among cuts of >= 2 tokens each the result does not depend on the cut.  Refused by every batched
 * entry point, behind everything they refused before, each message naming the option: a store with an MLA layer or without a GQA layer (KR_ERR_STATE), a GQA
 * layer outside the prompt pass's flash kernels -- heads per KV head must divide 128, head_dim 64 / 128 / 256 -- (KR_ERR_VALUE), an LDS window refusal (KR_ERR_HIP).
 * "multi_extend_la_chunk" (default 0; docs/design/26-multi-extend-la-chunk.md): in a non-verify batched pass (kr_decode_extend_multi) the linear-attention
 * layers give every run of counts[i] >= 64 tokens the chunked gated delta rule of the KR_ATTN_FAST prompt pass (closed form over sub-chunks of 64 tokens on
 * the bf16 matrix cores, fused form) instead of the walk token by token: run i carries the bits of kr_decode_prefill(tokens, positions[i]) under KR_ATTN_FAST
 * on a store whose own sequence holds the same prefix, as long as that pass takes the run as one chunk (any run of at most 1024 tokens by default) and
 * "la_conv_fused" is 1 -- the last token's logits and id, the conv and recurrent state left in the slot, the K / V rows appended -- on a store whose
 * attention layers are all linear attention, and on a hybrid store (linear attention + GQA) with "multi_extend_flash" set as well; whatever other rows share
 * the pass, flat and paged slots.  A hybrid store under this option alone has no single-sequence equal: within 3e-3 of the exact run
 * (docs/design/02-numerics.md 2b).  Runs of fewer than 64 tokens, one token included, keep the exact run kernels and their bits; verify passes are untouched.
 * Consequence: under the option a token's bits depend on whether its run had >= 64 tokens and on where the 64-token sub-chunks fall; a stream cut into calls
 * whose lengths are multiples of 64, the last one any length >= 64, gives the bits of one call.  Refused by every batched entry point, behind everything they
 * refused before, each message naming the option: a store without a linear-attention layer or with an MLA layer (KR_ERR_STATE), a linear-attention layer
 * outside dk = dv = 128 with nv = nk * hr (KR_ERR_VALUE), an LDS window refusal (KR_ERR_HIP).
 * "multi_extend_mla_flash" (default 0; docs/design/27-multi-extend-mla-flash.md): in a non-verify batched pass (kr_decode_extend_multi) the MLA layers give every
 * run of counts[i] >= 2 tokens causal flash attention over its slot's latent and rope-key rows, flat or paged, on the f16 matrix cores, 64 (token, head) query
 * rows per workgroup: run i carries the bits of kr_decode_prefill(tokens, positions[i]) under KR_ATTN_FAST on the store's own sequence holding the same prefix
 * -- the last token's logits and id and every latent / rope-key row the run appends -- whatever other rows share the pass; the slot's cache is streamed once per
 * 64 query rows instead of once per (token, 4 heads), and no score scratch is needed for those rows.  Runs of one token (kr_decode_step_multi*,
 * kr_decode_generate_multi*, decode rows of a mixed pass) keep exactly what they had -- the exact kernel, or the flash-decode of "multi_mla_fast", which
 * composes with this option --, verify passes are untouched; within 3e-3 (FP16 caches) / 2e-2 (E4M3) of the exact run (docs/design/02-numerics.md 2b).
 * Consequence: under the option a token's bits depend on whether it entered in a run of >= 2 tokens or alone -- as the store's KR_ATTN_FAST prompt pass differs
 * from its decode step; among cuts of >= 2 tokens each the result does not depend on the cut.  Refused by every batched entry point, behind everything they
 * refused before, each message naming the option: a store without an MLA layer (KR_ERR_STATE), an LDS window refusal (KR_ERR_HIP).  "multi_extend_flash" and
 * "multi_extend_la_chunk" keep refusing a store with an MLA layer.
 * "multi_extend_exact_mfma" (default 0; docs/design/28-multi-extend-exact-mfma.md): in a non-verify batched pass (kr_decode_extend_multi) the GQA layers give every
 * run of counts[i] >= 2 tokens the three attention passes of the exact prompt pass over its slot, flat or paged: scores on the f32 matrix cores (8 fma lanes per
 * (query, position), the reference's add tree, * sm_scale), the exact softmax (max, libm exp, sum in position order, 1 / sum), P.V on the f32 matrix cores (one fma
 * chain per output over ascending positions with p = e * inv, then the sigmoid gate) -- value for value the arithmetic of the per-slot kernel, so every call
 * gives, bit for bit, what it gives with the option off: ids, logits, every K / V row, every conv and recurrent state, on flat, paged and forked slots, FP16 and
 * E4M3 caches, whatever other rows share the pass and however the stream is cut.  The slot's K rows are staged once per 64 / G query tokens and its V rows once
 * per 32 / G (G = heads per KV head) instead of once per token; the score rows stay.  Runs of one token keep their kernel -- the exact per-slot kernel, or the
 * split-KV flash-decode under "multi_attn_fast" / "multi_attn_fast_paged": a mixed pass then gives its unit rows that option's bits and its runs of >= 2 the
 * exact bits --, verify passes, linear-attention and MLA layers are untouched, "multi_extend_la_chunk" composes with the option and keeps its own bits.  Refused
 * by every batched entry point, behind everything they refused before, each message naming the option: together with "multi_extend_flash" (KR_ERR_STATE: two
 * options claim the same runs), a store without a GQA layer (KR_ERR_STATE), a GQA layer whose heads per KV head do not divide 32 (KR_ERR_VALUE: an error, not a
 * fall-back to the per-slot kernel).
 * "multi_extend_mla_exact_mfma" (default 0; docs/design/29-multi-extend-mla-exact-mfma.md): the same for the MLA layers.  In a non-verify batched pass they give every
 * run of counts[i] >= 2 tokens the three attention passes of the exact MLA prompt pass over its slot, flat or paged: scores on the f32 matrix cores in two launches
 * (16 fma chains per dot folded by the AVX2 tree: the rope dot, then (the latent dot + that) * sm_scale), the exact softmax (max, libm exp, sum in position order,
 * 1 / sum), P.V over the latent rows on the f32 matrix cores (one fma chain per output over ascending positions with p = e * inv) -- value for value the arithmetic
 * of the per-slot kernel, so every call gives, bit for bit, what it gives with the option off: ids, logits, every latent and rope-key row, on flat, paged and
 * forked slots, FP16 and E4M3 caches, kv_lora_rank 512 / 256, whatever other rows share the pass and however the stream is cut.  The slot's rows are staged once
 * per 64 / nh query tokens (scores) and 32 / nh (P.V) instead of once per (token, 4 heads).  Runs of one token keep their kernel -- the exact per-slot kernel, or
 * the split-KV flash-decode under "multi_mla_fast": a mixed pass then gives its unit rows that option's bits and its runs of >= 2 the exact bits --, verify passes
 * and the other layer kinds are untouched; independent of "multi_extend_exact_mfma" and "multi_extend_la_chunk".  Refused by every batched entry point, behind
 * everything they refused before, each message naming the option: together with "multi_extend_mla_flash" (KR_ERR_STATE: two options claim the same runs), a store
 * without an MLA layer (KR_ERR_STATE), an MLA layer whose head count does not divide 32 (KR_ERR_VALUE: an error, not a fall-back to the per-slot kernel).
 * "multi_extend_la_exact" (default 0; docs/design/36-multi-extend-la-exact.md): in a non-verify batched pass (kr_decode_extend_multi and the steps that go
 * through the same pass) the linear-attention layers give every run of counts[i] >= "multi_extend_la_exact_min" tokens the staged form of the store's own exact
 * prompt pass: conv + SiLU + gates + L2 norms parallel over (key head, 16 tokens), the carried conv inputs, the delta rule alone in the serial loop (the output
 * chain of token t and the kv chain of token t + 1 interleaved, one barrier per token), the gated RMSNorm parallel over tokens -- the same kernel templates under
 * another placement (kr_pfm_la_dev.h), value for value the arithmetic of the run kernels, so every call gives, bit for bit, what it gives with the option off:
 * ids, logits, every conv input and recurrent state, every K / V or latent row, on flat, paged and forked slots, whatever other rows share the pass and however
 * the stream is cut.  Shorter runs and unit rows keep the run kernels; verify passes and the other layer kinds are untouched; it composes with
 * "multi_extend_exact_mfma", "multi_extend_mla_exact_mfma", "multi_attn_exact_split", "multi_mla_exact_split", "pass_few_rows" and the flash run options.
 * Refused by every batched entry point, behind everything they refused before, each message naming the option: together with "multi_extend_la_chunk"
 * (KR_ERR_STATE: two options claim the long runs), a store without a linear-attention layer (KR_ERR_STATE), a linear-attention layer outside dk 64 / 128,
 * dk <= dv <= 256, dv % 8 == 0, 16-byte in-projection rows, nv = nk hr (KR_ERR_VALUE: an error, not a fall-back to the run kernels).
 * "multi_extend_la_exact_min" (default 8, 2 .. 1024 -- outside: KR_ERR_VALUE): the shortest run that is staged; same bits either way, the value is a measured one.
 * "gguf_exact_pass" (default 0; docs/design/20-gguf-exact-pass.md): with 1, every multi-row pass of the store -- kr_decode_prefill, kr_decode_prefill_nll,
 * kr_decode_verify and the batched pass behind every slot entry point -- runs MoE layers that hold native GGUF blocks through the exact grouped block
 * kernels (kr_gguf_group.hip) instead of the int8-MFMA form: every row then carries the bits of kr_decode_step on that sequence alone, and the slot and
 * speculation entry points, which otherwise refuse a store with such layers, accept it.  Slower than the default form on long prompts.  A prompt pass
 * with the option and KR_GEMM_FAST both set is refused (KR_ERR_STATE).  Stores without native GGUF layers are unaffected.
 * "gguf_exact_grouped" (default 1): 0 = that pass through the streaming block kernels for every block type (A/B and test hook; same bits).
 * "slot_select" (default 1; docs/design/33-slot-select.md): KR_DECODE_FAST, MoE layers under the lean routing rule (softmax scoring, no score
 * correction, renormalised weights; E <= 512): with 1 every routed workgroup of the gate|up launch selects the expert id of its own rank only and one
 * extra grid row publishes ids and weights for the down launch; with 0 every workgroup runs the full top-k select and workgroup (0, 0) publishes.  Same
 * bits either way (tests/test_decode_fast_slot_select_gpu.py); every other routing rule keeps the 0 form whatever the value.  A/B and test hook.
 * "slot_rows_late_first" (default 1; docs/design/35-launch-stragglers.md): KR_DECODE_FAST, the gate|up launch under the per-slot select serves slot
 * topk - 1 - y in routed grid row y, so that the slots with the longest select are handed out first; with 0 row y serves slot y; without the per-slot select
 * the value changes nothing.  Scheduling only, no workgroup reads another's output inside the launch; same bits either way
 * (tests/test_decode_fast_stragglers_gpu.py).  A/B and test hook.
 * "pass_few_rows" (default 0; docs/design/34-pass-few-rows.md): with 1, a multi-row pass of T <= "pass_few_rows_max" token rows -- T = n_tokens for
 * kr_decode_prefill / kr_decode_prefill_nll / kr_decode_verify, the sum of the counts for the slot entry points; decided per pass, never per chunk -- runs every
 * projection (q|k|v, qkvz|ba, out / o, the MLA kv_a / q / q_a / q_b, the shared expert, the dense MLP, the all-row lm_head) on the few-row streaming matvec
 * (kr_rows_matvec.hip: the decode step's tile, one weight record applied to all rows of a row group) and the routed experts of INT4 / INT8-g128 layers as the
 * decode step's three launches over the rows.  Every output keeps the bits it has without the option (tests/test_pass_few_rows_gpu.py).  Passes under
 * KR_GEMM_FAST, larger passes, native-GGUF routed experts and expert-parallel engines' routed experts keep what they run now.  The option refuses nothing:
 * a call refused without it is refused with the same code and words.
 * "pass_few_rows_max" (1 .. 16, else KR_ERR_VALUE; default 16, a measured value: profiles/pass_few_rows.txt): the most token rows of a pass that takes those kernels.
 * "pass_few_rows_group" (0 .. 16, else KR_ERR_VALUE; default 0 = chosen per launch): the most rows one workgroup of the few-row matvec holds (A/B and test
 * hook; same bits).  kr_decode_matmul_rows reads it too. */
int kr_decode_set_option(kr_decode_store* s, const char* name, int value);                                                                        /* decode.rs:2471 */
/* Whole-model prompt pass.  Replaces the reference's GPU prefill (python/krasis/model.py forward_prefill_layer_grouped / server_prefill,
 * layer.py:242-461, attention.py:496-687, linear_attention.py:695-845 -- third-party kernels) AND the GPU->CPU state hand-off
 * (decode_setup.py:232-278): tokens[0..n) (host ints) at positions start_pos.. are run through every layer in chunks; afterwards the
 * logits of the LAST token (optional host/device f32 [vocab]), the greedy sample (kr_decode_last_token), the FP16 KV caches and the
 * conv / recurrent states are bit-identical to n successive kr_decode_step calls (decode.rs:2690-3520).  GEMM-shaped work runs on the
 * int8-MFMA grouped GEMM with the exact INT16-digit arithmetic.  INT4 / INT8-g128 weights; linear-attention, GQA and MLA layers. */
int kr_decode_prefill(kr_decode_store* s, const int32_t* tokens, int n_tokens, int start_pos, float* logits_out, void* stream);
/* Scoring prompt pass = the reference's model.forward(..., return_all_logits=True) + cross_entropy(logits[:-1], tokens[1:], reduction="none")
 * (perplexity/measure_ppl.py:212-227): as kr_decode_prefill, plus final norm + lm_head for EVERY position (one [chunk, vocab] GEMM per
 * chunk, never the [n, vocab] tensor) and nll_out[i] = logsumexp(logits_i) - logits_i[tokens[i+1]] for i in [0, n_tokens-1), f32, host or
 * device.  The logits are the decode step's bit for bit; the log-sum-exp sums f32 expf terms in double and rounds once (within one f32 ulp of a
 * float64 restatement; tests hold it to 4e-6 absolute at nll < 16). */
int kr_decode_prefill_nll(kr_decode_store* s, const int32_t* tokens, int n_tokens, int start_pos, float* nll_out, float* logits_out, void* stream);
/* fresh request state: zero caches / conv / recurrent states sized for kv_max_seq (measure_ppl.py:199-206: new SequenceKVState per window +
 * linear-attention reset_state()) */
int kr_decode_reset_state(kr_decode_store* s, int kv_max_seq);
/* tokens per chunk of the prompt pass (0 = default 1024).  Chunks rotate over `depth` HIP streams and scratch arenas: layer l of
 * chunk c+1 runs concurrently with layer l+1 of chunk c (per-layer events carry the state / KV dependencies). */
int kr_decode_set_prefill_chunk(kr_decode_store* s, int chunk);
int kr_decode_set_prefill_depth(kr_decode_store* s, int depth);   /* chunks in flight = streams = scratch arenas, 1..8 (0 = default 3) */
/* set_decode_state (decode.rs:2640): per-layer host pointers (NULL = not applicable / zero-init) */
int kr_decode_set_state(kr_decode_store* s, int seq_len, int kv_max_seq, const uint16_t* const* kv_k, const uint16_t* const* kv_v,
                        const float* const* conv_state, const float* const* recur_state);
int kr_decode_fill_state_synthetic(kr_decode_store* s, int kv_max_seq, uint64_t seed);
int kr_decode_get_state(kr_decode_store* s, int layer, uint16_t* kv_k, uint16_t* kv_v, float* conv_state, float* recur_state);
/* decode_step(token, pos, out_ptr) (decode.rs:2690): logits f32 [vocab] to a host or device pointer (NULL = keep on device) */
int kr_decode_step(kr_decode_store* s, int token_id, int position, float* logits_out, void* stream);
/* generate_batch (decode.rs:3525-3600) with the full sampler sample_from_logits (decode.rs:3718-3811): per step decode_step, presence
 * penalty on already seen tokens, 1/temperature, top-k (k largest, sorted descending; ties by ascending token id), libm softmax with
 * sequential sums in that order, top-p prefix, renormalisation, xorshift64 draw (x ^= x<<13; x ^= x>>7; x ^= x<<17; r = x / u64::MAX).
 * temperature == 0 is greedy (first maximum).  The sampled token is appended before the stop test, so a stop id is the last element.
 * rng_seed 0 = wall clock like the reference.  Everything runs on the GPU; one 4-byte DtoH per token returns the id. */
int kr_decode_generate(kr_decode_store* s, int first_token, int start_pos, int max_tokens, float temperature, int top_k, float top_p,
                       const int* stop_ids, int n_stop, float presence_penalty, uint64_t rng_seed, int* tokens_out, int* n_out, void* stream);
/* sample_from_logits on the logits of the last decode_step / prefill (modifies them in place like the reference) */
int kr_decode_sample(kr_decode_store* s, float temperature, int top_k, float top_p, float presence_penalty, uint64_t rng_seed, int reset_seen,
                     int* token_out, void* stream);
/* test aid (no reference counterpart): the token ids kr_decode_sample draws from, in its order -- the top_k largest of `logits` (host pointers), value descending,
   equal values by ascending id (decode.rs:3740-3760 sorts by value only; oracle.sample_from_logits fixes the same rule); top_k <= 0: the whole vocabulary */
int kr_sample_order(const float* logits_host, int vocab, int top_k, int32_t* ids_out_host);
/* generate_batch (decode.rs:3525), greedy sampling only in this round */
int kr_decode_generate_greedy(kr_decode_store* s, int first_token, int start_pos, int max_tokens, const int* stop_ids, int n_stop,
                              int* tokens_out, int* n_out, void* stream);
/* generate_stream (decode.rs:3611): the cancellable loop of the reference's Rust server.  on_token(token, finish_reason, user) is called once per
 * generated token -- finish_reason 0 none, 1 "stop" (a stop id, reported last), 2 "length" (max_tokens reached), 3 "cancelled" (cancel flag seen
 * before the step; token = the last token) -- and returns non-zero to continue.  Text decoding (tokenizers::Tokenizer in the reference) stays
 * with the host language.  *n_out = tokens generated (the return value of the reference method). */
typedef int (*kr_token_cb)(int token, int finish_reason, void* user);
int kr_decode_generate_stream(kr_decode_store* s, int first_token, int start_pos, int max_tokens, float temperature, int top_k, float top_p,
                              const int* stop_ids, int n_stop, float presence_penalty, uint64_t rng_seed, kr_token_cb on_token, void* user, int* n_out,
                              void* stream);
/* cancel / reset_cancel / last_decode_elapsed_s (decode.rs:253-265): the flag is read by generate_stream before every step; the elapsed time
 * is the wall time of the last generate / generate_stream loop */
int kr_decode_cancel(kr_decode_store* s);
int kr_decode_reset_cancel(kr_decode_store* s);
double kr_decode_last_elapsed_s(kr_decode_store* s);

/* ---- exact speculative greedy decoding (docs/design/12-speculative.md).  Exact mode only: any tolerance bit of kr_decode_set_attention_mode, a
 * native-GGUF MoE layer or expert parallelism is refused (KR_ERR_STATE), never run in another form. */
#define KR_VERIFY_MAX 16
#define KR_LOOKUP_NGRAM_MAX 32   /* largest ngram_max kr_decode_generate_lookup indexes */
/* tokens[0] = the token at start_pos (sampled, not yet consumed); tokens[1..n) = draft.  Runs all n through the model on top of the current state
 * (the exact prompt pass).  greedy_out[i] = first-maximum argmax of the logits after tokens[0..i] (the rule of kr_launch_argmax).
 * *n_match_out = largest m <= n-1 with tokens[i] == greedy_out[i-1] for 1 <= i <= m.  Leaves a PENDING verify: exactly one kr_decode_commit follows. */
int kr_decode_verify(kr_decode_store* s, const int32_t* tokens, int n_tokens, int start_pos, int32_t* greedy_out, int* n_match_out, void* stream);
/* 1 <= n_keep <= n_match + 1: afterwards the store is bit-identical to n_keep kr_decode_step calls on tokens[0..n_keep) from the pre-verify state
 * (KV rows [0, start_pos + n_keep), conv + recurrent states, s->logits = row n_keep-1, kr_decode_last_token = greedy_out[n_keep-1]).
 * KV rows at >= start_pos + n_keep are unspecified (the next pass overwrites them). */
int kr_decode_commit(kr_decode_store* s, int n_keep);
/* greedy generation with prompt-lookup drafts: tokens_out / *n_out / return code / state afterwards IDENTICAL to
 * kr_decode_generate_greedy(s, first_token, start_pos, max_tokens, stop_ids, n_stop, ...).  context = earlier tokens to search (e.g. the prompt).
 * max_draft in [0, KR_VERIFY_MAX-1] (0 = plain loop), ngram_max in [1, KR_LOOKUP_NGRAM_MAX].  *n_passes_out = model passes (verify passes + plain steps),
 * *n_accepted_out = accepted draft tokens (either may be NULL). */
int kr_decode_generate_lookup(kr_decode_store* s, const int32_t* context, int n_context, int first_token, int start_pos, int max_tokens,
                              int max_draft, int ngram_max, const int* stop_ids, int n_stop, int* tokens_out, int* n_out,
                              int* n_passes_out, int* n_accepted_out, void* stream);
/* host-only (test aid, like kr_sample_order): the draft the loop would propose after history[0..n).  For g = min(ngram_max, n-1) down to 1: the largest
 * j with j + g <= n-1 and history[j..j+g) == history[n-g..n); the first g that matches gives history[j+g .. min(j+g+max_draft, n)).  Returns the
 * draft length (0: no match), or a negative KR_ERR_* on bad arguments. */
int kr_lookup_draft(const int32_t* history, int n_history, int ngram_max, int max_draft, int32_t* draft_out);

/* ---- exact batched decode of many sequences held in device slots (docs/design/13-multi-sequence.md).  Row i of a step is bit-identical to
 * kr_decode_step on that sequence alone (logits, greedy id, the KV row it appends -- for an MLA layer the compressed-KV row [kv_lora_rank] and the
 * rope-key row [rope dim], docs/design/15-multi-mla.md -- conv and recurrent state).  Exact mode only: a tolerance bit of
 * kr_decode_set_attention_mode, native-GGUF MoE layers, expert parallelism, an MLA geometry other than kv_lora_rank 512 / 256 with rope dim 64 and
 * a pending verify are refused; a refused call changes nothing.  The steps touch only the named slots and their own scratch (never the store's own sequence, logits, last token or decode graph);
 * reset_state / set_state / fill_state_synthetic / prefill / verify never touch slots; kr_decode_destroy frees them. */
#define KR_MULTI_MAX 256
/* n_slots sequences of up to max_seq positions each, zero-initialised (like kr_decode_reset_state); replaces existing slots; n_slots == 0 frees
   them.  KV element type = the store's at this call.  *bytes_out (may be NULL) = device bytes of all slots. */
int kr_decode_slots_create(kr_decode_store* s, int n_slots, int max_seq, size_t* bytes_out);
/* the store's own sequence -> slot: KV rows [0, seq_len) of every GQA layer, compressed-KV and rope-key rows [0, seq_len) of every MLA layer,
   conv + recurrent state of every linear-attention layer.
   0 <= seq_len <= min(store kv_max_seq, slot max_seq) */
int kr_decode_slot_save(kr_decode_store* s, int slot, int seq_len);
/* slot -> the store's own sequence (the same parts): decode_step / prefill / verify then continue it at position seq_len */
int kr_decode_slot_load(kr_decode_store* s, int slot, int seq_len);
/* row i: slot slots[i] consumes tokens[i] at positions[i].  next_out[i] = first-maximum argmax of row i's logits (the rule of kr_launch_argmax);
   logits_out (NULL, host or device) = [n][vocab] f32.  Distinct slots, 1 <= n <= KR_MULTI_MAX.  Returns once next_out is written.
   Under kr_decode_set_option(s, "multi_attn_fast", 1) (default 0; docs/design/16-multi-attn-fast.md) the GQA layers of this and every other batched
   entry point below run split-KV flash-decode over slots of max_seq > 1024: row i then carries the bits of kr_decode_step under KR_ATTN_FAST on that
   sequence alone (logits within 1e-3 of the exact step, relative to their largest magnitude), whatever rows share the step; shorter slots keep the
   exact step.  The option changes nothing else in the store; the mode bits of kr_decode_set_attention_mode stay refused here, and with the option
   set a store with MLA layers is refused (KR_ERR_STATE).  "multi_attn_fast" reads flat slots only: alone it is refused on paged slots.
   kr_decode_set_option(s, "multi_attn_fast_paged", 1) (default 0; docs/design/23-multi-attn-fast-paged.md) is the same option over both kinds: on paged
   slots of max_seq > 1024 the flash-decode reads the pools through the slots' page tables and row i carries the bits of the same call on flat slots of
   the same n_slots and max_seq under "multi_attn_fast", for any page_tokens, any placement of the pages and pages shared by kr_decode_slot_fork; paged
   slots of max_seq <= 1024 keep the exact paged step; on flat slots it is "multi_attn_fast"; with both set it governs.  Its refusals are those of
   "multi_attn_fast", and the page pool behaves as without it.
   kr_decode_set_option(s, "multi_mla_fast", 1) (default 0; docs/design/24-multi-mla-fast.md) is the counterpart for MLA layers, one option for flat and
   paged slots: over slots of max_seq > 512 the MLA layers of every batched entry point run split-KV flash-decode on the f16 matrix cores (through the
   page tables on paged slots, pages shared by kr_decode_slot_fork included) and row i carries the bits of kr_decode_step under KR_ATTN_FAST on that
   sequence alone -- logits, id, the appended latent and rope-key rows, sampler state -- provided the store's kv_max_seq and the slots' max_seq are on the
   same side of 16 384 positions (64-position chunks up to there, 128 above); logits within 3e-3 (FP16 caches) / 5e-3 (E4M3) of the exact step,
   relative to their largest magnitude.  Slots of max_seq <= 512 keep the exact step, and GQA and linear-attention layers are not touched.  Refused,
   naming "multi_mla_fast": a store without an MLA layer (KR_ERR_STATE); an MLA layer of more than 64 heads or outside kv_lora_rank 512 / 256 with
   rope 64, and a position that needs more than 1024 chunks (KR_ERR_VALUE).  Everything the step refuses without the option stays refused first. */
int kr_decode_step_multi(kr_decode_store* s, int n, const int32_t* slots, const int32_t* tokens, const int32_t* positions,
                         int32_t* next_out, float* logits_out, void* stream);
/* greedy generation of n slots together.  Row i's tokens_out[i*max_tokens ...], n_out[i] and its slot's state afterwards are exactly those of
   kr_decode_generate_greedy(first_tokens[i], start_positions[i], max_tokens, stop ids) run on that sequence alone.  A row that finishes (stop id,
   max_tokens) leaves the batch; its slot is not stepped again.  start_positions[i] + max_tokens > slot max_seq is refused before the first step. */
int kr_decode_generate_multi(kr_decode_store* s, int n, const int32_t* slots, const int32_t* first_tokens, const int32_t* start_positions,
                             int max_tokens, const int* stop_ids, int n_stop, int32_t* tokens_out, int32_t* n_out, void* stream);
/* per-row sampling (docs/design/14-multi-sampling.md).  Each slot carries its own sampler: parameters, seen-token bitmap, xorshift64 state.
   Allocated for every slot on the first kr_decode_slot_sampler call; kr_decode_slots_create drops it (a fresh slot samples greedily).  Never
   touches the store's own sampler state (kr_decode_sample / kr_decode_generate behave as if no sampled multi step had run).
   The start of kr_decode_generate on a slot: seen-token set = {first_token} (if in range), xorshift64 state = rng_seed (0: a wall-clock seed,
   distinct per slot -- not reproducible), parameters kept with the slot.  temperature 0 and presence_penalty 0 = greedy (first maximum). */
int kr_decode_slot_sampler(kr_decode_store* s, int slot, int first_token, float temperature, int top_k, float top_p,
                           float presence_penalty, uint64_t rng_seed);
/* kr_decode_step_multi, but next_out[i] is drawn by slot slots[i]'s sampler, and the slot's RNG state and seen set advance as kr_decode_generate's
   do for that token.  logits_out (optional) = the model's logits before the penalty and temperature (bit-identical to kr_decode_step_multi's).
   Rows drawing from more than 4096 candidates (top_k 0 or > 4096), or every sampled row under kr_decode_set_option("multi_sample_loop", 1),
   run the single-row sampler one row after another: same tokens.  kr_decode_set_option("multi_attn_fast", 1): see kr_decode_step_multi. */
int kr_decode_step_multi_sample(kr_decode_store* s, int n, const int32_t* slots, const int32_t* tokens, const int32_t* positions,
                                int32_t* next_out, float* logits_out, void* stream);
/* kr_decode_generate_multi with per-row sampler parameters (arrays of n): sets every row's slot sampler, then loops.  Row i equals
   kr_decode_generate(first_tokens[i], start_positions[i], max_tokens, temperature[i], top_k[i], top_p[i], stop ids, presence_penalty[i],
   rng_seeds[i]) on that sequence alone: tokens, count, stop id as the last element, slot state afterwards. */
int kr_decode_generate_multi_sample(kr_decode_store* s, int n, const int32_t* slots, const int32_t* first_tokens,
                                    const int32_t* start_positions, int max_tokens, const float* temperature, const int* top_k,
                                    const float* top_p, const float* presence_penalty, const uint64_t* rng_seeds,
                                    const int* stop_ids, int n_stop, int32_t* tokens_out, int32_t* n_out, void* stream);
/* multi-token extend of slots (docs/design/17-multi-extend.md): kr_decode_step_multi with a run of counts[i] >= 1 tokens per row.  Row i: slot slots[i]
   consumes the next counts[i] entries of tokens (rows concatenated in order, T = sum of counts <= KR_EXTEND_MAX_TOKENS) at positions positions[i] ...
   positions[i] + counts[i] - 1.  Row i is bit-identical to counts[i] successive kr_decode_step calls on that sequence alone: every K / V row (MLA: latent
   and rope-key row) the tokens append, the conv and recurrent state afterwards, the last token's logits and the id -- so the result does not depend on how
   a token stream is cut into calls (one run of 12 = runs of 5 + 7 = twelve kr_decode_step_multi calls), on the rows that share the pass, on their order
   or on T.  next_out[i] = first-maximum argmax of the logits after row i's LAST token; logits_out (NULL, host or device) = [n][vocab] f32, those
   logits (the lm_head runs for n rows, not T).  sample != 0: next_out[i] is drawn by slot slots[i]'s sampler as kr_decode_step_multi_sample draws it,
   one draw per row on the last token's logits (seen set and RNG advance once).  A prompt enters a slot by calls of this alone, chunk by chunk, beside
   decode rows (counts 1) of other slots; the store's own sequence is never touched.  Distinct slots, 1 <= n <= KR_MULTI_MAX.  Refused as
   kr_decode_step_multi refuses (same codes), and as KR_ERR_VALUE naming the row: a count < 1, T > KR_EXTEND_MAX_TOKENS, a token of a run outside the
   vocabulary, a run that ends outside the slot or past a rope table; a refused call changes nothing.  Under "multi_attn_fast" over slots of
   max_seq > 1024 every token carries the bits kr_decode_step_multi gives it under the option.  Under "multi_extend_mla_flash" a run of counts[i] >= 2 tokens
   takes the KR_ATTN_FAST prompt pass's MLA flash attention over its slot instead and carries the bits of kr_decode_prefill under KR_ATTN_FAST, not of
   kr_decode_step (a tolerance form: see kr_decode_set_option); rows of one token keep the bits stated here. */
#define KR_EXTEND_MAX_TOKENS 1024      /* = the exact prompt pass's chunk */
int kr_decode_extend_multi(kr_decode_store* s, int n, const int32_t* slots, const int32_t* counts, const int32_t* tokens, const int32_t* positions,
                           int32_t* next_out, float* logits_out, int sample, void* stream);
/* exact greedy speculation over slots (docs/design/18-multi-verify.md): another schedule of kr_decode_extend_multi's arithmetic, not a tolerance mode.
   kr_decode_verify_multi: rows laid out as in kr_decode_extend_multi (runs concatenated in tokens, T = sum of counts <= KR_EXTEND_MAX_TOKENS), every
   counts[i] in [1, KR_VERIFY_MAX]: the first token of run i is the row's sampled, not yet consumed token at positions[i], the rest its draft.
   greedy_out [T], concatenated like tokens: entry (i, t) = first-maximum argmax (kr_decode_step_multi's rule, so ties agree) of the logits after the first
   t + 1 tokens of run i -- the id and logits bits kr_decode_step gives there on that sequence alone.  n_match_out[i] = the largest m <= counts[i] - 1 such
   that token j of the run equals greedy (i, j - 1) for 1 <= j <= m.  Greedy only: the slots' samplers are neither read nor advanced (the sampled form is
   kr_decode_verify_multi_sample below).  Returns once both
   outputs are written and leaves a PENDING verify over these rows: the linear-attention state of the slots is untouched (nothing to restore, no snapshot),
   the KV rows (MLA: latent and rope-key rows) of the runs are written.
   kr_decode_commit_multi: n_keep[i] in [0, n_match[i] + 1], one entry per row of the pending call.  Afterwards slot slots[i] is bit-identical to n_keep[i]
   kr_decode_step calls on the first n_keep[i] tokens of its run: KV rows below positions[i] + n_keep[i], conv and recurrent state of every linear-attention
   layer (n_keep[i] == 0: the slot exactly as before the verify -- a cancelled request drops out).  KV rows at or past the committed length are unspecified,
   as after kr_decode_commit.  Clears the pending state.  An out-of-range n_keep is KR_ERR_VALUE naming the row: nothing is applied, the verify stays
   pending.  Without a pending verify: KR_ERR_STATE.
   While a verify over slots is pending every other slot entry point (step_multi*, extend_multi, generate_multi*, slot_save / slot_load, slot_sampler,
   verify_multi) is refused with KR_ERR_STATE and changes nothing; kr_decode_slots_create discards the pending verify with the slots.  The store's own
   sequence (decode_step, prefill, verify / commit, logits, last token, graph) is never touched by either call, and its own pending verify is a separate
   flag.  kr_decode_verify_multi is refused wherever kr_decode_extend_multi is (same codes and row-naming messages), and for a count above KR_VERIFY_MAX.
   Under "multi_attn_fast" every token carries the bits kr_decode_extend_multi gives it under the option.  The records of a call grow on demand with T
   (per token row and linear-attention layer: conv_dim + nk dk + nv dv + 2 nv floats) beside [T][vocab] logits. */
int kr_decode_verify_multi(kr_decode_store* s, int n, const int32_t* slots, const int32_t* counts, const int32_t* tokens, const int32_t* positions,
                           int32_t* greedy_out, int32_t* n_match_out, void* stream);
int kr_decode_commit_multi(kr_decode_store* s, const int32_t* n_keep);
/* kr_decode_generate_multi in fewer passes: row i's tokens_out[i*max_tokens ...], n_out[i] and its slot's state afterwards equal kr_decode_generate_multi's.
   Each pass every active row drafts from its own history (contexts row i -- the rows concatenated, n_context[i] tokens each; contexts / n_context may be
   NULL for none -- then its first token, then its generated tokens) by the rule of kr_lookup_draft, clamped as kr_decode_generate_lookup clamps it (max_draft,
   the remaining tokens, the slot and rope limits, cut after its first stop id) and to KR_EXTEND_MAX_TOKENS / m - 1 for m active rows.  No draft anywhere:
   a plain step.  Otherwise one kr_decode_verify_multi and one kr_decode_commit_multi over all active rows (rows without a draft ride along with count 1).
   *n_passes_out = passes, n_accepted_out[i] = accepted draft tokens of row i (either may be NULL).  Arguments are checked before the first pass: those of
   kr_decode_generate_multi and the max_draft / ngram_max / context checks of kr_decode_generate_lookup. */
int kr_decode_generate_multi_lookup(kr_decode_store* s, int n, const int32_t* slots, const int32_t* contexts, const int32_t* n_context,
                                    const int32_t* first_tokens, const int32_t* start_positions, int max_tokens, int max_draft, int ngram_max,
                                    const int* stop_ids, int n_stop, int32_t* tokens_out, int32_t* n_out, int* n_passes_out, int32_t* n_accepted_out,
                                    void* stream);
/* exact sampled speculation over slots (docs/design/19-multi-verify-sample.md).
   kr_decode_verify_multi_sample: kr_decode_verify_multi (same arguments, checks, refusals and row-naming messages, same model pass, records and KV rows) whose
   ids are drawn by the slots' samplers.  sampled_out [T], concatenated like tokens: for t <= n_match_out[i], entry (i, t) = the id kr_decode_step_multi_sample
   gives after the first t + 1 tokens of run i are consumed one by one; entries past n_match_out[i] are unspecified (draws of a chain that assumes the
   rejected draft).  Row (i, t) is drawn under the hypothesis that the run's tokens 1 .. t were the sampler's t draws before it: they count as seen, the
   xorshift64 state is the slot's advanced t times more.  n_match_out as in kr_decode_verify_multi, over these ids.  Writes no sampler state and leaves the
   same pending verify, marked as sampled; a slot without a sampler is plain greedy and its row equals kr_decode_verify_multi's.
   kr_decode_commit_multi after it also applies the kept draws: slot slots[i]'s seen bitmap and xorshift64 state equal n_keep[i] kr_decode_step_multi_sample
   calls on the run's first n_keep[i] tokens (0: untouched); a refused n_keep applies nothing to either part. */
int kr_decode_verify_multi_sample(kr_decode_store* s, int n, const int32_t* slots, const int32_t* counts, const int32_t* tokens, const int32_t* positions,
                                  int32_t* sampled_out, int32_t* n_match_out, void* stream);
/* kr_decode_generate_multi_sample in fewer passes: every row's sampler is set first, then kr_decode_generate_multi_lookup's loop with sampled passes (a step,
   or one kr_decode_verify_multi_sample and one commit).  Row i's tokens, count, slot state and sampler state afterwards equal
   kr_decode_generate_multi_sample's for the same seeds.  Rows on the per-row sampler path (more than 4096 candidates, or "multi_sample_loop") do not draft.
   The argument checks of both functions apply before the first pass. */
int kr_decode_generate_multi_lookup_sample(kr_decode_store* s, int n, const int32_t* slots, const int32_t* contexts, const int32_t* n_context,
                                  const int32_t* first_tokens, const int32_t* start_positions, int max_tokens, int max_draft, int ngram_max,
                                  const float* temperature, const int* top_k, const float* top_p, const float* presence_penalty,
                                  const uint64_t* rng_seeds, const int* stop_ids, int n_stop, int32_t* tokens_out, int32_t* n_out,
                                  int* n_passes_out, int32_t* n_accepted_out, void* stream);
/* one slot's sampler state read back (a zero bitmap and a zero state before any sampler was set); refused while a verify over slots is pending */
int kr_decode_slot_sampler_get(kr_decode_store* s, int slot, uint32_t* seen_out /* (vocab + 31) / 32 words */, uint64_t* rng_out);
/* ---- paged slots (docs/design/21-paged-slots.md).  A paged slot set behaves as a flat one of the same n_slots and max_seq through every slot entry point --
   ids, logits, n_match, stored rows, conv / recurrent state and sampler state are the same bit for bit -- but the KV rows of every GQA layer (K and V pools
   [n_pages][page_tokens][nkv * hd]) and the latent and rope-key rows of every MLA layer ([n_pages][page_tokens][klr] / [..][rd]) live in pages shared by all
   slots, in the store's current KV element type; linear-attention state stays per slot.  One page table serves all layers: int32
   [n_slots][ceil(max_seq / page_tokens)], -1 = unmapped, page id p = page p of every pool.  So capacity is bounded by the pool, not by n_slots * max_seq,
   and rows in a page that is not mapped read as zero.
   Mapping is host-side and all or nothing per call: after its argument checks and before anything is queued, a call maps the pages its rows still need to
   cover [0, position + count), lowest free id first, and makes them read as zero; if the pool cannot give them it fails with KR_ERR_STATE naming the first
   row that does not fit, and nothing is mapped or run.  kr_decode_generate_multi* reserve [0, start + max_tokens) before the first pass and on return give
   back the pages that call mapped which lie wholly past each row's final position.  kr_decode_verify_multi* map the drafted positions and the commit leaves
   them mapped.  kr_decode_slot_save maps what [0, seq_len) needs; kr_decode_slot_load zeroes the store's rows of pages that are not mapped.
   With "multi_attn_fast" set and "multi_attn_fast_paged" clear every batched call on paged slots is refused (KR_ERR_STATE); "multi_attn_fast_paged" is
   the split-KV option that reads pages (kr_decode_step_multi).
   Replaces any earlier slots, flat or paged.  page_tokens: a power of two, at least 32; n_pages >= 1; n_slots >= 1.  ceil(max_seq / page_tokens) table
   entries must fit in the LDS of the GQA attention launch beside its tiles, for every GQA layer of the store (7168 entries at 16 query heads per KV head of
   head_dim 256, more for narrower layers): otherwise KR_ERR_VALUE naming max_seq, page_tokens, the layer and the largest number of entries, and, as for
   every bad argument, the earlier slots stay.  *bytes_out (may be NULL) = pools + linear-attention state + table. */
int kr_decode_slots_create_paged(kr_decode_store* s, int n_slots, int max_seq, int page_tokens, int n_pages, size_t* bytes_out);
/* every page of the slot with index >= ceil(seq_len / page_tokens) back to the pool (seq_len 0: all of them); linear-attention state and sampler untouched.
   On flat slots a no-op that still checks its arguments (slot in range, 0 <= seq_len <= max_seq).  Refused while a verify over slots is pending. */
int kr_decode_slot_trim(kr_decode_store* s, int slot, int seq_len);
/* the geometry, the free pages and the mapped pages of every slot (per_slot_out [n_slots], may be NULL; so may the others).  Flat slots: page_tokens 0, n_pages 0 */
int kr_decode_slots_pages(kr_decode_store* s, int32_t* page_tokens_out, int32_t* n_pages_out, int32_t* n_free_out, int32_t* per_slot_out);
/* ---- slot fork with shared, copy-on-write pages (docs/design/22-slot-fork.md).  After the call every dsts[i] behaves as a fresh slot into which src's first
   seq_len positions were prefilled: GQA rows (K, V) and MLA rows (latent, rope-key) [0, seq_len) have src's bits, rows at or past seq_len read as zero, and the
   conv + recurrent state of every linear-attention layer is copied from src as it stands.  The library keeps no per-slot length: on a store with
   linear-attention layers seq_len must therefore be the number of tokens src has consumed (this cannot be checked); a store of GQA / MLA layers only may
   fork at any prefix.  Whatever a dst held is released first, as kr_decode_slot_trim(dst, 0); its sampler (parameters, seen set, RNG) is not touched --
   n-best sampling is a fork followed by kr_decode_slot_sampler with different seeds.  src is unchanged bit for bit, and so are the store's own sequence, a
   captured decode graph and the options.
   Paged slots: the whole pages below seq_len are shared by reference count, not copied; if seq_len is not a multiple of page_tokens each dst gets a page of its
   own holding src's rows of the boundary page with zeroes behind them; later pages stay unmapped.  All or nothing: the call needs one page per dst (none at a
   page boundary) out of the free pages and those the dsts give back, else KR_ERR_STATE naming pages needed, free and the pool size, and nothing changes.
   A write never lands in a page with more than one reference: every batched entry point (and kr_decode_slot_save) first replaces such a page, where its rows
   will write, by a private copy, counted in its all-or-nothing reservation.  Trim and the give-back of kr_decode_generate_multi* drop a reference; a page
   returns to the pool with its last one.  Flat slots: rows [0, seq_len) are copied, rows [seq_len, max_seq) of each dst zeroed.
   KR_ERR_VALUE: src or a dst out of range, src among dsts, a dst named twice, n_dst outside [1, n_slots - 1], seq_len outside [0, max_seq].  KR_ERR_STATE:
   a verify over slots is pending; the pool cannot supply the call.  Returns with its stream drained. */
int kr_decode_slot_fork(kr_decode_store* s, int src, int n_dst, const int32_t* dsts, int seq_len);
/* a paged slot's table row (ids_out [ceil(max_seq / page_tokens)], -1 = unmapped) and the reference count of each mapped page (refs_out, 0 for unmapped);
   either may be NULL.  Flat slots: KR_ERR_STATE */
int kr_decode_slot_page_ids(kr_decode_store* s, int slot, int32_t* ids_out, int32_t* refs_out);
/* the entries of a paged slot's table row, ceil(max_seq / page_tokens): what kr_decode_slot_page_ids writes to each of its outputs.  Flat slots: 0 */
int kr_decode_slots_page_stride(kr_decode_store* s, int32_t* stride_out);
/* ---- slot export and import (docs/design/38-slot-swap.md): a slot's complete state out to host memory as one self-describing image and back into any slot of
   any compatible slot set, bit for bit -- what a scheduler needs to preempt a sequence when the page pool is full without prefilling its history again.
   An image is a 64-byte header (magic, format version, KV element type, seq_len, store layers, hidden size, vocab, whether a sampler is present, a 64-bit
   digest of the per-layer geometry, total bytes, section count, table offset), a table of {uint64 offset, uint64 bytes} per section, then the sections, each
   at a multiple of 16 bytes: two per store layer in layer order -- GQA: K rows [seq_len][row], V rows; MLA: latent rows, rope-key rows; linear attention: conv
   state, recurrent state; a layer without attention: two empty sections -- and last, if present, the slot's sampler: temperature, top_k, top_p, presence
   penalty (4 bytes each), the xorshift64 state (8 bytes), 8 zero bytes, the seen bitmap.  Little-endian throughout.  The image is canonical: position-major, nothing
   at or past seq_len, nothing that depends on n_slots, max_seq, flat or paged, page_tokens or page ids, so the same sequence state exports to the same bytes
   from any slot set; a page inside [0, seq_len) that is not mapped exports as zeros.  There is no payload checksum: an image is the caller's memory and is
   trusted beyond the header checks.
   As for kr_decode_slot_fork the library keeps no per-slot length: on a store with linear-attention layers seq_len must therefore be the number of tokens the
   slot has consumed (this cannot be checked); a store of GQA / MLA layers only may export any prefix.
   Both calls run on the store's stream through a staging buffer of two halves of "slot_swap_chunk_bytes" (kr_decode_set_option: a multiple of 16, at least 1024,
   else KR_ERR_VALUE; every value gives the same bytes), allocated on first use and freed with the slots, and return with their streams drained; neither touches the
   store's own sequence, and neither synchronises the whole device except where it has to (re)allocate: the first call, the first after a change of the option,
   and a call with more pieces than any earlier one, whose piece buffer grows (freeing device or pinned memory waits for the device).
   kr_decode_slot_image_bytes: the bytes of the image of seq_len positions (0 <= seq_len <= max_seq) of the current slots, with_sampler != 0 with the sampler
   section, with_sampler < 0 as kr_decode_slots_export would write it now.
   kr_decode_slots_export: slots[n] distinct, 1 <= n <= n_slots, 0 <= seq_lens[i] <= max_seq; image_bytes[i] must be what kr_decode_slot_image_bytes gives,
   with the sampler section if and only if the set's samplers are allocated (a kr_decode_slot_sampler or sampled generation call has been made since the slots
   were created).  The slots, their table rows, reference counts and shared pages are unchanged bit for bit: an export takes no copy-on-write.  release != 0:
   once every image is complete each exported slot gives all its pages back, as kr_decode_slot_trim(slot, 0) (flat slots: nothing to give).
   kr_decode_slots_import: afterwards slots[i] behaves as a fresh slot into which the image's sequence was prefilled: rows [0, seq_len) have the image's bits,
   rows at or past seq_len read as zero, linear-attention state and sampler come from the image; seq_lens_out[i] = the image's seq_len.  An image without a
   sampler leaves the slot sampling greedily with a zero seen set and a zero state, like a fresh slot; an image with one, entering a set without samplers,
   allocates them for every slot as the first kr_decode_slot_sampler call does.  Paged slots, all or nothing across the whole call: whatever the named slots
   held is released first, as kr_decode_slot_trim(slot, 0), then the pages [0, seq_len) of every image are mapped, each with one reference (an import never
   shares pages); the count is taken beforehand out of the free pages plus those the named slots give back, else KR_ERR_STATE naming pages needed, free pages
   and pool size, and nothing changes.
   KR_ERR_VALUE, naming the row: a null pointer, a slot out of range or named twice, a wrong byte count, a bad magic or version, a KV element type or geometry
   digest other than the store's, an image seq_len above max_seq, an image sampler whose temperature is not >= 0.  KR_ERR_STATE: what kr_decode_slot_fork refuses of the store, a pending verify over slots
   included.  A refused call changes nothing.
   kr_decode_slot_image_info: host only, no store: the header checks of an image and what it says; every output may be NULL. */
int kr_decode_slot_image_bytes(kr_decode_store* s, int seq_len, int with_sampler, size_t* bytes_out);
int kr_decode_slots_export(kr_decode_store* s, int n, const int32_t* slots, const int32_t* seq_lens, void* const* images, const size_t* image_bytes, int release);
int kr_decode_slots_import(kr_decode_store* s, int n, const int32_t* slots, const void* const* images, const size_t* image_bytes, int32_t* seq_lens_out);
int kr_decode_slot_image_info(const void* image, size_t bytes, int32_t* seq_len_out, int32_t* kv_fp8_out, int32_t* has_sampler_out, uint64_t* geometry_out);
/* test aid: the page-copy launch of a fork / a copy-on-write on one host pool [n_pages][page_bytes] (in / out), a row being page_bytes / page_tokens bytes:
   copy c = the first rows[c] rows of page src_pages[c] into page dst_pages[c], zeroes behind them.  No page may be a destination twice, or a source and a
   destination.  The device copy of the pool starts base_offset bytes (in [0, 256)) past an aligned address. */
int kr_copy_pages(void* pool, size_t page_bytes, int n_pages, int page_tokens, int n_copies, const int32_t* dst_pages, const int32_t* src_pages,
                  const int32_t* rows, int base_offset);
/* test aid beside kr_sample_rows: the verify-form sampler, the accept kernel and the sampler commit on host logits [T][vocab] in caller order (the runs
   concatenated: counts[n] in [1, KR_VERIFY_MAX], tokens[T]); run i is its own "slot" with per-run parameters, seen bitmap [n][(vocab+31)/32] and xorshift64
   state (both in / out: the state after the commit).  ids_out[T] and n_match_out[n] as kr_decode_verify_multi_sample's.  n_keep[n] in / out: the wanted
   number of kept tokens (negative: all), clamped to n_match + 1; what was applied is written back.  force_loop as in kr_sample_rows. */
int kr_sample_runs(const float* logits, int n, const int32_t* counts, const int32_t* tokens, int vocab, const float* temperature, const int* top_k,
                   const float* top_p, const float* presence_penalty, uint32_t* seen, uint64_t* rng_state, int32_t* n_keep, int32_t* ids_out,
                   int32_t* n_match_out, int force_loop);
/* test aid (like kr_sample_order): the batched sampler on host logits [n][vocab] with per-row parameters, seen bitmaps [n][(vocab+31)/32]
   (may be NULL: none seen) and xorshift64 states (in / out); tokens_out[n].  force_loop != 0: every sampled row takes the single-row sampler
   (the "multi_sample_loop" form). */
int kr_sample_rows(const float* logits, int n, int vocab, const float* temperature, const int* top_k, const float* top_p,
                   const float* presence_penalty, const uint32_t* seen, uint64_t* rng_state, int32_t* tokens_out, int force_loop);
/* test aid (no reference counterpart; docs/design/32-multi-pass-plan.md): which forms the multi-row passes of this store took.  Host-side counters held in the
   store: no device work, no launch reads them, nothing on the path of kr_decode_step touches them.  The batched pass over device slots counts once per pass
   that was queued without an error, from the pass's plan (kr_multi_plan.h), its few-row flag and the store's options -- exactly the values the sections of the
   layer loop branch on, so a counter that moved means the section took that branch; a pass that failed counts nothing.  The two position-split counters
   count a pass only where the three launches exist: not for flash-decode rows, and under a flash or matrix-core run form only if the pass holds a unit row,
   since the runs then leave the per-row kernels (a pass of runs alone launches no split whatever the plan's flag says).  The store's own prompt / verify
   passes count where the few-row form is decided for the pass.  Writes the first n counters to out (0 <= n <= KR_MPC_COUNT; out may be NULL with n 0), then
   clears all of them if reset != 0.  KR_ERR_VALUE: a null store, a null out with n > 0, n out of range -- a caller that names more counters than the library
   has learns it here. */
enum {
    KR_MPC_PASSES = 0,      /* batched passes over slots (every slot entry point; a generation loop counts each of its passes) */
    KR_MPC_VERIFY,          /* ... that were verify passes */
    KR_MPC_FEW,             /* ... that took the few-row kernels ("pass_few_rows") */
    KR_MPC_XS_SPLIT,        /* ... whose per-row GQA attention was the three position-split launches ("multi_attn_exact_split") */
    KR_MPC_MLA_XS_SPLIT,    /* ... the same for MLA ("multi_mla_exact_split") */
    KR_MPC_GQA_XM,          /* ... whose runs of >= 2 tokens took the exact matrix-core passes in the GQA layers ("multi_extend_exact_mfma") */
    KR_MPC_MLA_XM,          /* ... in the MLA layers ("multi_extend_mla_exact_mfma") */
    KR_MPC_LX,              /* ... with at least one staged linear-attention run ("multi_extend_la_exact") */
    KR_MPC_LX_RUNS,         /* the staged runs of those passes, summed */
    KR_MPC_LX_SHORT,        /* the runs those passes left to the run kernels, summed */
    KR_MPC_FD,              /* passes whose unit rows took split-KV flash-decode in the GQA layers ("multi_attn_fast*") */
    KR_MPC_MLA_FD,          /* ... in the MLA layers ("multi_mla_fast") */
    KR_MPC_GQA_FLASH,       /* passes whose runs took the flash run kernels in the GQA layers ("multi_extend_flash") */
    KR_MPC_MLA_FLASH,       /* ... in the MLA layers ("multi_extend_mla_flash") */
    KR_MPC_LC,              /* passes with at least one chunked delta-rule run ("multi_extend_la_chunk") */
    KR_MPC_RUNS,            /* non-verify passes with a run of >= 2 tokens (the plan's any_run): the passes a run option can apply to */
    KR_MPC_GGUF_EXACT,      /* passes over a store with native-GGUF experts under "gguf_exact_pass" */
    KR_MPC_GGUF_GROUPED,    /* ... that took the grouped form ("gguf_exact_grouped" 1), not the streaming kernels */
    KR_MPC_SEQ_PASSES,      /* prompt / verify passes of the store's own sequence (kr_decode_prefill*, kr_decode_verify) */
    KR_MPC_SEQ_FEW,         /* ... that took the few-row kernels */
    KR_MPC_COUNT
};
int kr_decode_multi_path_counts(kr_decode_store* s, int64_t* out, int n, int reset);

/* ---- stand-alone CpuDecodeStore operators (decode.rs:328-1086).  Every pointer may be a host or a device pointer; host buffers are staged and
 * the call returns after the results are back.  Bit-identical to the reference methods (tests/test_standalone_ops_gpu.py against the oracle's
 * kro_op_* restatements); several differ from the decode graph's arithmetic exactly as they do in the reference (scalar loops, libm exp). */
int kr_decode_matmul(kr_decode_store* s, int weight_id, const float* input, float* output);                                   /* decode.rs:328 */
int kr_decode_matmul_batch(kr_decode_store* s, const int* weight_ids, int n, const float* input, float* const* outputs);      /* decode.rs:364 */
/* kr_decode_matmul over n_rows input rows (no reference counterpart; docs/design/34-pass-few-rows.md): input [n_rows][cols], output [n_rows][rows]; output row r
   holds the bits of kr_decode_matmul on input row r.  1 <= n_rows <= 16 and cols a multiple of 128, else KR_ERR_VALUE.  The weights are read once per row group. */
int kr_decode_matmul_rows(kr_decode_store* s, int weight_id, const float* input, int n_rows, float* output);
/* fused_add_rmsnorm (weight != NULL, decode.rs:406) / fused_add_rmsnorm_id (weight == NULL, stored norm `norm_id`, decode.rs:447) */
int kr_decode_fused_add_rmsnorm(kr_decode_store* s, float* hidden, float* residual, const float* weight, int norm_id, float eps, int size, int first_call);
int kr_decode_rmsnorm(kr_decode_store* s, const float* input, const float* weight, float eps, float* output, int size);      /* decode.rs:473 */
int kr_decode_silu_mul(kr_decode_store* s, const float* gate, const float* up, float* output, int size);                      /* decode.rs:511 */
int kr_decode_fused_shared_expert(kr_decode_store* s, int gate_up_wid, int down_wid, const float* input, float* output);      /* decode.rs:542 */
int kr_decode_linear_attention_recurrent(kr_decode_store* s, float* state, const float* q, const float* k, const float* v, const float* g, const float* beta,
                                         float* output, int nv, int dk, int dv);                                              /* decode.rs:609 */
int kr_decode_gated_rmsnorm_silu(kr_decode_store* s, const float* x, const float* z, const float* norm_weight, float* output, float eps, int nv, int dv); /* decode.rs:650 */
int kr_decode_linear_attention_conv(kr_decode_store* s, const float* qkvz, const float* ba, float* conv_state, const float* conv_weight, const float* a_log,
                                    const float* dt_bias, float scale, float* q_out, float* k_out, float* v_out, float* z_out, float* g_out, float* beta_out,
                                    int nk, int nv, int dk, int dv, int hr, int kernel_dim);                                  /* decode.rs:713 */
/* store_route_weight (decode.rs:895) / moe_route (decode.rs:955): f32 gate [E, H], optional bias / e_score_correction [E] (NULL = none) */
int kr_decode_store_route_weight(kr_decode_store* s, const float* gate, int num_experts, int hidden_dim, const float* bias, const float* e_score_corr, int* route_id_out);
int kr_decode_moe_route(kr_decode_store* s, int route_id, const float* hidden, int32_t* topk_ids_out, float* topk_weights_out, int topk, int scoring_func, int norm_topk_prob);
int kr_decode_num_route_weights(kr_decode_store* s);                                                                          /* decode.rs:1113 */
size_t kr_decode_weight_bytes(kr_decode_store* s, int weight_id);                                                             /* decode.rs:1107 */
int kr_decode_last_token(kr_decode_store* s, int* token);
int kr_decode_set_use_graph(kr_decode_store* s, int enable);
int kr_decode_read_buffer(kr_decode_store* s, int which /* 0 hidden, 1 residual, 2 router ids (i32 bits), 3 router weights, 4 router logits, 5 second residual (KR_DECODE_FAST), 6 logits [vocab] */, float* out, int n);
size_t kr_decode_device_bytes(const kr_decode_store* s);
/* measurement hook (bench.py): one un-graphed step with HIP events around every launch; per-kind totals (ms) and launch counts.
 * kinds: 0 embed 1 fused_add_rmsnorm 2 projection matvec 3 la_conv 4 la_recurrent 5 gated_rmsnorm_silu 6 gqa 7 route_logits
 *        8 route_select 9 moe_w13 10 moe_w2 11 moe_combine 12 lm_head 13 argmax 14 shared-gate matvec */
int kr_decode_profile_step(kr_decode_store* s, int token_id, int position, double* ms_by_kind, long* launches_by_kind, int n_kinds);

/* ---- measurement hooks (bench.py): HIP events around each kernel launch on the launch stream ----
 * kinds: 0 kr_moe_w13_kernel, 1 kr_moe_w2_kernel, 2 kr_moe_combine_kernel.  Enabling profiling serialises calls. */
int kr_set_profiling(kr_engine* e, int enable);
int kr_get_profile(kr_engine* e, int kind, double* total_ms, long* launches);

#ifdef __cplusplus
}
#endif
#endif
