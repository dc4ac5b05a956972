"""CpuDecodeStore -- host mirror of the reference's decode-graph class (src/decode.rs:193-3602) over the HIP C ABI.

The class keeps the reference's NAME and builder methods so `decode_setup.py`-style callers are source compatible; the
graph it builds runs on the MI355X (all weights / KV / recurrent state in HBM, one hipGraph replay per token).
Pointer arguments are integer HOST addresses exactly like the reference (decode.rs:280-286).
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import check, load_library
from .engine import KrasisEngine, _addr

# default draft length of generate_lookup: chosen from the verify-cost table of tools/probes/spec_verify_cost.py (docs/design/12-speculative.md)
LOOKUP_MAX_DRAFT = 8


def _per_row(v, default, ctype, n):
    """a sampler parameter of generate_multi / generate_multi_lookup_sample as a C array of n: a scalar for every row, or one value per row"""
    v = default if v is None else v
    v = list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v] * n
    if len(v) != n:
        raise ValueError(f"{len(v)} sampler values for {n} rows")
    return (ctype * max(n, 1))(*v)


def lookup_draft(history: Sequence[int], ngram_max: int, max_draft: int) -> List[int]:
    """The draft generate_lookup proposes after `history` (kr_lookup_draft; host only): for g = min(ngram_max, n-1) down to 1, the continuation of
    the LATEST earlier occurrence of the trailing g-gram that has one, at most max_draft tokens; [] when no g-gram recurs."""
    lib = load_library()
    h = (C.c_int32 * max(len(history), 1))(*history)
    out = (C.c_int32 * max(max_draft, 1))()
    n = lib.kr_lookup_draft(h, len(history), ngram_max, max_draft, out)
    if n < 0:
        check(-n)
    return list(out[:n])


def _image_bytes(image) -> np.ndarray:
    """a slot image as a contiguous uint8 array over the same bytes: bytes-like objects and arrays of any dtype are reinterpreted, never converted"""
    if isinstance(image, np.ndarray):
        return np.ascontiguousarray(image).reshape(-1).view(np.uint8)
    return np.frombuffer(image, np.uint8)


def slot_image_info(image) -> dict:
    """kr_decode_slot_image_info (host only, no store): the header checks of a slot image (export_slots) and what it says --
    dict(seq_len, kv_fp8, has_sampler, geometry); ValueError for anything that is not a whole image of this format version"""
    lib = load_library()
    a = _image_bytes(image)
    seq, fp8, smp, geo = C.c_int32(), C.c_int32(), C.c_int32(), C.c_uint64()
    check(lib.kr_decode_slot_image_info(a.ctypes.data, a.size, C.byref(seq), C.byref(fp8), C.byref(smp), C.byref(geo)))
    return dict(seq_len=seq.value, kv_fp8=bool(fp8.value), has_sampler=bool(smp.value), geometry=geo.value)


class CpuDecodeStore:
    def __init__(self, group_size: int = 128, parallel: bool = True, norm_bias_one: bool = False, device: Optional[int] = None):
        # Like the reference (decode.rs:229) the store exists BEFORE an engine is bound: weights, norms and router gates can be stored first and
        # set_moe_store(engine) may come last (decode_setup.py:1010) -- or first, as the synthetic benchmark does.  Until then the store runs on
        # the current HIP device with a bare engine inside the library.
        self._lib = load_library()
        self._group_size = group_size
        self._norm_bias_one = norm_bias_one
        self._h = C.c_void_p()
        if device is None:
            check(self._lib.kr_decode_create(None, group_size, int(norm_bias_one), C.byref(self._h)))
        else:     # a named device: the store must live where the engine it will be bound to lives
            check(self._lib.kr_decode_create_on(int(device), group_size, int(norm_bias_one), C.byref(self._h)))
        self._engine: Optional[KrasisEngine] = None
        self._vocab = 0
        self._n_layers = 0
        self._n_weights = 0
        self._routes: list = []          # route_id -> (gate f32 [E,H], bias | None, e_score_corr | None)   (store_route_weight)
        self._route_layer: dict = {}     # route_id -> engine MoE layer (set_decode_layer_moe)
        self._route_cfg = None           # (scoring code, norm_topk_prob, topk) from configure_decode
        self._routes_pushed: set = set()

    def __del__(self):
        try:
            if getattr(self, "_h", None) is not None and self._h.value:
                self._lib.kr_decode_destroy(self._h); self._h = C.c_void_p()
        except Exception:
            pass

    # set_moe_store (decode.rs:2250): the engine owns the routed experts and the routers; bound at any point of the build
    def set_moe_store(self, engine: KrasisEngine) -> None:
        engine._need("Model not loaded")
        if self._engine is not None and self._engine is not engine:
            raise RuntimeError("MoE store already set")
        check(self._lib.kr_decode_set_moe_store(self._h, engine._h))
        self._engine = engine
        self._push_routes()

    def _push_routes(self) -> None:
        """router gates handed to store_route_weight live in the engine's router store (one per MoE layer): pushed once the engine, the routing
        configuration (configure_decode) and the route_id -> moe_layer_idx mapping (set_decode_layer_moe) are all known"""
        eng = self._engine
        if eng is None or self._route_cfg is None:
            return
        for rid, layer in self._route_layer.items():
            if rid in self._routes_pushed or rid >= len(self._routes):
                continue
            gate, bias, esc = self._routes[rid]
            E, H = gate.shape
            if eng._routing_cfg is None:
                sf, norm, topk = self._route_cfg
                check(self._lib.kr_set_routing_config(eng._h, sf, int(norm), topk, E, H))
                eng._routing_cfg = ({0: "sigmoid", 1: "softmax", 2: "swiglu"}[sf], norm, topk, E, H)
            eng.set_route_weight_f32(layer, gate, bias, esc)
            self._routes_pushed.add(rid)

    def _need(self):
        if not self._h.value:
            raise RuntimeError("decode store was destroyed")

    # ------------------------------------------------------------------ weights
    def store_weight_f32(self, data_ptr: int, rows: int, cols: int, num_bits: int = 4) -> int:
        self._need()
        if num_bits not in (4, 8):
            raise ValueError(f"num_bits must be 4 or 8, got {num_bits}")
        wid = C.c_int()
        check(self._lib.kr_decode_store_weight_f32(self._h, data_ptr, rows, cols, num_bits, C.byref(wid)))
        self._n_weights += 1
        return wid.value

    def store_weight_synthetic(self, rows: int, cols: int, num_bits: int = 4, seed: int = 1) -> int:
        self._need()
        wid = C.c_int()
        check(self._lib.kr_decode_store_weight_synthetic(self._h, rows, cols, num_bits, seed, C.byref(wid)))
        self._n_weights += 1
        return wid.value

    def download_weight(self, wid: int, rows: int, cols: int, num_bits: int = 4):
        self._need()
        packed = np.empty((cols // 8, rows), np.uint32) if num_bits == 4 else np.empty((cols, rows), np.int8)
        scales = np.empty((cols // 128, rows), np.uint16)
        check(self._lib.kr_decode_download_weight(self._h, wid, _addr(packed), _addr(scales)))
        return packed, scales

    def store_norm_weight(self, data_ptr: int, size: int) -> int:
        self._need()
        nid = C.c_int()
        check(self._lib.kr_decode_store_norm_weight(self._h, data_ptr, size, C.byref(nid)))
        return nid.value

    def store_route_weight(self, data_ptr: int, num_experts: int, hidden_dim: int, bias_ptr: Optional[int] = None, bias_len: int = 0,
                           e_score_corr_ptr: Optional[int] = None, e_score_corr_len: int = 0) -> int:
        """decode.rs:895 -- f32 gate [E, H] (+ optional bias / e_score_correction [E]) -> route_id.  The data is copied (the caller may free
        its tensors, decode_setup.py:563-567)."""
        self._need()
        if not data_ptr:
            raise ValueError("null gate pointer")
        rd = lambda p, n: np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_float)), shape=(n,)).copy()
        gate = rd(data_ptr, num_experts * hidden_dim).reshape(num_experts, hidden_dim)
        bias = rd(bias_ptr, bias_len) if bias_ptr and bias_len else None
        esc = rd(e_score_corr_ptr, e_score_corr_len) if e_score_corr_ptr and e_score_corr_len else None
        self._routes.append((gate, bias, esc))
        # the device copy serves the stand-alone moe_route (decode.rs:955); the engine's routers get theirs through _push_routes
        rid = C.c_int()
        check(self._lib.kr_decode_store_route_weight(self._h, _addr(gate), num_experts, hidden_dim, _addr(bias) if bias is not None else None,
                                                     _addr(esc) if esc is not None else None, C.byref(rid)))
        assert rid.value == len(self._routes) - 1
        return rid.value

    def num_weights(self) -> int:
        return self._n_weights

    def num_route_weights(self) -> int:
        return len(self._routes)

    def total_bytes(self) -> int:
        return self.device_bytes()

    def weight_bytes(self, weight_id: int) -> int:
        """decode.rs:1107 -- packed words * 4 + bf16 scales * 2 of one stored weight"""
        return int(self._lib.kr_decode_weight_bytes(self._h, weight_id))

    def self_addr(self) -> int:
        """decode.rs:269 -- raw address of the store for GIL-free callers: here the kr_decode_store* handle of the C ABI"""
        return int(self._h.value or 0)

    def consolidate_weights_mmap(self) -> None:
        """decode.rs:2341 consolidates the CPU engine's weights into one NUMA-interleaved mmap; HBM allocations need no such step."""

    # ------------------------------------------------------------------ stand-alone operators (decode.rs:328-1086)
    # Pointers are plain addresses like the reference's (tensor.data_ptr()); host AND device addresses are accepted.  The arithmetic runs on
    # the GPU (csrc/kr_decode_standalone.cpp); results are bit-identical to the reference methods.
    def matmul(self, weight_id: int, input_ptr: int, output_ptr: int) -> None:
        check(self._lib.kr_decode_matmul(self._h, weight_id, input_ptr, output_ptr))

    def matmul_rows(self, weight_id: int, input_ptr: int, n_rows: int, output_ptr: int) -> None:
        """matmul over 1 .. 16 input rows (no reference counterpart): input [n_rows][cols], output [n_rows][rows]; row r carries the bits of matmul on row r,
        the weights are read once per row group (docs/design/34-pass-few-rows.md)"""
        check(self._lib.kr_decode_matmul_rows(self._h, weight_id, input_ptr, int(n_rows), output_ptr))

    def matmul_batch(self, weight_ids: Sequence[int], input_ptr: int, output_ptrs: Sequence[int]) -> None:
        if len(weight_ids) != len(output_ptrs):
            raise ValueError("weight_ids and output_ptrs must have same length")          # decode.rs:370
        n = len(weight_ids)
        ids = (C.c_int * max(n, 1))(*weight_ids); outs = (C.c_void_p * max(n, 1))(*output_ptrs)
        check(self._lib.kr_decode_matmul_batch(self._h, ids, n, input_ptr, outs))

    def fused_add_rmsnorm(self, hidden_ptr: int, residual_ptr: int, weight_ptr: int, eps: float, size: int, first_call: bool) -> None:
        if not weight_ptr:
            raise ValueError("null weight pointer")
        check(self._lib.kr_decode_fused_add_rmsnorm(self._h, hidden_ptr, residual_ptr, weight_ptr, -1, eps, size, int(first_call)))

    def fused_add_rmsnorm_id(self, hidden_ptr: int, residual_ptr: int, norm_id: int, eps: float, size: int, first_call: bool) -> None:
        check(self._lib.kr_decode_fused_add_rmsnorm(self._h, hidden_ptr, residual_ptr, None, norm_id, eps, size, int(first_call)))

    def rmsnorm(self, input_ptr: int, weight_ptr: int, eps: float, output_ptr: int, size: int) -> None:
        check(self._lib.kr_decode_rmsnorm(self._h, input_ptr, weight_ptr, eps, output_ptr, size))

    def silu_mul(self, gate_ptr: int, up_ptr: int, output_ptr: int, size: int) -> None:
        check(self._lib.kr_decode_silu_mul(self._h, gate_ptr, up_ptr, output_ptr, size))

    def fused_shared_expert(self, gate_up_wid: int, down_wid: int, input_ptr: int, output_ptr: int) -> None:
        check(self._lib.kr_decode_fused_shared_expert(self._h, gate_up_wid, down_wid, input_ptr, output_ptr))

    def linear_attention_recurrent(self, state_ptr: int, q_ptr: int, k_ptr: int, v_ptr: int, g_ptr: int, beta_ptr: int, output_ptr: int,
                                   nv: int, dk: int, dv: int) -> None:
        check(self._lib.kr_decode_linear_attention_recurrent(self._h, state_ptr, q_ptr, k_ptr, v_ptr, g_ptr, beta_ptr, output_ptr, nv, dk, dv))

    def gated_rmsnorm_silu(self, x_ptr: int, z_ptr: int, norm_weight_ptr: int, output_ptr: int, eps: float, nv: int, dv: int) -> None:
        check(self._lib.kr_decode_gated_rmsnorm_silu(self._h, x_ptr, z_ptr, norm_weight_ptr, output_ptr, eps, nv, dv))

    def linear_attention_conv(self, qkvz_ptr: int, ba_ptr: int, conv_state_ptr: int, conv_weight_ptr: int, a_log_ptr: int, dt_bias_ptr: int, scale: float,
                              q_out_ptr: int, k_out_ptr: int, v_out_ptr: int, z_out_ptr: int, g_out_ptr: int, beta_out_ptr: int,
                              nk: int, nv: int, dk: int, dv: int, hr: int, kernel_dim: int) -> None:
        check(self._lib.kr_decode_linear_attention_conv(self._h, qkvz_ptr, ba_ptr, conv_state_ptr, conv_weight_ptr, a_log_ptr, dt_bias_ptr, scale,
                                                        q_out_ptr, k_out_ptr, v_out_ptr, z_out_ptr, g_out_ptr, beta_out_ptr, nk, nv, dk, dv, hr, kernel_dim))

    def moe_route(self, route_id: int, hidden_ptr: int, topk_ids_out_ptr: int, topk_weights_out_ptr: int, topk: int, scoring_func: int,
                  norm_topk_prob: bool) -> None:
        check(self._lib.kr_decode_moe_route(self._h, route_id, hidden_ptr, topk_ids_out_ptr, topk_weights_out_ptr, topk, scoring_func, int(norm_topk_prob)))

    # ------------------------------------------------------------------ cancellation / timing (decode.rs:253-265)
    @property
    def last_decode_elapsed_s(self) -> float:
        return float(self._lib.kr_decode_last_elapsed_s(self._h))

    def cancel(self) -> None:
        check(self._lib.kr_decode_cancel(self._h))

    def reset_cancel(self) -> None:
        check(self._lib.kr_decode_reset_cancel(self._h))

    def repack_to_tiled(self) -> None:
        """decode.rs repack_to_tiled: the CPU engine re-tiles its weights for bandwidth; the HBM layout is already lane-tiled."""

    # ------------------------------------------------------------------ graph
    def configure_decode(self, hidden_size: int, num_layers: int, eps: float, final_norm_id: int, lm_head_wid: int, vocab_size: int,
                         topk: int, scoring_func: int, norm_topk_prob: bool, routed_scaling_factor: float, embedding_ptr: int,
                         synth_seed: int = 0) -> None:
        self._need()
        check(self._lib.kr_decode_configure(self._h, hidden_size, num_layers, eps, final_norm_id, lm_head_wid, vocab_size, topk,
                                            scoring_func, int(norm_topk_prob), routed_scaling_factor, embedding_ptr or None, synth_seed))
        self._vocab, self._n_layers = vocab_size, num_layers
        self._route_cfg = (scoring_func, bool(norm_topk_prob), topk)

    def add_decode_la_layer(self, input_norm_id, post_attn_norm_id, in_proj_qkvz_wid, in_proj_ba_wid, out_proj_wid, conv_weight_ptr,
                            a_log_ptr, dt_bias_ptr, norm_weight_ptr, nk, nv, dk, dv, hr, kernel_dim, scale) -> None:
        """decode.rs:2036 (same positional arguments; hr = value heads per key head)"""
        self._need()
        if hr * nk != nv:
            raise ValueError(f"head ratio {hr} does not match {nv} value / {nk} key heads")
        check(self._lib.kr_decode_add_la_layer(self._h, input_norm_id, post_attn_norm_id, in_proj_qkvz_wid, in_proj_ba_wid, out_proj_wid,
                                               conv_weight_ptr, a_log_ptr, dt_bias_ptr, norm_weight_ptr, nk, nv, dk, dv, kernel_dim, scale))

    def add_decode_gqa_layer(self, input_norm_id, post_attn_norm_id, q_proj_wid, k_proj_wid, v_proj_wid, o_proj_wid, q_norm_ptr, q_norm_len,
                             k_norm_ptr, k_norm_len, gated, num_heads, num_kv_heads, head_dim, sm_scale) -> None:
        self._need()
        check(self._lib.kr_decode_add_gqa_layer(self._h, input_norm_id, post_attn_norm_id, q_proj_wid, k_proj_wid, v_proj_wid, o_proj_wid,
                                                q_norm_ptr or None, q_norm_len, k_norm_ptr or None, k_norm_len, int(gated), num_heads,
                                                num_kv_heads, head_dim, sm_scale))

    def add_decode_mla_layer(self, input_norm_id, post_attn_norm_id, kv_a_proj_wid, o_proj_wid, q_proj_wid, q_a_proj_wid, q_b_proj_wid,
                             w_kc_ptr, w_kc_len, w_vc_ptr, w_vc_len, kv_a_norm_ptr, kv_a_norm_len, q_a_norm_ptr, q_a_norm_len, rope_cos_ptr,
                             rope_sin_ptr, rope_len, rope_max_seq, num_heads, kv_lora_rank, qk_nope_dim, qk_rope_dim, v_head_dim, sm_scale) -> None:
        """decode.rs:2131 (same positional arguments; None for an absent projection id)."""
        self._need()
        f = lambda v: -1 if v is None else v
        check(self._lib.kr_decode_add_mla_layer(self._h, input_norm_id, post_attn_norm_id, kv_a_proj_wid, o_proj_wid, f(q_proj_wid),
                                                f(q_a_proj_wid), f(q_b_proj_wid), w_kc_ptr, w_kc_len, w_vc_ptr, w_vc_len, kv_a_norm_ptr,
                                                kv_a_norm_len, q_a_norm_ptr or None, q_a_norm_len, rope_cos_ptr, rope_sin_ptr, rope_max_seq,
                                                num_heads, kv_lora_rank, qk_nope_dim, qk_rope_dim, v_head_dim, sm_scale))

    def set_decode_layer_moe(self, layer_idx: int, route_id: int, moe_layer_idx: int, shared_gate_up_wid: Optional[int] = None,
                             shared_down_wid: Optional[int] = None, shared_gate_wid: Optional[int] = None) -> None:
        self._need()
        f = lambda v: -1 if v is None else v
        check(self._lib.kr_decode_set_layer_moe(self._h, layer_idx, moe_layer_idx, f(shared_gate_up_wid), f(shared_down_wid), f(shared_gate_wid)))
        self._route_layer[route_id] = moe_layer_idx
        self._push_routes()

    def set_decode_layer_dense(self, layer_idx: int, gate_proj_wid: int, up_proj_wid: int, down_proj_wid: int) -> None:
        self._need()
        check(self._lib.kr_decode_set_layer_dense(self._h, layer_idx, gate_proj_wid, up_proj_wid, down_proj_wid))

    def set_decode_rope(self, cos_ptr: int, sin_ptr: int, half_dim: int, max_seq: int) -> None:
        self._need()
        check(self._lib.kr_decode_set_rope(self._h, cos_ptr, sin_ptr, half_dim, max_seq))

    def set_kv_dtype(self, fp8_e4m3: bool) -> None:
        """GQA KV cache element type: FP16 (reference CPU decode, default) or FP8-E4M3 (reference GPU cache, kv_cache.py:38)."""
        self._need(); check(self._lib.kr_decode_set_kv_dtype(self._h, 1 if fp8_e4m3 else 0))
        self._kv_fp8 = bool(fp8_e4m3)

    def set_attention_mode(self, fast: bool, gemm_fast: bool = False, decode_fast: bool = False) -> None:
        """fast False (default): the reference's sequential softmax / p.v order (bit-exact).  True: split-KV / flash attention and the chunked
        delta rule -- tolerance mode (logits within ~1e-4 relative).  gemm_fast True: the GEMMs of the prompt pass in the tolerance form as well
        (f16 activations, f32 accumulation over the whole k range: the dataflow of the reference's GPU prompt pass); decode steps are unaffected.
        decode_fast True (KR_DECODE_FAST): decode steps on the tolerance-mode kernels -- the reference's products, tree reductions instead of its
        sequential chains, norms / top-k / activation / combine folded into the matvec launches; the prompt pass is unaffected."""
        self._need(); check(self._lib.kr_decode_set_attention_mode(self._h, (1 if fast else 0) | (2 if gemm_fast else 0) | (4 if decode_fast else 0)))

    def set_option(self, name: str, value: int) -> None:
        """options by name.  Test / tuning hooks ("gqa_stream", "pfm_timing", "multi_sample_loop", ...), and "multi_attn_fast" (default 0): with 1
        the GQA layers of every batched step (step_multi, step_multi_sample, generate_multi) run split-KV flash-decode over slots of max_seq > 1024
        -- tolerance form, row i bit-identical to decode_step under set_attention_mode(True) on that sequence alone; shorter slots keep the exact
        step; nothing else in the store changes; a store with MLA layers is then refused by the batched calls (docs/design/16-multi-attn-fast.md).
        "multi_attn_fast" alone reads flat slots only and is refused on paged ones; "multi_attn_fast_paged" (default 0) is the same option for both
        kinds: on paged slots the flash-decode reads the page pool through the slots' tables, row i bit-identical to the same call on flat slots
        under "multi_attn_fast"; on flat slots it is "multi_attn_fast"; with both set it governs (docs/design/23-multi-attn-fast-paged.md).
        "multi_mla_fast" (default 0): the counterpart for MLA layers, one option for flat and paged slots -- with 1 the MLA layers of every batched call
        run split-KV flash-decode over slots of max_seq > 512, row i bit-identical to decode_step under set_attention_mode(True) on that sequence alone;
        shorter slots keep the exact step; GQA and linear-attention layers are untouched; a store without MLA layers, or an MLA layer of more than 64
        heads, is then refused by the batched calls (docs/design/24-multi-mla-fast.md).
        "multi_extend_flash" (default 0): with 1 a run of two or more tokens entering a slot (extend_multi, prefill_slot) takes causal flash attention
        over the slot in its GQA layers, flat or paged -- tolerance form, the run bit-identical to prefill(run, position) under
        set_attention_mode(True) on a store of GQA layers whose own sequence holds the same prefix; runs of one token (step_multi, generate_multi,
        decode rows beside a chunk) and verify passes keep what they had; linear-attention layers stay exact (there: within 3e-3 of the exact run).
        A token's bits then depend on whether it entered in a run of >= 2 or alone.  A store with an MLA layer or without a GQA layer, or a GQA
        layer whose heads per KV head do not divide 128, is then refused by the batched calls (docs/design/25-multi-extend-flash.md).
        "multi_extend_la_chunk" (default 0): with 1 a run of 64 or more tokens entering a slot (extend_multi, prefill_slot) takes the prompt pass's
        chunked delta rule in its linear-attention layers (closed form over sub-chunks of 64 tokens on the matrix cores) -- tolerance form, the run
        bit-identical to prefill(run, position) under set_attention_mode(True) on a store whose own sequence holds the same prefix: on a store of
        linear-attention layers, and on a hybrid store with "multi_extend_flash" set as well (this option alone there: within 3e-3 of the exact run).
        Runs of fewer than 64 tokens and verify passes keep what they had.  A token's bits then depend on whether its run had >= 64 tokens and on
        where the 64-token sub-chunk edges fall: calls cut at multiples of 64 (the last one any length >= 64) give the bits of one call.  A store
        without a linear-attention layer or with an MLA layer, or a linear-attention layer outside dk = dv = 128, is then refused by the batched
        calls (docs/design/26-multi-extend-la-chunk.md).
        "multi_extend_mla_flash" (default 0): with 1 a run of two or more tokens entering a slot (extend_multi, prefill_slot) takes the prompt pass's
        causal flash attention over the slot's latent and rope-key rows in its MLA layers, flat or paged -- tolerance form, the run bit-identical to
        prefill(run, position) under set_attention_mode(True) on the store's own sequence holding the same prefix; runs of one token (step_multi,
        generate_multi, decode rows beside a chunk) keep what they had, "multi_mla_fast" included, and verify passes are untouched.  A token's bits
        then depend on whether it entered in a run of >= 2 or alone.  Within 3e-3 (FP16 caches) / 2e-2 (E4M3) of the exact run.  A store without an
        MLA layer is then refused by the batched calls (docs/design/27-multi-extend-mla-flash.md).
        "multi_extend_exact_mfma" (default 0): with 1 a run of two or more tokens entering a slot (extend_multi, prefill_slot) takes the exact prompt
        pass's three attention passes over the slot in its GQA layers, flat or paged -- scores and P.V on the f32 matrix cores, the exact softmax
        between them -- and every call gives, bit for bit, what it gives with the option off: ids, logits, every K / V row and every conv and
        recurrent state, however the stream is cut.  Only the speed of the admission changes.  Runs of one token keep their kernel (the exact
        per-slot kernel, or the split-KV flash-decode under "multi_attn_fast" / "multi_attn_fast_paged": a mixed pass then gives its unit rows
        that option's bits and its runs of >= 2 the exact bits); verify passes, linear-attention and MLA layers are untouched, and
        "multi_extend_la_chunk" composes with it and keeps its own bits.  Refused by the batched calls together with "multi_extend_flash" (both
        claim the same runs), on a store without a GQA layer, and on a GQA layer whose heads per KV head do not divide 32
        (docs/design/28-multi-extend-exact-mfma.md).
        "multi_extend_mla_exact_mfma" (default 0): the same for the MLA layers.  With 1 a run of two or more tokens entering a slot (extend_multi,
        prefill_slot) takes the exact MLA prompt pass's three attention passes over the slot's latent and rope-key rows, flat or paged -- the two
        score dots and P.V on the f32 matrix cores, the exact softmax between them -- and every call gives, bit for bit, what it gives with the
        option off: ids, logits, every latent and rope-key row, however the stream is cut.  Only the speed of the admission changes.  Runs of one
        token keep their kernel (the exact per-slot kernel, or the split-KV flash-decode under "multi_mla_fast": a mixed pass then gives its unit
        rows that option's bits and its runs of >= 2 the exact bits); verify passes and the other layer kinds are untouched, and the option is
        independent of "multi_extend_exact_mfma" and "multi_extend_la_chunk".  Refused by the batched calls together with
        "multi_extend_mla_flash" (both claim the same runs), on a store without an MLA layer, and on an MLA layer whose head count does not divide
        32 (docs/design/29-multi-extend-mla-exact-mfma.md).
        "multi_extend_la_exact" (default 0): with 1 a run of "multi_extend_la_exact_min" or more tokens entering a slot (extend_multi, prefill_slot)
        takes the staged form of the exact prompt pass in its linear-attention layers -- conv, gates and L2 norms parallel over tokens, the delta
        rule alone in the serial loop with its two chains interleaved, the gated RMSNorm parallel over tokens -- where the run kernels walk the run
        with five barriers per token.  Every call gives, bit for bit, what it gives with the option off: ids, logits, every conv input and
        recurrent state, every K / V or latent row, however the stream is cut and whatever rows share the pass, on flat, paged and forked slots.
        Only the speed of the admission changes.  Shorter runs and unit rows keep the run kernels; verify passes, GQA and MLA layers are
        untouched, and the option composes with the attention options of the other layer kinds.  Refused by the batched calls together with
        "multi_extend_la_chunk" (both claim the long runs), on a store without a linear-attention layer, and on a linear-attention layer outside
        dk 64 / 128, dk <= dv <= 256 (docs/design/36-multi-extend-la-exact.md).
        "multi_extend_la_exact_min" (default 8, 2 .. 1024 -- outside: ValueError): the shortest run that is staged; both forms give the same
        bits, the value is a measured one.
        "multi_attn_exact_split" (default 0): with 1 every batched pass over slots (step_multi, the unit rows of extend_multi / prefill_slot, all token
        rows of verify_multi / verify_multi_sample, every pass of the generate_multi* loops) launches the exact per-slot GQA attention as three
        kernels -- scores spread over tiles of 256 positions, the softmax one wave per (row, head), P.V spread over heads and slices of 32 outputs
        -- where it launched one workgroup per (row, KV head).  Every call gives, bit for bit, what it gives with the option off: ids, logits,
        every K / V row and state; only the time changes.  Over slots longer than gqa_split_min "multi_attn_fast" / "multi_attn_fast_paged" still
        take the rows for the flash-decode, and the runs of "multi_extend_flash" / "multi_extend_exact_mfma" keep their run kernels; MLA and
        linear-attention layers are untouched.  Refused by the batched calls on a store without a GQA layer
        (docs/design/30-multi-attn-exact-split.md).
        "multi_attn_exact_split_min" (default 512, at least 1 -- below: ValueError): a pass takes the split when the longest attention of its
        per-row kernels, position + 1, is at least this; both forms give the same bits, the value is a measured one.
        "multi_mla_exact_split" (default 0): the same for MLA layers -- with 1 every batched pass over slots (step_multi, the unit rows of
        extend_multi / prefill_slot, all token rows of verify_multi / verify_multi_sample, every pass of the generate_multi* loops) launches the
        exact per-slot MLA attention as three kernels -- scores spread over tiles of 64 positions and groups of 4 heads, the softmax one wave per
        (row, head), the weighted sum spread over heads and slices of 32 latent elements -- where it launched one workgroup per (row, 4 heads).
        Every call gives, bit for bit, what it gives with the option off: ids, logits, every latent and rope-key row and sampler state; only the
        time changes.  Over slots longer than mla_split_min "multi_mla_fast" still takes the rows for the flash-decode, and the runs of
        "multi_extend_mla_flash" / "multi_extend_mla_exact_mfma" keep their run kernels; GQA and linear-attention layers are untouched, and the
        option is independent of "multi_attn_exact_split".  Refused by the batched calls on a store without an MLA layer
        (docs/design/31-multi-mla-exact-split.md).
        "multi_mla_exact_split_min" (default 512, at least 1 -- below: ValueError): a pass takes the split when the longest attention of its
        per-row MLA kernels, position + 1, is at least this; both forms give the same bits, the value is a measured one.
        "gguf_exact_pass" (default 0): with 1 every multi-row pass (prefill, prefill_nll, verify, and the batched pass behind every slot call) runs
        native-GGUF MoE layers through the exact grouped block kernels -- every row carries the bits of decode_step on that sequence alone -- and the
        slot and speculation calls accept a store with such layers; slower than the default int8-MFMA form on long prompts; refused together with
        gemm_fast; nothing changes for other weight forms (docs/design/20-gguf-exact-pass.md).  "gguf_exact_grouped" (default 1): 0 makes that pass
        take the streaming block kernels for every type (A/B and test hook, same bits).
        "pass_few_rows" (default 0): with 1 a multi-row pass of at most "pass_few_rows_max" token rows (prefill / prefill_nll / verify: the number of
        tokens; the slot calls: the sum of their counts) runs every projection on a few-row form of the decode step's streaming matvec and the INT4 /
        INT8 routed experts as the step's three launches.  Every call gives, bit for bit, what it gives with the option off; passes under gemm_fast,
        larger passes, native-GGUF and expert-parallel routed experts keep what they run; nothing is refused that was not refused before
        (docs/design/34-pass-few-rows.md).  "pass_few_rows_max" (1 .. 16 -- outside: ValueError; default 16, a measured value).
        "pass_few_rows_group" (0 .. 16, default 0 = chosen per launch): the most rows one workgroup of that matvec holds (A/B and test hook, same
        bits; matmul_rows reads it too)"""
        self._need(); check(self._lib.kr_decode_set_option(self._h, name.encode(), int(value)))

    def finalize_decode(self) -> None:
        self._need()
        self._push_routes()
        check(self._lib.kr_decode_finalize(self._h))

    def set_decode_state(self, seq_len: int, kv_max_seq: int, kv_k_ptrs: Sequence[int], kv_v_ptrs: Sequence[int],
                         conv_state_ptrs: Sequence[int], recur_state_ptrs: Sequence[int], mla_ckv_ptrs=None, mla_kpe_ptrs=None) -> None:
        self._need()
        n = self._n_layers
        mk = lambda xs: (C.c_void_p * n)(*[(x or None) for x in xs])
        if mla_ckv_ptrs is not None:   # MLA layers keep their caches in the kv_k / kv_v slots of the C ABI
            kv_k_ptrs = [a or b for a, b in zip(list(kv_k_ptrs) + [0] * n, mla_ckv_ptrs)][:n]
            kv_v_ptrs = [a or b for a, b in zip(list(kv_v_ptrs) + [0] * n, mla_kpe_ptrs)][:n]
        check(self._lib.kr_decode_set_state(self._h, seq_len, kv_max_seq, mk(kv_k_ptrs), mk(kv_v_ptrs), mk(conv_state_ptrs), mk(recur_state_ptrs)))

    def fill_state_synthetic(self, kv_max_seq: int, seed: int = 7) -> None:
        self._need()
        check(self._lib.kr_decode_fill_state_synthetic(self._h, kv_max_seq, seed))

    def get_decode_state(self, layer: int, kv_k=None, kv_v=None, conv_state=None, recur_state=None) -> None:
        self._need()
        check(self._lib.kr_decode_get_state(self._h, layer, _addr(kv_k) or None, _addr(kv_v) or None, _addr(conv_state) or None,
                                            _addr(recur_state) or None))

    # ------------------------------------------------------------------ run
    def decode_step(self, token_id: int, position: int, output_ptr: int = 0, stream: int = 0) -> None:
        self._need()
        check(self._lib.kr_decode_step(self._h, token_id, position, output_ptr or None, stream or None))

    def prefill(self, tokens: Sequence[int], start_pos: int = 0, output_ptr: int = 0, stream: int = 0) -> int:
        """Whole-model prompt pass on the GPU (kr_decode_prefill): equivalent to calling decode_step for every prompt token, which is what
        replaces model.server_prefill + CpuDecoder.prepare (decode_setup.py:232-278).  Returns the greedy sample of the last position."""
        self._need()
        arr = (C.c_int32 * len(tokens))(*tokens)
        check(self._lib.kr_decode_prefill(self._h, arr, len(tokens), start_pos, output_ptr or None, stream or None))
        return self.last_token()

    def prefill_nll(self, tokens: Sequence[int], start_pos: int = 0, output_ptr: int = 0, stream: int = 0) -> np.ndarray:
        """Scoring prompt pass (kr_decode_prefill_nll): the prompt pass plus, per position i < n-1, the next-token negative log-likelihood
        -log softmax(logits_i)[tokens[i+1]] -- model.forward(return_all_logits=True) + cross_entropy(reduction="none") of the perplexity
        harness (perplexity/measure_ppl.py:212-227) without materialising [n, vocab].  Returns f32 [n-1]."""
        self._need()
        if len(tokens) < 2:
            raise ValueError(f"Need at least 2 tokens, got {len(tokens)}")
        arr = (C.c_int32 * len(tokens))(*tokens)
        nll = np.empty(len(tokens) - 1, np.float32)
        check(self._lib.kr_decode_prefill_nll(self._h, arr, len(tokens), start_pos, nll.ctypes.data, output_ptr or None, stream or None))
        return nll

    def reset_decode_state(self, kv_max_seq: int) -> None:
        """fresh request: zeroed KV / latent caches, conv and recurrent states (measure_ppl.py:199-206)"""
        self._need()
        check(self._lib.kr_decode_reset_state(self._h, kv_max_seq))

    def set_prefill_chunk(self, chunk: int) -> None:
        """Tokens per chunk of the prompt pass (0 = default); chunks alternate between two streams."""
        self._need(); check(self._lib.kr_decode_set_prefill_chunk(self._h, chunk))

    def set_prefill_depth(self, depth: int) -> None:
        """Chunks of the prompt pass in flight (streams / scratch arenas), 1..8; 0 = default."""
        self._need(); check(self._lib.kr_decode_set_prefill_depth(self._h, depth))

    def generate_batch(self, first_token: int, start_pos: int, max_tokens: int, temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0,
                       stop_ids: Sequence[int] = (), presence_penalty: float = 0.0, rng_seed: int = 0) -> List[int]:
        """decode.rs:3525 -- decode loop + sampler on the GPU; `rng_seed` (extra, 0 = wall clock like the reference) makes draws reproducible."""
        self._need()
        out = (C.c_int * max(max_tokens, 1))(); n = C.c_int()
        stops = (C.c_int * max(len(stop_ids), 1))(*stop_ids)
        check(self._lib.kr_decode_generate(self._h, first_token, start_pos, max_tokens, temperature, top_k, top_p, stops, len(stop_ids),
                                           presence_penalty, rng_seed, out, C.byref(n), None))
        return list(out[: n.value])

    def verify(self, tokens: Sequence[int], start_pos: int):
        """kr_decode_verify: runs tokens[0] (the last sampled token, not yet consumed) and the draft tokens[1:] through the exact prompt pass at
        start_pos.. -> (greedy, n_match): greedy[i] = the greedy token after tokens[0..i]; n_match = how many leading drafts equal the greedy choice.
        Exactly one commit() must follow."""
        self._need()
        n = len(tokens)
        arr = (C.c_int32 * max(n, 1))(*tokens)
        g = (C.c_int32 * max(n, 1))(); m = C.c_int()
        check(self._lib.kr_decode_verify(self._h, arr, n, start_pos, g, C.byref(m), None))
        return list(g[:n]), m.value

    def commit(self, n_keep: int) -> None:
        """kr_decode_commit: keep the first n_keep tokens of the pending verify (1 <= n_keep <= n_match + 1); the state is then bit-identical to
        n_keep decode_step calls (logits, last_token, KV rows below start_pos + n_keep, conv and recurrent states)."""
        self._need()
        check(self._lib.kr_decode_commit(self._h, n_keep))

    def generate_lookup(self, first_token: int, start_pos: int, max_tokens: int, context: Sequence[int] = (), max_draft: int = LOOKUP_MAX_DRAFT,
                        ngram_max: int = 3, stop_ids: Sequence[int] = ()) -> List[int]:
        """Greedy generation with prompt-lookup drafts (kr_decode_generate_lookup): the same tokens and final state as
        generate_batch(first_token, start_pos, max_tokens, stop_ids=stop_ids) at temperature 0, in fewer model passes when the text repeats
        `context` (e.g. the prompt) or itself.  last_lookup_stats = {"passes": model passes, "accepted": accepted draft tokens}."""
        self._need()
        ctx = (C.c_int32 * max(len(context), 1))(*context)
        out = (C.c_int * max(max_tokens, 1))(); n = C.c_int(); passes = C.c_int(); acc = C.c_int()
        stops = (C.c_int * max(len(stop_ids), 1))(*stop_ids)
        check(self._lib.kr_decode_generate_lookup(self._h, ctx, len(context), first_token, start_pos, max_tokens, max_draft, ngram_max, stops, len(stop_ids),
                                                  out, C.byref(n), C.byref(passes), C.byref(acc), None))
        self.last_lookup_stats = {"passes": passes.value, "accepted": acc.value}
        return list(out[: n.value])

    # ------------------------------------------------------------------ sequence slots (docs/design/13-multi-sequence.md)
    def create_slots(self, n: int, max_seq: int, page_tokens: Optional[int] = None, n_pages: Optional[int] = None) -> int:
        """kr_decode_slots_create: n zeroed sequence slots of up to max_seq positions (replacing any earlier ones; n = 0 frees them), KV rows
        (for an MLA layer: compressed-KV rows [kv_lora_rank] and rope-key rows [rope dim]) of the store's current element type.  Returns their device bytes.
        With page_tokens and n_pages (kr_decode_slots_create_paged, docs/design/21-paged-slots.md) the GQA / MLA rows live in a pool of n_pages pages of
        page_tokens positions (a power of two, at least 32) shared by all slots: same results bit for bit, capacity bounded by the pool; a call that
        needs more pages than are free fails with KR_ERR_STATE and changes nothing.  Of the two split-KV options, paged slots take
        "multi_attn_fast_paged"; "multi_attn_fast" alone is refused on them (set_option).  "multi_mla_fast", the split-KV option of MLA layers, reads flat
        and paged slots alike (over slots of max_seq > 512)."""
        self._need()
        if (page_tokens is None) != (n_pages is None):
            raise ValueError("create_slots: page_tokens and n_pages go together")
        b = C.c_size_t()
        if page_tokens is None:
            check(self._lib.kr_decode_slots_create(self._h, n, max_seq, C.byref(b)))
        else:
            check(self._lib.kr_decode_slots_create_paged(self._h, n, max_seq, page_tokens, n_pages, C.byref(b)))
        self._multi_verify_rows = None      # a pending verify_multi goes with the slots
        self._n_slots = n
        return b.value

    def trim_slot(self, slot: int, seq_len: int) -> None:
        """kr_decode_slot_trim: the pages of a paged slot wholly at or past position seq_len go back to the pool (0: all); a checked no-op on flat slots"""
        self._need(); check(self._lib.kr_decode_slot_trim(self._h, slot, seq_len))

    def slot_pages(self) -> dict:
        """kr_decode_slots_pages: dict(page_tokens, n_pages, free, per_slot) -- per_slot[i] = pages mapped to slot i; flat slots: page_tokens 0, n_pages 0"""
        self._need()
        pt, npg, free = C.c_int32(), C.c_int32(), C.c_int32()
        per = np.zeros(max(int(getattr(self, "_n_slots", 0)), 1), dtype=np.int32)
        check(self._lib.kr_decode_slots_pages(self._h, C.byref(pt), C.byref(npg), C.byref(free), per.ctypes.data))
        return dict(page_tokens=pt.value, n_pages=npg.value, free=free.value, per_slot=[int(x) for x in per[: int(getattr(self, "_n_slots", 0))]])

    def fork_slot(self, src: int, dsts, seq_len: int) -> None:
        """kr_decode_slot_fork (docs/design/22-slot-fork.md): every slot of dsts (an int or a sequence) becomes a fresh slot into which src's first seq_len
        positions were prefilled -- GQA / MLA rows [0, seq_len) with src's bits, zero from there on, the linear-attention state copied as it stands.  The
        library keeps no per-slot length: on a store with linear-attention layers seq_len must be the number of tokens src has consumed (this cannot be
        checked); a store of GQA / MLA layers only may fork at any prefix.  What a dst held is released first; its sampler is not touched (n-best: fork,
        then set_slot_sampler with different seeds).  Paged slots share the whole pages below seq_len by reference and copy on write; all or nothing:
        a pool that cannot give each dst its boundary page refuses the call (RuntimeError) and nothing changes."""
        self._need()
        d = np.ascontiguousarray([dsts] if isinstance(dsts, (int, np.integer)) else list(dsts), dtype=np.int32)
        check(self._lib.kr_decode_slot_fork(self._h, src, len(d), d.ctypes.data, seq_len))

    def slot_page_ids(self, slot: int):
        """kr_decode_slot_page_ids: (ids, refs) of a paged slot -- its table row (-1 = unmapped) and the reference count of each mapped page (0 for
        unmapped); flat slots: RuntimeError"""
        self._need()
        stride = C.c_int32()      # the row length comes from the library: the slots may have been made through another wrapper on this handle
        check(self._lib.kr_decode_slots_page_stride(self._h, C.byref(stride)))
        ids, refs = np.full(max(stride.value, 1), -1, np.int32), np.zeros(max(stride.value, 1), np.int32)
        check(self._lib.kr_decode_slot_page_ids(self._h, slot, ids.ctypes.data, refs.ctypes.data))
        return [int(x) for x in ids], [int(x) for x in refs]

    # ------------------------------------------------------------------ slot export / import (docs/design/38-slot-swap.md)
    def slot_image_bytes(self, seq_len: int) -> int:
        """kr_decode_slot_image_bytes: the bytes of the image export_slot(slot, seq_len) would write now -- with the sampler section if and only if the
        set's samplers are allocated"""
        self._need()
        b = C.c_size_t()
        check(self._lib.kr_decode_slot_image_bytes(self._h, seq_len, -1, C.byref(b)))
        return b.value

    def export_slots(self, slots: Sequence[int], seq_lens: Sequence[int], release: bool = False) -> List[np.ndarray]:
        """kr_decode_slots_export: the complete state of every slots[i] at seq_lens[i] positions as one self-describing host image each (uint8 arrays):
        GQA / MLA rows [0, seq_len), the linear-attention state as it stands, the slot's sampler if the set has samplers.  The image is canonical -- the
        same sequence state gives the same bytes from flat or paged slots, any page size and placement -- and import_slots brings it back into any slot
        of any compatible slot set, bit for bit.  The slots, their pages and reference counts are unchanged (no copy-on-write); release=True then gives
        every exported slot's pages back, as trim_slot(slot, 0).  The library keeps no per-slot length: on a store with linear-attention layers
        seq_len must be the number of tokens the slot has consumed (this cannot be checked).  Refused while a verify over slots is pending."""
        self._need()
        slots, seq_lens = [int(x) for x in slots], [int(x) for x in seq_lens]
        if len(slots) != len(seq_lens):
            raise ValueError(f"{len(slots)} slots but {len(seq_lens)} seq_lens")
        n = len(slots)
        images = []
        for q in seq_lens:
            b = C.c_size_t()
            check(self._lib.kr_decode_slot_image_bytes(self._h, q, -1, C.byref(b)))
            images.append(np.empty(b.value, np.uint8))
        ptrs = (C.c_void_p * max(n, 1))(*[im.ctypes.data for im in images])
        sizes = (C.c_size_t * max(n, 1))(*[im.size for im in images])
        check(self._lib.kr_decode_slots_export(self._h, n, (C.c_int32 * max(n, 1))(*slots), (C.c_int32 * max(n, 1))(*seq_lens), ptrs, sizes, int(bool(release))))
        return images

    def import_slots(self, slots: Sequence[int], images) -> List[int]:
        """kr_decode_slots_import: every slots[i] becomes a fresh slot into which the sequence of images[i] (uint8 arrays or bytes, from export_slots of
        any slot set of the same model and KV element type) was prefilled -- rows, linear-attention state and sampler from the image, zero rows behind
        them; an image without a sampler leaves the slot greedy.  Returns the images' seq_lens.  What the slots held is released first.  Paged slots:
        all or nothing, every page mapped with one reference; a pool that cannot hold the images, counting the pages the named slots give back,
        refuses the call (RuntimeError) and nothing changes.  A bad image (size, magic, version, KV type, geometry, seq_len above max_seq) is a ValueError."""
        self._need()
        slots = [int(x) for x in slots]
        if len(slots) != len(images):
            raise ValueError(f"{len(slots)} slots but {len(images)} images")
        n = len(slots)
        arrs = [_image_bytes(im) for im in images]
        ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrs])
        sizes = (C.c_size_t * max(n, 1))(*[a.size for a in arrs])
        out = (C.c_int32 * max(n, 1))()
        check(self._lib.kr_decode_slots_import(self._h, n, (C.c_int32 * max(n, 1))(*slots), ptrs, sizes, out))
        return list(out[:n])

    def export_slot(self, slot: int, seq_len: int, release: bool = False) -> np.ndarray:
        """export_slots for one slot"""
        return self.export_slots([slot], [seq_len], release)[0]

    def import_slot(self, slot: int, image) -> int:
        """import_slots for one slot -> the image's seq_len"""
        return self.import_slots([slot], [image])[0]

    def save_slot(self, slot: int, seq_len: int) -> None:
        """the store's own sequence -> slot: KV rows [0, seq_len) of every GQA layer, compressed-KV and rope-key rows [0, seq_len) of every MLA
        layer, conv + recurrent state of every linear-attention layer"""
        self._need(); check(self._lib.kr_decode_slot_save(self._h, slot, seq_len))

    def load_slot(self, slot: int, seq_len: int) -> None:
        """slot -> the store's own sequence (the same parts); decode_step / prefill / verify then continue it at position seq_len"""
        self._need(); check(self._lib.kr_decode_slot_load(self._h, slot, seq_len))

    def step_multi(self, slots: Sequence[int], tokens: Sequence[int], positions: Sequence[int], logits: bool = False):
        """kr_decode_step_multi: row i = slot slots[i] consumes tokens[i] at positions[i], bit-identical to decode_step on that sequence alone
        (logits, id, the KV row -- or MLA latent and rope-key rows -- it appends to the slot).  Returns the greedy ids, or (ids, logits f32 [n, vocab]) with logits=True.
        After set_option("multi_attn_fast", 1), over slots of max_seq > 1024: row i is bit-identical to decode_step under set_attention_mode(True) on that
        sequence alone instead (GQA attention as split-KV flash-decode; logits within 1e-3 of the exact step relative to their largest magnitude).
        On paged slots that takes set_option("multi_attn_fast_paged", 1), which gives the same bits through the page table.
        After set_option("multi_mla_fast", 1), over flat or paged slots of max_seq > 512, the same holds for MLA layers: their attention runs as split-KV
        flash-decode and row i is bit-identical to decode_step under set_attention_mode(True) on that sequence alone (logits within 3e-3 of the exact
        step with FP16 caches, 5e-3 with E4M3, relative to their largest magnitude)."""
        return self._step_multi(self._lib.kr_decode_step_multi, slots, None, tokens, positions, logits)

    def _step_multi(self, entry, slots, counts, tokens, positions, logits, *flags):
        """step_multi / step_multi_sample / extend_multi: the rows in (counts None: the entry point takes none, one token per row), one id per row out,
        optionally with the logits"""
        self._need()
        n = len(slots)
        arr = lambda xs, k=n: (C.c_int32 * max(k, 1))(*xs)      # one value per row unless told otherwise
        ids = (C.c_int32 * max(n, 1))()
        out = np.empty((n, self._vocab), np.float32) if logits else None
        runs = (arr(tokens),) if counts is None else (arr(counts), arr(tokens, len(tokens)))
        check(entry(self._h, n, arr(slots), *runs, arr(positions), ids, out.ctypes.data if logits else None, *flags, None))
        return (list(ids[:n]), out) if logits else list(ids[:n])

    def generate_multi(self, slots: Sequence[int], first_tokens: Sequence[int], start_positions: Sequence[int], max_tokens: int,
                       stop_ids: Sequence[int] = (), temperature=None, top_k=None, top_p=None, presence_penalty=None, rng_seeds=None) -> List[List[int]]:
        """kr_decode_generate_multi: greedy generation of the slots together; row i's tokens (and its slot afterwards) are those of
        generate_batch(first_tokens[i], start_positions[i], max_tokens, stop_ids=stop_ids) at temperature 0 on that sequence alone.
        Any of temperature / top_k / top_p / presence_penalty / rng_seeds given (a scalar or one value per row; the others default to 0, 0, 1.0,
        0, 0): kr_decode_generate_multi_sample, row i = generate_batch(..., temperature[i], top_k[i], top_p[i], stop_ids, presence_penalty[i],
        rng_seeds[i]) on that sequence alone."""
        sampler = (temperature, top_k, top_p, presence_penalty, rng_seeds)
        if all(p is None for p in sampler):
            return self._generate_multi(self._lib.kr_decode_generate_multi, slots, first_tokens, start_positions, max_tokens, stop_ids)
        return self._generate_multi(self._lib.kr_decode_generate_multi_sample, slots, first_tokens, start_positions, max_tokens, stop_ids, sampler=sampler)

    def _generate_multi(self, entry, slots, first_tokens, start_positions, max_tokens, stop_ids, lookup=None, sampler=None):
        """the four generation entry points over slots: lookup = (contexts, max_draft, ngram_max) for the lookup forms, which also leave
        last_multi_lookup_stats; sampler = (temperature, top_k, top_p, presence_penalty, rng_seeds) for the sampled forms, each a scalar, one value per row
        or None for its default.  Returns the tokens of every row."""
        self._need()
        n = len(slots)
        arr = lambda xs, k=n: (C.c_int32 * max(k, 1))(*xs)      # one value per row unless told otherwise
        out = (C.c_int32 * max(n * max_tokens, 1))(); cnt = (C.c_int32 * max(n, 1))(); acc = (C.c_int32 * max(n, 1))(); passes = C.c_int()
        ctx, draft, stats = (), (), ()
        if lookup is not None:
            contexts, max_draft, ngram_max = lookup
            contexts = [[] for _ in range(n)] if contexts is None else [list(c) for c in contexts]
            if len(contexts) != n:
                raise ValueError(f"{len(contexts)} contexts for {n} rows")
            flat = [int(t) for c in contexts for t in c]
            ctx, draft, stats = (arr(flat, len(flat)), arr([len(c) for c in contexts])), (max_draft, ngram_max), (C.byref(passes), acc)
        cols = () if sampler is None else tuple(_per_row(v, default, ctype, n) for v, (default, ctype) in
                                                zip(sampler, ((0.0, C.c_float), (0, C.c_int), (1.0, C.c_float), (0.0, C.c_float), (0, C.c_uint64))))
        check(entry(self._h, n, arr(slots), *ctx, arr(first_tokens), arr(start_positions), max_tokens, *draft, *cols,
                    (C.c_int * max(len(stop_ids), 1))(*stop_ids), len(stop_ids), out, cnt, *stats, None))
        if lookup is not None:
            self.last_multi_lookup_stats = {"passes": passes.value, "accepted": list(acc[:n])}
        return [list(out[i * max_tokens: i * max_tokens + cnt[i]]) for i in range(n)]

    def set_slot_sampler(self, slot: int, first_token: int, temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0,
                         presence_penalty: float = 0.0, rng_seed: int = 0) -> None:
        """kr_decode_slot_sampler: start a request's sampler on a slot, as generate_batch starts its own: seen tokens = {first_token},
        xorshift64 state = rng_seed (0 = wall clock), parameters kept with the slot for step_multi_sample (temperature 0, penalty 0 = greedy)."""
        self._need()
        check(self._lib.kr_decode_slot_sampler(self._h, slot, first_token, temperature, top_k, top_p, presence_penalty, rng_seed))

    def step_multi_sample(self, slots: Sequence[int], tokens: Sequence[int], positions: Sequence[int], logits: bool = False):
        """kr_decode_step_multi_sample: step_multi, but row i's id is drawn by slot slots[i]'s sampler (set_slot_sampler), exactly as
        generate_batch draws it for that sequence alone.  Returns the ids, or (ids, logits f32 [n, vocab]) with logits=True (the model's
        logits, before penalty and temperature)."""
        return self._step_multi(self._lib.kr_decode_step_multi_sample, slots, None, tokens, positions, logits)

    def extend_multi(self, slots: Sequence[int], token_lists: Sequence[Sequence[int]], positions: Sequence[int], logits: bool = False,
                     sample: bool = False):
        """kr_decode_extend_multi: row i = slot slots[i] consumes the tokens token_lists[i] (at least one) at positions[i], positions[i] + 1, ...,
        bit-identical to that many decode_step calls on that sequence alone (every KV row -- or MLA latent and rope-key row -- they append, conv and
        recurrent state, the last token's logits and id), however a token stream is cut into calls and whatever rows share the pass.  At most
        KR_EXTEND_MAX_TOKENS tokens per call, all rows together.  Returns one id per row -- the greedy id after its last token, or with sample=True the
        draw of the slot's sampler (set_slot_sampler) on those logits, as step_multi_sample draws it -- or (ids, logits f32 [n, vocab]) with logits=True.
        After set_option("multi_extend_flash", 1) a run of two or more tokens takes the prompt pass's flash attention in its GQA layers instead
        (tolerance form, docs/design/25-multi-extend-flash.md): it then equals prefill(run, position) under set_attention_mode(True), not decode_step,
        and a token's bits depend on whether it entered in a run of >= 2 or alone (among cuts of >= 2 tokens each the cut does not matter).
        After set_option("multi_extend_la_chunk", 1) a run of >= 64 tokens takes the prompt pass's chunked delta rule in its linear-attention
        layers (tolerance form, docs/design/26-multi-extend-la-chunk.md): with both options a run of 2 .. 1024 tokens on a hybrid store equals
        prefill(run, position) under set_attention_mode(True).  A token's bits then also depend on whether its run had >= 64 tokens and on where
        the 64-token sub-chunk edges fall: cuts at multiples of 64 tokens (the last call any length >= 64) give the bits of one call.
        After set_option("multi_extend_mla_flash", 1) a run of two or more tokens takes the prompt pass's flash attention in its MLA layers
        (tolerance form, docs/design/27-multi-extend-mla-flash.md): it then equals prefill(run, position) under set_attention_mode(True), not
        decode_step, and a token's bits depend on whether it entered in a run of >= 2 or alone (among cuts of >= 2 tokens each the cut does not
        matter).
        After set_option("multi_extend_exact_mfma", 1) a run of two or more tokens takes the exact prompt pass's matrix-core scores, softmax and
        P.V over its slot in the GQA layers (docs/design/28-multi-extend-exact-mfma.md): no bit changes -- the call still equals that many
        decode_step calls, whatever the cut.  Runs of one token keep their kernel: with "multi_attn_fast" / "multi_attn_fast_paged" also set a
        mixed pass gives its unit rows that option's bits and its runs of >= 2 the exact bits.
        After set_option("multi_extend_mla_exact_mfma", 1) a run of two or more tokens takes the exact MLA prompt pass's matrix-core scores,
        softmax and P.V over its slot in the MLA layers (docs/design/29-multi-extend-mla-exact-mfma.md): again no bit changes, whatever the cut.
        Runs of one token keep their kernel: with "multi_mla_fast" also set a mixed pass gives its unit rows that option's bits and its runs of
        >= 2 the exact bits.
        After set_option("multi_extend_la_exact", 1) a run of "multi_extend_la_exact_min" or more tokens takes the staged form of the exact
        prompt pass in its linear-attention layers (docs/design/36-multi-extend-la-exact.md): no bit changes -- the call still equals that many
        decode_step calls, whatever the cut; shorter runs and unit rows keep the run kernels."""
        if len(token_lists) != len(slots) or len(positions) != len(slots):
            raise ValueError(f"{len(slots)} slots, {len(token_lists)} token lists, {len(positions)} positions")
        return self._step_multi(self._lib.kr_decode_extend_multi, slots, [len(run) for run in token_lists], [int(t) for run in token_lists for t in run],
                                positions, logits, 1 if sample else 0)

    def verify_multi(self, slots: Sequence[int], token_lists: Sequence[Sequence[int]], positions: Sequence[int]):
        """kr_decode_verify_multi (docs/design/18-multi-verify.md): row i = slot slots[i] runs token_lists[i] = [its sampled, not yet consumed token, its
        draft ...] (1 to KR_VERIFY_MAX tokens) at positions[i] ....  Returns (greedy_lists, n_match): greedy_lists[i][t] = the greedy id after the first t + 1
        tokens of the run, bit for bit decode_step's on that sequence alone; n_match[i] = the leading draft tokens the model agrees with.  The rows stay
        PENDING until commit_multi: the slots' linear-attention state is untouched, and every other slot call is refused."""
        return self._verify_multi(self._lib.kr_decode_verify_multi, slots, token_lists, positions)

    def _verify_multi(self, entry, slots, token_lists, positions):
        """verify_multi / verify_multi_sample: the runs flattened, the call, the ids cut back into one list per row"""
        self._need()
        n = len(slots)
        if len(token_lists) != n or len(positions) != n:
            raise ValueError(f"{n} slots, {len(token_lists)} token lists, {len(positions)} positions")
        flat = [int(t) for run in token_lists for t in run]
        arr = lambda xs: (C.c_int32 * max(len(xs), 1))(*xs)
        counts = [len(run) for run in token_lists]
        ids = (C.c_int32 * max(len(flat), 1))(); nm = (C.c_int32 * max(n, 1))()
        check(entry(self._h, n, arr(list(slots)), arr(counts), arr(flat), arr(list(positions)), ids, nm, None))
        self._multi_verify_rows = n
        out, o = [], 0
        for c in counts:
            out.append(list(ids[o:o + c])); o += c
        return out, list(nm[:n])

    def commit_multi(self, n_keep: Sequence[int]) -> None:
        """kr_decode_commit_multi: keep the first n_keep[i] tokens of row i of the pending verify_multi (0 <= n_keep[i] <= n_match[i] + 1; 0 leaves the slot
        as it was before the verify).  Each slot is then bit-identical to n_keep[i] decode_step calls on those tokens."""
        self._need()
        rows = getattr(self, "_multi_verify_rows", None)
        if rows is not None and len(n_keep) != rows:
            raise ValueError(f"{len(n_keep)} n_keep values for the {rows} rows of the pending verify")
        check(self._lib.kr_decode_commit_multi(self._h, (C.c_int32 * max(len(n_keep), 1))(*[int(k) for k in n_keep])))
        self._multi_verify_rows = None

    def generate_multi_lookup(self, slots: Sequence[int], first_tokens: Sequence[int], start_positions: Sequence[int], max_tokens: int,
                              contexts: Optional[Sequence[Sequence[int]]] = None, max_draft: int = LOOKUP_MAX_DRAFT, ngram_max: int = 3,
                              stop_ids: Sequence[int] = ()) -> List[List[int]]:
        """kr_decode_generate_multi_lookup: the tokens and slot states of generate_multi(slots, first_tokens, start_positions, max_tokens, stop_ids) in fewer
        passes where a row's text repeats its context (contexts[i], e.g. its prompt) or itself: prompt-lookup drafts per row, one verify_multi +
        commit_multi per pass.  last_multi_lookup_stats = {"passes": passes, "accepted": accepted draft tokens per row}."""
        return self._generate_multi(self._lib.kr_decode_generate_multi_lookup, slots, first_tokens, start_positions, max_tokens, stop_ids,
                                    lookup=(contexts, max_draft, ngram_max))

    # ------------------------------------------------------------------ sampled speculation over slots (docs/design/19-multi-verify-sample.md)
    def verify_multi_sample(self, slots: Sequence[int], token_lists: Sequence[Sequence[int]], positions: Sequence[int]):
        """kr_decode_verify_multi_sample: verify_multi whose ids are drawn by the slots' samplers (set_slot_sampler).  Returns (sampled_lists, n_match):
        sampled_lists[i][t] for t <= n_match[i] = the id step_multi_sample gives after the first t + 1 tokens of the run are consumed one by one (entries past
        n_match[i] are unspecified); n_match[i] = the leading draft tokens that equal those draws.  No sampler state is written; the rows stay PENDING until
        commit_multi, which then also advances each slot's seen set and RNG state by the draws kept."""
        return self._verify_multi(self._lib.kr_decode_verify_multi_sample, slots, token_lists, positions)

    def generate_multi_lookup_sample(self, slots: Sequence[int], first_tokens: Sequence[int], start_positions: Sequence[int], max_tokens: int,
                                     contexts: Optional[Sequence[Sequence[int]]] = None, max_draft: int = LOOKUP_MAX_DRAFT, ngram_max: int = 3,
                                     stop_ids: Sequence[int] = (), temperature=None, top_k=None, top_p=None, presence_penalty=None,
                                     rng_seeds=None) -> List[List[int]]:
        """kr_decode_generate_multi_lookup_sample: the tokens, slot states and sampler states of generate_multi(..., temperature=, top_k=, top_p=,
        presence_penalty=, rng_seeds=) (a scalar or one value per row; defaults 0, 0, 1.0, 0, 0) in fewer passes: prompt-lookup drafts per row, one
        verify_multi_sample + commit_multi per pass.  last_multi_lookup_stats = {"passes": passes, "accepted": accepted draft tokens per row}."""
        return self._generate_multi(self._lib.kr_decode_generate_multi_lookup_sample, slots, first_tokens, start_positions, max_tokens, stop_ids,
                                    lookup=(contexts, max_draft, ngram_max), sampler=(temperature, top_k, top_p, presence_penalty, rng_seeds))

    def slot_sampler_state(self, slot: int):
        """kr_decode_slot_sampler_get: (seen-token bitmap as uint32 [(vocab + 31) // 32], xorshift64 state) of the slot's sampler; zeros before any
        sampler was set."""
        self._need()
        seen = np.zeros((self._vocab + 31) // 32, np.uint32)
        rng = C.c_uint64()
        check(self._lib.kr_decode_slot_sampler_get(self._h, slot, seen.ctypes.data, C.byref(rng)))
        return seen, rng.value

    MULTI_PATH_COUNTS = ("passes", "verify", "few", "xs_split", "mla_xs_split", "gqa_xm", "mla_xm", "lx", "lx_runs", "lx_short", "fd", "mla_fd",
                         "gqa_flash", "mla_flash", "lc", "runs", "gguf_exact", "gguf_grouped", "seq_passes", "seq_few")      # KR_MPC_* of krasis_hip.h, in order

    def multi_path_counts(self, reset: bool = False) -> dict:
        """kr_decode_multi_path_counts (test aid): which forms the multi-row passes of this store took so far -- host-side counters, one count per batched
        pass over slots that was queued without an error, read from the pass's plan, its few-row flag and the GGUF option bits (the values the layer loop
        branches on); "seq_passes" / "seq_few" count the store's own prompt / verify passes.  reset=True clears them after the read."""
        self._need()
        out = (C.c_int64 * len(self.MULTI_PATH_COUNTS))()
        check(self._lib.kr_decode_multi_path_counts(self._h, out, len(out), 1 if reset else 0))
        return dict(zip(self.MULTI_PATH_COUNTS, (int(x) for x in out)))

    def prefill_slot(self, slot: int, tokens: Sequence[int], start_pos: int = 0, chunk: Optional[int] = None) -> int:
        """A prompt straight into a slot: extend_multi over chunks of `chunk` tokens (default KR_EXTEND_MAX_TOKENS).  The slot afterwards equals
        prefill(tokens, start_pos) + save_slot bit for bit, and the store's own sequence, logits and last token are never touched.  Returns the greedy id
        after the last token.  After set_option("multi_extend_flash", 1) every chunk of two or more tokens takes the prompt pass's flash attention in
        its GQA layers (see extend_multi): the slot then equals prefill under set_attention_mode(True) on a store of GQA layers, and a last chunk
        of one token is an exact step.  After set_option("multi_extend_la_chunk", 1) every chunk of 64 or more tokens takes the prompt pass's chunked
        delta rule in its linear-attention layers (see extend_multi); a last chunk of fewer than 64 tokens takes the exact run kernels, as the
        store's own fast prompt pass does.  After set_option("multi_extend_mla_flash", 1) every chunk of two or more tokens takes the prompt pass's
        flash attention in its MLA layers (see extend_multi): the slot then equals prefill under set_attention_mode(True), and a last chunk of one
        token is an exact step.  After set_option("multi_extend_exact_mfma", 1) every chunk of two or more tokens takes the exact matrix-core
        attention passes in its GQA layers (see extend_multi): the slot is bit for bit what it is with the option off, only sooner; a last
        chunk of one token keeps its kernel (with "multi_attn_fast" set: that option's bits for that token).  After
        set_option("multi_extend_mla_exact_mfma", 1) the same holds for the MLA layers (see extend_multi): the slot is bit for bit what it is with
        the option off; a last chunk of one token keeps its kernel (with "multi_mla_fast" set: that option's bits for that token, a unit row,
        while the chunks of two or more tokens carry the exact bits).  After set_option("multi_extend_la_exact", 1) every chunk of
        "multi_extend_la_exact_min" or more tokens takes the staged exact form in its linear-attention layers (see extend_multi): the slot is bit
        for bit what it is with the option off; a shorter last chunk keeps the run kernels."""
        from ._lib import KR_EXTEND_MAX_TOKENS
        chunk = KR_EXTEND_MAX_TOKENS if chunk is None else int(chunk)
        if not 1 <= chunk <= KR_EXTEND_MAX_TOKENS:
            raise ValueError(f"chunk {chunk} outside [1, {KR_EXTEND_MAX_TOKENS}]")
        tokens = list(tokens)
        if not tokens:
            raise ValueError("prefill_slot: empty prompt")
        last = -1
        for i in range(0, len(tokens), chunk):
            last = self.extend_multi([slot], [tokens[i:i + chunk]], [start_pos + i])[0]
        return last

    def generate_stream(self, first_token: int, start_position: int, max_tokens: int, temperature: float, top_k: int, top_p: float,
                        stop_ids: Sequence[int], tokenizer, presence_penalty: float, on_token, rng_seed: int = 0) -> int:
        """decode.rs:3611 -- the cancellable loop of the reference's Rust server.  on_token(token_id, text, finish_reason) -> bool (False cancels);
        finish_reason is None, "stop", "length" or "cancelled".  `tokenizer` is anything with decode(ids, skip_special_tokens=...) (tokenizers /
        transformers) or None (text = "").  Returns the number of generated tokens."""
        self._need()
        from ._lib import TOKEN_CB
        reasons = {0: None, 1: "stop", 2: "length", 3: "cancelled"}
        err: list = []

        def cb(token, reason, _user):
            try:
                text = ""
                if tokenizer is not None and reason != 3:
                    try:
                        text = tokenizer.decode([int(token)], skip_special_tokens=True)
                    except TypeError:
                        text = tokenizer.decode([int(token)])
                return 1 if on_token(int(token), text or "", reasons[reason]) else 0
            except BaseException as e:        # an exception must not unwind through the C frame
                err.append(e)
                return 0

        cfn = TOKEN_CB(cb)
        n = C.c_int()
        stops = (C.c_int * max(len(stop_ids), 1))(*stop_ids)
        check(self._lib.kr_decode_generate_stream(self._h, first_token, start_position, max_tokens, temperature, top_k, top_p, stops, len(stop_ids),
                                                  presence_penalty, rng_seed, cfn, None, C.byref(n), None))
        if err:
            raise err[0]
        return n.value

    def sample(self, temperature: float, top_k: int = 0, top_p: float = 1.0, presence_penalty: float = 0.0, rng_seed: int = 0, reset_seen: bool = False) -> int:
        """sample_from_logits (decode.rs:3718) on the logits of the last decode_step / prefill."""
        self._need()
        t = C.c_int()
        check(self._lib.kr_decode_sample(self._h, temperature, top_k, top_p, presence_penalty, rng_seed, int(reset_seen), C.byref(t), None))
        return t.value

    def last_token(self) -> int:
        t = C.c_int(); check(self._lib.kr_decode_last_token(self._h, C.byref(t))); return t.value

    def set_use_graph(self, enable: bool) -> None:
        self._need(); check(self._lib.kr_decode_set_use_graph(self._h, int(enable)))

    def read_hidden(self, n: int) -> np.ndarray:
        out = np.empty(n, np.float32); check(self._lib.kr_decode_read_buffer(self._h, 0, _addr(out), n)); return out

    def read_logits(self) -> np.ndarray:
        """the f32 [vocab] logits the next sample() draws from (last decode_step, prefill or commit)"""
        out = np.empty(self._vocab, np.float32); check(self._lib.kr_decode_read_buffer(self._h, 6, _addr(out), self._vocab)); return out

    def read_router(self, n_experts: int, topk: int):
        """(logits [E], ids [k], weights [k]) the router of the LAST MoE layer produced in the most recent decode step (test / debug aid)"""
        lg = np.empty(n_experts, np.float32); ids = np.empty(topk, np.int32); w = np.empty(topk, np.float32)
        check(self._lib.kr_decode_read_buffer(self._h, 4, _addr(lg), n_experts))
        check(self._lib.kr_decode_read_buffer(self._h, 2, _addr(ids), topk))
        check(self._lib.kr_decode_read_buffer(self._h, 3, _addr(w), topk))
        return lg, ids, w

    def device_bytes(self) -> int:
        self._need(); return int(self._lib.kr_decode_device_bytes(self._h))

    def profile_step(self, token_id: int, position: int):
        """one un-graphed decode step with HIP events around every launch -> [(ms, launches)] per kernel kind (include/krasis_hip.h lists the kinds);
        the stand-in for KRASIS_CPU_DECODE_TIMING's per-op buckets (decode.rs:3477-3517)"""
        self._need()
        ms = (C.c_double * 16)(); cnt = (C.c_long * 16)()
        check(self._lib.kr_decode_profile_step(self._h, token_id, position, ms, cnt, 16))
        return [(ms[i], cnt[i]) for i in range(16)]
