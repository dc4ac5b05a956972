// kr_decode_multi.cpp -- exact batched decode of many sequences held in device slots (docs/design/13-multi-sequence.md).
//
// A slot holds one sequence's per-layer state on the device: the KV rows of every GQA layer, the conv + recurrent state of every
// linear-attention layer.  kr_decode_step_multi advances B slots by one token each in one pass through the prompt pass's per-layer sequence
// (kr_multi_pass, kr_decode_prefill.cpp): the row-wise sections (norms, projection GEMMs, router, experts, lm_head) are the prompt pass's own,
// and each row of them equals the decode step bit for bit whatever rows share the pass; the two sections that tie rows to one sequence run
// per-slot kernels (kr_multi.hip) with the decode step's arithmetic.  So row i of a step carries exactly the bits kr_decode_step gives on
// that sequence alone.  The store's own sequence is the hand-over point: prompt pass -> kr_decode_slot_save -> steps -> kr_decode_slot_load.
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/krasis_hip.h"
#include "kr_decode_internal.h"

namespace {
int multi_ready(kr_decode_store* s) {
    if (!s) return kr_fail(KR_ERR_VALUE, "null decode store");
    if (!s->configured) return kr_fail(KR_ERR_STATE, "Call configure_decode first");
    if ((int)s->layers.size() != s->n_layers) return kr_fail(KR_ERR_STATE, "finalize_decode was not called");
    return KR_OK;
}
// what the multi-sequence step does not run (cf. kr_spec_refuse): tolerance modes, MLA, native-GGUF MoE layers, expert parallelism, geometries
// the per-slot kernels do not cover; a pending verify
int multi_refuse(kr_decode_store* s) {
    if (int rc = kr_spec_pending_fail(s)) return rc;
    if (s->attn_fast || s->gemm_fast || s->decode_fast)
        return kr_fail(KR_ERR_STATE, "the multi-sequence step is exact-mode only: the attention mode has tolerance bits set (%d)", s->attn_fast | s->gemm_fast << 1 | s->decode_fast << 2);
    kr_engine* e = s->eng;
    if (e->ep) return kr_fail(KR_ERR_STATE, "the multi-sequence step does not run under expert parallelism");
    for (size_t i = 0; i < s->layers.size(); i++) {
        const DLayer& L = s->layers[i];
        if (L.attn == ATTN_MLA) return kr_fail(KR_ERR_STATE, "the multi-sequence step does not cover MLA layers (layer %zu)", i);
        if (L.mlp == MLP_MOE) {
            if (s->own_eng || L.moe_layer >= (int)e->layers.size()) return kr_fail(KR_ERR_STATE, "set_moe_store was not called (MoE layer %d has no engine)", L.moe_layer);
            if (e->layers[L.moe_layer].gguf)
                return kr_fail(KR_ERR_STATE, "the multi-sequence step is exact-mode only: MoE layer %d holds native GGUF experts (their prompt pass is tolerance-only)", L.moe_layer);
        }
        if (L.attn == ATTN_LA && (L.kd != 4 || (L.dk != 64 && L.dk != 128) || L.dv > 256 || L.dv % 8 || L.nv != L.nk * (L.nv / L.nk)))
            return kr_fail(KR_ERR_VALUE, "multi-sequence step: linear-attention geometry kd %d dk %d dv %d not covered (kd 4, dk 64 / 128, dv <= 256)", L.kd, L.dk, L.dv);
        if (L.attn == ATTN_GQA && ((L.hd != 64 && L.hd != 128 && L.hd != 256) || L.nkv < 1 || L.nh % L.nkv || (L.nh / L.nkv) * (L.hd + 64) > 12288))
            return kr_fail(KR_ERR_VALUE, "multi-sequence step: GQA geometry nh %d nkv %d head_dim %d not covered (head_dim 64 / 128 / 256)", L.nh, L.nkv, L.hd);
    }
    return KR_OK;
}
int need_slots(kr_decode_store* s) {
    if (!s->multi || s->multi->n_slots == 0) return kr_fail(KR_ERR_STATE, "no sequence slots: call kr_decode_slots_create first");
    if (s->multi->kv_fp8 != s->kv_fp8)
        return kr_fail(KR_ERR_STATE, "the slots hold %s KV rows but the store uses %s now: create them again", s->multi->kv_fp8 ? "E4M3" : "FP16", s->kv_fp8 ? "E4M3" : "FP16");
    return KR_OK;
}
// the rows of one step: distinct slots in range, tokens in the vocabulary, positions inside the slot and the rope table
int check_rows(kr_decode_store* s, int n, const int32_t* slots, const int32_t* tokens, const int32_t* positions, int extra) {
    const kr_multi_state& M = *s->multi;
    if (n < 1 || n > KR_MULTI_MAX) return kr_fail(KR_ERR_VALUE, "%d rows, must be in [1, %d]", n, KR_MULTI_MAX);
    if (!slots || !tokens || !positions) return kr_fail(KR_ERR_VALUE, "null slots / tokens / positions");
    std::vector<char> seen((size_t)M.n_slots, 0);
    for (int i = 0; i < n; i++) {
        if (slots[i] < 0 || slots[i] >= M.n_slots) return kr_fail(KR_ERR_VALUE, "row %d: slot %d out of range [0, %d)", i, slots[i], M.n_slots);
        if (seen[(size_t)slots[i]]++) return kr_fail(KR_ERR_VALUE, "slot %d is named twice", slots[i]);
        if (tokens[i] < 0 || tokens[i] >= s->vocab) return kr_fail(KR_ERR_VALUE, "row %d: token id %d out of range (vocab %d)", i, tokens[i], s->vocab);
        const int last = positions[i] + extra;     // the last position this call consumes
        if (positions[i] < 0 || last >= M.max_seq) return kr_fail(KR_ERR_VALUE, "row %d: positions [%d, %d] outside the slot's [0, %d)", i, positions[i], last, M.max_seq);
        if (s->max_rope_seq > 0 && last >= s->max_rope_seq) return kr_fail(KR_ERR_VALUE, "row %d: position %d past the rope table (%d)", i, last, s->max_rope_seq);
    }
    return KR_OK;
}
// one step, arguments checked: rows -> device, the pass, per-row argmax, ids (and logits) back; returns once next_out is written
int step_impl(kr_decode_store* s, int n, const int32_t* slots, const int32_t* tokens, const int32_t* positions, int32_t* next_out, float* logits_out, hipStream_t st) {
    kr_multi_state& M = *s->multi;
    if (M.rows.ensure((size_t)3 * KR_MULTI_MAX * 4) || M.ids.ensure((size_t)KR_MULTI_MAX * 4)) return kr_fail(KR_ERR_HIP, "hipMalloc of the step's row buffers failed");
    std::vector<int32_t> h((size_t)3 * n);
    int max_pos = 0;
    for (int i = 0; i < n; i++) { h[(size_t)i] = slots[i]; h[(size_t)n + i] = tokens[i]; h[(size_t)2 * n + i] = positions[i]; max_pos = std::max(max_pos, positions[i]); }
    KR_HIP(hipMemcpyAsync(M.rows.p, h.data(), h.size() * 4, hipMemcpyHostToDevice, st));
    if (int rc = kr_multi_pass(s, n, (const int32_t*)M.rows.p, max_pos, st)) { (void)hipStreamSynchronize(st); return rc; }
    const size_t V = (size_t)s->vocab;
    kr_launch_multi_argmax((const float*)M.logits.p, V, (int)V, n, (int*)M.ids.p, st);
    KR_HIP(hipGetLastError());
    KR_HIP(hipMemcpyAsync(next_out, M.ids.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (logits_out) KR_HIP(hipMemcpyAsync(logits_out, M.logits.p, (size_t)n * V * 4, is_device_ptr(logits_out) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    KR_HIP(hipStreamSynchronize(st));
    return KR_OK;
}
// the step runs after everything the store has queued (its last step / prompt pass, whose side streams joined that stream)
int order_after_store(kr_decode_store* s, hipStream_t st) {
    kr_multi_state& M = *s->multi;
    if (!s->last_stream || s->last_stream == st) return KR_OK;
    if (!M.ev) KR_HIP(hipEventCreateWithFlags(&M.ev, hipEventDisableTiming));
    KR_HIP(hipEventRecord(M.ev, s->last_stream));
    KR_HIP(hipStreamWaitEvent(st, M.ev, 0));
    return KR_OK;
}
// slot <-> the store's own sequence: KV rows [0, seq_len) of every GQA layer, conv + recurrent state of every linear-attention layer
int slot_copy(kr_decode_store* s, int slot, int seq_len, bool save) {
    if (int rc = multi_ready(s)) return rc;
    if (int rc = need_slots(s)) return rc;
    if (int rc = multi_refuse(s)) return rc;
    kr_multi_state& M = *s->multi;
    if (slot < 0 || slot >= M.n_slots) return kr_fail(KR_ERR_VALUE, "slot %d out of range [0, %d)", slot, M.n_slots);
    const int lim = std::min(s->kv_max_seq, M.max_seq);
    if (seq_len < 0 || seq_len > lim) return kr_fail(KR_ERR_VALUE, "seq_len %d outside [0, %d] (store kv_max_seq %d, slot max_seq %d)", seq_len, lim, s->kv_max_seq, M.max_seq);
    for (size_t i = 0; i < s->layers.size(); i++)
        if (s->layers[i].attn == ATTN_GQA && !s->layers[i].kv_k.p) return kr_fail(KR_ERR_STATE, "set_decode_state was not called (no KV cache for layer %zu)", i);
    KR_HIP(hipSetDevice(s->eng->device));
    KR_HIP(hipDeviceSynchronize());          // steps / prompt passes still in flight on any stream read or write both sides
    hipStream_t st = s->eng->stream;
    for (size_t i = 0; i < s->layers.size(); i++) {
        DLayer& L = s->layers[i];
        char* a = (char*)M.a[i].p + (size_t)slot * M.a_stride[i];
        char* b = (char*)M.b[i].p + (size_t)slot * M.b_stride[i];
        void *sa, *sb; size_t na, nb;
        if (L.attn == ATTN_LA) { sa = L.conv_state.p; sb = L.recur_state.p; na = M.a_stride[i]; nb = M.b_stride[i]; }
        else if (L.attn == ATTN_GQA) { sa = L.kv_k.p; sb = L.kv_v.p; na = nb = (size_t)seq_len * L.nkv * L.hd * (M.kv_fp8 ? 1 : 2); }
        else continue;
        if (na) KR_HIP(hipMemcpyAsync(save ? (void*)a : sa, save ? sa : (void*)a, na, hipMemcpyDeviceToDevice, st));
        if (nb) KR_HIP(hipMemcpyAsync(save ? (void*)b : sb, save ? sb : (void*)b, nb, hipMemcpyDeviceToDevice, st));
    }
    KR_HIP(hipStreamSynchronize(st));
    return KR_OK;
}
}  // namespace

extern "C" int kr_decode_slots_create(kr_decode_store* s, int n_slots, int max_seq, size_t* bytes_out) {
    if (int rc = multi_ready(s)) return rc;
    if (n_slots < 0 || (n_slots > 0 && max_seq < 1)) return kr_fail(KR_ERR_VALUE, "bad slot geometry: %d slots of %d positions", n_slots, max_seq);
    for (size_t i = 0; i < s->layers.size(); i++)
        if (s->layers[i].attn == ATTN_MLA) return kr_fail(KR_ERR_STATE, "sequence slots do not cover MLA layers (layer %zu)", i);
    KR_HIP(hipSetDevice(s->eng->device));
    KR_HIP(hipDeviceSynchronize());          // a step in flight may still use the old slots
    s->multi.reset();
    if (bytes_out) *bytes_out = 0;
    if (n_slots == 0) return KR_OK;
    auto M = std::make_unique<kr_multi_state>();
    M->n_slots = n_slots; M->max_seq = max_seq; M->kv_fp8 = s->kv_fp8;
    const size_t nl = s->layers.size();
    M->a.resize(nl); M->b.resize(nl); M->a_stride.assign(nl, 0); M->b_stride.assign(nl, 0);
    size_t total = 0;
    for (size_t i = 0; i < nl; i++) {
        const DLayer& L = s->layers[i];
        if (L.attn == ATTN_LA) { M->a_stride[i] = (size_t)(2 * L.nk * L.dk + L.nv * L.dv) * L.kd * 4; M->b_stride[i] = (size_t)L.nv * L.dk * L.dv * 4; }
        else if (L.attn == ATTN_GQA) M->a_stride[i] = M->b_stride[i] = (size_t)max_seq * L.nkv * L.hd * (s->kv_fp8 ? 1 : 2);
        for (int h = 0; h < 2; h++) {
            DevBuf& d = h ? M->b[i] : M->a[i];
            const size_t bytes = (h ? M->b_stride[i] : M->a_stride[i]) * (size_t)n_slots;
            if (!bytes) continue;
            if (d.ensure(bytes)) return kr_fail(KR_ERR_HIP, "hipMalloc of %d sequence slots (%zu MiB so far) failed", n_slots, (total + bytes) >> 20);
            KR_HIP(hipMemsetAsync(d.p, 0, bytes, s->eng->stream));
            total += bytes;
        }
    }
    KR_HIP(hipStreamSynchronize(s->eng->stream));
    s->multi = std::move(M);
    if (bytes_out) *bytes_out = total;
    return KR_OK;
}

extern "C" int kr_decode_slot_save(kr_decode_store* s, int slot, int seq_len) { return slot_copy(s, slot, seq_len, true); }
extern "C" int kr_decode_slot_load(kr_decode_store* s, int slot, int seq_len) { return slot_copy(s, slot, seq_len, false); }

extern "C" int kr_decode_step_multi(kr_decode_store* s, int n, const int32_t* slots, const int32_t* tokens, const int32_t* positions,
                                    int32_t* next_out, float* logits_out, void* stream) {
    if (int rc = multi_ready(s)) return rc;
    if (int rc = need_slots(s)) return rc;
    if (int rc = multi_refuse(s)) return rc;
    if (int rc = check_rows(s, n, slots, tokens, positions, 0)) return rc;
    if (!next_out) return kr_fail(KR_ERR_VALUE, "null next_out");
    KR_HIP(hipSetDevice(s->eng->device));
    hipStream_t st = kr_pick_stream(s->eng, stream);
    if (int rc = order_after_store(s, st)) return rc;
    return step_impl(s, n, slots, tokens, positions, next_out, logits_out, st);
}

extern "C" int kr_decode_generate_multi(kr_decode_store* s, int n, const int32_t* slots, const int32_t* first_tokens, const int32_t* start_positions,
                                        int max_tokens, const int* stop_ids, int n_stop, int32_t* tokens_out, int32_t* n_out, void* stream) {
    if (int rc = multi_ready(s)) return rc;
    if (int rc = need_slots(s)) return rc;
    if (int rc = multi_refuse(s)) return rc;
    if (max_tokens < 0) return kr_fail(KR_ERR_VALUE, "max_tokens %d < 0", max_tokens);
    if (n_stop < 0 || (n_stop > 0 && !stop_ids)) return kr_fail(KR_ERR_VALUE, "bad stop ids (%d)", n_stop);
    if (!n_out || (max_tokens > 0 && !tokens_out)) return kr_fail(KR_ERR_VALUE, "null output pointer");
    // every row's last step (position start + max_tokens - 1) must fit its slot: checked here, before the first step
    if (int rc = check_rows(s, n, slots, first_tokens, start_positions, std::max(max_tokens - 1, 0))) return rc;
    for (int i = 0; i < n; i++) n_out[i] = 0;
    if (max_tokens == 0) return KR_OK;
    KR_HIP(hipSetDevice(s->eng->device));
    hipStream_t st = kr_pick_stream(s->eng, stream);
    if (int rc = order_after_store(s, st)) return rc;
    auto is_stop = [&](int t) { for (int j = 0; j < n_stop; j++) if (stop_ids[j] == t) return true; return false; };
    std::vector<int> act((size_t)n);                           // rows still generating, in caller order
    std::vector<int32_t> sl((size_t)n), tk((size_t)n), ps((size_t)n), nx((size_t)n);
    for (int i = 0; i < n; i++) { act[(size_t)i] = i; tk[(size_t)i] = first_tokens[i]; ps[(size_t)i] = start_positions[i]; }
    while (!act.empty()) {
        const int m = (int)act.size();
        std::vector<int32_t> rt((size_t)m), rp((size_t)m);
        for (int k = 0; k < m; k++) { const int i = act[(size_t)k]; sl[(size_t)k] = slots[i]; rt[(size_t)k] = tk[(size_t)i]; rp[(size_t)k] = ps[(size_t)i]; }
        if (int rc = step_impl(s, m, sl.data(), rt.data(), rp.data(), nx.data(), nullptr, st)) return rc;
        std::vector<int> keep;
        for (int k = 0; k < m; k++) {
            const int i = act[(size_t)k], t = nx[(size_t)k];
            tokens_out[(size_t)i * max_tokens + n_out[i]++] = t;
            tk[(size_t)i] = t; ps[(size_t)i]++;
            if (!is_stop(t) && n_out[i] < max_tokens) keep.push_back(i);   // a finished row leaves the batch: its slot is not stepped again
        }
        act.swap(keep);
    }
    return KR_OK;
}
