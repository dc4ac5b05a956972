// kr_decode_multi.cpp -- exact batched decode of many sequences held in device slots (docs/design/13-multi-sequence.md).
//
// A slot holds one sequence's per-layer state on the device: the KV rows of every GQA layer, the compressed-KV and rope-key rows of every MLA
// layer (docs/design/15-multi-mla.md), the conv + recurrent state of every linear-attention layer.  kr_decode_step_multi advances B slots by one token each in one pass through the prompt pass's per-layer sequence
// (kr_multi_pass, kr_decode_prefill.cpp): the row-wise sections (norms, projection GEMMs, router, experts, lm_head) are the prompt pass's own,
// and each row of them equals the decode step bit for bit whatever rows share the pass; the sections that tie rows to one sequence (linear attention, GQA, MLA) run
// per-slot kernels (kr_multi.hip) with the decode step's arithmetic.  So row i of a step carries exactly the bits kr_decode_step gives on
// that sequence alone.  The store's own sequence is the hand-over point: prompt pass -> kr_decode_slot_save -> steps -> kr_decode_slot_load.
// kr_decode_extend_multi (docs/design/17-multi-extend.md) is the same pass with a run of tokens per row: a prompt enters a slot chunk by chunk beside the
// decode rows of other slots, each run bit-identical to that many kr_decode_step calls, without the store's own sequence.  A step is an extend whose every
// run has one token: both take one argument check, one flatten and one pass (step_entry / step_impl below).  The rows of a call travel as one Rows value
// from the entry points inward.
// kr_decode_verify_multi / kr_decode_commit_multi (docs/design/18-multi-verify.md) are that pass once more, for exact greedy speculation: runs of [sampled token,
// draft] whose linear-attention sections record instead of storing state, the greedy id after every token, and a commit that advances each slot by the tokens
// kept.  kr_decode_verify_multi_sample (docs/design/19-multi-verify-sample.md) draws every token row with its slot's sampler instead, under the hypothesis
// that the drafts before it were the sampler's draws; the commit applies the kept draws to the samplers.  All four generation entry points
// (kr_decode_generate_multi, its _sample, _lookup and _lookup_sample forms) are one loop, generate_slots: steps where no row drafts (max_draft 0: always),
// verify + commit where one does, with the draft rule of kr_lookup_index.h.
// Paged slots (kr_decode_slots_create_paged, docs/design/21-paged-slots.md): the GQA / MLA rows live in pools of pages shared by all slots; every entry point maps
// the pages its rows need on the host first, all or nothing, and the pass opens by sending the changed table entries and zeroing the new pages.  The table, the
// free list and the queue of unseen mappings are KrPagePool's (kr_page_pool.h), which prunes the queue itself; here: its members, and flush_plan() carried out (pg_flush).
// kr_decode_slot_fork (docs/design/22-slot-fork.md): a slot's prefix into other slots without the prompt pass -- paged slots share the whole pages below the fork
// point by reference count, and the reservation of every call that writes rows first gives a row a private copy of a page other slots hold too.
// kr_decode_slots_export / kr_decode_slots_import (docs/design/38-slot-swap.md): a slot's whole state out to one self-describing host image (kr_slot_image.h) and back
// into any slot of any compatible slot set, through a staging buffer of two halves and the two kernels of kr_multi_swap.hip.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "../../include/krasis_hip.h"
#include "kr_decode_internal.h"
#include "kr_lookup_index.h"
#include "kr_multi_sample.h"
#include "kr_sampler.h"

namespace {
int multi_ready(kr_decode_store* s) {
    if (!s) return kr_fail(KR_ERR_VALUE, "null decode store");
    if (!s->configured) return kr_fail(KR_ERR_STATE, "Call configure_decode first");
    if ((int)s->layers.size() != s->n_layers) return kr_fail(KR_ERR_STATE, "finalize_decode was not called");
    return KR_OK;
}
// what the multi-sequence step does not run: a pending verify of the store's own sequence, then what kr_exact_refuse (kr_decode_prefill.cpp) lists for the
// slots -- the base clauses of every exact pass and, among them, those of the per-slot kernels -- then the slot options' ordered rule list (kr_option_rules)
int multi_refuse(kr_decode_store* s) {
    if (int rc = kr_spec_pending_fail(s)) return rc;
    if (int rc = kr_exact_refuse(s, true)) return rc;
    return kr_option_rules(s, false);
}
int need_slots(kr_decode_store* s) {
    if (!s->multi || s->multi->n_slots == 0) return kr_fail(KR_ERR_STATE, "no sequence slots: call kr_decode_slots_create first");
    if (s->multi->kv_fp8 != s->kv_fp8)
        return kr_fail(KR_ERR_STATE, "the slots hold %s KV rows but the store uses %s now: create them again", s->multi->kv_fp8 ? "E4M3" : "FP16", s->kv_fp8 ? "E4M3" : "FP16");
    return KR_OK;
}
// what every entry point that touches the slots starts with (kr_decode_commit_multi apart): between a verify over slots and its commit nothing else runs on
// them -- the run table and the records belong to the pending rows
int multi_begin(kr_decode_store* s) {
    if (int rc = multi_ready(s)) return rc;
    if (int rc = need_slots(s)) return rc;
    if (s->multi->v_pending) return kr_fail(KR_ERR_STATE, "a verify over slots is pending: call kr_decode_commit_multi first");
    if (int rc = multi_refuse(s)) return rc;
    return kr_option_rules(s, true);      // preparing is not refusing: the options' LDS windows, once every refusal has passed
}
int slot_in_range(kr_decode_store* s, int slot) {
    return slot < 0 || slot >= s->multi->n_slots ? kr_fail(KR_ERR_VALUE, "slot %d out of range [0, %d)", slot, s->multi->n_slots) : KR_OK;
}
// ---- paged slots (docs/design/21-paged-slots.md): the GQA / MLA rows live in pools of pages shared by all slots; M.pg is the allocator and the table
// "multi_attn_fast" reads flat slots only: with that option alone every batched call on paged slots is refused (an option that silently does nothing is a
// trap); "multi_attn_fast_paged" is the option that reads both kinds (docs/design/23-multi-attn-fast-paged.md)
int paged_refuse(kr_decode_store* s) {
    if (paged_refused(s))
        return kr_fail(KR_ERR_STATE, "\"multi_attn_fast\" does not read paged slots (kr_decode_slots_create_paged): set \"multi_attn_fast_paged\", clear the option or create flat slots");
    return KR_OK;
}
// all or nothing, on the host: slot slots[i] gets the pages that cover [0, lens[i]), lowest free id first; the mappings wait in the pool's queue for pg_flush
// and are appended to log (a caller that gives some back later).  from (null: the call writes no rows) = the first position each slot writes: a page there
// that other slots hold too is replaced by a private copy, counted in the same sum (docs/design/22-slot-fork.md)
int pg_reserve(kr_decode_store* s, int n, const int32_t* slots, const long long* lens, const long long* from, std::vector<KrPageChange>* log) {
    kr_multi_state& M = *s->multi;
    if (!M.pg.paged()) return KR_OK;
    int need = 0, have = 0;
    const int bad = M.pg.reserve(n, slots, lens, log, &need, &have, from);
    if (bad < 0) return KR_OK;
    return kr_fail(KR_ERR_STATE, "row %d: slot %d does not fit the page pool: positions [0, %lld) bring the call to %d more pages of %d positions, %d of %d are free",
                   bad, slots[bad], lens[bad], need, M.pg.page_tokens, have, M.pg.n_pages);
}
// table entries [lo, hi] of a slot -> the device copy (pageable source: staged before the call returns)
int pg_upload(kr_multi_state& M, int slot, int lo, int hi, hipStream_t st) {
    const size_t o = (size_t)slot * M.pg.stride + (size_t)lo;
    KR_HIP(hipMemcpyAsync((int32_t*)M.pg_table.p + o, M.pg.table.data() + o, (size_t)(hi - lo + 1) * 4, hipMemcpyHostToDevice, st));
    return KR_OK;
}
// what the host mapped since the last pass -> the device, on the pass's stream ahead of the pass: the changed table entries, then ONE launch that makes the
// new pages read as zero in every layer's pools, as a freshly created flat slot does, then ONE launch for the pages that start as a copy of another (a fork's
// boundary page, a private copy of a shared page: written whole by that launch, so not zeroed first).  A copy that reads the page an earlier queued copy
// writes goes into a launch of its own behind it.  What to send is the pool's plan (flush_plan); sources are held until flushed(): an error leaves all queued and held
int pg_flush(kr_multi_state& M, hipStream_t st) {
    if (M.pg.pending.empty()) return KR_OK;
    const KrPageFlush f = M.pg.flush_plan();
    for (const KrPageFlush::Range& r : f.ranges) if (int rc = pg_upload(M, r.slot, r.lo, r.hi, st)) return rc;
    if (!f.zero.empty()) {
        KR_HIP(hipMemcpyAsync(M.pg_new.p, f.zero.data(), f.zero.size() * 4, hipMemcpyHostToDevice, st));      // pg_new holds n_pages ids, and a page is pending once
        kr_launch_multi_zero_pages((const KrPagePoolDev*)M.pg_pools.p, M.pg_npools, (const int*)M.pg_new.p, (int)f.zero.size(), st);
    }
    if (const size_t nc = f.copies[0].size()) {      // behind the ids to zero: [dst | src | rows], n_pages each (a page is a destination once)
        int32_t* ids = (int32_t*)M.pg_new.p + (size_t)M.pg.n_pages;
        for (int k = 0; k < 3; k++) KR_HIP(hipMemcpyAsync(ids + (size_t)k * M.pg.n_pages, f.copies[k].data(), nc * 4, hipMemcpyHostToDevice, st));
        size_t c0 = 0;
        for (size_t end : f.ends) {      // one launch, unless a copy reads what an earlier one writes
            kr_launch_multi_copy_pages((const KrPagePoolDev*)M.pg_pools.p, M.pg_npools, ids + c0, ids + (size_t)M.pg.n_pages + c0, ids + (size_t)2 * M.pg.n_pages + c0, (int)(end - c0),
                                       M.pg.page_tokens, st);
            c0 = end;
        }
    }
    KR_HIP(hipGetLastError());
    M.pg.flushed();      // enqueued: what follows on this stream may take the copies' sources
    return KR_OK;
}
// pages went back to the pool (freed; the pool has dropped the queued mappings of them): the slots' whole table rows go to the device
int pg_released(kr_decode_store* s, const std::vector<KrPageChange>& freed) {
    kr_multi_state& M = *s->multi;
    if (freed.empty()) return KR_OK;
    KR_HIP(hipSetDevice(s->eng->device));
    std::vector<char> hit((size_t)M.n_slots, 0);
    for (const KrPageChange& c : freed) hit[(size_t)c.slot] = 1;
    for (int sl = 0; sl < M.n_slots; sl++) if (hit[(size_t)sl]) if (int rc = pg_upload(M, sl, 0, M.pg.stride - 1, s->eng->stream)) return rc;
    KR_HIP(hipStreamSynchronize(s->eng->stream));
    return KR_OK;
}
// the rows of one call, as they travel from the entry points inward: row i = slot slots[i] runs cnt(i) tokens of `tokens` (the runs in call order) at
// positions[i] ...
struct Rows {
    int n; const int32_t *slots, *counts, *tokens, *positions;      // counts null: one token per row
    int cnt(int i) const { return counts ? counts[i] : 1; }
};
// their check, every refusal naming its row: distinct slots in range, tokens in the vocabulary, positions inside the slot and the rope tables (the store's, and
// every MLA layer's own: the shortest bounds the call).  extra = further positions the caller will consume after the run (generate_slots)
int check_args(kr_decode_store* s, const Rows& r, int extra) {
    const kr_multi_state& M = *s->multi;
    if (r.n < 1 || r.n > KR_MULTI_MAX) return kr_fail(KR_ERR_VALUE, "%d rows, must be in [1, %d]", r.n, KR_MULTI_MAX);
    if (!r.slots || !r.tokens || !r.positions) return kr_fail(KR_ERR_VALUE, "null slots / counts / tokens / positions");
    std::vector<char> seen((size_t)M.n_slots, 0);
    int mla_rope = 0; bool has_mla = false;
    for (const DLayer& L : s->layers) if (L.attn == ATTN_MLA) { mla_rope = has_mla ? std::min(mla_rope, L.mla_rope_seq) : L.mla_rope_seq; has_mla = true; }
    // "multi_mla_fast" over long slots: the merge has one thread per chunk (kr_multi_pass takes the same chunk size)
    const int mla_chunk = s->mopt.mla_fast && has_mla && M.max_seq > s->mla_split_min ? kr_mla_flash_decode_chunk(M.max_seq) : 0;
    int total = 0;
    for (int i = 0; i < r.n; i++) {      // the runs first: everything below indexes tokens by them
        if (r.cnt(i) < 1) return kr_fail(KR_ERR_VALUE, "row %d: a run of %d tokens, must be at least 1", i, r.cnt(i));
        if (r.cnt(i) > KR_EXTEND_MAX_TOKENS - total)
            return kr_fail(KR_ERR_VALUE, "row %d: its run of %d tokens brings the call past %d tokens (KR_EXTEND_MAX_TOKENS)", i, r.cnt(i), KR_EXTEND_MAX_TOKENS);
        total += r.cnt(i);
    }
    total = 0;
    for (int i = 0; i < r.n; i++) {
        const int slot = r.slots[i], pos = r.positions[i];
        if (slot < 0 || slot >= M.n_slots) return kr_fail(KR_ERR_VALUE, "row %d: slot %d out of range [0, %d)", i, slot, M.n_slots);
        if (seen[(size_t)slot]++) return kr_fail(KR_ERR_VALUE, "row %d: slot %d is named twice", i, slot);
        for (int t = 0; t < r.cnt(i); t++) {
            const int tk = r.tokens[(size_t)total + t];
            if (tk < 0 || tk >= s->vocab) return kr_fail(KR_ERR_VALUE, "row %d: token %d of its run, id %d, out of range (vocab %d)", i, t, tk, s->vocab);
        }
        total += r.cnt(i);
        const long long last = (long long)pos + r.cnt(i) - 1 + extra;     // the last position this row consumes
        if (pos < 0 || last >= M.max_seq) return kr_fail(KR_ERR_VALUE, "row %d: positions [%d, %lld] outside the slot's [0, %d)", i, pos, last, M.max_seq);
        if (s->max_rope_seq > 0 && last >= s->max_rope_seq) return kr_fail(KR_ERR_VALUE, "row %d: position %lld past the rope table (%d)", i, last, s->max_rope_seq);
        if (has_mla && last >= mla_rope) return kr_fail(KR_ERR_VALUE, "row %d: position %lld past the MLA rope table (%d)", i, last, mla_rope);
        if (mla_chunk && last / mla_chunk >= 1024)
            return kr_fail(KR_ERR_VALUE, "row %d: multi_mla_fast: position %lld needs %lld chunks of %d positions (at most 1024)", i, last, last / mla_chunk + 1, mla_chunk);
    }
    return KR_OK;
}
// paged slots: the pages row i still needs to cover [0, positions[i] + cnt(i) + extra), and a page of its own wherever it will write, from positions[i] on
int pg_reserve_rows(kr_decode_store* s, const Rows& r, int extra, std::vector<KrPageChange>* log) {
    if (!s->multi->pg.paged()) return KR_OK;
    std::vector<long long> lens((size_t)r.n), from((size_t)r.n);
    for (int i = 0; i < r.n; i++) { from[(size_t)i] = r.positions[i]; lens[(size_t)i] = (long long)r.positions[i] + r.cnt(i) + extra; }
    return pg_reserve(s, r.n, r.slots, lens.data(), from.data(), log);
}
// what a row with these sampler parameters does: the three paths of kr_decode_generate's loop (kr_decode.cpp generate_core)
KrMsRow mode_row(int slot, float temperature, int top_k, float top_p, float penalty, int vocab, bool force_loop) {
    KrMsRow r{KR_MS_GREEDY, slot, 0, top_k, temperature, 0.0f, top_p, penalty};
    r.k = (top_k > 0 && top_k < vocab) ? top_k : vocab;
    if (temperature == 0.0f) r.mode = penalty != 0.0f ? KR_MS_PENALTY : KR_MS_GREEDY;
    else { r.mode = (r.k <= KR_MS_SEL_CAP && !force_loop) ? KR_MS_SAMPLE : KR_MS_LOOP; r.inv_temp = 1.0f / temperature; }
    return r;
}
// row b of a sampled step: its slot's sampler (greedy while no slot has one)
KrMsRow sample_row(kr_decode_store* s, int slot) {
    const kr_multi_state& M = *s->multi;
    if (M.smp.empty()) return KrMsRow{KR_MS_GREEDY, slot, 0, 0, 0.0f, 0.0f, 1.0f, 0.0f};
    const kr_multi_state::Sampler& p = M.smp[(size_t)slot];
    return mode_row(slot, p.temperature, p.top_k, p.top_p, p.penalty, s->vocab, s->opt_multi_sample_loop != 0);
}
// device scratch of the batched sampler for n rows of these modes (the sampled step and verify, kr_sample_rows / kr_sample_runs), grown on demand: the
// rows and, behind them, their (run, t) table; the work copy [n][V]; the top-k keys [n][KR_MS_SEL_CAP]; the per-row path's scratch with the staged sampler
// of the verify form
int sampler_scratch(kr_multi_state& M, int vocab, int n, const std::vector<KrMsRow>& rows) {
    bool prep = false, sample = false, loop = false;
    for (const KrMsRow& r : rows) { prep |= r.mode != KR_MS_GREEDY; sample |= r.mode == KR_MS_SAMPLE; loop |= r.mode == KR_MS_LOOP; }
    const size_t V = (size_t)vocab, N = (size_t)std::max(n, KR_MULTI_MAX);
    const size_t work = prep ? (size_t)n * V * 4 : 0, sorted = sample ? (size_t)n * KR_MS_SEL_CAP * 8 : 0;
    bool bad = M.smp_rows.ensure(N * (sizeof(KrMsRow) + sizeof(KrMsAt))) || (work && M.smp_work.ensure(work)) || (sorted && M.smp_sorted.ensure(sorted));
    if (!bad && loop) {
        if (M.smp_temp_bytes == 0) M.smp_temp_bytes = kr_sampler_temp_bytes(vocab);
        bad = M.smp_keys.ensure(2 * V * 8) || M.smp_temp.ensure(M.smp_temp_bytes + 256) || M.smp_probs.ensure(V * 4) || M.smp_hyp.ensure(((V + 31) / 32) * 4 + 16);      // the staged bitmap, then its state on the next 8-byte boundary
    }
    if (bad) return kr_fail(KR_ERR_HIP, "hipMalloc of the batched sampler's scratch failed (%d rows: work copy %zu MiB, sorted keys %zu MiB)", n, work >> 20, sorted >> 20);
    return KR_OK;
}
// the (run, t) table of a verify-form call sits behind the rows
KrMsAt* sampler_at(kr_multi_state& M, int n) { return (KrMsAt*)((KrMsRow*)M.smp_rows.p + std::max(n, KR_MULTI_MAX)); }
KrMsArgs sampler_args(kr_multi_state& M, const float* logits, int vocab, int n, const std::vector<KrMsRow>& rows, uint32_t* seen, size_t words, uint64_t* rng, int* ids) {
    KrMsArgs a{};
    a.logits = logits; a.ld = (size_t)vocab; a.V = vocab; a.B = n;
    a.rows_dev = (const KrMsRow*)M.smp_rows.p; a.rows_host = rows.data();
    a.work = (float*)M.smp_work.p; a.sorted = (uint64_t*)M.smp_sorted.p;
    a.seen = seen; a.seen_words = words; a.rng = rng; a.ids = ids;
    a.loop_keys = (uint64_t*)M.smp_keys.p; a.loop_temp = M.smp_temp.p; a.loop_temp_bytes = M.smp_temp_bytes; a.loop_probs = (float*)M.smp_probs.p;
    return a;
}
// the rows of a pass -> M.rows on the device: [slots | tokens | positions] of T token rows, then the runs [n][slot, off, cnt] (kr_multi.h).  The last token of
// run i is row i and the others follow from row n on in call order (unit counts: row i = token i, off = n)
// lay_rows: that layout on the host (row_of, optional: the pass row of every token in call order)
std::vector<int32_t> lay_rows(const Rows& r, size_t& T, int& max_pos, std::vector<int>* row_of = nullptr) {
    const int n = r.n;
    T = 0;
    for (int i = 0; i < n; i++) T += (size_t)r.cnt(i);
    std::vector<int32_t> h(3 * T + (size_t)3 * n);
    if (row_of) row_of->resize(T);
    max_pos = 0;
    size_t src = 0, off = (size_t)n;
    for (int i = 0; i < n; i++) {
        const int c = r.cnt(i);
        int32_t* run = &h[3 * T + (size_t)3 * i];
        run[0] = r.slots[i]; run[1] = (int32_t)off; run[2] = c;
        for (int t = 0; t < c; t++) {
            const size_t row = t == c - 1 ? (size_t)i : off + t;
            h[row] = r.slots[i]; h[T + row] = r.tokens[src + t]; h[2 * T + row] = r.positions[i] + t;
            if (row_of) (*row_of)[src + t] = (int)row;
        }
        src += (size_t)c; off += (size_t)c - 1;
        max_pos = std::max(max_pos, r.positions[i] + c - 1);
    }
    return h;
}
int put_rows(kr_multi_state& M, const Rows& r, hipStream_t st, size_t& T, int& max_pos, std::vector<int>* row_of = nullptr) {
    if (M.rows.ensure((size_t)3 * (KR_EXTEND_MAX_TOKENS + KR_MULTI_MAX) * 4)) return kr_fail(KR_ERR_HIP, "hipMalloc of the step's row buffers failed");
    const std::vector<int32_t> h = lay_rows(r, T, max_pos, row_of);
    KR_HIP(hipMemcpyAsync(M.rows.p, h.data(), h.size() * 4, hipMemcpyHostToDevice, st));      // pageable source: staged before the call returns
    return KR_OK;
}
// the rows and (run, t) table of a verify-form sampler call in pass-row order: token t of run i draws with run i's sampler row
void run_rows(int n, const int32_t* counts, const std::vector<int>& row_of, const std::vector<KrMsRow>& per_run, std::vector<KrMsRow>& rows, std::vector<KrMsAt>& at) {
    rows.resize(row_of.size()); at.resize(row_of.size());
    size_t src = 0;
    for (int i = 0; i < n; i++)
        for (int t = 0; t < counts[i]; t++, src++) { rows[(size_t)row_of[src]] = per_run[(size_t)i]; at[(size_t)row_of[src]] = KrMsAt{i, t}; }
}
// the verify-form launches over the T token rows the pass left in `logits`: rows and table to the device, then every row's draw into ids [T]
int sample_runs(kr_multi_state& M, const float* logits, int vocab, const std::vector<KrMsRow>& rows, const std::vector<KrMsAt>& at, const int32_t* d_rows, uint32_t* seen,
                size_t words, uint64_t* rng, int* ids, hipStream_t st) {
    const int T = (int)rows.size();
    KR_HIP(hipMemcpyAsync(M.smp_rows.p, rows.data(), rows.size() * sizeof(KrMsRow), hipMemcpyHostToDevice, st));
    KR_HIP(hipMemcpyAsync(sampler_at(M, T), at.data(), at.size() * sizeof(KrMsAt), hipMemcpyHostToDevice, st));
    KrMsArgs a = sampler_args(M, logits, vocab, T, rows, seen, words, rng, ids);
    a.runs = d_rows + 3 * (size_t)T; a.tokens = d_rows + T; a.at_dev = sampler_at(M, T); a.at_host = at.data();
    a.hyp_seen = (uint32_t*)M.smp_hyp.p; a.hyp_rng = M.smp_hyp.p ? (uint64_t*)((char*)M.smp_hyp.p + ((words * 4 + 7) & ~(size_t)7)) : nullptr;
    if (kr_launch_multi_sample(a, st)) return kr_fail(KR_ERR_HIP, "batched sampler launch failed");
    return KR_OK;
}
// what step_impl and verify_impl open with: the rows to the device, then the pass's sampler rows -- one per run, or in the verify form one per token row
// with the (run, t) table -- and the scratch for them.  sr stays empty when the pass is greedy: sample unset, or no slot of it has a sampler that draws
struct Pass { size_t T = 0; int max_pos = 0; std::vector<KrMsRow> sr; std::vector<KrMsAt> at; };
int open_pass(kr_decode_store* s, const Rows& r, bool sample, bool verify, hipStream_t st, Pass& p) {
    kr_multi_state& M = *s->multi;
    std::vector<int> row_of;
    if (int rc = pg_flush(M, st)) return rc;      // paged slots: the table entries and zeroed pages of this pass's rows, ahead of the pass
    if (int rc = put_rows(M, r, st, p.T, p.max_pos, verify ? &row_of : nullptr)) return rc;
    std::vector<KrMsRow> per_run;
    bool greedy = true;
    if (sample) for (int i = 0; i < r.n; i++) { per_run.push_back(sample_row(s, r.slots[i])); greedy &= per_run.back().mode == KR_MS_GREEDY; }
    if (greedy) return KR_OK;
    if (verify) run_rows(r.n, r.counts, row_of, per_run, p.sr, p.at);
    else p.sr.swap(per_run);
    return sampler_scratch(M, s->vocab, (int)p.sr.size(), p.sr);
}
// and what they close with when the pass or a sampler launch failed: nothing of it is left in flight
int fail_pass(hipStream_t st, int rc) { (void)hipStreamSynchronize(st); return rc; }
// one pass, arguments checked: rows -> device, the pass, per-row argmax (sample: each slot's sampler), ids (and logits) back; returns once next_out is written.
// The pass has one row per token, the last token of run i in row i and the others from row n on in call order, so everything after the pass (logits, argmax,
// sampler) sees n rows
int step_impl(kr_decode_store* s, const Rows& r, int32_t* next_out, float* logits_out, hipStream_t st, bool sample) {
    kr_multi_state& M = *s->multi;
    const int n = r.n;
    if (M.ids.ensure((size_t)KR_MULTI_MAX * 4)) return kr_fail(KR_ERR_HIP, "hipMalloc of the step's row buffers failed");
    Pass p;
    if (int rc = open_pass(s, r, sample, false, st, p)) return rc;
    const bool greedy = p.sr.empty();
    if (!greedy) KR_HIP(hipMemcpyAsync(M.smp_rows.p, p.sr.data(), p.sr.size() * sizeof(KrMsRow), hipMemcpyHostToDevice, st));
    if (int rc = kr_multi_pass(s, (int)p.T, n, (const int32_t*)M.rows.p, (const int32_t*)M.rows.p + 3 * p.T, p.max_pos, st, false, r.counts, r.positions)) return fail_pass(st, rc);
    const size_t V = (size_t)s->vocab;
    if (greedy) kr_launch_multi_argmax((const float*)M.logits.p, V, (int)V, n, (int*)M.ids.p, st);
    else if (kr_launch_multi_sample(sampler_args(M, (const float*)M.logits.p, s->vocab, n, p.sr, (uint32_t*)M.smp_seen.p, M.smp_words, (uint64_t*)M.smp_rng.p, (int*)M.ids.p), st))
        return fail_pass(st, kr_fail(KR_ERR_HIP, "batched sampler launch failed"));
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
// the three stepping entry points: refusals, then the pass on the caller's stream
int step_entry(kr_decode_store* s, const Rows& r, int32_t* next_out, float* logits_out, bool sample, void* stream) {
    if (int rc = multi_begin(s)) return rc;
    if (int rc = check_args(s, r, 0)) return rc;
    if (!next_out) return kr_fail(KR_ERR_VALUE, "null next_out");
    if (int rc = paged_refuse(s)) return rc;
    if (int rc = pg_reserve_rows(s, r, 0, nullptr)) return rc;      // all or nothing, before anything is queued
    KR_HIP(hipSetDevice(s->eng->device));
    hipStream_t st = kr_pick_stream(s->eng, stream);
    if (int rc = order_after_store(s, st)) return rc;
    return step_impl(s, r, next_out, logits_out, st, sample);
}
// slot <-> the store's own sequence: KV rows [0, seq_len) of every GQA layer, compressed-KV and rope-key rows [0, seq_len) of every MLA layer, conv +
// recurrent state of every linear-attention layer
int slot_copy(kr_decode_store* s, int slot, int seq_len, bool save) {
    if (int rc = multi_begin(s)) return rc;
    if (int rc = slot_in_range(s, slot)) return rc;
    kr_multi_state& M = *s->multi;
    const int lim = std::min(s->kv_max_seq, M.max_seq);
    if (seq_len < 0 || seq_len > lim) return kr_fail(KR_ERR_VALUE, "seq_len %d outside [0, %d] (store kv_max_seq %d, slot max_seq %d)", seq_len, lim, s->kv_max_seq, M.max_seq);
    for (size_t i = 0; i < s->layers.size(); i++)
        if ((s->layers[i].attn == ATTN_GQA || s->layers[i].attn == ATTN_MLA) && (!s->layers[i].kv_k.p || !s->layers[i].kv_v.p))
            return kr_fail(KR_ERR_STATE, "set_decode_state was not called (no %s cache for layer %zu)", s->layers[i].attn == ATTN_MLA ? "MLA" : "KV", i);
    const bool paged = M.pg.paged();
    if (paged && save) { const int32_t sl = slot; const long long len = seq_len, from = 0; if (int rc = pg_reserve(s, 1, &sl, &len, &from, nullptr)) return rc; }      // what [0, seq_len) needs; the save writes all of it
    KR_HIP(hipSetDevice(s->eng->device));
    KR_HIP(hipDeviceSynchronize());          // steps / prompt passes still in flight on any stream read or write both sides
    hipStream_t st = s->eng->stream;
    if (int rc = pg_flush(M, st)) return rc;
    for (size_t i = 0; i < s->layers.size(); i++) {
        DLayer& L = s->layers[i];
        if (paged && (L.attn == ATTN_GQA || L.attn == ATTN_MLA)) {      // page by page; a page that is not mapped reads as zero (load only: save has mapped them)
            const size_t row[2] = {M.a_row[i], M.b_row[i]};
            for (int j = 0; j < M.pg.pages_of(seq_len); j++) {
                const int pg = M.pg.row(slot)[j];
                const size_t r0 = (size_t)j << M.pg.shift, nr = std::min((size_t)M.pg.page_tokens, (size_t)seq_len - r0);
                for (int h = 0; h < 2; h++) {
                    char* own = (char*)(h ? L.kv_v.p : L.kv_k.p) + r0 * row[h];
                    char* pool = (char*)(h ? M.b[i].p : M.a[i].p) + (size_t)std::max(pg, 0) * (h ? M.b_stride[i] : M.a_stride[i]);
                    if (pg < 0) KR_HIP(hipMemsetAsync(own, 0, nr * row[h], st));
                    else KR_HIP(hipMemcpyAsync(save ? pool : own, save ? own : pool, nr * row[h], hipMemcpyDeviceToDevice, st));
                }
            }
            continue;
        }
        char* a = (char*)M.a[i].p + (size_t)slot * M.a_stride[i];
        char* b = (char*)M.b[i].p + (size_t)slot * M.b_stride[i];
        void *sa, *sb; size_t na, nb;
        if (L.attn == ATTN_LA) { sa = L.conv_state.p; sb = L.recur_state.p; na = M.a_stride[i]; nb = M.b_stride[i]; }
        else if (L.attn == ATTN_GQA || L.attn == ATTN_MLA) { sa = L.kv_k.p; sb = L.kv_v.p; na = (size_t)seq_len * M.a_row[i]; nb = (size_t)seq_len * M.b_row[i]; }
        else continue;
        if (na) KR_HIP(hipMemcpyAsync(save ? (void*)a : sa, save ? sa : (void*)a, na, hipMemcpyDeviceToDevice, st));
        if (nb) KR_HIP(hipMemcpyAsync(save ? (void*)b : sb, save ? sb : (void*)b, nb, hipMemcpyDeviceToDevice, st));
    }
    KR_HIP(hipStreamSynchronize(st));
    return KR_OK;
}
// the start of kr_decode_generate for one slot (generate_core): seen = {first_token} (if in range), xorshift64 state = rng_seed (0: the wall clock,
// distinct per slot), parameters kept.  Arguments checked; allocates every slot's sampler state on the first call.
int set_sampler(kr_decode_store* s, int slot, int first_token, float temperature, int top_k, float top_p, float presence_penalty, uint64_t rng_seed, hipStream_t st) {
    kr_multi_state& M = *s->multi;
    if (M.smp.empty()) {      // swap_samplers (slot import) allocates the same way: keep the two alike
        const size_t words = ((size_t)s->vocab + 31) / 32;
        if (M.smp_seen.ensure((size_t)M.n_slots * words * 4) || M.smp_rng.ensure((size_t)M.n_slots * 8)) return kr_fail(KR_ERR_HIP, "hipMalloc of the slot samplers failed");
        KR_HIP(hipMemsetAsync(M.smp_seen.p, 0, M.smp_seen.bytes, st));
        KR_HIP(hipMemsetAsync(M.smp_rng.p, 0, M.smp_rng.bytes, st));
        M.smp_words = words;
        M.smp.assign((size_t)M.n_slots, kr_multi_state::Sampler());
    }
    std::vector<uint32_t> seen(M.smp_words, 0u);
    if (first_token >= 0 && first_token < s->vocab) seen[(size_t)first_token >> 5] |= 1u << (first_token & 31);
    if (rng_seed == 0) {
        rng_seed = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::system_clock::now().time_since_epoch()).count() + 0x9E3779B97F4A7C15ull * (uint64_t)(slot + 1);
        if (rng_seed == 0) rng_seed = 0xDEADBEEFull;
    }
    KR_HIP(hipMemcpyAsync((uint32_t*)M.smp_seen.p + (size_t)slot * M.smp_words, seen.data(), M.smp_words * 4, hipMemcpyHostToDevice, st));
    KR_HIP(hipMemcpyAsync((uint64_t*)M.smp_rng.p + slot, &rng_seed, 8, hipMemcpyHostToDevice, st));
    KR_HIP(hipStreamSynchronize(st));
    kr_multi_state::Sampler& p = M.smp[(size_t)slot];
    p.temperature = temperature; p.top_k = top_k; p.top_p = top_p; p.penalty = presence_penalty;
    return KR_OK;
}

// ---- verify over slots (docs/design/18-multi-verify.md)
// the record slices of every linear-attention layer for T token rows and the table of those layers, host and device.  Per row and layer: conv_dim + nk dk +
// nv dv + 2 nv floats
int verify_records(kr_decode_store* s, size_t T, hipStream_t st) {
    kr_multi_state& M = *s->multi;
    M.v_host.clear(); M.v_la_of.assign(s->layers.size(), -1);
    M.v_has64 = M.v_has128 = false; M.v_nv_max = M.v_dv_max = 0;
    size_t floats = 0;
    for (const DLayer& L : s->layers) if (L.attn == ATTN_LA) floats += T * ((size_t)2 * L.nk * L.dk + (size_t)L.nv * L.dv + (size_t)L.nk * L.dk + (size_t)L.nv * L.dv + 2 * (size_t)L.nv);
    if (!floats) return KR_OK;
    if (M.v_rec.ensure(floats * 4)) return kr_fail(KR_ERR_HIP, "hipMalloc of the verify records (%zu MiB for %zu token rows) failed", (floats * 4) >> 20, T);
    float* p = (float*)M.v_rec.p;
    auto take = [&](size_t n) { float* r = p; p += n; return r; };
    for (size_t li = 0; li < s->layers.size(); li++) {
        const DLayer& L = s->layers[li];
        if (L.attn != ATTN_LA) continue;
        KrMultiLaCommit E{};
        E.conv_state = (float*)M.a[li].p; E.conv_stride = M.a_stride[li] / 4; E.recur = (float*)M.b[li].p; E.recur_stride = M.b_stride[li] / 4;
        E.nk = L.nk; E.nv = L.nv; E.dk = L.dk; E.dv = L.dv; E.hr = L.nv / L.nk;
        E.rec_x = take(T * ((size_t)2 * L.nk * L.dk + (size_t)L.nv * L.dv)); E.rec_k = take(T * (size_t)L.nk * L.dk); E.rec_v = take(T * (size_t)L.nv * L.dv);
        E.rec_ge = take(T * (size_t)L.nv); E.rec_be = take(T * (size_t)L.nv);
        M.v_la_of[li] = (int)M.v_host.size(); M.v_host.push_back(E);
        (L.dk == 128 ? M.v_has128 : M.v_has64) = true;
        M.v_nv_max = std::max(M.v_nv_max, L.nv); M.v_dv_max = std::max(M.v_dv_max, L.dv);
    }
    if (M.v_tab.ensure(M.v_host.size() * sizeof(KrMultiLaCommit))) return kr_fail(KR_ERR_HIP, "hipMalloc of the verify layer table failed");
    KR_HIP(hipMemcpyAsync(M.v_tab.p, M.v_host.data(), M.v_host.size() * sizeof(KrMultiLaCommit), hipMemcpyHostToDevice, st));
    return KR_OK;
}
// one verify pass, arguments checked: rows -> device, the pass in its verify form, the greedy id of every token row (sample: the draw of its slot's sampler
// under the hypothesis that the run's drafts before it were drawn; no sampler state is written), the accept kernel, one copy back.  Leaves the rows pending
int verify_impl(kr_decode_store* s, const Rows& r, int32_t* ids_out, int32_t* n_match_out, hipStream_t st, bool sample) {
    kr_multi_state& M = *s->multi;
    const int n = r.n;
    Pass p;
    if (int rc = open_pass(s, r, sample, true, st, p)) return rc;
    const size_t T = p.T;
    const bool greedy = p.sr.empty();
    if (M.ids.ensure((size_t)KR_EXTEND_MAX_TOKENS * 4) || M.v_out.ensure((size_t)(KR_EXTEND_MAX_TOKENS + KR_MULTI_MAX) * 4) || M.v_keep.ensure((size_t)KR_MULTI_MAX * 4))
        return kr_fail(KR_ERR_HIP, "hipMalloc of the verify's row buffers failed");
    if (int rc = verify_records(s, T, st)) return fail_pass(st, rc);
    const int32_t* d_rows = (const int32_t*)M.rows.p;
    if (int rc = kr_multi_pass(s, (int)T, n, d_rows, d_rows + 3 * T, p.max_pos, st, true)) return fail_pass(st, rc);
    const size_t V = (size_t)s->vocab;
    if (greedy) kr_launch_multi_argmax((const float*)M.logits.p, V, (int)V, (int)T, (int*)M.ids.p, st);
    else if (int rc = sample_runs(M, (const float*)M.logits.p, s->vocab, p.sr, p.at, d_rows, (uint32_t*)M.smp_seen.p, M.smp_words, (uint64_t*)M.smp_rng.p, (int*)M.ids.p, st))
        return fail_pass(st, rc);
    kr_launch_multi_accept((const int*)M.ids.p, d_rows + T, d_rows + 3 * T, n, (int)T, (int*)M.v_out.p, st);
    KR_HIP(hipGetLastError());
    std::vector<int32_t> out(T + (size_t)n);
    KR_HIP(hipMemcpyAsync(out.data(), M.v_out.p, out.size() * 4, hipMemcpyDeviceToHost, st));
    KR_HIP(hipStreamSynchronize(st));
    std::copy(out.begin(), out.begin() + (ptrdiff_t)T, ids_out);
    M.v_match.assign(out.begin() + (ptrdiff_t)T, out.end());
    std::copy(M.v_match.begin(), M.v_match.end(), n_match_out);
    M.v_pending = true; M.v_sampled = !greedy; M.v_st = st; M.v_rows = T;
    return KR_OK;
}
int commit_impl(kr_decode_store* s, const int32_t* n_keep) {
    kr_multi_state& M = *s->multi;
    const int n = (int)M.v_match.size();
    if (!n_keep) return kr_fail(KR_ERR_VALUE, "null n_keep");
    for (int i = 0; i < n; i++)
        if (n_keep[i] < 0 || n_keep[i] > M.v_match[(size_t)i] + 1)
            return kr_fail(KR_ERR_VALUE, "row %d: n_keep %d outside [0, %d] (n_match + 1)", i, n_keep[i], M.v_match[(size_t)i] + 1);
    if (!M.v_host.empty() || M.v_sampled) {
        KR_HIP(hipSetDevice(s->eng->device));
        hipStream_t st = M.v_st;
        KR_HIP(hipMemcpyAsync(M.v_keep.p, n_keep, (size_t)n * 4, hipMemcpyHostToDevice, st));
        const size_t T = M.v_rows;      // the run table follows the 3 T row words the verify left in M.rows
        const int* runs = (const int*)M.rows.p + 3 * T;
        if (!M.v_host.empty())
            kr_launch_multi_la_commit((const KrMultiLaCommit*)M.v_tab.p, (int)M.v_host.size(), M.v_has64, M.v_has128, M.v_nv_max, M.v_dv_max, runs,
                                      (const int*)M.v_keep.p, n, st);
        if (M.v_sampled)      // the kept draws, from the sampler rows and ids the verify left (nothing else has run on the slots since)
            kr_launch_ms_commit((const KrMsRow*)M.smp_rows.p, runs, (const int*)M.v_keep.p, n, (const int*)M.ids.p, s->vocab, (uint32_t*)M.smp_seen.p, M.smp_words,
                                (uint64_t*)M.smp_rng.p, st);
        KR_HIP(hipGetLastError());
        KR_HIP(hipStreamSynchronize(st));
    }
    M.v_pending = false;
    return KR_OK;
}
// the arguments of the generation entry points that travel together: the per-row sampler columns of the sampled forms (the greedy forms pass no SamplerCols),
// the drafting of the lookup forms (the plain forms: no contexts, max_draft 0), the outputs (the plain forms: no stats)
struct SamplerCols { const float* temperature; const int* top_k; const float* top_p; const float* presence_penalty; const uint64_t* rng_seeds; };
struct Drafting { const int32_t *contexts, *n_context; int max_draft, ngram_max; };
struct GenOut { int32_t *tokens, *n; int* n_passes; int32_t* n_accepted; };
// the one generation loop over slots, behind all four entry points: row i starts with first.tokens[i] at first.positions[i]; every row's sampler is set first
// (smp), then passes over the rows still generating -- a finished row leaves the batch and its slot is not touched again.  A pass is a step (step_impl) where no
// row drafts -- with max_draft 0 every pass, and then no index is kept -- and a verify + commit where one does: prompt-lookup drafts per row under the
// rule of kr_lookup_index.h (kr_decode_generate_lookup's); a row on the per-row sampler path (KR_MS_LOOP) does not draft
int generate_slots(kr_decode_store* s, const Rows& first, int max_tokens, const Drafting& dr, const SamplerCols* smp, const int* stop_ids, int n_stop, const GenOut& out,
                   void* stream) {
    if (smp && !smp->temperature) return kr_fail(KR_ERR_VALUE, "null sampler parameter array");      // ahead of every other check, the store's included
    const int n = first.n, max_draft = dr.max_draft;
    if (int rc = multi_begin(s)) return rc;
    if (max_tokens < 0) return kr_fail(KR_ERR_VALUE, "max_tokens %d < 0", max_tokens);
    if (n_stop < 0 || (n_stop > 0 && !stop_ids)) return kr_fail(KR_ERR_VALUE, "bad stop ids (%d)", n_stop);
    if (!out.n || (max_tokens > 0 && !out.tokens)) return kr_fail(KR_ERR_VALUE, "null output pointer");
    if (max_draft < 0 || max_draft > KR_VERIFY_MAX - 1) return kr_fail(KR_ERR_VALUE, "max_draft %d out of range [0, %d]", max_draft, KR_VERIFY_MAX - 1);
    if (dr.ngram_max < 1 || dr.ngram_max > KR_LOOKUP_NGRAM_MAX) return kr_fail(KR_ERR_VALUE, "ngram_max %d out of range [1, %d]", dr.ngram_max, KR_LOOKUP_NGRAM_MAX);
    // every row's last step (position start + max_tokens - 1) must fit its slot: checked here, before the first pass
    if (int rc = check_args(s, first, std::max(max_tokens - 1, 0))) return rc;
    std::vector<size_t> c0((size_t)n + 1, 0);      // row i's context = contexts[c0[i] .. c0[i + 1])
    for (int i = 0; i < n; i++) {
        const int nc = dr.n_context ? dr.n_context[i] : 0;
        if (nc < 0 || (nc > 0 && !dr.contexts)) return kr_fail(KR_ERR_VALUE, "row %d: bad context (%d tokens)", i, nc);
        c0[(size_t)i + 1] = c0[(size_t)i] + (size_t)nc;
        for (size_t j = c0[(size_t)i]; j < c0[(size_t)i + 1]; j++)      // a context token becomes a draft token: it must be a valid id
            if (dr.contexts[j] < 0 || dr.contexts[j] >= s->vocab) return kr_fail(KR_ERR_VALUE, "row %d: context token id %d out of range (vocab %d)", i, dr.contexts[j], s->vocab);
    }
    if (smp) {      // the other four columns come after the rows: a call wrong in both names its row
        if (!smp->top_k || !smp->top_p || !smp->presence_penalty || !smp->rng_seeds) return kr_fail(KR_ERR_VALUE, "null sampler parameter array");
        for (int i = 0; i < n; i++) if (!(smp->temperature[i] >= 0.0f)) return kr_fail(KR_ERR_VALUE, "row %d: temperature must be >= 0", i);
    }
    if (int rc = paged_refuse(s)) return rc;
    // paged slots: [0, start + max_tokens) of every row is reserved here, before the first pass; on return, success or error, the pages THIS call mapped that lie
    // wholly past a row's final position go back (ps: the position each row consumes next)
    std::vector<int32_t> ps(first.positions, first.positions + n);
    struct PageGuard {
        kr_decode_store* s; const Rows& first; const std::vector<int32_t>& ps; std::vector<KrPageChange> log;
        ~PageGuard() {
            if (log.empty()) return;
            std::vector<KrPageChange> freed;
            for (int i = 0; i < first.n; i++) s->multi->pg.release_logged(log, first.slots[i], ps[(size_t)i], &freed);
            (void)pg_released(s, freed);
        }
    } guard{s, first, ps, {}};
    if (int rc = pg_reserve_rows(s, first, std::max(max_tokens - 1, 0), &guard.log)) return rc;
    for (int i = 0; i < n; i++) { out.n[i] = 0; if (out.n_accepted) out.n_accepted[i] = 0; }
    if (out.n_passes) *out.n_passes = 0;
    if (max_tokens == 0 && !smp) return KR_OK;
    KR_HIP(hipSetDevice(s->eng->device));
    hipStream_t st = kr_pick_stream(s->eng, stream);
    if (int rc = order_after_store(s, st)) return rc;
    std::vector<char> drafts((size_t)n, 1);
    if (smp)
        for (int i = 0; i < n; i++) {
            if (int rc = set_sampler(s, first.slots[i], first.tokens[i], smp->temperature[i], smp->top_k[i], smp->top_p[i], smp->presence_penalty[i], smp->rng_seeds[i], st)) return rc;
            drafts[(size_t)i] = sample_row(s, first.slots[i]).mode != KR_MS_LOOP;
        }
    if (max_tokens == 0) return KR_OK;
    // a run over positions [pos, pos + k] must stay inside the slot and the rope tables (check_args' limits)
    int limit = s->multi->max_seq;
    if (s->max_rope_seq > 0) limit = std::min(limit, s->max_rope_seq);
    for (const DLayer& L : s->layers) if (L.attn == ATTN_MLA) limit = std::min(limit, L.mla_rope_seq);
    std::vector<LookupIndex> ix;      // one per row; none without drafting
    if (max_draft > 0) ix.reserve((size_t)n);
    for (int i = 0; max_draft > 0 && i < n; i++) {
        ix.emplace_back(dr.ngram_max);
        for (size_t j = c0[(size_t)i]; j < c0[(size_t)i + 1]; j++) ix.back().push(dr.contexts[j]);
        ix.back().push(first.tokens[i]);
    }
    auto is_stop = [&](int t) { for (int j = 0; j < n_stop; j++) if (stop_ids[j] == t) return true; return false; };
    std::vector<int> act((size_t)n);                           // rows still generating, in caller order
    std::vector<int32_t> tk(first.tokens, first.tokens + n);
    for (int i = 0; i < n; i++) act[(size_t)i] = i;
    int passes = 0;
    while (!act.empty()) {
        const int m = (int)act.size(), fit = KR_EXTEND_MAX_TOKENS / m - 1;      // m rows of 1 + fit tokens always fit a pass
        std::vector<int32_t> sl((size_t)m), rp((size_t)m), cn((size_t)m), run, ids, nm((size_t)m, 0), keep((size_t)m);
        for (int k = 0; k < m; k++) {
            const int i = act[(size_t)k];
            int32_t draft[KR_VERIFY_MAX];
            const int d = lookup_clamp(max_draft > 0 && drafts[(size_t)i] ? ix[(size_t)i].draft(max_draft, draft) : 0, draft, max_tokens - out.n[i], limit - ps[(size_t)i], fit, is_stop);
            sl[(size_t)k] = first.slots[i]; rp[(size_t)k] = ps[(size_t)i]; cn[(size_t)k] = 1 + d;
            run.push_back(tk[(size_t)i]);
            run.insert(run.end(), draft, draft + d);
        }
        const bool any = run.size() > (size_t)m;      // a row drafts
        passes++;
        ids.resize(run.size());
        const Rows rows{m, sl.data(), any ? cn.data() : nullptr, run.data(), rp.data()};
        if (any) { if (int rc = verify_impl(s, rows, ids.data(), nm.data(), st, smp != nullptr)) return rc; }
        else if (int rc = step_impl(s, rows, ids.data(), nullptr, st, smp != nullptr)) return rc;      // the plain loop's step
        std::vector<int> next;
        size_t g0 = 0;
        for (int k = 0; k < m; k++) {
            const int i = act[(size_t)k], mt = nm[(size_t)k];
            const LookupKept kept = lookup_emit(&ids[g0], mt, out.tokens + (size_t)i * max_tokens, out.n[i], ix.empty() ? nullptr : &ix[(size_t)i], is_stop);
            if (out.n_accepted) out.n_accepted[i] += std::min(mt, kept.keep);
            keep[(size_t)k] = kept.keep;
            tk[(size_t)i] = ids[g0 + (size_t)kept.keep - 1]; ps[(size_t)i] += kept.keep;
            g0 += (size_t)cn[(size_t)k];
            if (!kept.stop && out.n[i] < max_tokens) next.push_back(i);
        }
        if (any) if (int rc = commit_impl(s, keep.data())) return rc;
        act.swap(next);
    }
    if (out.n_passes) *out.n_passes = passes;
    return KR_OK;
}
}  // namespace

// flat slots (page_tokens 0), or paged ones: every GQA / MLA layer then gets pools [n_pages][page_tokens][row] instead of [n_slots][max_seq][row]
static int slots_create(kr_decode_store* s, int n_slots, int max_seq, int page_tokens, int n_pages, size_t* bytes_out) {
    if (int rc = multi_ready(s)) return rc;
    if (n_slots < 0 || (n_slots > 0 && max_seq < 1)) return kr_fail(KR_ERR_VALUE, "bad slot geometry: %d slots of %d positions", n_slots, max_seq);
    const bool paged = page_tokens != 0;
    KrPagePool pool;
    if (paged) {
        if (n_slots < 1) return kr_fail(KR_ERR_VALUE, "bad slot geometry: %d slots of %d positions", n_slots, max_seq);
        const int bad = pool.init(n_slots, max_seq, page_tokens, n_pages, KR_PAGE_MIN_TOKENS);
        if (bad == 1) return kr_fail(KR_ERR_VALUE, "page_tokens %d: must be a power of two and at least %d (a stage of the MLA attention kernel)", page_tokens, KR_PAGE_MIN_TOKENS);
        if (bad) return kr_fail(KR_ERR_VALUE, "n_pages %d: must be at least 1", n_pages);
        // the paged GQA attention kernel keeps a slot's whole table row in LDS beside its tiles: a capacity it could not launch with is refused here, not by
        // the first pass, which has mapped pages and advanced linear-attention state by the time it reaches a GQA layer
        for (size_t i = 0; i < s->layers.size(); i++) {
            const DLayer& L = s->layers[i];
            if (L.attn != ATTN_GQA || L.nkv < 1 || L.nh % L.nkv) continue;
            const size_t tiles = kr_multi_gqa_lds_bytes(L.nh / L.nkv, L.hd, 0);
            if (tiles > KR_MULTI_GQA_LDS_MAX) continue;      // no slots of this geometry step, flat or paged: the pass says so
            const long long fit = (long long)((KR_MULTI_GQA_LDS_MAX - tiles) / 4);
            if (pool.stride > fit)
                return kr_fail(KR_ERR_VALUE, "max_seq %d at page_tokens %d is a page table of %d entries per slot: GQA layer %zu (%d query heads per KV head, head_dim %d) "
                               "has room for at most %lld entries beside its tiles (max_seq %lld)", max_seq, page_tokens, pool.stride, i, L.nh / L.nkv, L.hd, fit, fit * page_tokens);
        }
    }
    KR_HIP(hipSetDevice(s->eng->device));
    KR_HIP(hipDeviceSynchronize());          // a step in flight may still use the old slots
    s->multi.reset();
    if (bytes_out) *bytes_out = 0;
    if (n_slots == 0) return KR_OK;
    auto M = std::make_unique<kr_multi_state>();
    M->n_slots = n_slots; M->max_seq = max_seq; M->kv_fp8 = s->kv_fp8;
    const size_t nl = s->layers.size(), seq_rows = paged ? (size_t)page_tokens : (size_t)max_seq;      // rows per slot, or per page
    std::vector<KrPagePoolDev> pools, la_pools;
    M->a.resize(nl); M->b.resize(nl); M->a_stride.assign(nl, 0); M->b_stride.assign(nl, 0); M->a_row.assign(nl, 0); M->b_row.assign(nl, 0);
    size_t total = 0;
    for (size_t i = 0; i < nl; i++) {
        const DLayer& L = s->layers[i];
        if (L.attn == ATTN_LA) { M->a_stride[i] = (size_t)(2 * L.nk * L.dk + L.nv * L.dv) * L.kd * 4; M->b_stride[i] = (size_t)L.nv * L.dk * L.dv * 4; }
        else if (L.attn == ATTN_GQA) M->a_row[i] = M->b_row[i] = (size_t)L.nkv * L.hd * (s->kv_fp8 ? 1 : 2);
        else if (L.attn == ATTN_MLA) { M->a_row[i] = (size_t)L.klr * (s->kv_fp8 ? 1 : 2); M->b_row[i] = (size_t)L.rd * (s->kv_fp8 ? 1 : 2); }
        if (L.attn == ATTN_GQA || L.attn == ATTN_MLA) { M->a_stride[i] = seq_rows * M->a_row[i]; M->b_stride[i] = seq_rows * M->b_row[i]; }
        const bool pooled = paged && (L.attn == ATTN_GQA || L.attn == ATTN_MLA);
        for (int h = 0; h < 2; h++) {
            DevBuf& d = h ? M->b[i] : M->a[i];
            const size_t stride = h ? M->b_stride[i] : M->a_stride[i], bytes = stride * (size_t)(pooled ? n_pages : n_slots);
            if (!bytes) continue;
            if (pooled && stride % 16) return kr_fail(KR_ERR_VALUE, "layer %zu: a page of %zu bytes is not a multiple of 16", i, stride);
            if (d.ensure(bytes)) return kr_fail(KR_ERR_HIP, "hipMalloc of %d sequence slots (%zu MiB so far) failed", n_slots, (total + bytes) >> 20);
            if (pooled) pools.push_back(KrPagePoolDev{d.p, stride});      // a page is zeroed when it is mapped (pg_flush)
            else KR_HIP(hipMemsetAsync(d.p, 0, bytes, s->eng->stream));
            if (L.attn == ATTN_LA) la_pools.push_back(KrPagePoolDev{d.p, stride});      // a fork copies a slot's state as one "page" (docs/design/22-slot-fork.md)
            total += bytes;
        }
    }
    if (paged) {      // the table (-1 everywhere), the pools' addresses and room for the ids of the pages a pass zeroes
        const size_t tb = pool.table.size() * 4;
        if (M->pg_table.ensure(tb) || M->pg_pools.ensure(std::max(pools.size(), (size_t)1) * sizeof(KrPagePoolDev)) || M->pg_new.ensure((size_t)n_pages * 4 * 4))      // ids to zero, then [dst | src | rows] of the copies
            return kr_fail(KR_ERR_HIP, "hipMalloc of the page table (%zu KiB) failed", tb >> 10);
        KR_HIP(hipMemsetAsync(M->pg_table.p, 0xFF, tb, s->eng->stream));
        if (!pools.empty()) KR_HIP(hipMemcpyAsync(M->pg_pools.p, pools.data(), pools.size() * sizeof(KrPagePoolDev), hipMemcpyHostToDevice, s->eng->stream));
        M->pg_npools = (int)pools.size(); M->pg = std::move(pool);
        total += tb;
    }
    if (!la_pools.empty()) {
        if (M->la_pools.ensure(la_pools.size() * sizeof(KrPagePoolDev))) return kr_fail(KR_ERR_HIP, "hipMalloc of the linear-attention state table failed");
        KR_HIP(hipMemcpyAsync(M->la_pools.p, la_pools.data(), la_pools.size() * sizeof(KrPagePoolDev), hipMemcpyHostToDevice, s->eng->stream));
        M->la_npools = (int)la_pools.size();
    }
    KR_HIP(hipStreamSynchronize(s->eng->stream));
    s->multi = std::move(M);
    if (bytes_out) *bytes_out = total;
    return KR_OK;
}

extern "C" int kr_decode_slots_create(kr_decode_store* s, int n_slots, int max_seq, size_t* bytes_out) { return slots_create(s, n_slots, max_seq, 0, 0, bytes_out); }

// ---- paged slots (docs/design/21-paged-slots.md)
extern "C" int kr_decode_slots_create_paged(kr_decode_store* s, int n_slots, int max_seq, int page_tokens, int n_pages, size_t* bytes_out) {
    if (page_tokens == 0) return kr_fail(KR_ERR_VALUE, "page_tokens 0: must be a power of two and at least %d (a stage of the MLA attention kernel)", KR_PAGE_MIN_TOKENS);
    return slots_create(s, n_slots, max_seq, page_tokens, n_pages, bytes_out);
}
extern "C" int kr_decode_slot_trim(kr_decode_store* s, int slot, int seq_len) {
    if (int rc = multi_begin(s)) return rc;
    if (int rc = slot_in_range(s, slot)) return rc;
    kr_multi_state& M = *s->multi;
    if (seq_len < 0 || seq_len > M.max_seq) return kr_fail(KR_ERR_VALUE, "seq_len %d outside [0, %d] (slot max_seq)", seq_len, M.max_seq);
    if (!M.pg.paged()) return KR_OK;
    std::vector<KrPageChange> freed;
    M.pg.trim(slot, seq_len, &freed);
    return pg_released(s, freed);      // every slot call returns with its stream drained: nothing in flight reads the pages
}
extern "C" int kr_decode_slots_pages(kr_decode_store* s, int32_t* page_tokens_out, int32_t* n_pages_out, int32_t* n_free_out, int32_t* per_slot_out) {
    if (int rc = multi_ready(s)) return rc;
    if (int rc = need_slots(s)) return rc;
    const kr_multi_state& M = *s->multi;
    if (page_tokens_out) *page_tokens_out = M.pg.page_tokens;
    if (n_pages_out) *n_pages_out = M.pg.n_pages;
    if (n_free_out) *n_free_out = M.pg.n_free;
    if (per_slot_out) for (int i = 0; i < M.n_slots; i++) per_slot_out[i] = M.pg.paged() ? M.pg.mapped(i) : 0;
    return KR_OK;
}

// ---- slot fork (docs/design/22-slot-fork.md)
extern "C" int kr_decode_slot_page_ids(kr_decode_store* s, int slot, int32_t* ids_out, int32_t* refs_out) {
    if (int rc = multi_ready(s)) return rc;
    if (int rc = need_slots(s)) return rc;
    if (int rc = slot_in_range(s, slot)) return rc;
    const kr_multi_state& M = *s->multi;
    if (!M.pg.paged()) return kr_fail(KR_ERR_STATE, "flat slots have no pages: create them with kr_decode_slots_create_paged");
    for (int j = 0; j < M.pg.stride; j++) {
        const int32_t t = M.pg.row(slot)[j];
        if (ids_out) ids_out[j] = t;
        if (refs_out) refs_out[j] = t >= 0 ? M.pg.refs[(size_t)t] : 0;
    }
    return KR_OK;
}
extern "C" int kr_decode_slots_page_stride(kr_decode_store* s, int32_t* stride_out) {
    if (int rc = multi_ready(s)) return rc;
    if (int rc = need_slots(s)) return rc;
    if (!stride_out) return kr_fail(KR_ERR_VALUE, "null stride_out");
    *stride_out = s->multi->pg.paged() ? s->multi->pg.stride : 0;
    return KR_OK;
}
// test aid: kr_multi_copy_pages_kernel on one host pool [n_pages][page_bytes] (in / out), its device copy placed base_offset bytes past a 256-byte boundary
extern "C" int kr_copy_pages(void* pool, size_t page_bytes, int n_pages, int page_tokens, int n_copies, const int32_t* dst_pages, const int32_t* src_pages,
                             const int32_t* rows, int base_offset) {
    if (!pool || !dst_pages || !src_pages || !rows) return kr_fail(KR_ERR_VALUE, "kr_copy_pages: null pointer");
    if (page_bytes < 1 || n_pages < 1 || page_tokens < 1 || page_bytes % (size_t)page_tokens) return kr_fail(KR_ERR_VALUE, "kr_copy_pages: %d pages of %zu bytes and %d rows", n_pages, page_bytes, page_tokens);
    if (n_copies < 1 || n_copies > n_pages) return kr_fail(KR_ERR_VALUE, "n_copies %d outside [1, %d]", n_copies, n_pages);
    if (base_offset < 0 || base_offset >= 256) return kr_fail(KR_ERR_VALUE, "base_offset %d outside [0, 256)", base_offset);
    std::vector<char> written((size_t)n_pages, 0);
    for (int c = 0; c < n_copies; c++) {      // a launch's copies have no order: a destination is written once and never read
        if (dst_pages[c] < 0 || dst_pages[c] >= n_pages || src_pages[c] < 0 || src_pages[c] >= n_pages) return kr_fail(KR_ERR_VALUE, "copy %d: page out of range [0, %d)", c, n_pages);
        if (rows[c] < 0 || rows[c] > page_tokens) return kr_fail(KR_ERR_VALUE, "copy %d: %d rows outside [0, %d]", c, rows[c], page_tokens);
        if (written[(size_t)dst_pages[c]]++) return kr_fail(KR_ERR_VALUE, "copy %d: page %d is a destination twice", c, dst_pages[c]);
    }
    for (int c = 0; c < n_copies; c++) if (written[(size_t)src_pages[c]]) return kr_fail(KR_ERR_VALUE, "copy %d: page %d is a source and a destination", c, src_pages[c]);
    int dev_count = 0;
    if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count == 0) return kr_fail(KR_ERR_HIP, "no HIP device");
    const size_t bytes = page_bytes * (size_t)n_pages;
    DevBuf buf, tab, ids;
    if (buf.ensure(bytes + 256) || tab.ensure(sizeof(KrPagePoolDev)) || ids.ensure((size_t)3 * n_copies * 4)) return kr_fail(KR_ERR_HIP, "hipMalloc failed");
    const KrPagePoolDev P{(char*)buf.p + base_offset, page_bytes};
    int32_t* d = (int32_t*)ids.p;
    KR_HIP(hipMemcpy(P.base, pool, bytes, hipMemcpyHostToDevice));
    KR_HIP(hipMemcpy(tab.p, &P, sizeof(P), hipMemcpyHostToDevice));
    KR_HIP(hipMemcpy(d, dst_pages, (size_t)n_copies * 4, hipMemcpyHostToDevice));
    KR_HIP(hipMemcpy(d + n_copies, src_pages, (size_t)n_copies * 4, hipMemcpyHostToDevice));
    KR_HIP(hipMemcpy(d + 2 * n_copies, rows, (size_t)n_copies * 4, hipMemcpyHostToDevice));
    kr_launch_multi_copy_pages((const KrPagePoolDev*)tab.p, 1, d, d + n_copies, d + 2 * n_copies, n_copies, page_tokens, nullptr);
    KR_HIP(hipGetLastError());
    KR_HIP(hipDeviceSynchronize());
    KR_HIP(hipMemcpy(pool, P.base, bytes, hipMemcpyDeviceToHost));
    return KR_OK;
}
// every dsts[i] becomes a fresh slot into which src's first seq_len positions were prefilled.  Paged slots: whole pages below seq_len are shared by reference,
// the boundary page is a copy of src's rows with zeroes behind them; flat slots: device copies.  The linear-attention state goes over as it stands
extern "C" int kr_decode_slot_fork(kr_decode_store* s, int src, int n_dst, const int32_t* dsts, int seq_len) {
    if (int rc = multi_begin(s)) return rc;
    kr_multi_state& M = *s->multi;
    if (src < 0 || src >= M.n_slots) return kr_fail(KR_ERR_VALUE, "src: slot %d out of range [0, %d)", src, M.n_slots);
    if (n_dst < 1 || n_dst > M.n_slots - 1) return kr_fail(KR_ERR_VALUE, "n_dst %d outside [1, %d] (n_slots - 1)", n_dst, M.n_slots - 1);
    if (!dsts) return kr_fail(KR_ERR_VALUE, "null dsts");
    std::vector<char> seen((size_t)M.n_slots, 0);
    for (int i = 0; i < n_dst; i++) {
        if (dsts[i] < 0 || dsts[i] >= M.n_slots) return kr_fail(KR_ERR_VALUE, "dsts[%d]: slot %d out of range [0, %d)", i, dsts[i], M.n_slots);
        if (dsts[i] == src) return kr_fail(KR_ERR_VALUE, "dsts[%d]: slot %d is src", i, src);
        if (seen[(size_t)dsts[i]]++) return kr_fail(KR_ERR_VALUE, "dsts[%d]: slot %d is named twice", i, dsts[i]);
    }
    if (seq_len < 0 || seq_len > M.max_seq) return kr_fail(KR_ERR_VALUE, "seq_len %d outside [0, %d] (slot max_seq)", seq_len, M.max_seq);
    const bool paged = M.pg.paged();
    if (paged) {      // all or nothing: the boundary pages, out of the free pages and those the dsts give back
        const KrPageFork fit = M.pg.fork_fit(src, n_dst, dsts, seq_len);
        if (!fit.fits())
            return kr_fail(KR_ERR_STATE, "the fork of slot %d at seq_len %d does not fit the page pool: %d more pages of %d positions, %d of %d are free (%d of them once the dsts are released)",
                           src, seq_len, fit.need, M.pg.page_tokens, fit.free + fit.gain, M.pg.n_pages, fit.gain);
    }
    if (M.fk_ids.ensure((size_t)3 * M.n_slots * 4)) return kr_fail(KR_ERR_HIP, "hipMalloc of the fork's slot ids failed");
    KR_HIP(hipSetDevice(s->eng->device));
    KR_HIP(hipDeviceSynchronize());          // steps still in flight on any stream read or write both sides
    hipStream_t st = s->eng->stream;
    if (paged) {
        (void)M.pg.fork(src, n_dst, dsts, seq_len);      // the count above again, on the same state: it fits.  The dsts release what they held (as kr_decode_slot_trim(dst, 0)), share, queue their copies
        if (int rc = pg_flush(M, st)) return rc;      // src's own pending pages are zeroed, or copied in an earlier launch, ahead of the boundary copies
        for (int i = 0; i < n_dst; i++) if (int rc = pg_upload(M, dsts[i], 0, M.pg.stride - 1, st)) return rc;
    }
    for (size_t li = 0; li < s->layers.size() && !paged; li++) {      // flat slots: rows [0, seq_len) copied, the rest zeroed
        const DLayer& L = s->layers[li];
        if (L.attn != ATTN_GQA && L.attn != ATTN_MLA) continue;
        for (int h = 0; h < 2; h++) {
            const size_t stride = h ? M.b_stride[li] : M.a_stride[li], head = (h ? M.b_row[li] : M.a_row[li]) * (size_t)seq_len;
            char* base = (char*)(h ? M.b[li].p : M.a[li].p);
            for (int i = 0; i < n_dst; i++) {
                char* d = base + (size_t)dsts[i] * stride;
                if (head) KR_HIP(hipMemcpyAsync(d, base + (size_t)src * stride, head, hipMemcpyDeviceToDevice, st));
                if (stride > head) KR_HIP(hipMemsetAsync(d + head, 0, stride - head, st));
            }
        }
    }
    if (M.la_npools) {      // conv and recurrent state of every linear-attention layer: one launch, a slot being the page
        std::vector<int32_t> ids((size_t)3 * n_dst);
        for (int i = 0; i < n_dst; i++) { ids[(size_t)i] = dsts[i]; ids[(size_t)n_dst + i] = src; ids[(size_t)2 * n_dst + i] = 1; }
        KR_HIP(hipMemcpyAsync(M.fk_ids.p, ids.data(), ids.size() * 4, hipMemcpyHostToDevice, st));
        const int32_t* d = (const int32_t*)M.fk_ids.p;
        kr_launch_multi_copy_pages((const KrPagePoolDev*)M.la_pools.p, M.la_npools, d, d + n_dst, d + 2 * n_dst, n_dst, 1, st);
        KR_HIP(hipGetLastError());
    }
    KR_HIP(hipStreamSynchronize(st));
    return KR_OK;
}

// ---- slot export / import (docs/design/38-slot-swap.md): a slot's whole state <-> one self-describing host image (kr_slot_image.h), in staged ranges of
// "slot_swap_chunk_bytes": the call's stream packs / unpacks one half of the staging buffer (kr_multi_swap.hip) while the second stream copies the other between
// device and pinned host memory and the host memcpy's between that and the caller's image.  No device-wide synchronisation: every slot entry point returns with its
// pass finished (step_impl, verify_impl, commit_impl and the others end in a stream synchronise) and a pending verify is refused, so it suffices to order after the
// store's last stream, to flush the page queue, and to wait for the call's own two streams
namespace {
KrSlotGeo swap_geo(const kr_decode_store* s) {
    const kr_multi_state& M = *s->multi;
    KrSlotGeo g;
    g.kv_fp8 = M.kv_fp8; g.hidden = s->hidden; g.vocab = s->vocab;
    for (size_t i = 0; i < s->layers.size(); i++) {
        const int attn = s->layers[i].attn;
        KrSlotLayerGeo x{KR_SLOT_NONE, 0, 0, 0, 0};
        if (attn == ATTN_LA) x = KrSlotLayerGeo{KR_SLOT_LA, 0, 0, M.a_stride[i], M.b_stride[i]};
        else if (attn == ATTN_GQA || attn == ATTN_MLA) x = KrSlotLayerGeo{attn == ATTN_GQA ? KR_SLOT_GQA : KR_SLOT_MLA, M.a_row[i], M.b_row[i], 0, 0};
        g.layers.push_back(x);
    }
    return g;
}
// distinct slots in range, 1 <= n <= n_slots
int swap_slots_ok(const kr_multi_state& M, int n, const int32_t* slots) {
    if (n < 1 || n > M.n_slots) return kr_fail(KR_ERR_VALUE, "%d slots, must be in [1, %d] (n_slots)", n, M.n_slots);
    if (!slots) return kr_fail(KR_ERR_VALUE, "null slots");
    std::vector<char> seen((size_t)M.n_slots, 0);
    for (int i = 0; i < n; i++) {
        if (slots[i] < 0 || slots[i] >= M.n_slots) return kr_fail(KR_ERR_VALUE, "row %d: slot %d out of range [0, %d)", i, slots[i], M.n_slots);
        if (seen[(size_t)slots[i]]++) return kr_fail(KR_ERR_VALUE, "row %d: slot %d is named twice", i, slots[i]);
    }
    return KR_OK;
}
// the staging buffers, the second stream and the events, on first use and whenever the half size changes (nothing is in flight: every call drains its streams)
int swap_ensure(kr_decode_store* s) {
    kr_multi_state& M = *s->multi;
    const size_t half = (size_t)s->opt_slot_swap_chunk_bytes;
    if (!M.sw_stream) KR_HIP(hipStreamCreateWithFlags(&M.sw_stream, hipStreamNonBlocking));
    for (hipEvent_t& e : M.sw_ev) if (!e) KR_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (M.sw_half != half) {
        if (M.sw_pinned) { (void)hipHostFree(M.sw_pinned); M.sw_pinned = nullptr; }
        M.sw_half = 0;
        if (M.sw_stage.ensure(2 * half)) return kr_fail(KR_ERR_HIP, "hipMalloc of the slot swap staging buffer (2 x %zu bytes) failed", half);
        KR_HIP(hipHostMalloc(&M.sw_pinned, 2 * half, hipHostMallocDefault));
        M.sw_half = half;
    }
    return KR_OK;
}
// the samplers of every slot, as the first kr_decode_slot_sampler call allocates them: zero seen sets, zero states, greedy parameters.  The twin of the allocation
// block at the head of set_sampler (which this change leaves as it was): a new sampler buffer or another seen-set layout goes into both
int swap_samplers(kr_decode_store* s, hipStream_t st) {
    kr_multi_state& M = *s->multi;
    if (!M.smp.empty()) return KR_OK;
    const size_t words = ((size_t)s->vocab + 31) / 32;
    if (M.smp_seen.ensure((size_t)M.n_slots * words * 4) || M.smp_rng.ensure((size_t)M.n_slots * 8)) return kr_fail(KR_ERR_HIP, "hipMalloc of the slot samplers failed");
    KR_HIP(hipMemsetAsync(M.smp_seen.p, 0, M.smp_seen.bytes, st));
    KR_HIP(hipMemsetAsync(M.smp_rng.p, 0, M.smp_rng.bytes, st));
    M.smp_words = words;
    M.smp.assign((size_t)M.n_slots, kr_multi_state::Sampler());
    return KR_OK;
}
// one staged range: bytes [r0, r1) of row `row`'s image, its pieces [p0, p1) of the call's list
struct SwapRange { int row; uint64_t r0, r1; size_t p0, p1; };
// the pools and the pieces of a call -> the device, and the ranges: every image's payload in chunks of the half size
int swap_plan(kr_decode_store* s, int n, const int32_t* slots, const std::vector<KrSlotLayout>& lay, hipStream_t st, std::vector<SwapRange>& ranges) {
    kr_multi_state& M = *s->multi;
    const size_t nl = s->layers.size();
    std::vector<KrPagePoolDev> pools(2 * nl + 2, KrPagePoolDev{nullptr, 0});
    for (size_t i = 0; i < nl; i++) { pools[2 * i] = KrPagePoolDev{M.a[i].p, M.a_stride[i]}; pools[2 * i + 1] = KrPagePoolDev{M.b[i].p, M.b_stride[i]}; }
    pools[2 * nl] = KrPagePoolDev{M.smp_rng.p, 8}; pools[2 * nl + 1] = KrPagePoolDev{M.smp_seen.p, M.smp_words * 4};
    std::vector<KrSlotPiece> pieces;
    for (int i = 0; i < n; i++) {
        const KrSlotPlace place{slots[i], M.pg.page_tokens, M.pg.paged() ? M.pg.row(slots[i]) : nullptr};
        for (uint64_t r0 = lay[(size_t)i].payload; r0 < lay[(size_t)i].total; r0 += M.sw_half) {
            SwapRange r{i, r0, std::min<uint64_t>(r0 + M.sw_half, lay[(size_t)i].total), pieces.size(), 0};
            kr_slot_pieces(lay[(size_t)i], place, r.r0, r.r1, &pieces);
            r.p1 = pieces.size();
            ranges.push_back(r);
        }
    }
    if (M.sw_pools.ensure(pools.size() * sizeof(KrPagePoolDev)) || M.sw_pieces.ensure(std::max(pieces.size(), (size_t)1) * sizeof(KrSlotPiece)))
        return kr_fail(KR_ERR_HIP, "hipMalloc of the slot swap piece list (%zu pieces) failed", pieces.size());
    KR_HIP(hipMemcpyAsync(M.sw_pools.p, pools.data(), pools.size() * sizeof(KrPagePoolDev), hipMemcpyHostToDevice, st));      // pageable sources: staged before the call returns
    if (!pieces.empty()) KR_HIP(hipMemcpyAsync(M.sw_pieces.p, pieces.data(), pieces.size() * sizeof(KrSlotPiece), hipMemcpyHostToDevice, st));
    KR_HIP(hipStreamSynchronize(st));      // the lists are the device's before the host's vectors go; what the store had queued ahead has finished with it
    return KR_OK;
}
// whatever happens, the call leaves nothing in flight on its two streams
struct SwapDrain { hipStream_t a, b; ~SwapDrain() { (void)hipStreamSynchronize(b); (void)hipStreamSynchronize(a); } };
// export: range k is packed into half k & 1 on st and copied to the pinned half on the second stream, while the host takes range k - 1 out of the other half
int swap_out(kr_multi_state& M, const std::vector<SwapRange>& ranges, void* const* images, hipStream_t st) {
    const KrSlotPiece* pieces = (const KrSlotPiece*)M.sw_pieces.p;
    auto issue = [&](size_t k) -> int {
        const SwapRange& r = ranges[k];
        const int h = (int)(k & 1);
        char* dev = (char*)M.sw_stage.p + (size_t)h * M.sw_half;
        if (k >= 2) KR_HIP(hipStreamWaitEvent(st, M.sw_ev[2 + h], 0));      // the copy of range k - 2 has left this half
        kr_launch_multi_pack((const KrPagePoolDev*)M.sw_pools.p, pieces + r.p0, (int)(r.p1 - r.p0), dev, st);
        KR_HIP(hipGetLastError());
        KR_HIP(hipEventRecord(M.sw_ev[h], st));
        KR_HIP(hipStreamWaitEvent(M.sw_stream, M.sw_ev[h], 0));
        KR_HIP(hipMemcpyAsync((char*)M.sw_pinned + (size_t)h * M.sw_half, dev, (size_t)(r.r1 - r.r0), hipMemcpyDeviceToHost, M.sw_stream));
        KR_HIP(hipEventRecord(M.sw_ev[2 + h], M.sw_stream));
        return KR_OK;
    };
    if (!ranges.empty()) if (int rc = issue(0)) return rc;
    for (size_t k = 0; k < ranges.size(); k++) {
        if (k + 1 < ranges.size()) if (int rc = issue(k + 1)) return rc;      // its pinned half was emptied by the host one turn ago
        const SwapRange& r = ranges[k];
        KR_HIP(hipEventSynchronize(M.sw_ev[2 + (k & 1)]));
        memcpy((char*)images[r.row] + r.r0, (const char*)M.sw_pinned + (k & 1) * M.sw_half, (size_t)(r.r1 - r.r0));
    }
    return KR_OK;
}
// import, the mirror image: the host fills pinned half k & 1 while range k - 1 travels; the copy waits for the unpack of range k - 2 to have left the device half
int swap_in(kr_multi_state& M, const std::vector<SwapRange>& ranges, const void* const* images, hipStream_t st) {
    const KrSlotPiece* pieces = (const KrSlotPiece*)M.sw_pieces.p;
    for (size_t k = 0; k < ranges.size(); k++) {
        const SwapRange& r = ranges[k];
        const int h = (int)(k & 1);
        char* dev = (char*)M.sw_stage.p + (size_t)h * M.sw_half;
        char* pin = (char*)M.sw_pinned + (size_t)h * M.sw_half;
        if (k >= 2) KR_HIP(hipEventSynchronize(M.sw_ev[2 + h]));      // the copy of range k - 2 has read this pinned half
        memcpy(pin, (const char*)images[r.row] + r.r0, (size_t)(r.r1 - r.r0));
        if (k >= 2) KR_HIP(hipStreamWaitEvent(M.sw_stream, M.sw_ev[h], 0));
        KR_HIP(hipMemcpyAsync(dev, pin, (size_t)(r.r1 - r.r0), hipMemcpyHostToDevice, M.sw_stream));
        KR_HIP(hipEventRecord(M.sw_ev[2 + h], M.sw_stream));
        KR_HIP(hipStreamWaitEvent(st, M.sw_ev[2 + h], 0));
        kr_launch_multi_unpack((const KrPagePoolDev*)M.sw_pools.p, pieces + r.p0, (int)(r.p1 - r.p0), dev, st);
        KR_HIP(hipGetLastError());
        KR_HIP(hipEventRecord(M.sw_ev[h], st));
    }
    return KR_OK;
}
const char* swap_image_fault(int code) {
    switch (code) {
        case 1: return "shorter than an image header";
        case 2: return "bad magic: not a slot image";
        case 3: return "an image format version this library does not read";
        case 4: return "image_bytes is not the header's total_bytes";
        case 6: return "its KV element type is not the slots'";
        case 7: return "its geometry (layers, hidden size, vocabulary or the per-layer digest) is not the store's";
        case 8: return "its seq_len is above the slots' max_seq";
        default: return "a malformed header or section table";
    }
}
}  // namespace

extern "C" int kr_decode_slot_image_bytes(kr_decode_store* s, int seq_len, int with_sampler, size_t* bytes_out) {
    if (int rc = multi_ready(s)) return rc;
    if (int rc = need_slots(s)) return rc;
    const kr_multi_state& M = *s->multi;
    if (!bytes_out) return kr_fail(KR_ERR_VALUE, "null bytes_out");
    if (seq_len < 0 || seq_len > M.max_seq) return kr_fail(KR_ERR_VALUE, "seq_len %d outside [0, %d] (slot max_seq)", seq_len, M.max_seq);
    *bytes_out = (size_t)kr_slot_image_layout(swap_geo(s), seq_len, with_sampler < 0 ? !M.smp.empty() : with_sampler != 0).total;
    return KR_OK;
}
extern "C" int kr_decode_slot_image_info(const void* image, size_t bytes, int32_t* seq_len_out, int32_t* kv_fp8_out, int32_t* has_sampler_out, uint64_t* geometry_out) {
    if (!image) return kr_fail(KR_ERR_VALUE, "null image");
    KrSlotImageHeader h;
    if (const int bad = kr_slot_image_check(image, bytes, &h)) return kr_fail(KR_ERR_VALUE, "slot image: %s", swap_image_fault(bad));
    if (seq_len_out) *seq_len_out = (int32_t)h.seq_len;
    if (kv_fp8_out) *kv_fp8_out = (int32_t)h.kv_fp8;
    if (has_sampler_out) *has_sampler_out = (int32_t)h.has_sampler;
    if (geometry_out) *geometry_out = h.geometry;
    return KR_OK;
}
extern "C" int kr_decode_slots_export(kr_decode_store* s, int n, const int32_t* slots, const int32_t* seq_lens, void* const* images, const size_t* image_bytes,
                                      int release) {
    if (int rc = multi_begin(s)) return rc;
    kr_multi_state& M = *s->multi;
    if (int rc = swap_slots_ok(M, n, slots)) return rc;
    if (!seq_lens || !images || !image_bytes) return kr_fail(KR_ERR_VALUE, "null seq_lens / images / image_bytes");
    const KrSlotGeo geo = swap_geo(s);
    const bool smp = !M.smp.empty();
    std::vector<KrSlotLayout> lay;
    for (int i = 0; i < n; i++) {
        if (seq_lens[i] < 0 || seq_lens[i] > M.max_seq) return kr_fail(KR_ERR_VALUE, "row %d: seq_len %d outside [0, %d] (slot max_seq)", i, seq_lens[i], M.max_seq);
        if (!images[i]) return kr_fail(KR_ERR_VALUE, "row %d: null image", i);
        lay.push_back(kr_slot_image_layout(geo, seq_lens[i], smp));
        if (image_bytes[i] != (size_t)lay.back().total)
            return kr_fail(KR_ERR_VALUE, "row %d: image_bytes %zu, but the image of %d positions %s a sampler has %zu (kr_decode_slot_image_bytes)", i, image_bytes[i], seq_lens[i],
                           smp ? "with" : "without", (size_t)lay.back().total);
    }
    KR_HIP(hipSetDevice(s->eng->device));
    hipStream_t st = s->eng->stream;
    if (int rc = swap_ensure(s)) return rc;
    if (int rc = order_after_store(s, st)) return rc;
    SwapDrain drain{st, M.sw_stream};
    if (int rc = pg_flush(M, st)) return rc;      // a fork's queued boundary copies and the zeroes of freshly mapped pages land ahead of the pack launches
    std::vector<SwapRange> ranges;
    if (int rc = swap_plan(s, n, slots, lay, st, ranges)) return rc;
    if (int rc = swap_out(M, ranges, images, st)) return rc;
    for (int i = 0; i < n; i++) {      // the host's part of every image: header, table, zero gaps, the sampler's parameters
        kr_slot_image_frame(lay[(size_t)i], images[i]);
        if (!smp) continue;
        const kr_multi_state::Sampler& p = M.smp[(size_t)slots[i]];
        const int32_t top_k = p.top_k;
        char* at = (char*)images[i] + lay[(size_t)i].sampler;
        memcpy(at, &p.temperature, 4); memcpy(at + 4, &top_k, 4); memcpy(at + 8, &p.top_p, 4); memcpy(at + 12, &p.penalty, 4);
    }
    KR_HIP(hipStreamSynchronize(M.sw_stream));
    KR_HIP(hipStreamSynchronize(st));
    if (release && M.pg.paged()) {      // only now, with every image complete: each slot's pages back, as kr_decode_slot_trim(slot, 0)
        std::vector<KrPageChange> freed;
        for (int i = 0; i < n; i++) M.pg.trim(slots[i], 0, &freed);
        return pg_released(s, freed);
    }
    return KR_OK;
}
extern "C" int kr_decode_slots_import(kr_decode_store* s, int n, const int32_t* slots, const void* const* images, const size_t* image_bytes, int32_t* seq_lens_out) {
    if (int rc = multi_begin(s)) return rc;
    kr_multi_state& M = *s->multi;
    if (int rc = swap_slots_ok(M, n, slots)) return rc;
    if (!images || !image_bytes || !seq_lens_out) return kr_fail(KR_ERR_VALUE, "null images / image_bytes / seq_lens_out");
    const KrSlotGeo geo = swap_geo(s);
    std::vector<KrSlotLayout> lay;
    std::vector<long long> lens((size_t)n);
    bool any_sampler = false;
    for (int i = 0; i < n; i++) {
        if (!images[i]) return kr_fail(KR_ERR_VALUE, "row %d: null image", i);
        KrSlotImageHeader h;
        int bad = kr_slot_image_check(images[i], image_bytes[i], &h);
        if (!bad) bad = kr_slot_image_match(images[i], h, geo, M.max_seq);
        if (bad) return kr_fail(KR_ERR_VALUE, "row %d: slot image of %zu bytes: %s", i, image_bytes[i], swap_image_fault(bad));
        lay.push_back(kr_slot_image_layout(geo, (int)h.seq_len, h.has_sampler != 0));
        lens[(size_t)i] = h.seq_len; any_sampler |= h.has_sampler != 0;
        if (h.has_sampler) {      // what kr_decode_slot_sampler refuses of its own argument: the image may not bring a sampler the setter would never leave
            float t; memcpy(&t, (const char*)images[i] + lay.back().sampler, 4);
            if (!(t >= 0.0f)) return kr_fail(KR_ERR_VALUE, "row %d: slot image: its sampler's temperature must be >= 0", i);
        }
    }
    const bool paged = M.pg.paged();
    if (paged) {      // all or nothing: the pages [0, seq_len) of every image, out of the free pages and those the named slots give back (as fork_fit counts)
        long long need = 0;
        for (int i = 0; i < n; i++) need += M.pg.pages_of(lens[(size_t)i]);
        const int gain = M.pg.would_free(n, slots);
        if (need > (long long)M.pg.n_free + gain)
            return kr_fail(KR_ERR_STATE, "the import of %d slot images does not fit the page pool: %lld pages of %d positions, %d of %d are free (%d of them once the named slots are released)",
                           n, need, M.pg.page_tokens, M.pg.n_free + gain, M.pg.n_pages, gain);
    }
    KR_HIP(hipSetDevice(s->eng->device));
    hipStream_t st = s->eng->stream;
    if (int rc = swap_ensure(s)) return rc;
    if (int rc = order_after_store(s, st)) return rc;
    SwapDrain drain{st, M.sw_stream};
    if (any_sampler) if (int rc = swap_samplers(s, st)) return rc;
    if (paged) {      // the named slots release what they held (as kr_decode_slot_trim(slot, 0)), then map fresh pages, one reference each: an import never shares
        for (int i = 0; i < n; i++) for (int j = 0; j < M.pg.stride; j++) M.pg.drop(slots[i], j, nullptr);
        M.pg.prune();
        int need = 0, have = 0;
        if (M.pg.reserve(n, slots, lens.data(), nullptr, &need, &have) >= 0) return kr_fail(KR_ERR_STATE, "slot import: the page count above no longer holds (%d needed, %d free)", need, have);
        if (int rc = pg_flush(M, st)) return rc;      // the new pages read as zero: the tail of a boundary page comes from here
        for (int i = 0; i < n; i++) if (int rc = pg_upload(M, slots[i], 0, M.pg.stride - 1, st)) return rc;
    }
    for (int i = 0; i < n; i++) {
        const size_t slot = (size_t)slots[i];
        for (size_t li = 0; li < s->layers.size() && !paged; li++) {      // flat slots: rows [seq_len, max_seq) zeroed, as fork does
            if (s->layers[li].attn != ATTN_GQA && s->layers[li].attn != ATTN_MLA) continue;
            for (int hb = 0; hb < 2; hb++) {
                const size_t stride = hb ? M.b_stride[li] : M.a_stride[li], head = (hb ? M.b_row[li] : M.a_row[li]) * (size_t)lens[(size_t)i];
                if (stride > head) KR_HIP(hipMemsetAsync((char*)(hb ? M.b[li].p : M.a[li].p) + slot * stride + head, 0, stride - head, st));
            }
        }
        if (M.smp.empty()) continue;
        kr_multi_state::Sampler p;
        if (lay[(size_t)i].sampler) {
            int32_t top_k = 0;
            const char* at = (const char*)images[i] + lay[(size_t)i].sampler;
            memcpy(&p.temperature, at, 4); memcpy(&top_k, at + 4, 4); memcpy(&p.top_p, at + 8, 4); memcpy(&p.penalty, at + 12, 4);
            p.top_k = top_k;
        } else {      // an image without a sampler: greedy, a zero seen set and a zero state, like a fresh slot
            KR_HIP(hipMemsetAsync((uint32_t*)M.smp_seen.p + slot * M.smp_words, 0, M.smp_words * 4, st));
            KR_HIP(hipMemsetAsync((uint64_t*)M.smp_rng.p + slot, 0, 8, st));
        }
        M.smp[slot] = p;
    }
    std::vector<SwapRange> ranges;
    if (int rc = swap_plan(s, n, slots, lay, st, ranges)) return rc;
    if (int rc = swap_in(M, ranges, images, st)) return rc;
    KR_HIP(hipStreamSynchronize(M.sw_stream));
    KR_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < n; i++) seq_lens_out[i] = (int32_t)lens[(size_t)i];
    return KR_OK;
}

extern "C" int kr_decode_slot_save(kr_decode_store* s, int slot, int seq_len) { return slot_copy(s, slot, seq_len, true); }
extern "C" int kr_decode_slot_load(kr_decode_store* s, int slot, int seq_len) { return slot_copy(s, slot, seq_len, false); }

extern "C" int kr_decode_step_multi(kr_decode_store* s, int n, const int32_t* slots, const int32_t* tokens, const int32_t* positions,
                                    int32_t* next_out, float* logits_out, void* stream) {
    return step_entry(s, Rows{n, slots, nullptr, tokens, positions}, next_out, logits_out, false, stream);
}

extern "C" int kr_decode_generate_multi(kr_decode_store* s, int n, const int32_t* slots, const int32_t* first_tokens, const int32_t* start_positions,
                                        int max_tokens, const int* stop_ids, int n_stop, int32_t* tokens_out, int32_t* n_out, void* stream) {
    return generate_slots(s, Rows{n, slots, nullptr, first_tokens, start_positions}, max_tokens, Drafting{nullptr, nullptr, 0, 1}, nullptr, stop_ids, n_stop,
                          GenOut{tokens_out, n_out, nullptr, nullptr}, stream);
}

// ---- per-row sampling (docs/design/14-multi-sampling.md)
extern "C" int kr_decode_slot_sampler(kr_decode_store* s, int slot, int first_token, float temperature, int top_k, float top_p, float presence_penalty,
                                      uint64_t rng_seed) {
    if (int rc = multi_begin(s)) return rc;
    if (int rc = slot_in_range(s, slot)) return rc;
    if (!(temperature >= 0.0f)) return kr_fail(KR_ERR_VALUE, "temperature must be >= 0");
    KR_HIP(hipSetDevice(s->eng->device));
    return set_sampler(s, slot, first_token, temperature, top_k, top_p, presence_penalty, rng_seed, s->eng->stream);
}

extern "C" int kr_decode_step_multi_sample(kr_decode_store* s, int n, const int32_t* slots, const int32_t* tokens, const int32_t* positions,
                                           int32_t* next_out, float* logits_out, void* stream) {
    return step_entry(s, Rows{n, slots, nullptr, tokens, positions}, next_out, logits_out, true, stream);
}

// ---- multi-token extend of slots (docs/design/17-multi-extend.md)
extern "C" int kr_decode_extend_multi(kr_decode_store* s, int n, const int32_t* slots, const int32_t* counts, const int32_t* tokens, const int32_t* positions,
                                      int32_t* next_out, float* logits_out, int sample, void* stream) {
    // null counts are refused with the other null arguments (to the pass they would mean one token per row)
    return step_entry(s, Rows{n, counts ? slots : nullptr, counts, tokens, positions}, next_out, logits_out, sample != 0, stream);
}

extern "C" int kr_decode_generate_multi_sample(kr_decode_store* s, int n, const int32_t* slots, const int32_t* first_tokens, const int32_t* start_positions,
                                               int max_tokens, const float* temperature, const int* top_k, const float* top_p, const float* presence_penalty,
                                               const uint64_t* rng_seeds, const int* stop_ids, int n_stop, int32_t* tokens_out, int32_t* n_out, void* stream) {
    const SamplerCols smp{temperature, top_k, top_p, presence_penalty, rng_seeds};
    return generate_slots(s, Rows{n, slots, nullptr, first_tokens, start_positions}, max_tokens, Drafting{nullptr, nullptr, 0, 1}, &smp, stop_ids, n_stop,
                          GenOut{tokens_out, n_out, nullptr, nullptr}, stream);
}

// test aid: the batched sampler on host rows, row b = "slot" b (its own seen bitmap and xorshift64 state)
extern "C" int kr_sample_rows(const float* logits, int n, int vocab, const float* temperature, const int* top_k, const float* top_p,
                              const float* presence_penalty, const uint32_t* seen, uint64_t* rng_state, int32_t* tokens_out, int force_loop) {
    if (!logits || !temperature || !top_k || !top_p || !presence_penalty || !rng_state || !tokens_out || vocab <= 0)
        return kr_fail(KR_ERR_VALUE, "kr_sample_rows: null pointer or empty vocabulary");
    if (n < 1 || n > KR_MULTI_MAX) return kr_fail(KR_ERR_VALUE, "%d rows, must be in [1, %d]", n, KR_MULTI_MAX);
    for (int i = 0; i < n; i++) if (!(temperature[i] >= 0.0f)) return kr_fail(KR_ERR_VALUE, "row %d: temperature must be >= 0", i);
    int dev_count = 0;
    if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count == 0) return kr_fail(KR_ERR_HIP, "no HIP device");
    std::vector<KrMsRow> rows((size_t)n);
    for (int b = 0; b < n; b++) rows[(size_t)b] = mode_row(b, temperature[b], top_k[b], top_p[b], presence_penalty[b], vocab, force_loop != 0);
    const size_t V = (size_t)vocab, words = (V + 31) / 32;
    kr_multi_state M;
    DevBuf lg, sn, rg, ids;
    if (int rc = sampler_scratch(M, vocab, n, rows)) return rc;
    if (lg.ensure((size_t)n * V * 4) || sn.ensure((size_t)n * words * 4) || rg.ensure((size_t)n * 8) || ids.ensure((size_t)n * 4))
        return kr_fail(KR_ERR_HIP, "hipMalloc failed");
    KR_HIP(hipMemcpy(lg.p, logits, (size_t)n * V * 4, hipMemcpyHostToDevice));
    if (seen) KR_HIP(hipMemcpy(sn.p, seen, (size_t)n * words * 4, hipMemcpyHostToDevice));
    else KR_HIP(hipMemset(sn.p, 0, (size_t)n * words * 4));
    KR_HIP(hipMemcpy(rg.p, rng_state, (size_t)n * 8, hipMemcpyHostToDevice));
    KR_HIP(hipMemcpy(M.smp_rows.p, rows.data(), (size_t)n * sizeof(KrMsRow), hipMemcpyHostToDevice));
    if (kr_launch_multi_sample(sampler_args(M, (const float*)lg.p, vocab, n, rows, (uint32_t*)sn.p, words, (uint64_t*)rg.p, (int*)ids.p), nullptr))
        return kr_fail(KR_ERR_HIP, "batched sampler launch failed");
    KR_HIP(hipDeviceSynchronize());
    KR_HIP(hipMemcpy(tokens_out, ids.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    KR_HIP(hipMemcpy(rng_state, rg.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    return KR_OK;
}

// ---- verify and commit over slots (docs/design/18-multi-verify.md, 19-multi-verify-sample.md)
static int verify_entry(kr_decode_store* s, Rows r, int32_t* ids_out, int32_t* n_match_out, bool sample, void* stream) {
    if (!r.counts) r.slots = nullptr;      // null counts are refused with the other null arguments
    if (int rc = multi_begin(s)) return rc;
    if (int rc = check_args(s, r, 0)) return rc;
    if (!ids_out || !n_match_out) return kr_fail(KR_ERR_VALUE, "null %s / n_match_out", sample ? "sampled_out" : "greedy_out");
    for (int i = 0; i < r.n; i++)
        if (r.counts[i] > KR_VERIFY_MAX) return kr_fail(KR_ERR_VALUE, "row %d: a run of %d tokens, at most %d (KR_VERIFY_MAX) in a verify", i, r.counts[i], KR_VERIFY_MAX);
    if (int rc = paged_refuse(s)) return rc;
    if (int rc = pg_reserve_rows(s, r, 0, nullptr)) return rc;      // the drafted positions too: the commit leaves them mapped (the caller may trim)
    KR_HIP(hipSetDevice(s->eng->device));
    hipStream_t st = kr_pick_stream(s->eng, stream);
    if (int rc = order_after_store(s, st)) return rc;
    return verify_impl(s, r, ids_out, n_match_out, st, sample);
}
extern "C" int kr_decode_verify_multi(kr_decode_store* s, int n, const int32_t* slots, const int32_t* counts, const int32_t* tokens, const int32_t* positions,
                                      int32_t* greedy_out, int32_t* n_match_out, void* stream) {
    return verify_entry(s, Rows{n, slots, counts, tokens, positions}, greedy_out, n_match_out, false, stream);
}
extern "C" int kr_decode_verify_multi_sample(kr_decode_store* s, int n, const int32_t* slots, const int32_t* counts, const int32_t* tokens, const int32_t* positions,
                                             int32_t* sampled_out, int32_t* n_match_out, void* stream) {
    return verify_entry(s, Rows{n, slots, counts, tokens, positions}, sampled_out, n_match_out, true, stream);
}

extern "C" int kr_decode_commit_multi(kr_decode_store* s, const int32_t* n_keep) {
    if (int rc = multi_ready(s)) return rc;
    if (!s->multi || !s->multi->v_pending) return kr_fail(KR_ERR_STATE, "no verify over slots is pending");
    return commit_impl(s, n_keep);
}

extern "C" int kr_decode_generate_multi_lookup(kr_decode_store* s, int n, const int32_t* slots, const int32_t* contexts, const int32_t* n_context,
                                               const int32_t* first_tokens, const int32_t* start_positions, int max_tokens, int max_draft, int ngram_max,
                                               const int* stop_ids, int n_stop, int32_t* tokens_out, int32_t* n_out, int* n_passes_out,
                                               int32_t* n_accepted_out, void* stream) {
    return generate_slots(s, Rows{n, slots, nullptr, first_tokens, start_positions}, max_tokens, Drafting{contexts, n_context, max_draft, ngram_max}, nullptr, stop_ids,
                          n_stop, GenOut{tokens_out, n_out, n_passes_out, n_accepted_out}, stream);
}
extern "C" int kr_decode_generate_multi_lookup_sample(kr_decode_store* s, int n, const int32_t* slots, const int32_t* contexts, const int32_t* n_context,
                                                      const int32_t* first_tokens, const int32_t* start_positions, int max_tokens, int max_draft, int ngram_max,
                                                      const float* temperature, const int* top_k, const float* top_p, const float* presence_penalty,
                                                      const uint64_t* rng_seeds, const int* stop_ids, int n_stop, int32_t* tokens_out, int32_t* n_out,
                                                      int* n_passes_out, int32_t* n_accepted_out, void* stream) {
    const SamplerCols smp{temperature, top_k, top_p, presence_penalty, rng_seeds};
    return generate_slots(s, Rows{n, slots, nullptr, first_tokens, start_positions}, max_tokens, Drafting{contexts, n_context, max_draft, ngram_max}, &smp, stop_ids,
                          n_stop, GenOut{tokens_out, n_out, n_passes_out, n_accepted_out}, stream);
}

extern "C" int kr_decode_slot_sampler_get(kr_decode_store* s, int slot, uint32_t* seen_out, uint64_t* rng_out) {
    if (int rc = multi_begin(s)) return rc;
    if (int rc = slot_in_range(s, slot)) return rc;
    kr_multi_state& M = *s->multi;
    if (!seen_out || !rng_out) return kr_fail(KR_ERR_VALUE, "null seen_out / rng_out");
    const size_t words = ((size_t)s->vocab + 31) / 32;
    if (M.smp.empty()) { std::fill(seen_out, seen_out + words, 0u); *rng_out = 0; return KR_OK; }      // no sampler was ever set
    KR_HIP(hipSetDevice(s->eng->device));
    KR_HIP(hipDeviceSynchronize());          // a sampled step may still be in flight on the caller's stream
    KR_HIP(hipMemcpy(seen_out, (const uint32_t*)M.smp_seen.p + (size_t)slot * words, words * 4, hipMemcpyDeviceToHost));
    KR_HIP(hipMemcpy(rng_out, (const uint64_t*)M.smp_rng.p + slot, 8, hipMemcpyDeviceToHost));
    return KR_OK;
}

// test aid: the verify-form sampler, the accept kernel and the sampler commit on host rows, run i = "slot" i
extern "C" int kr_sample_runs(const float* logits, int n, const int32_t* counts, const int32_t* tokens, int vocab, const float* temperature, const int* top_k,
                              const float* top_p, const float* presence_penalty, uint32_t* seen, uint64_t* rng_state, int32_t* n_keep, int32_t* ids_out,
                              int32_t* n_match_out, int force_loop) {
    if (!logits || !counts || !tokens || !temperature || !top_k || !top_p || !presence_penalty || !seen || !rng_state || !n_keep || !ids_out || !n_match_out || vocab <= 0)
        return kr_fail(KR_ERR_VALUE, "kr_sample_runs: null pointer or empty vocabulary");
    if (n < 1 || n > KR_MULTI_MAX) return kr_fail(KR_ERR_VALUE, "%d rows, must be in [1, %d]", n, KR_MULTI_MAX);
    size_t total = 0;
    for (int i = 0; i < n; i++) {
        if (!(temperature[i] >= 0.0f)) return kr_fail(KR_ERR_VALUE, "row %d: temperature must be >= 0", i);
        if (counts[i] < 1 || counts[i] > KR_VERIFY_MAX) return kr_fail(KR_ERR_VALUE, "row %d: a run of %d tokens, must be in [1, %d]", i, counts[i], KR_VERIFY_MAX);
        for (int t = 0; t < counts[i]; t++)
            if (tokens[total + t] < 0 || tokens[total + t] >= vocab) return kr_fail(KR_ERR_VALUE, "row %d: token %d of its run, id %d, out of range (vocab %d)", i, t, tokens[total + t], vocab);
        total += (size_t)counts[i];
    }
    int dev_count = 0;
    if (hipGetDeviceCount(&dev_count) != hipSuccess || dev_count == 0) return kr_fail(KR_ERR_HIP, "no HIP device");
    std::vector<int32_t> slots((size_t)n), zeros((size_t)n, 0);
    std::vector<KrMsRow> per_run, rows; std::vector<KrMsAt> at;
    for (int i = 0; i < n; i++) { slots[(size_t)i] = i; per_run.push_back(mode_row(i, temperature[i], top_k[i], top_p[i], presence_penalty[i], vocab, force_loop != 0)); }
    size_t T = 0; int max_pos = 0;
    std::vector<int> row_of;
    const std::vector<int32_t> h = lay_rows(Rows{n, slots.data(), counts, tokens, zeros.data()}, T, max_pos, &row_of);
    run_rows(n, counts, row_of, per_run, rows, at);
    const size_t V = (size_t)vocab, words = (V + 31) / 32;
    kr_multi_state M;
    DevBuf lg, sn, rg, ids, dr, out, keep;
    if (int rc = sampler_scratch(M, vocab, (int)T, rows)) return rc;
    if (lg.ensure(T * V * 4) || sn.ensure((size_t)n * words * 4) || rg.ensure((size_t)n * 8) || ids.ensure(T * 4) || dr.ensure(h.size() * 4) ||
        out.ensure((T + (size_t)n) * 4) || keep.ensure((size_t)n * 4))
        return kr_fail(KR_ERR_HIP, "hipMalloc failed");
    for (size_t j = 0; j < T; j++) KR_HIP(hipMemcpy((float*)lg.p + (size_t)row_of[j] * V, logits + j * V, V * 4, hipMemcpyHostToDevice));
    KR_HIP(hipMemcpy(sn.p, seen, (size_t)n * words * 4, hipMemcpyHostToDevice));
    KR_HIP(hipMemcpy(rg.p, rng_state, (size_t)n * 8, hipMemcpyHostToDevice));
    KR_HIP(hipMemcpy(dr.p, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    const int32_t* d_rows = (const int32_t*)dr.p;
    if (int rc = sample_runs(M, (const float*)lg.p, vocab, rows, at, d_rows, (uint32_t*)sn.p, words, (uint64_t*)rg.p, (int*)ids.p, nullptr)) return rc;
    kr_launch_multi_accept((const int*)ids.p, d_rows + T, d_rows + 3 * T, n, (int)T, (int*)out.p, nullptr);
    KR_HIP(hipGetLastError());
    KR_HIP(hipDeviceSynchronize());
    KR_HIP(hipMemcpy(ids_out, out.p, T * 4, hipMemcpyDeviceToHost));
    KR_HIP(hipMemcpy(n_match_out, (const int32_t*)out.p + T, (size_t)n * 4, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) n_keep[i] = n_keep[i] < 0 ? n_match_out[i] + 1 : std::min(n_keep[i], n_match_out[i] + 1);
    KR_HIP(hipMemcpy(keep.p, n_keep, (size_t)n * 4, hipMemcpyHostToDevice));
    kr_launch_ms_commit((const KrMsRow*)M.smp_rows.p, d_rows + 3 * T, (const int*)keep.p, n, (const int*)ids.p, vocab, (uint32_t*)sn.p, words, (uint64_t*)rg.p, nullptr);
    KR_HIP(hipGetLastError());
    KR_HIP(hipDeviceSynchronize());
    KR_HIP(hipMemcpy(seen, sn.p, (size_t)n * words * 4, hipMemcpyDeviceToHost));
    KR_HIP(hipMemcpy(rng_state, rg.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    return KR_OK;
}
