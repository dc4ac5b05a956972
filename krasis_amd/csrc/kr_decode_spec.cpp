// kr_decode_spec.cpp -- greedy generation with prompt-lookup drafts (docs/design/12-speculative.md).  Each pass proposes the continuation of the
// latest earlier occurrence of the history's trailing n-gram, runs [last token, draft] through kr_decode_verify (the exact prompt pass) and keeps the
// longest prefix the model agrees with plus its own next token; kr_decode_commit rolls the linear-attention states back to exactly what the plain loop
// (kr_decode_generate_greedy) would have consumed.  No draft: the plain decode step.  Tokens, count, return code and state equal the plain loop's.
#include <algorithm>
#include <chrono>
#include <climits>
#include <cstring>
#include <vector>

#include "../../include/krasis_hip.h"
#include "kr_decode_internal.h"
#include "kr_lookup_index.h"

extern "C" int kr_lookup_draft(const int32_t* history, int n_history, int ngram_max, int max_draft, int32_t* draft_out) {
    if (n_history < 0 || (n_history > 0 && !history)) return -kr_fail(KR_ERR_VALUE, "kr_lookup_draft: bad history (%d tokens)", n_history);
    if (ngram_max < 1) return -kr_fail(KR_ERR_VALUE, "kr_lookup_draft: ngram_max %d must be >= 1", ngram_max);
    if (max_draft < 0 || (max_draft > 0 && !draft_out)) return -kr_fail(KR_ERR_VALUE, "kr_lookup_draft: bad max_draft %d / output", max_draft);
    const int n = n_history;
    for (int g = std::min(ngram_max, n - 1); g >= 1; g--)
        for (int j = n - 1 - g; j >= 0; j--) {
            if (memcmp(history + j, history + n - g, (size_t)g * 4)) continue;
            const int b = j + g, e = std::min(b + max_draft, n);
            for (int i = b; i < e; i++) draft_out[i - b] = history[i];
            return e - b;
        }
    return 0;
}

extern "C" int kr_decode_generate_lookup(kr_decode_store* s, const int32_t* context, int n_context, int first_token, int start_pos, int max_tokens,
                                         int max_draft, int ngram_max, const int* stop_ids, int n_stop, int* tokens_out, int* n_out,
                                         int* n_passes_out, int* n_accepted_out, void* stream) {
    if (!s) return kr_fail(KR_ERR_VALUE, "null decode store");
    if (!s->configured) return kr_fail(KR_ERR_STATE, "Call configure_decode first");
    if (!n_out || !tokens_out) return kr_fail(KR_ERR_VALUE, "null output pointer");
    if (int rc = kr_spec_pending_fail(s)) return rc;
    if (int rc = kr_spec_refuse(s)) return rc;
    if (max_draft < 0 || max_draft > KR_VERIFY_MAX - 1) return kr_fail(KR_ERR_VALUE, "max_draft %d out of range [0, %d]", max_draft, KR_VERIFY_MAX - 1);
    if (ngram_max < 1 || ngram_max > KR_LOOKUP_NGRAM_MAX) return kr_fail(KR_ERR_VALUE, "ngram_max %d out of range [1, %d]", ngram_max, KR_LOOKUP_NGRAM_MAX);
    if (n_context < 0 || (n_context > 0 && !context)) return kr_fail(KR_ERR_VALUE, "bad context (%d tokens)", n_context);
    if (n_stop < 0 || (n_stop > 0 && !stop_ids)) return kr_fail(KR_ERR_VALUE, "bad stop ids (%d)", n_stop);
    for (int i = 0; i < n_context; i++)      // a context token becomes a draft token: it must be a valid id
        if (context[i] < 0 || context[i] >= s->vocab) return kr_fail(KR_ERR_VALUE, "context token id %d out of range (vocab %d)", context[i], s->vocab);
    KR_HIP(hipSetDevice(s->eng->device));
    hipStream_t st = kr_pick_stream(s->eng, stream);
    // a pass over positions [pos, pos + k] must stay inside the KV cache and the rope tables; where it cannot, the plain step runs (and fails where the plain loop fails)
    int limit = INT_MAX;
    if (s->kv_max_seq > 0) limit = std::min(limit, s->kv_max_seq);
    if (s->max_rope_seq > 0) limit = std::min(limit, s->max_rope_seq);
    for (const DLayer& L : s->layers) if (L.attn == ATTN_MLA) limit = std::min(limit, L.mla_rope_seq);
    LookupIndex ix(ngram_max);
    ix.h.reserve((size_t)n_context + 1 + (size_t)std::max(max_tokens, 0));
    for (int i = 0; i < n_context; i++) ix.push(context[i]);
    ix.push(first_token);
    auto is_stop = [&](int t) { for (int j = 0; j < n_stop; j++) if (stop_ids[j] == t) return true; return false; };
    const auto t_start = std::chrono::steady_clock::now();
    auto stamp = [&]() { kr_standalone_set_elapsed(s, std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count()); };
    int tok = first_token, pos = start_pos, n = 0, passes = 0, accepted = 0;
    int32_t draft[KR_VERIFY_MAX], pass[KR_VERIFY_MAX], greedy[KR_VERIFY_MAX];
    while (n < max_tokens) {
        // a negative position drafts nothing: the plain step refuses it as the plain loop does
        const int k = pos < 0 ? 0 : lookup_clamp(max_draft > 0 ? ix.draft(max_draft, draft) : 0, draft, max_tokens - n, limit - pos, INT_MAX, is_stop);
        passes++;
        int m = 0;
        if (k == 0) {      // the plain loop's step (graph replay)
            if (int rc = kr_decode_step(s, tok, pos, nullptr, stream)) { stamp(); return rc; }
            KR_HIP(hipMemcpyAsync(greedy, s->tok.p, 4, hipMemcpyDeviceToHost, st));
            KR_HIP(hipStreamSynchronize(st));
        } else {
            pass[0] = tok;
            for (int i = 0; i < k; i++) pass[i + 1] = draft[i];
            if (int rc = kr_decode_verify(s, pass, k + 1, pos, greedy, &m, stream)) { stamp(); return rc; }
        }
        const LookupKept kept = lookup_emit(greedy, m, tokens_out, n, &ix, is_stop);
        if (k > 0) {
            accepted += std::min(m, kept.keep);
            if (int rc = kr_decode_commit(s, kept.keep)) { stamp(); return rc; }
        }
        tok = greedy[kept.keep - 1]; pos += kept.keep;
        if (kept.stop) break;
    }
    KR_HIP(hipStreamSynchronize(st));
    stamp();
    *n_out = n;
    if (n_passes_out) *n_passes_out = passes;
    if (n_accepted_out) *n_accepted_out = accepted;
    return KR_OK;
}
