// kr_lookup_index.h -- the prompt-lookup drafting rule, indexed incrementally, and the rule that decides what a pass runs and keeps
// (docs/design/12-speculative.md): the one copy behind kr_decode_generate_lookup (kr_decode_spec.cpp) and the slot generation loop
// (generate_slots in kr_decode_multi.cpp, one index per row)
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

// the drafting rule of kr_lookup_draft, indexed incrementally: maps[g - 1] holds, per g-gram, the largest start j with j + g <= n - 1 (an occurrence
// that has a continuation).  Appending token n - 1 makes the g-grams ending at n - 2 eligible; later starts overwrite earlier ones.
struct LookupIndex {
    int G;
    std::vector<int32_t> h;
    std::vector<std::unordered_map<std::string, int>> maps;
    explicit LookupIndex(int g) : G(g), maps((size_t)g) {}
    static std::string key(const int32_t* p, int g) { return std::string((const char*)p, (size_t)g * 4); }
    void push(int32_t t) {
        h.push_back(t);
        const int n = (int)h.size();
        for (int g = 1; g <= G && n - 1 - g >= 0; g++) maps[(size_t)g - 1][key(&h[(size_t)(n - 1 - g)], g)] = n - 1 - g;
    }
    int draft(int max_draft, int32_t* out) const {
        const int n = (int)h.size();
        for (int g = std::min(G, n - 1); g >= 1; g--) {
            const auto& m = maps[(size_t)g - 1];
            const auto it = m.find(key(&h[(size_t)(n - g)], g));
            if (it == m.end()) continue;
            const int b = it->second + g, e = std::min(b + max_draft, n);
            for (int i = b; i < e; i++) out[i - b] = h[(size_t)i];
            return e - b;
        }
        return 0;
    }
};

// The two halves of the draft rule, which make speculation exact.  is_stop(id): whether the id ends a sequence.
// lookup_clamp: how many of the d proposed draft tokens a pass runs.  want = tokens the row still wants (the pass yields at most d + 1), room = positions
// from the pass's first one to the end of the cache and rope tables (it occupies d + 1), cap = the most one row may draft in this pass; never below 0, and
// nothing after a stop id, which cannot be kept
template <class Stop>
inline int lookup_clamp(int d, const int32_t* draft, int want, int room, int cap, Stop is_stop) {
    d = std::max(std::min(std::min(d, cap), std::min(want, room) - 1), 0);
    for (int j = 0; j < d; j++) if (is_stop(draft[j])) return j + 1;
    return d;
}
// lookup_emit: ids[0 .. n_match] of a pass are what the plain loop generates next: appended to out (n_out counts them) and to the index (ix null: no index
// is kept), up to and with the first stop id.  After emitting ids[j] the plain loop has consumed tokens 0 .. j of the run: that many are kept
struct LookupKept { int keep; bool stop; };
template <class Stop>
inline LookupKept lookup_emit(const int32_t* ids, int n_match, int32_t* out, int32_t& n_out, LookupIndex* ix, Stop is_stop) {
    for (int j = 0; j <= n_match; j++) {
        out[n_out++] = ids[j];
        if (ix) ix->push(ids[j]);
        if (is_stop(ids[j])) return {j + 1, true};
    }
    return {n_match + 1, false};
}
