// kr_lookup_index.h -- the prompt-lookup drafting rule, indexed incrementally (docs/design/12-speculative.md): the one copy behind
// kr_decode_generate_lookup (kr_decode_spec.cpp) and kr_decode_generate_multi_lookup (kr_decode_multi.cpp, one index per row)
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
