// Host-only check of retile_gguf for Q3_K (docs/design/47-gguf-q3k.md): random raw blocks of a few ragged rows are re-tiled and every record and header byte is
// compared against the block definition; bytes of rows past N must stay zero.  Needs no GPU: it includes kr_engine.cpp for the static function and takes the size
// functions from the built library.  Meant to run under the host sanitizers:
//   hipcc -std=c++17 -O1 -g -fsanitize=address,undefined -Ikrasis_amd/csrc -Iinclude tools/probes/retile_q3k_check.cpp -Lkrasis_amd -lkrasis_hip -Wl,-rpath,$PWD/krasis_amd -o retile_q3k_check
#include "kr_engine.cpp"

#include <cstdio>
#include <random>

int main() {
    std::mt19937 rng(11);
    int bad = 0;
    for (int N : {1, 8, 11, 20}) for (int K : {256, 768}) {
        const int nb = K / 256, nt = (N + 7) / 8;
        std::vector<uint8_t> src((size_t)N * nb * 110), dq(gg_q_bytes(GG_Q3_K, K, N), 0xAA), dh(gg_h_bytes(GG_Q3_K, K, N), 0xAA);
        for (auto& b : src) b = (uint8_t)rng();
        if (dq.size() != (size_t)nt * nb * 768 || dh.size() != (size_t)nt * nb * 128) { printf("N %d K %d: sizes %zu %zu\n", N, K, dq.size(), dh.size()); return 1; }
        retile_gguf(GG_Q3_K, src.data(), K, N, dq.data(), dh.data());
        for (int row = 0; row < nt * 8; row++) for (int b = 0; b < nb; b++) {
            const int t = row >> 3, r = row & 7;
            const uint8_t* blk = src.data() + (row < N ? ((size_t)row * nb + b) * 110 : 0);      // {hmask[32], qs[64], scales[12], f16 d}; not read for row >= N
            const uint8_t* hd = dh.data() + (((size_t)t * nb + b) * 8 + r) * 16;
            for (int i = 0; i < 16; i++) bad += hd[i] != (row < N && i < 14 ? blk[96 + i] : 0);
            for (int l = 0; l < 8; l++) {
                const uint8_t* rec = dq.data() + (((size_t)t * nb + b) * 64 + r * 8 + l) * 12;
                const int pos[4] = {2 * l, 2 * l + 1, 16 + 2 * l, 17 + 2 * l};
                for (int i = 0; i < 4; i++) {
                    bad += rec[i] != (row < N ? blk[32 + pos[i]] : 0);
                    bad += rec[4 + i] != (row < N ? blk[64 + pos[i]] : 0);
                    bad += rec[8 + i] != (row < N ? blk[pos[i]] : 0);
                }
                if (row < N) for (int c = 0; c < 8; c++) for (int i = 0; i < 4; i++) {      // the word-wise unpack gives the element's code: e = 32 c + pos[i], n = c >> 2, j = c & 3
                    const int n = c >> 2, j = c & 3, p = pos[i];
                    const int want = ((blk[32 + 32 * n + p] >> (2 * j)) & 3) | (((blk[p] >> (4 * n + j)) & 1) << 2);
                    uint32_t w[3]; memcpy(w, rec, 12);
                    const uint32_t codes = ((w[n] >> (2 * j)) & 0x03030303u) | (((w[2] >> c) & 0x01010101u) << 2);
                    bad += (int)((codes >> (8 * i)) & 0xFF) != want;
                }
            }
        }
    }
    printf("retile_gguf Q3_K: %d mismatching bytes\n", bad);
    return bad != 0;
}
