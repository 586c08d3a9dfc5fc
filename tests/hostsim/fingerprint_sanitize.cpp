// The fingerprint driver (fingerprint_sim.cpp) as a program of its own, for -fsanitize=address,undefined: seeded random batches -- runs of
// empty documents, documents of one token, documents around the shingle length and around the tile, ids all over uint32 -- in heap blocks
// of exactly their size, several specs, at tiles of 8, 64 and TK_FP_TILE positions: the runs must be clean, agree with each other array for
// array and keep the pass's invariants (the shingle counts follow from the lengths, a document without shingles keeps TK_FP_NONE, two
// documents with the same ids have the same fingerprint).  Host code only.
#include <stdio.h>

#include <algorithm>
#include <random>

#include "fingerprint_sim.cpp"

namespace {
struct Result {
    int64_t rc;
    std::vector<uint32_t> sig;
    std::vector<uint64_t> band, exact, nsh;
    bool operator==(const Result& o) const { return rc == o.rc && sig == o.sig && band == o.band && exact == o.exact && nsh == o.nsh; }
};
Result run(const std::vector<uint32_t>& tok, const std::vector<uint64_t>& off, uint32_t k, uint32_t P, uint32_t B, uint64_t seed, uint32_t tile) {
    const uint64_t n = off.size() - 1;
    Result r;
    r.sig.assign(n * P, 1), r.band.assign(n * B, 1), r.exact.assign(n, 1), r.nsh.assign(n, 1);
    r.rc = fingerprint_sim(tok.data(), tok.size(), off.data(), n, k, P, B, seed, tile, r.sig.data(), r.band.data(), r.exact.data(), r.nsh.data());
    return r;
}
}  // namespace

int main() {
    std::mt19937_64 rng(0xF1A6);
    const uint32_t specs[][3] = {{5, 128, 16}, {1, 1, 1}, {32, 256, 256}, {5, 20, 4}, {32, 64, 1}, {3, 65, 13}};
    const uint32_t lens[] = {0, 0, 0, 1, 1, 2, 4, 5, 6, 7, 8, 9, 31, 32, 33, 63, 64, 65, 200, TK_FP_TILE - 1, TK_FP_TILE, TK_FP_TILE + 1};
    for (int it = 0; it < 60; ++it) {
        std::vector<uint64_t> off{0};
        const int docs = (int)(rng() % 40);
        for (int d = 0; d < docs; ++d) off.push_back(off.back() + lens[rng() % (it % 5 == 0 ? 22 : 19)]);
        // the last document repeats the one before it, where there is one
        if (docs > 1) off.push_back(off.back() + (off[docs] - off[docs - 1]));
        std::vector<uint32_t> tok(off.back());
        for (auto& t : tok) t = rng() % 4 == 0 ? (uint32_t)(rng() % 3) * 0x7FFFFFFFu + (uint32_t)(rng() % 2) : (uint32_t)rng();
        if (docs > 1)
            for (uint64_t i = off[docs]; i < off[docs + 1]; ++i) tok[i] = tok[i - (off[docs] - off[docs - 1])];
        const uint64_t n = off.size() - 1;
        for (const auto& s : specs) {
            const uint32_t k = s[0], P = s[1], B = s[2];
            const uint64_t seed = rng();
            const Result a = run(tok, off, k, P, B, seed, 8);
            if (a.rc != 0) return printf("rc %lld at %d\n", (long long)a.rc, it), 1;
            if (!(a == run(tok, off, k, P, B, seed, 64)) || !(a == run(tok, off, k, P, B, seed, TK_FP_TILE))) return printf("the tile size changes the result at %d k %u\n", it, k), 1;
            for (uint64_t d = 0; d < n; ++d) {
                const uint64_t L = off[d + 1] - off[d], want = L == 0 ? 0 : L < k ? 1 : L - k + 1;
                if (a.nsh[d] != want) return printf("n_shingles at %d doc %llu\n", it, (unsigned long long)d), 1;
                for (uint32_t p = 0; p < P; ++p)
                    if (L == 0 && a.sig[d * P + p] != TK_FP_NONE) return printf("an empty document's signature at %d\n", it), 1;
            }
            if (docs > 1) {
                const uint64_t x = n - 1, y = n - 2;
                if (a.exact[x] != a.exact[y] || !std::equal(a.sig.begin() + x * P, a.sig.begin() + (x + 1) * P, a.sig.begin() + y * P) ||
                    !std::equal(a.band.begin() + x * B, a.band.begin() + (x + 1) * B, a.band.begin() + y * B))
                    return printf("two equal documents differ at %d\n", it), 1;
            }
        }
    }
    printf("fingerprint_sanitize ok\n");
    return 0;
}
