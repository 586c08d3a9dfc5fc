// The n-gram driver (ngram_sim.cpp) as a program of its own, for -fsanitize=address,undefined: seeded random batches over a small
// alphabet in heap blocks of exactly their size, a set of the batch's first half in a table as full as it may get, at tiles of 8, 64 and
// TK_NG_TILE positions: the runs must be clean, agree with each other and keep the pass's invariants.  Host code only.
#include <stdio.h>

#include <random>

#include "ngram_sim.cpp"

using V = std::vector<uint64_t>;
static V run(const std::vector<uint32_t>& tok, const V& off, uint64_t n_add, uint32_t k, uint64_t seed, uint32_t tile, std::vector<uint8_t>& mask) {
    const uint64_t n = off.size() - 1;
    int64_t rc;
    void* set = ngram_sim_create(k, seed, off[n_add] ? off[n_add] : 1, &rc);
    V r(4 * n + 2, 1);  // n_hit, n_covered, n_ngrams, first_hit, the count, the status
    mask.assign(tok.size(), 7);
    r[4 * n + 1] = ngram_sim_add(set, tok.data(), off[n_add], off.data(), n_add, tile);
    r[4 * n] = ngram_sim_count(set);
    r[4 * n + 1] |= ngram_sim_overlap(set, tok.data(), tok.size(), off.data(), n, tile, &r[0], &r[n], &r[2 * n], &r[3 * n], mask.data());
    ngram_sim_destroy(set);
    return r;
}

int main() {
    std::mt19937_64 rng(0x96A3);
    const uint32_t lens[] = {0, 0, 0, 1, 2, 12, 13, 14, 26, 31, 32, 33, 63, 64, 65, 200, TK_NG_TILE - 1, TK_NG_TILE, TK_NG_TILE + 1};
    for (int it = 0; it < 40; ++it) {
        V off{0};
        for (int d = 1 + (int)(rng() % 40); d > 0; --d) off.push_back(off.back() + lens[rng() % (it % 5 == 0 ? 19 : 16)]);
        std::vector<uint32_t> tok(off.back());
        for (auto& t : tok) t = rng() % 16 == 0 ? 0xFFFFFFFFu : (uint32_t)(rng() % 3);
        const uint64_t n = off.size() - 1, n_add = n / 2;
        for (uint32_t k : {1u, 2u, 13u, 32u}) {
            const uint64_t seed = rng();
            std::vector<uint8_t> mask, m2, m3;
            const V a = run(tok, off, n_add, k, seed, 8, mask);
            if (a[4 * n + 1] || a != run(tok, off, n_add, k, seed, 64, m2) || a != run(tok, off, n_add, k, seed, TK_NG_TILE, m3) || mask != m2 || mask != m3)
                return printf("a status, or the tile size changes the result, at %d k %u\n", it, k), 1;
            for (uint64_t d = 0; d < n; ++d) {  // (a document that was added is made of hits)
                const uint64_t L = off[d + 1] - off[d], hit = a[d], cov = a[n + d], ng = a[2 * n + d], first = a[3 * n + d];
                uint64_t ones = 0;
                for (uint64_t g = off[d]; g < off[d + 1]; ++g) ones += mask[g];
                if (ng != (L >= k ? L - k + 1 : 0) || hit > ng || cov != ones || (hit == 0) != (first == TK_NG_NONE) || (d < n_add && (hit != ng || cov != (ng ? L : 0))) ||
                    (hit && (cov < k || first + k > L)))
                    return printf("an invariant at %d k %u doc %llu\n", it, k, (unsigned long long)d), 1;
            }
        }
    }
    printf("ngram_sanitize ok\n");
    return 0;
}
