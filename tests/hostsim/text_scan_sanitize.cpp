// The driver of the words' and the cleaning's scan elements (text_scan_sim.cpp) as a program of its own, for
// -fsanitize=address,undefined: seeded random batches over a small alphabet -- space, '\n', '.', 'a', 'A', a continuation byte, C3, A9,
// U+2028 -- with random document boundaries, empty documents among them, in heap blocks of exactly their size, at five geometries: the
// runs must be clean and give the same values whatever the grouping.  Host code only.
#include <stdio.h>

#include <memory>
#include <random>

#include "text_scan_sim.cpp"

using V = std::vector<uint64_t>;
static const uint32_t GEOMETRY[5][3] = {{256, 1, 64}, {4, 1, 4}, {4, 2, 4}, {1, 3, 2}, {16, 3, 4}};

int main() {
    std::mt19937_64 rng(0x7C5A);
    std::unique_ptr<uint8_t[]> letters(new uint8_t[0x110000 / 8]());
    for (uint32_t cp = 0; cp < 0x100; ++cp)
        if ((cp | 0x20u) - 'a' < 26u || (cp >= 0xC0u && cp != 0xD7u && cp != 0xF7u)) letters[cp >> 3] |= (uint8_t)(1u << (cp & 7u));
    const char* unit[] = {" ", "\n", ".", "a", "A", "\x96", "\xC3", "\xA9", "\xE2\x80\xA8"};
    const char stop[] = "aaAa.a";
    const uint64_t stop_off[] = {0, 1, 3, 6}, phrase_off[] = {0, 3, 5};
    const uint8_t terminal[] = {'.', 'a'}, phrases[] = {'a', ' ', 'A', '.', '.'};
    for (int it = 0; it < 60; ++it) {
        std::vector<uint8_t> bytes;
        const uint64_t n_units = it % 6 == 0 ? rng() % 4 : rng() % 1500, n_docs = rng() % 12;
        for (uint64_t i = 0; i < n_units; ++i) {
            const uint64_t u = (rng() % 4 == 0) ? 3 : rng() % 9;
            for (const char* c = unit[u]; *c; ++c) bytes.push_back((uint8_t)*c);
        }
        const uint64_t N = n_docs ? bytes.size() : 0;  // (no document: no byte)
        std::unique_ptr<uint8_t[]> text(new uint8_t[N]);
        std::copy(bytes.begin(), bytes.begin() + N, text.get());
        std::unique_ptr<uint64_t[]> off(new uint64_t[n_docs + 1]);
        for (uint64_t d = 0; d <= n_docs; ++d) off[d] = d == 0 ? 0 : d == n_docs ? N : rng() % 3 == 0 ? off[d - 1] : rng() % (N + 1);
        std::sort(off.get(), off.get() + n_docs + 1);
        V first_w, first_c;
        for (int g = 0; g < 5; ++g) {
            const uint32_t L = GEOMETRY[g][0], P = GEOMETRY[g][1], W = GEOMETRY[g][2];
            V w(5 * n_docs + 1, 7), c(6 * n_docs + N + 2, 7);
            w[5 * n_docs] = (uint64_t)text_scan_sim_words(text.get(), off.get(), n_docs, (const uint8_t*)stop, stop_off, 3, letters.get(), L, P, W, w.data());
            const int64_t n = text_scan_sim_clean(text.get(), off.get(), n_docs, 1 + it % 4, it % 3 ? 3 : 0, it % 2, terminal, it % 5 ? 2 : 0, phrases, phrase_off, 2, L, P, W, c.data(),
                                                  c.data() + 6 * n_docs, N + 1);
            if (w[5 * n_docs] != 0 || n < 0) return printf("a status at batch %d geometry %d: %lld %lld\n", it, g, (long long)w[5 * n_docs], (long long)n), 1;
            c.resize(6 * n_docs + (uint64_t)n);
            if (g == 0) first_w = w, first_c = c;
            if (w != first_w || c != first_c) return printf("the grouping changes the result at batch %d geometry %d\n", it, g), 1;
        }
    }
    printf("text_scan_sanitize ok\n");
    return 0;
}
