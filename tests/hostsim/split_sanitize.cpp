// The split driver (split_sim.cpp) as a program of its own, for -fsanitize=address,undefined: random batches -- prose with paragraph, line
// and sentence breaks, multi-byte chars cut by tokens, separator-free runs, empty documents -- in heap blocks of exactly their size, every
// K and block shape the simulation test uses.  Checks what holds for every result: C chunks in document order, every chunk within the
// budget, starts ascending, byte ranges that tile a document when there is no overlap.  Host code only.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "split_sim.cpp"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 20) % n);
}
template <class T>
static T* exact(const std::vector<T>& v) {  // a heap block of exactly v.size() entries (at least one byte)
    T* p = (T*)malloc(v.size() * sizeof(T) + (v.empty() ? 1 : 0));
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}
static void sep(tk_split_sep* s, const char* tail, const char* head) {
    s->tail_len = (uint8_t)strlen(tail);
    s->head_len = (uint8_t)strlen(head);
    memcpy(s->tail, tail, s->tail_len);
    memcpy(s->head, head, s->head_len);
}
#define REQUIRE(x)                                                \
    do {                                                          \
        if (!(x)) {                                               \
            printf("split_sanitize: %s fails (case %d)\n", #x, it); \
            return 1;                                             \
        }                                                         \
    } while (0)

int main() {
    const char* words[] = {"a", "the", "chunk", "x", "3.14", "\xC3\xA9", "\xE6\x97\xA5\xE6\x9C\xAC", "\xF0\x9F\x98\x80", "\x80\x80\x80"};
    const uint32_t Ks[] = {64, 128, 4096}, blocks[] = {64, 2048};
    for (int it = 0; it < 60; ++it) {
        const uint64_t n_docs = 1 + rnd(6);
        std::vector<uint8_t> text;
        std::vector<uint64_t> doc_off{0}, tok_off{0}, byte_off{0}, char_off{0};
        std::vector<uint32_t> byte_start, char_start;
        for (uint64_t d = 0; d < n_docs; ++d) {
            const uint32_t kind = rnd(5), n_words = kind == 0 ? 0 : rnd(kind == 4 ? 1500 : 200);
            std::string doc;
            for (uint32_t w = 0; w < n_words; ++w) {
                doc += kind == 3 ? "x" : words[rnd(9)];
                if (kind != 3) {
                    const uint32_t r = rnd(20);
                    doc += r == 0 ? "\n\n" : r < 3 ? "\n" : r < 6 ? ". " : " ";
                }
            }
            uint64_t p = 0, chars = 0;
            while (p < doc.size()) {  // tokens of 1 .. 4 bytes, wherever they fall
                uint64_t n = 1 + rnd(4);
                if (n > doc.size() - p) n = doc.size() - p;
                const bool cont = ((uint8_t)doc[p] & 0xC0) == 0x80;
                byte_start.push_back((uint32_t)p);
                char_start.push_back((uint32_t)(cont && chars ? chars - 1 : chars));
                for (uint64_t i = 0; i < n; ++i) chars += ((uint8_t)doc[p + i] & 0xC0) != 0x80;
                p += n;
            }
            text.insert(text.end(), doc.begin(), doc.end());
            doc_off.push_back(text.size());
            tok_off.push_back(byte_start.size());
            byte_off.push_back(text.size());
            char_off.push_back(char_off.back() + chars);
        }
        const uint64_t T = byte_start.size();
        tk_split_spec spec;
        memset(&spec, 0, sizeof spec);
        spec.min_tokens = 1 + rnd(12);
        spec.max_tokens = spec.min_tokens + 3 + rnd(it % 3 ? 20 : 300);
        spec.overlap = it % 2 ? rnd(spec.min_tokens) : 0;
        spec.n_levels = rnd(5);
        const char* tails[4] = {"\n\n", "\n", ".", ""};
        const char* heads[4] = {"", "", " ", " "};
        for (uint32_t l = 0; l < spec.n_levels; ++l) {
            spec.n_seps[l] = 1;
            sep(&spec.sep[l][0], tails[l], heads[l]);
        }
        spec.seg_tokens = Ks[it % 3];
        uint8_t* x_text = exact(text);
        uint64_t *x_doc = exact(doc_off), *x_tok = exact(tok_off), *x_bo = exact(byte_off), *x_co = exact(char_off);
        uint32_t *x_bs = exact(byte_start), *x_cs = exact(char_start);
        std::vector<uint32_t> blank(T + 1, 0), blank_d(n_docs + 1, 0);
        std::vector<uint8_t> blank8(T + 1, 0);
        uint32_t* o[7];
        for (auto& a : o) a = exact(blank);
        uint8_t* cut = exact(blank8);
        uint32_t* doc_chunk = exact(blank_d);
        uint64_t stats[4];
        const uint32_t block = blocks[it % 2];
        const int64_t C = split_sim(x_text, text.size(), x_doc, x_tok, n_docs, T, x_bs, x_cs, x_bo, x_co, &spec, block, block, o[0], o[1], o[2], o[3], o[4], o[5], o[6], cut,
                                    doc_chunk, stats);
        REQUIRE(C >= 0);
        REQUIRE(doc_chunk[n_docs] == (uint64_t)C && doc_chunk[0] == 0);
        for (uint64_t d = 0; d < n_docs; ++d) {
            const uint64_t n = tok_off[d + 1] - tok_off[d], len = doc_off[d + 1] - doc_off[d];
            REQUIRE(doc_chunk[d] <= doc_chunk[d + 1] && (doc_chunk[d] < doc_chunk[d + 1]) == (n > 0));
            for (uint32_t i = doc_chunk[d]; i < doc_chunk[d + 1]; ++i) {
                const bool first = i == doc_chunk[d], last = i + 1 == doc_chunk[d + 1];
                REQUIRE(o[0][i] == d && o[1][i] < o[2][i] && o[2][i] - o[1][i] <= spec.max_tokens && o[2][i] <= n);
                REQUIRE(first ? o[1][i] == 0 && o[3][i] == 0 : o[1][i] > o[1][i - 1] && o[1][i] <= o[2][i - 1] && o[2][i - 1] - o[1][i] <= spec.overlap);
                REQUIRE(last == (cut[i] == TK_SPLIT_END) && (!last || (o[2][i] == n && o[4][i] == len)));
                if (!spec.overlap && !first) REQUIRE(o[3][i] == o[4][i - 1]);
                REQUIRE(o[3][i] < o[4][i] && o[5][i] <= o[6][i]);
            }
        }
        free(x_text), free(x_doc), free(x_tok), free(x_bo), free(x_co), free(x_bs), free(x_cs), free(cut), free(doc_chunk);
        for (auto& a : o) free(a);
    }
    printf("split_sanitize ok\n");
    return 0;
}
