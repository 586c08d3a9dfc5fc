// The training passes of tiktoken_amd/csrc/tk_train.h on the CPU: the plain C++ they are made of (tk_train_rule.h), driven the way the
// kernels drive it -- a lane per piece for the word table, a lane per symbol in workgroups of `block` for the step, with the workgroup
// reductions, the carry across workgroups and the scans done where the kernels do them.  Built twice by tests/test_train_sim.py: as a
// shared library, and (-DTRAIN_SIM_MAIN) as a program of its own under the address and undefined-behaviour sanitizers, which reads a case
// file and writes the results.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../tiktoken_amd/csrc/tk_train_rule.h"

namespace {
struct PlainCas {  // (one lane at a time: the claim order is the lane order)
    unsigned long long operator()(unsigned long long* p, unsigned long long expect, unsigned long long want) const {
        const unsigned long long old = *p;
        if (old == expect) *p = want;
        return old;
    }
};

struct Tab {
    std::vector<unsigned long long> key, weight, first;
    uint64_t mask;
    explicit Tab(uint64_t slots) : key(slots, 0ull), weight(slots, 0ull), first(slots, ~0ull), mask(slots - 1) {}
};
}  // namespace

// Words: blob[off[w] .. off[w + 1]) with weight[w] occurrences, the first one at corpus offset first[w]; the same bytes may come twice
// (they are one word).  The list goes into the table as two chunks -- the second one meets keys that name the blob -- and, with
// flags & 1, the table is moved into a fresh one of the same size before the symbols are laid out.  The device lays the words of a chunk
// out in the order in which its atomics land, i.e. in any order; here it is the order of the slots or, with flags & 2, the order of
// the text, so that a test can put a word where it wants it.  slots: a power of two.
// Returns 0, 1 (no pair left: *n_done merges were made), 2 (a probe found no slot), -1 (an index out of range: a bug).
extern "C" int64_t train_sim(const uint8_t* blob_in, const uint64_t* off, const uint64_t* weight, const uint64_t* first, uint64_t n_words, uint64_t slots,
                             uint64_t seed, uint32_t block, uint32_t n_merges, int flags, uint32_t* pairs_out, uint64_t* counts_out, uint64_t* n_done,
                             uint32_t* sym_out, uint64_t* pos_out, uint64_t cap, uint64_t* n_sym_out) {
    *n_done = 0;
    *n_sym_out = 0;
    if (!slots || (slots & (slots - 1)) || !block) return -1;
    Tab tab(slots);
    std::vector<uint8_t> blob;
    const uint64_t half = n_words / 2;
    for (int chunk = 0; chunk < 2; ++chunk) {
        const uint64_t w0 = chunk ? half : 0, w1 = chunk ? n_words : half;
        const uint64_t base = off[w0];
        const uint8_t* text = blob_in + base;  // the chunk's text: its words back to back
        for (uint64_t w = w0; w < w1; ++w) {   // tk_k_train_words, a lane per piece
            const uint32_t s = (uint32_t)(off[w] - base), len = (uint32_t)(off[w + 1] - off[w]);
            if (!len) continue;
            const uint8_t* mine = text + s;
            const uint64_t h = tk_train_hash([&](uint32_t j) { return mine[j]; }, len, seed);
            const uint64_t slot = tk_train_word_slot(tab.key.data(), tab.mask, h, tk_train_text_ref(s, len), mine, len, text, blob.data(), PlainCas());
            if (slot == ~0ull) return 2;
            tab.weight[slot] += weight[w];
            tab.first[slot] = std::min<unsigned long long>(tab.first[slot], first[w]);
        }
        std::vector<uint64_t> fresh;  // tk_k_train_blob: the slots claimed in this chunk, in slot order or (flags & 2) in the order of the text
        for (uint64_t s = 0; s < slots; ++s)
            if (tab.key[s] && !(tab.key[s] & TK_TRAIN_IN_BLOB)) fresh.push_back(s);
        if (flags & 2) std::sort(fresh.begin(), fresh.end(), [&](uint64_t x, uint64_t y) { return (uint32_t)tab.key[x] < (uint32_t)tab.key[y]; });
        for (const uint64_t s : fresh) {
            const unsigned long long k = tab.key[s];
            const uint32_t len = tk_train_ref_len(k);
            const uint8_t* src = tk_train_ref_bytes(k, text, blob.data());
            const uint64_t at = blob.size();
            blob.insert(blob.end(), src, src + len);
            tab.key[s] = tk_train_blob_ref((uint32_t)at, len);
        }
    }
    if (flags & 1) {  // tk_k_train_rehash
        Tab to(slots);
        for (uint64_t s = 0; s < slots; ++s) {
            const unsigned long long k = tab.key[s];
            if (!k) continue;
            const uint8_t* w = tk_train_ref_bytes(k, nullptr, blob.data());
            const uint64_t h = tk_train_hash([&](uint32_t j) { return w[j]; }, tk_train_ref_len(k), seed);
            const uint64_t d = tk_train_word_place(to.key.data(), to.mask, h, k, PlainCas());
            if (d == ~0ull) return 2;
            to.weight[d] = tab.weight[s];
            to.first[d] = tab.first[s];
        }
        tab = std::move(to);
    }
    // tk_k_train_expand
    const uint64_t N = blob.size();
    std::vector<uint32_t> sym[2], wid[2];
    std::vector<unsigned long long> pos[2];
    for (int p = 0; p < 2; ++p) {
        sym[p].assign(N, 0xDEADBEEFu);
        wid[p].assign(N, 0xDEADBEEFu);
        pos[p].assign(N, ~0ull);
    }
    for (uint64_t s = 0; s < slots; ++s) {
        const unsigned long long k = tab.key[s];
        if (!(k & TK_TRAIN_IN_BLOB)) continue;
        const uint32_t len = tk_train_ref_len(k), o = (uint32_t)k;
        if ((uint64_t)o + len > N) return -1;
        for (uint32_t j = 0; j < len; ++j) {
            sym[0][o + j] = blob[o + j];
            wid[0][o + j] = (uint32_t)s;
            pos[0][o + j] = tk_train_pos(tab.first[s], j);
        }
    }
    uint64_t pair_slots = 16;
    while (pair_slots < 2 * N) pair_slots <<= 1;
    std::vector<TkTrainPair> pair(pair_slots);
    const uint64_t pmask = pair_slots - 1;
    const uint64_t nb0 = (N + block - 1) / block;
    std::vector<uint32_t> blk_mark(nb0 + 1, 0u);
    std::vector<unsigned long long> blk_cnt(nb0 + 1, 0ull);
    std::vector<uint8_t> dec(N + 1, 0xEE);
    uint64_t live[2] = {N, 0};
    int rc = 0;
    uint32_t par = 0;
    for (uint32_t step = 0; step < n_merges; ++step, par ^= 1u) {
        const uint64_t n = live[par], nb = (n + block - 1) / block;
        const std::vector<uint32_t>&S = sym[par], &W = wid[par];
        const std::vector<unsigned long long>& P = pos[par];
        std::fill(pair.begin(), pair.end(), TkTrainPair{0ull, 0ull});
        unsigned long long cmax = 0, best = ~0ull;
        for (uint64_t i = 0; i + 1 < n; ++i) {  // tk_k_train_count
            if (W[i] != W[i + 1]) continue;
            const uint64_t s = tk_train_pair_slot(pair.data(), pmask, tk_train_pair_key(S[i], S[i + 1]), PlainCas());
            if (s == ~0ull) return 2;
            pair[s].cnt += tab.weight[W[i]];
            cmax = std::max(cmax, pair[s].cnt);  // (the largest sum any add produces)
        }
        if (!cmax) {  // tk_k_train_pick: no pair left
            rc = 1;
            break;
        }
        for (uint64_t i = 0; i + 1 < n; ++i) {  // tk_k_train_best
            if (W[i] != W[i + 1]) continue;
            const uint64_t s = tk_train_pair_find(pair.data(), pmask, tk_train_pair_key(S[i], S[i + 1]));
            if (s == ~0ull) return -1;
            if (pair[s].cnt == cmax) best = std::min(best, P[i]);
        }
        uint32_t a = 0, b = 0, found = 0;
        for (uint64_t i = 0; i + 1 < n; ++i)  // tk_k_train_pick
            if (P[i] == best) {
                a = S[i];
                b = S[i + 1];
                ++found;
            }
        if (found != 1) return -1;
        pairs_out[2 * step] = a;
        pairs_out[2 * step + 1] = b;
        counts_out[step] = cmax;
        auto prev_of = [&](uint64_t i, uint32_t* sp) {
            const bool has = i > 0 && W[i - 1] == W[i];
            *sp = has ? S[i - 1] : 0u;
            return has;
        };
        if (a == b) {
            for (uint64_t g = 0; g < nb; ++g) {  // tk_k_train_breaks: the largest mark of every workgroup
                uint32_t m = 0;
                for (uint64_t i = g * block; i < std::min<uint64_t>(n, (g + 1) * block); ++i) {
                    uint32_t sp;
                    const bool hp = prev_of(i, &sp);
                    m = std::max(m, tk_train_break_mark((uint32_t)i, tk_train_continues(hp, sp, S[i], a)));
                }
                blk_mark[g] = m;
            }
            uint32_t carry = 0;
            for (uint64_t g = 0; g < nb; ++g) {  // tk_k_train_carry: in place, the largest mark before every workgroup
                const uint32_t m = blk_mark[g];
                blk_mark[g] = carry;
                carry = std::max(carry, m);
            }
        }
        for (uint64_t g = 0; g < nb; ++g) {  // tk_k_train_decide
            uint32_t run = a == b ? blk_mark[g] : 0u;  // the largest mark at or before the lane: the carry, then the workgroup's own scan
            unsigned long long kept = 0;
            for (uint64_t i = g * block; i < std::min<uint64_t>(n, (g + 1) * block); ++i) {
                uint32_t sp;
                const bool hp = prev_of(i, &sp);
                const bool hn = i + 1 < n && W[i + 1] == W[i];
                const uint32_t sn = hn ? S[i + 1] : 0u;
                uint32_t d = 0;
                if (a == b) {
                    run = std::max(run, tk_train_break_mark((uint32_t)i, tk_train_continues(hp, sp, S[i], a)));
                    if (!run) return -1;
                    d = (uint32_t)i - (run - 1u);
                }
                dec[i] = (uint8_t)tk_train_decide(a, b, hp, sp, S[i], hn, sn, d);
                kept += dec[i] != TK_TRAIN_RIGHT;
            }
            blk_cnt[g] = kept;
        }
        unsigned long long total = 0;
        for (uint64_t g = 0; g < nb; ++g) {  // tk_k_train_offsets
            const unsigned long long c = blk_cnt[g];
            blk_cnt[g] = total;
            total += c;
        }
        live[par ^ 1u] = total;
        for (uint64_t g = 0; g < nb; ++g) {  // tk_k_train_rewrite
            uint64_t at = blk_cnt[g];
            for (uint64_t i = g * block; i < std::min<uint64_t>(n, (g + 1) * block); ++i) {
                if (dec[i] == TK_TRAIN_RIGHT) continue;
                if (at >= N) return -1;
                sym[par ^ 1u][at] = dec[i] == TK_TRAIN_LEFT ? 256u + step : S[i];
                wid[par ^ 1u][at] = W[i];
                pos[par ^ 1u][at] = P[i];
                ++at;
            }
        }
        *n_done = step + 1;
    }
    const uint64_t n = live[par];
    if (n > cap) return -1;
    for (uint64_t i = 0; i < n; ++i) {
        sym_out[i] = sym[par][i];
        pos_out[i] = pos[par][i];
    }
    *n_sym_out = n;
    return rc;
}

// tk_train_hash of a word: where its probe chain starts (tests/test_train_shapes.py shows that its words share one)
extern "C" uint64_t train_sim_hash(const uint8_t* word, uint32_t len, uint64_t seed) {
    return tk_train_hash([&](uint32_t j) { return word[j]; }, len, seed);
}

#ifdef TRAIN_SIM_MAIN
// Case file: per case nine uint64 {n_words, slots, seed, block, n_merges, flags, blob bytes, 0, 0}, off[n_words + 1], weight[n_words],
// first[n_words], the blob.  Result file: per case {rc, n_done, n_sym} (int64 / uint64), pairs[2 * n_merges] uint32, counts[n_merges],
// sym[n_sym] uint32, pos[n_sym].
template <class T>
static bool get(FILE* f, std::vector<T>& v, uint64_t n) {
    v.resize(n);
    return !n || fread(v.data(), sizeof(T), n, f) == n;
}
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint64_t head[9];
    int n_cases = 0;
    while (fread(head, 8, 9, in) == 9) {
        std::vector<uint64_t> off, weight, first;
        std::vector<uint8_t> blob;
        if (!get(in, off, head[0] + 1) || !get(in, weight, head[0]) || !get(in, first, head[0]) || !get(in, blob, head[6])) return 3;
        const uint32_t n_merges = (uint32_t)head[4];
        std::vector<uint32_t> pairs(2 * (uint64_t)n_merges + 1, 0u), sym(blob.size() + 1);
        std::vector<uint64_t> counts((uint64_t)n_merges + 1, 0ull), pos(blob.size() + 1);
        uint64_t n_done = 0, n_sym = 0;
        const int64_t rc = train_sim(blob.data(), off.data(), weight.data(), first.data(), head[0], head[1], head[2], (uint32_t)head[3], n_merges, (int)head[5],
                                     pairs.data(), counts.data(), &n_done, sym.data(), pos.data(), blob.size(), &n_sym);
        const uint64_t res[3] = {(uint64_t)rc, n_done, n_sym};
        fwrite(res, 8, 3, out);
        fwrite(pairs.data(), 4, 2 * (size_t)n_merges, out);
        fwrite(counts.data(), 8, n_merges, out);
        fwrite(sym.data(), 4, n_sym, out);
        fwrite(pos.data(), 8, n_sym, out);
        ++n_cases;
    }
    fclose(in);
    fclose(out);
    printf("%d cases\n", n_cases);
    return 0;
}
#endif
