// Experiment: how many table steps a whole-piece lookup of phase F of tk_k_front takes on the bench corpus, per lookup and per wavefront ROW
// (a row of 64 pieces of one length class runs as long as its slowest lane), for the three whole-piece tables -- short (<= 4 bytes), mid
// (5..8), long-by-identity (9..23) -- under linear probing with one slot per step and under bucket layouts of several widths and sizes.
// Pieces: the first N MiB of the bench corpus (libtkcorpus, seed 0x5EED0003, mix 1), split per document by the C oracle, grouped as phase F
// does: by tile of 3840 bytes, by length class, in rows of 64 in text order.  Host code over the product's headers.
//   g++ -O2 -std=c++17 tools/experiments/probe_lengths.cpp tiktoken_amd/csrc/tk_tables.cpp tiktoken_amd/csrc/tk_pattern.cpp tiktoken_amd/csrc/tk_regex.cpp -ldl -pthread -o probe_lengths
//   ./probe_lengths VOCAB.tiktoken [MiB = 64] [libtkcorpus.so] [libtk_oracle.so] > profiles/probe_lengths.txt
#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../tiktoken_amd/csrc/tk_tables.h"

namespace {
struct Key {
    uint64_t w0, w1, w2;
    bool operator==(const Key& o) const { return w0 == o.w0 && w1 == o.w1 && w2 == o.w2; }
};
enum { SHORT = 0, MID = 1, XL = 2 };
const char* const kName[3] = {"short (<= 4 B, 8-byte slots)", "mid (5..8 B, 16-byte slots)", "long by identity (9..23 B, 32-byte slots)"};
const uint32_t kSlotBytes[3] = {8, 16, 32};

Key key_of(const uint8_t* p, uint32_t len) {
    Key k{0, 0, 0};
    if (len <= 8) {
        memcpy(&k.w0, p, len);
        k.w1 = len;
        return k;
    }
    tk_ident([&](uint32_t at) {
        uint64_t w = 0;
        memcpy(&w, p + at, at < len ? std::min<uint32_t>(8u, len - at) : 0u);
        return w;
    }, len, 0u, k.w0, k.w1, k.w2);
    return k;
}
// the slot of a key in a table of 2^bits slots, by the product's hash of that table
uint32_t slot_of(int cls, const Key& k, uint32_t bits) {
    if (cls == SHORT) return tk_short_slot((uint32_t)k.w0, 32 - bits);
    if (cls == MID) return tk_mid_slot(k.w0, 32 - bits);
    return (uint32_t)tk_ident_hash(k.w0, k.w1, k.w2, true) & ((1u << bits) - 1u);
}

// open addressing over buckets of W slots (W = 1: linear probing as it was): a key lives in the first bucket of its sequence that had room
struct Layout {
    int cls;
    uint32_t W, bits;  // slots per bucket, log2 of the slots
    bool flag;         // a full bucket that no key was ever carried past ends a search as well (one "passed" bit per bucket)
    std::vector<uint8_t> passed;
    std::vector<int32_t> slot;  // index into keys, -1 = free
    const std::vector<Key>* keys;
    uint32_t base(const Key& k) const { return slot_of(cls, k, bits) & ~(W - 1u); }
    void build(const std::vector<Key>& ks) {
        keys = &ks;
        slot.assign((size_t)1 << bits, -1);
        passed.assign((size_t)1 << bits, 0);
        for (size_t i = 0; i < ks.size(); ++i) {
            uint32_t b = base(ks[i]);
            for (;; b = (b + W) & (((uint32_t)1 << bits) - 1u)) {
                uint32_t j = 0;
                while (j < W && slot[b + j] >= 0) ++j;
                if (j < W) {
                    slot[b + j] = (int32_t)i;
                    break;
                }
                passed[b] = 1;
            }
        }
    }
    // steps (buckets fetched) of a lookup; *hit = found
    uint32_t steps(const Key& k, bool* hit) const {
        uint32_t b = base(k), n = 1;
        for (;; b = (b + W) & (((uint32_t)1 << bits) - 1u), ++n) {
            for (uint32_t j = 0; j < W; ++j) {
                if (slot[b + j] < 0) return *hit = false, n;
                if ((*keys)[(size_t)slot[b + j]] == k) return *hit = true, n;
            }
            if (flag && !passed[b]) return *hit = false, n;
        }
    }
};
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return fprintf(stderr, "usage: %s VOCAB.tiktoken [MiB] [libtkcorpus.so] [libtk_oracle.so]\n", argv[0]), 2;
    const uint64_t n = (uint64_t)(argc > 2 ? atoll(argv[2]) : 64) << 20;
    void* lc = dlopen(argc > 3 ? argv[3] : "tiktoken_amd/csrc/libtkcorpus.so", RTLD_NOW);
    void* lo = dlopen(argc > 4 ? argv[4] : "oracle/libtk_oracle.so", RTLD_NOW);
    if (!lc || !lo) return fprintf(stderr, "dlopen: %s\n", dlerror()), 2;
    auto gen = (int (*)(uint64_t, int, uint64_t, void*, void*, uint64_t, void*, int))dlsym(lc, "tkc_generate");
    auto split = (int64_t (*)(int, const uint8_t*, uint64_t, uint64_t*, uint64_t))dlsym(lo, "tko_split");
    if (!gen || !split) return fprintf(stderr, "dlsym failed\n"), 2;

    // the vocabulary and the tables as shipped
    std::vector<uint8_t> file;
    {
        FILE* f = fopen(argv[1], "rb");
        if (!f) return perror(argv[1]), 2;
        uint8_t buf[65536];
        for (size_t r; (r = fread(buf, 1, sizeof buf, f)) > 0;) file.insert(file.end(), buf, buf + r);
        fclose(f);
    }
    std::vector<uint8_t> blob;
    std::vector<uint64_t> off;
    std::vector<uint32_t> ids;
    std::string err = tk_parse_tiktoken(file.data(), file.size(), &blob, &off, &ids);
    if (!err.empty()) return fprintf(stderr, "%s\n", err.c_str()), 2;
    const char* pat = "[^\\r\\n\\p{L}\\p{N}]?[\\p{Lu}\\p{Lt}\\p{Lm}\\p{Lo}\\p{M}]*[\\p{Ll}\\p{Lm}\\p{Lo}\\p{M}]+(?i:'s|'t|'re|'ve|'m|'ll|'d)?|[^\\r\\n\\p{L}\\p{N}]?[\\p{Lu}\\p{Lt}\\p{Lm}\\p{Lo}\\p{M}]+[\\p{Ll}\\p{Lm}\\p{Lo}\\p{M}]*(?i:'s|'t|'re|'ve|'m|'ll|'d)?|\\p{N}{1,3}| ?[^\\s\\p{L}\\p{N}]+[\\r\\n/]*|\\s*[\\r\\n]+|\\s+(?!\\S)|\\s+";
    TkHostTables H;
    const uint64_t soff[1] = {0};
    err = tk_build_tables(blob.data(), off.data(), ids.data(), ids.size(), nullptr, soff, nullptr, 0, pat, &H);
    if (!err.empty()) return fprintf(stderr, "tk_build_tables: %s\n", err.c_str()), 2;
    std::vector<Key> keys[3];
    for (size_t k = 0; k < ids.size(); ++k) {
        const uint32_t len = (uint32_t)(off[k + 1] - off[k]);
        if (len > TK_XL_MAX) continue;
        keys[len <= 4 ? SHORT : (len <= 8 ? MID : XL)].push_back(key_of(blob.data() + off[k], len));
    }
    printf("vocabulary: %zu tokens; short %zu, mid %zu, long-by-identity %zu\n", ids.size(), keys[0].size(), keys[1].size(), keys[2].size());
    printf("tables as built by tk_build_tables: short %zu slots (%zu KiB, load %.3f), mid %zu slots (%zu KiB, load %.3f), long-by-identity %zu slots (%zu KiB, load %.3f)\n",
           H.short_tab.size(), H.short_tab.size() * 8 >> 10, (double)keys[0].size() / H.short_tab.size(), H.mid_tab.size(), H.mid_tab.size() * 16 >> 10,
           (double)keys[1].size() / H.mid_tab.size(), H.xl.size(), H.xl.size() * 32 >> 10, (double)keys[2].size() / H.xl.size());
    const uint32_t bits0[3] = {(uint32_t)__builtin_ctzll(H.short_tab.size()), (uint32_t)__builtin_ctzll(H.mid_tab.size()), (uint32_t)__builtin_ctzll(H.xl.size())};

    // the corpus and its pieces, by tile and class
    std::vector<uint8_t> text(n + 128, 0);
    std::vector<uint64_t> doff(n / 64 + 4);
    uint64_t nd = 0;
    if (gen(0x5EED0003ull, 1, n, text.data(), doff.data(), n / 64 + 2, &nd, 8) != 0) return fprintf(stderr, "tkc_generate failed\n"), 2;
    const uint64_t TILE = 3840;
    std::vector<Key> lk[3];            // the lookups, in the order phase F makes them
    std::vector<uint32_t> row_end[3];  // index behind the last lookup of every row
    uint64_t pieces = 0, longer = 0;
    {
        std::vector<uint64_t> ends;
        std::vector<std::pair<uint64_t, uint32_t>> pc;  // (start, length) of every piece
        for (uint64_t d = 0; d < nd; ++d) {
            const uint64_t a = doff[d], len = doff[d + 1] - a;
            ends.resize(len + 1);
            const int64_t np = split(2, text.data() + a, len, ends.data(), ends.size());
            if (np < 0) return fprintf(stderr, "tko_split failed\n"), 2;
            uint64_t s = 0;
            for (int64_t i = 0; i < np; ++i) {
                pc.push_back({a + s, (uint32_t)(ends[i] - s)});
                s = ends[i];
            }
        }
        pieces = pc.size();
        size_t i = 0;
        for (uint64_t t0 = 0; t0 < n; t0 += TILE) {
            size_t first[3] = {lk[0].size(), lk[1].size(), lk[2].size()};
            for (; i < pc.size() && pc[i].first < t0 + TILE; ++i) {
                const uint32_t len = pc[i].second;
                if (len > TK_XL_MAX) {
                    ++longer;
                    continue;
                }
                lk[len <= 4 ? SHORT : (len <= 8 ? MID : XL)].push_back(key_of(text.data() + pc[i].first, len));
            }
            for (int c = 0; c < 3; ++c)
                for (size_t q = first[c]; q < lk[c].size(); q += 64) row_end[c].push_back((uint32_t)std::min(q + 64, lk[c].size()));
        }
    }
    printf("corpus: %llu MiB, %llu documents, %llu pieces (%llu of more than %u bytes, never looked up by phase F's rows)\n\n", (unsigned long long)(n >> 20),
           (unsigned long long)nd, (unsigned long long)pieces, (unsigned long long)longer, TK_XL_MAX);

    for (int c = 0; c < 3; ++c) {
        printf("== %s: %zu keys, %zu lookups in %zu rows\n", kName[c], keys[c].size(), lk[c].size(), row_end[c].size());
        printf("   %-34s %6s %8s | %9s %9s %11s | %8s  %s\n", "layout", "load", "KiB", "steps/hit", "steps/miss", "first step", "row max", "rows by their maximum: 1 2 3 4 5+ (%)");
        struct Cand {
            uint32_t W;
            int dbits;
            bool flag;
        };
        double misspct = 0;
        const Cand cands[] = {{1, 0, false}, {2, 0, false}, {4, 0, false}, {8, 0, false}, {2, 0, true}, {4, 0, true}, {1, 1, false}, {2, 1, false}, {4, 1, false}, {8, 1, false}};
        for (const Cand& cd : cands) {
            if (cd.W * kSlotBytes[c] > 128) continue;
            Layout L{c, cd.W, bits0[c] + (uint32_t)cd.dbits, cd.flag, {}, {}, nullptr};
            L.build(keys[c]);
            uint64_t sh = 0, nh = 0, sm = 0, nm = 0, first = 0, rowsum = 0, hist[5] = {0, 0, 0, 0, 0};
            size_t q = 0;
            for (uint32_t re : row_end[c]) {
                uint32_t mx = 0;
                for (; q < re; ++q) {
                    bool hit;
                    const uint32_t s = L.steps(lk[c][q], &hit);
                    (hit ? sh : sm) += s;
                    (hit ? nh : nm) += 1;
                    first += s == 1;
                    mx = std::max(mx, s);
                }
                rowsum += mx;
                hist[std::min(mx, 5u) - 1]++;
            }
            char name[64];
            snprintf(name, sizeof name, "%s %u slot%s / %u B%s", cd.W == 1 ? "linear," : "bucket,", cd.W, cd.W == 1 ? "" : "s", cd.W * kSlotBytes[c], cd.dbits ? ", 2x" : (cd.flag ? ", +bit" : ""));
            const double R = (double)row_end[c].size();
            misspct = 100.0 * (double)nm / (double)(nh + nm);
            printf("   %-34s %6.3f %8zu | %9.3f %9.3f %10.2f%% | %8.3f  %5.1f %5.1f %5.1f %5.1f %5.1f\n", name, (double)keys[c].size() / (double)L.slot.size(),
                   (L.slot.size() * kSlotBytes[c]) >> 10, nh ? (double)sh / nh : 0.0, nm ? (double)sm / nm : 0.0, 100.0 * first / (double)(nh + nm), rowsum / R,
                   100 * hist[0] / R, 100 * hist[1] / R, 100 * hist[2] / R, 100 * hist[3] / R, 100 * hist[4] / R);
        }
        printf("   (misses: %.1f %% of the lookups)\n\n", misspct);
    }
    return 0;
}
