// The builder of the bucketed tables and their three probes (tk_common.h, "bucketed tables") under AddressSanitizer / UBSan, as a program
// of its own (tests/test_probe_buckets_sim.py builds and runs it; nothing of it is loaded into Python).  Every table is copied into a
// heap block of exactly its size, so that a bucket fetched beyond the last one -- the wrap-around -- ends the run here.
// Reads a case file: u64 {n_tokens, blob bytes, n_keys, keys bytes}, token offsets (n + 1 u64), ids (n u32), the blob, key offsets
// (n_keys + 1 u64), expected ranks (n_keys u32), the keys' bytes.  Prints
//   ok <keys> short <slots> <most keys with one home bucket> <probed keys whose home is the last bucket> mid ... xl ...
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <vector>

#include "../../tiktoken_amd/csrc/tk_tables.h"

template <class T>
static std::vector<T> rd(FILE* f, uint64_t count) {
    std::vector<T> v(count);
    if (count && fread(v.data(), sizeof(T), count, f) != count) {
        fprintf(stderr, "case file is short\n");
        exit(2);
    }
    return v;
}
template <class T>
static T* exact(const std::vector<T>& v) {  // a heap block of exactly the table's bytes
    T* p = (T*)malloc(v.size() ? v.size() * sizeof(T) : 1);
    if (!v.empty()) memcpy((void*)p, (const void*)v.data(), v.size() * sizeof(T));
    return p;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    const std::vector<uint64_t> h = rd<uint64_t>(f, 4);
    const std::vector<uint64_t> off = rd<uint64_t>(f, h[0] + 1);
    const std::vector<uint32_t> ids = rd<uint32_t>(f, h[0]);
    const std::vector<uint8_t> blob = rd<uint8_t>(f, h[1]);
    const std::vector<uint64_t> koff = rd<uint64_t>(f, h[2] + 1);
    const std::vector<uint32_t> want = rd<uint32_t>(f, h[2]);
    const std::vector<uint8_t> keys = rd<uint8_t>(f, h[3]);
    fclose(f);
    TkHostTables H;
    const uint64_t soff[1] = {0};
    const std::string err = tk_build_tables(blob.data(), off.data(), ids.data(), h[0], nullptr, soff, nullptr, 0, argv[2], &H);
    if (!err.empty()) return fprintf(stderr, "tk_build_tables: %s\n", err.c_str()), 1;
    TkShortSlot* st = exact(H.short_tab);
    TkPieceSlot* mt = exact(H.mid_tab);
    TkXlSlot* xt = exact(H.xl);
    const uint32_t slots[3] = {(uint32_t)H.short_tab.size(), (uint32_t)H.mid_tab.size(), (uint32_t)H.xl.size()};
    const uint32_t bw[3] = {TK_SHORT_BW, TK_MID_BW, TK_XL_BW};
    std::map<uint32_t, uint32_t> homes[3];  // tokens per home bucket
    uint32_t at_last[3] = {0, 0, 0};
    // class and hash slot of a byte string, as the callers of the probes compute them
    auto home = [&](const uint8_t* p, uint32_t len, int* cls, uint64_t* w) {
        if (len <= 8) {
            uint64_t key = 0;
            memcpy(&key, p, len);
            w[0] = key;
            *cls = len <= 4 && !H.short_tab.empty() ? 0 : 1;
            return *cls == 0 ? tk_short_slot((uint32_t)key, H.short_shift) : tk_mid_slot(key, H.mid_shift);
        }
        tk_ident([&](uint32_t at) {
            uint64_t x = 0;
            memcpy(&x, p + at, at < len ? std::min<uint32_t>(8u, len - at) : 0u);
            return x;
        }, len, 0u, w[0], w[1], w[2]);
        *cls = 2;
        return (uint32_t)tk_ident_hash(w[0], w[1], w[2], true) & H.xl_mask;
    };
    for (uint64_t k = 0; k < h[0]; ++k) {
        const uint32_t len = (uint32_t)(off[k + 1] - off[k]);
        if (len > TK_XL_MAX) continue;
        int cls;
        uint64_t w[3];
        const uint32_t s = home(blob.data() + off[k], len, &cls, w);
        homes[cls][s / bw[cls]]++;
    }
    for (uint64_t k = 0; k < h[2]; ++k) {
        const uint8_t* p = keys.data() + koff[k];
        const uint32_t len = (uint32_t)(koff[k + 1] - koff[k]);
        if (len == 0 || len > TK_XL_MAX) return fprintf(stderr, "key %llu: length %u\n", (unsigned long long)k, len), 2;
        int cls;
        uint64_t w[3];
        const uint32_t s = home(p, len, &cls, w);
        at_last[cls] += s / bw[cls] == slots[cls] / bw[cls] - 1u;
        const uint32_t got = cls == 0   ? tk_bucket_probe_short(st, H.short_mask, s, (uint32_t)w[0], len)
                             : cls == 1 ? tk_bucket_probe_mid(mt, H.mid_mask, s, w[0], len)
                                        : tk_bucket_probe_xl(xt, H.xl_mask, s, w[0], w[1], w[2]);
        if (got != want[k] || H.lookup_piece(p, len) != want[k]) return fprintf(stderr, "key %llu: %u, expected %u\n", (unsigned long long)k, got, want[k]), 1;
    }
    printf("ok %llu", (unsigned long long)h[2]);
    const char* names[3] = {"short", "mid", "xl"};
    for (int c = 0; c < 3; ++c) {
        uint32_t most = 0;
        for (const auto& kv : homes[c]) most = std::max(most, kv.second);
        printf(" %s %u %u %u", names[c], slots[c], most, at_last[c]);
    }
    printf("\n");
    free(st), free(mt), free(xt);
    return 0;
}
