// The bucketed whole-piece tables (tk_common.h, "bucketed tables") for tests/test_probe_buckets_sim.py, as a shared library over
// tk_tables.cpp: the builder, the three probes, where a key's sequence starts, a digest of every word a probe depends on, and the check
// of a whole vocabulary -- every token found, every neighbour that is not a token absent -- in one call (two million lookups for the
// o200k-shaped vocabulary: too many for a Python loop).  "Is it a token" is answered by a std::unordered_set of the token strings, which
// shares nothing with the tables.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../tiktoken_amd/csrc/tk_tables.h"

namespace {
struct Sim {
    TkHostTables H;
    std::vector<uint8_t> blob;
    std::vector<uint64_t> off;
    std::vector<uint32_t> ids;
};
// class (0 short, 1 mid, 2 by identity), hash slot and probe words of a byte string of 1..TK_XL_MAX bytes, as the probes' callers compute them
uint32_t home_of(const TkHostTables& H, const uint8_t* p, uint32_t len, int* cls, uint64_t* w) {
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
}
const uint32_t kBw[3] = {TK_SHORT_BW, TK_MID_BW, TK_XL_BW};
// the rank of a byte string by the bucket probe of its class
uint32_t probe(const TkHostTables& H, const uint8_t* p, uint32_t len) {
    int cls;
    uint64_t w[3];
    const uint32_t s = home_of(H, p, len, &cls, w);
    if (cls == 0) return tk_bucket_probe_short(H.short_tab.data(), H.short_mask, s, (uint32_t)w[0], len);
    if (cls == 1) return tk_bucket_probe_mid(H.mid_tab.data(), H.mid_mask, s, w[0], len);
    return tk_bucket_probe_xl(H.xl.data(), H.xl_mask, s, w[0], w[1], w[2]);
}
}  // namespace

extern "C" {
void* pbs_create(const uint8_t* blob, const uint64_t* off, const uint32_t* ids, uint64_t n, const char* pat, char* err, uint64_t errcap) {
    Sim* s = new Sim;
    s->blob.assign(blob, blob + off[n]);
    s->off.assign(off, off + n + 1);
    s->ids.assign(ids, ids + n);
    const uint64_t soff[1] = {0};
    const std::string e = tk_build_tables(s->blob.data(), s->off.data(), s->ids.data(), n, nullptr, soff, nullptr, 0, pat, &s->H);
    if (!e.empty()) {
        snprintf(err, errcap, "%s", e.c_str());
        delete s;
        return nullptr;
    }
    return s;
}
void pbs_destroy(void* p) { delete (Sim*)p; }

// class << 32 | home bucket of a byte string of 1..TK_XL_MAX bytes
uint64_t pbs_home(void* p, const uint8_t* key, uint32_t len) {
    const Sim* s = (const Sim*)p;
    int cls;
    uint64_t w[3];
    const uint32_t slot = home_of(s->H, key, len, &cls, w);
    return ((uint64_t)cls << 32) | (slot / kBw[cls]);
}
// per class {slots, buckets, the most tokens that share a home bucket, that bucket}
void pbs_home_stats(void* p, uint64_t* out) {
    const Sim* s = (const Sim*)p;
    std::map<uint32_t, uint32_t> homes[3];
    for (size_t k = 0; k < s->ids.size(); ++k) {
        const uint32_t len = (uint32_t)(s->off[k + 1] - s->off[k]);
        if (len > TK_XL_MAX) continue;
        int cls;
        uint64_t w[3];
        const uint32_t slot = home_of(s->H, s->blob.data() + s->off[k], len, &cls, w);
        homes[cls][slot / kBw[cls]]++;
    }
    const uint64_t slots[3] = {s->H.short_tab.size(), s->H.mid_tab.size(), s->H.xl.size()};
    for (int c = 0; c < 3; ++c) {
        uint64_t most = 0, at = 0;
        for (const auto& kv : homes[c])
            if (kv.second > most) most = kv.second, at = kv.first;
        out[4 * c] = slots[c], out[4 * c + 1] = slots[c] / kBw[c], out[4 * c + 2] = most, out[4 * c + 3] = at;
    }
}
uint32_t pbs_probe(void* p, const uint8_t* key, uint32_t len) { return probe(((const Sim*)p)->H, key, len); }

// every word of the three tables a probe depends on (the by-identity slots' `passed` word among them), FNV-1a
uint64_t pbs_digest(void* p) {
    const TkHostTables& H = ((const Sim*)p)->H;
    uint64_t h = 0xCBF29CE484222325ull;
    auto mix = [&](const void* q, size_t n) {
        for (size_t i = 0; i < n; ++i) h = (h ^ ((const uint8_t*)q)[i]) * 0x100000001B3ull;
    };
    for (const TkShortSlot& e : H.short_tab) { mix(&e.key, 4); mix(&e.val, 4); }
    for (const TkPieceSlot& e : H.mid_tab) { mix(&e.key, 8); mix(&e.rank, 4); mix(&e.len, 4); }
    for (const TkXlSlot& e : H.xl) { mix(&e.w0, 8); mix(&e.w1, 8); mix(&e.w2, 8); mix(&e.rank, 4); mix(&e.passed, 4); }
    return h;
}

// Every token of at most TK_XL_MAX bytes: found with its rank by the probe of its class and by TkHostTables::lookup_piece; each of its
// proper prefixes, an extension by one byte and a one-byte mutation (seeded) that is not a token: absent by both.
// out = {tokens checked, neighbours checked, failures}; first_bad = the index of the first token at which something failed
void pbs_check_all(void* p, uint64_t seed, uint64_t* out, uint64_t* first_bad) {
    const Sim* s = (const Sim*)p;
    const TkHostTables& H = s->H;
    std::unordered_set<std::string> have;
    for (size_t k = 0; k < s->ids.size(); ++k) have.emplace((const char*)s->blob.data() + s->off[k], s->off[k + 1] - s->off[k]);
    uint64_t rng = seed * 0x9E3779B97F4A7C15ull + 1;
    auto next = [&] {
        rng ^= rng << 13, rng ^= rng >> 7, rng ^= rng << 17;
        return rng;
    };
    out[0] = out[1] = out[2] = 0;
    *first_bad = ~0ull;
    auto absent = [&](const std::string& c, size_t k) {
        if (c.empty() || c.size() > TK_XL_MAX || have.count(c)) return;
        ++out[1];
        const uint8_t* q = (const uint8_t*)c.data();
        const uint32_t len = (uint32_t)c.size();
        if (probe(H, q, len) != TK_RANK_MAX || H.lookup_piece(q, len) != TK_RANK_MAX) {
            if (!out[2]++) *first_bad = k;
        }
    };
    for (size_t k = 0; k < s->ids.size(); ++k) {
        const uint8_t* t = s->blob.data() + s->off[k];
        const uint32_t len = (uint32_t)(s->off[k + 1] - s->off[k]);
        if (len > TK_XL_MAX) continue;
        ++out[0];
        if (probe(H, t, len) != s->ids[k] || H.lookup_piece(t, len) != s->ids[k]) {
            if (!out[2]++) *first_bad = k;
        }
        const std::string tok((const char*)t, len);
        for (uint32_t cut = 1; cut < len; ++cut) absent(tok.substr(0, cut), k);
        absent(tok + (char)(next() & 0xFF), k);
        std::string m = tok;
        m[next() % len] ^= (char)(1u << (next() & 7u));
        absent(m, k);
    }
}
}  // extern "C"
