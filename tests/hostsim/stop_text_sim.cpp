// The stop-string passes (tiktoken_amd/csrc/tk_stop_text.h) on the CPU: the plain C++ they are made of -- tk_stop_text_rule.h: the stop set,
// a lane of the search, a document's kept length, a lane of the cut, a row's token count -- compiled for the host and driven the way the
// kernels drive it: sixteen bytes per lane, workgroups of `wg_lanes` lanes, workgroups and lanes in any order.  The text is read through
// readers that refuse an index outside what the contract allows (a staged tile: the workgroup's bytes and TK_STOPS_TAIL behind them,
// whole 16-byte units that start at or before n; the cut's source: aligned units inside [0, n + 16), single bytes inside [0, n)); every
// store goes through a writer that counts the stores per output byte and refuses a wide store that leaves [0, n_text).  The buffers the
// driver makes itself are heap blocks of exactly their contract sizes (stop_text_sanitize.cpp runs this under ASan).
// Test infrastructure only (tests/test_stop_text_sim.py builds it).
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <random>
#include <vector>

#include "../../tiktoken_amd/csrc/tk_stop_text_rule.h"

namespace {
struct Fault {
    int64_t code = 0;  // 1: a byte read outside the contract, 3: a byte stored twice, 4: a store that leaves the text, 5: a byte never stored
    void set(int64_t c) {
        if (!code) code = c;
    }
};
struct Tile {  // a workgroup's staged bytes
    const uint8_t* staged;
    uint64_t base, size, n;
    Fault* f;
    uint32_t operator()(uint64_t p) const {
        if (p < base || p >= base + size || p >= n + 16) {
            f->set(1);
            return 0u;
        }
        return staged[p - base];
    }
};
struct Src {  // the cut's source
    const uint8_t* bytes;
    uint64_t n;
    Fault* f;
    void load16(uint64_t pos, uint64_t* lo, uint64_t* hi) const {
        *lo = *hi = 0;
        if ((pos & 15u) || pos + 16 > n + 16) return f->set(1);
        memcpy(lo, bytes + pos, 8);
        memcpy(hi, bytes + pos + 8, 8);
    }
    uint8_t byte(uint64_t pos) const {
        if (pos >= n) {
            f->set(1);
            return 0;
        }
        return bytes[pos];
    }
};
struct Stores {
    uint8_t* out;
    uint64_t n_text;
    uint8_t* times;
    Fault* f;
    void store16(uint64_t q, uint64_t lo, uint64_t hi) const {
        if ((q & 15u) || q + 16 > n_text) return f->set(4);
        for (int k = 0; k < 16; ++k)
            if (times[q + k]++) f->set(3);
        memcpy(out + q, &lo, 8);
        memcpy(out + q + 8, &hi, 8);
    }
    void byte(uint64_t q, uint8_t v) const {
        if (q >= n_text) return f->set(4);
        if (times[q]++) f->set(3);
        out[q] = v;
    }
};
std::vector<uint64_t> order_of(uint64_t count, uint32_t order, uint64_t seed) {
    std::vector<uint64_t> v(count);
    std::iota(v.begin(), v.end(), 0ull);
    if (order == 1) std::reverse(v.begin(), v.end());
    if (order == 2) std::shuffle(v.begin(), v.end(), std::mt19937_64(seed));
    return v;
}
}  // namespace

extern "C" {
// The passes over packed text: bytes[0, n) readable to n + 16, off[n_docs + 1]; the stop set as tk_stops gives it.  order: 0 ascending, 1
// descending, 2 shuffled -- of the workgroups and of the lanes inside each.  text: room for n + 16 bytes; text_off: n_docs + 1; hit:
// n_docs; totals: {n_text, n_hit, wrote (0: no hit anywhere -- the input is the output, no cut pass)}.
// Returns 0, a Fault code, 1000 + the first document whose offset offends, or 2000 + the refusal of the stop set.
int64_t stops_run(const uint8_t* bytes, uint64_t n, const uint64_t* off, uint64_t n_docs, const uint8_t* blob, const uint32_t* stop_off, uint32_t n_stops, uint32_t flags,
                  uint32_t wg_lanes, uint32_t order, uint8_t* text, uint64_t* text_off, uint32_t* hit, uint64_t* totals) {
    Fault f;
    TkStopSet set;
    const int why = tk_stops_make(n_stops, blob, stop_off, flags, &set);
    if (why) return 2000 + why;
    // tk_k_u8r_check
    for (uint64_t d = 0; d <= n_docs; ++d)
        if ((d == 0 && off[0] != 0) || (d < n_docs ? off[d] > off[d + 1] : off[d] != n)) return 1000 + (int64_t)d;
    // tk_k_stops_find
    const uint64_t wg_bytes = 16ull * wg_lanes, tile_size = wg_bytes + TK_STOPS_TAIL;
    std::vector<unsigned long long> word(n_docs, ~0ull);
    if (n && n_docs && set.n) {
        uint8_t* staged = (uint8_t*)malloc(tile_size);
        for (uint64_t b : order_of((n + wg_bytes - 1) / wg_bytes, order, 1)) {
            const uint64_t base = b * wg_bytes;
            memset(staged, 0, tile_size);
            for (uint64_t u = 0; u < tile_size / 16; ++u)
                if (base + 16 * u <= n) memcpy(staged + 16 * u, bytes + base + 16 * u, 16);  // (a whole unit: the text is readable to n + 16)
            const Tile tile{staged, base, tile_size, n, &f};
            for (uint64_t l : order_of(wg_lanes, order, b + 2))
                tk_stops_lane(tile, set, off, n_docs, n, base + 16 * l, [&](uint64_t d, unsigned long long key) {
                    if (d >= n_docs) return f.set(1);
                    word[d] = std::min(word[d], key);  // atomicMin
                });
        }
        free(staged);
    }
    // tk_k_stops_rows, tk_k_stops_scan, tk_k_stops_docs
    uint64_t n_text = 0, n_hit = 0;
    for (uint64_t d = 0; d < n_docs; ++d) {
        text_off[d] = n_text;
        n_text += tk_stops_kept(word[d], off[d + 1] - off[d], set, &hit[d]);
        n_hit += hit[d] != TK_STOPS_NO_HIT;
    }
    text_off[n_docs] = n_text;
    totals[0] = n_text, totals[1] = n_hit, totals[2] = n_hit ? 1 : 0;
    // tk_k_stops_cut
    if (n_hit) {
        uint8_t* out = (uint8_t*)malloc(n_text + 16);
        uint8_t* times = (uint8_t*)calloc(n_text + 16, 1);
        const Src src{bytes, n, &f};
        Stores st{out, n_text, times, &f};
        for (uint64_t lane : order_of((n_text + 15) / 16, order, 7)) tk_stops_cut_lane(src, off, (const uint64_t*)text_off, n_docs, n_text, lane * 16, st);
        for (uint64_t i = 0; i < n_text; ++i)
            if (times[i] != 1) f.set(times[i] ? 3 : 5);
        memcpy(text, out, n_text);
        free(out), free(times);
    } else if (n) {
        memcpy(text, bytes, n);
    }
    return f.code;
}

// tk_k_stops_ntok for one row
uint32_t stops_ntok(const unsigned long long* tok_byte, uint64_t t0, uint64_t t1, uint64_t kept_end) { return tk_stops_ntok(tok_byte, t0, t1, kept_end); }
}
