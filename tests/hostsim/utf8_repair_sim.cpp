// The UTF-8 repair passes (tiktoken_amd/csrc/tk_utf8_repair.h) on the CPU: the plain C++ they are made of -- tk_utf8_repair_rule.h: the state
// a lane starts in, its step, the stream its output leaves through, the bounds from the bitmap -- compiled for the host and driven the way
// the kernels drive it: sixteen bytes per lane, workgroups of `wg_lanes` lanes, workgroups and lanes in any order.  Every read goes
// through a reader that refuses an index outside what the contract allows (bytes: [0, n + 16); bitmap: up to one word past bit n + 16);
// every store goes through a writer that counts the stores per output byte and refuses a wide store that leaves [0, n_text).  The
// buffers the driver makes itself are heap blocks of exactly their contract sizes (utf8_repair_sanitize.cpp runs this under ASan).
// Test infrastructure only (tests/test_utf8_repair_sim.py builds it).
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <random>
#include <vector>

#include "../../tiktoken_amd/csrc/tk_utf8_repair_rule.h"

namespace {
struct Fault {
    int64_t code = 0;  // 1: a byte read outside the contract, 2: a bitmap word, 3: a byte stored twice, 4: a wide store that leaves the text, 5: a byte never stored
    void set(int64_t c) {
        if (!code) code = c;
    }
};
struct Bits {  // the bitmap over the bytes: words [0, n_words)
    const uint32_t* w;
    uint64_t n_words;
    Fault* f;
    uint32_t operator[](uint64_t i) const {
        if (i >= n_words) {
            f->set(2);
            return 0u;
        }
        return w[i];
    }
};
struct Stores {  // the kernel's TkDecStores with the books kept
    uint8_t* out;
    uint64_t n_text;
    uint8_t* times;
    Fault* f;
    void byte(unsigned long long off, uint8_t v) const {
        if (off >= n_text) return f->set(4);
        if (times[off]++) f->set(3);
        out[off] = v;
    }
    void word(unsigned long long off, uint64_t v) const {
        if ((off & 7ull) || off + 8 > n_text) return f->set(4);
        for (int k = 0; k < 8; ++k)
            if (times[off + k]++) f->set(3);
        memcpy(out + off, &v, 8);
    }
};
struct LaneIn {
    uint64_t lo = 0, hi = 0;
    uint32_t nvalid = 0, prev = 0, bounds = 0, before = 0;
};
// tk_u8r_load: one 16-byte read at p0 where the lane has text, the four bytes before it, the bounds
LaneIn load(const uint8_t* bytes, uint64_t n, const Bits& docb, uint64_t p0, Fault* f) {
    LaneIn in;
    in.nvalid = p0 < n ? (n - p0 < 16 ? (uint32_t)(n - p0) : 16u) : 0u;
    if (in.nvalid) {
        if (p0 + 16 > n + 16) f->set(1);
        memcpy(&in.lo, bytes + p0, 8);
        memcpy(&in.hi, bytes + p0 + 8, 8);
        if (p0) {
            uint32_t w;
            memcpy(&w, bytes + p0 - 4, 4);
            in.prev = w >> 8;
        }
    }
    if (p0 <= n) in.bounds = tk_u8r_bounds(docb, p0, &in.before);
    return in;
}
bool plain(const LaneIn& in) { return !((in.lo | in.hi | (uint64_t)in.prev) & 0x8080808080808080ull); }
uint64_t lower_bound(const uint64_t* off, uint64_t count, uint64_t v) {
    uint64_t lo = 0, hi = count;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (off[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
std::vector<uint64_t> order_of(uint64_t count, uint32_t order, uint64_t seed) {
    std::vector<uint64_t> v(count);
    std::iota(v.begin(), v.end(), 0ull);
    if (order == 1) std::reverse(v.begin(), v.end());
    if (order == 2) std::shuffle(v.begin(), v.end(), std::mt19937_64(seed));
    return v;
}
}  // namespace

extern "C" {
// The passes over packed text: bytes[0, n) readable to n + 16, off[n_docs + 1].  order: 0 ascending, 1 descending, 2 shuffled -- of the
// workgroups and of the lanes inside each.  text: room for 3 * n + 16 bytes; the offsets: 3 x (n_docs + 1); totals: {n_text, chars,
// replaced, wrote (0: nothing replaced -- the input is the output, no write pass), searches (the most any lane made)}.
// Returns 0, a Fault code, or 1000 + the first document whose offset offends.
int64_t u8r_run(const uint8_t* bytes, uint64_t n, const uint64_t* off, uint64_t n_docs, uint32_t mode, uint32_t wg_lanes, uint32_t order, uint8_t* text, uint64_t* text_off,
                uint64_t* char_off, uint64_t* repl_off, uint64_t* totals) {
    Fault f;
    // tk_k_u8r_check
    for (uint64_t d = 0; d <= n_docs; ++d)
        if ((d == 0 && off[0] != 0) || (d < n_docs ? off[d] > off[d + 1] : off[d] != n)) return 1000 + (int64_t)d;
    // tk_k_span_mark: one word past bit n + 16, and not a word more
    const uint64_t n_words = ((n + 16) >> 5) + 2;
    uint32_t* bm = (uint32_t*)calloc(n_words, 4);
    for (uint64_t d = 0; d <= n_docs; ++d)
        if (off[d] <= n) bm[off[d] >> 5] |= 1u << (off[d] & 31);
    const Bits docb{bm, n_words, &f};
    const uint64_t wg_bytes = 16ull * wg_lanes, nb = n / wg_bytes + 1, lanes = n / 16 + 1;
    std::vector<uint64_t> sums(3 * nb, 0);
    // (the kernel's workgroup of 256 lanes leaves at most 3 x 4096 bytes: its places are 16-bit, and so are they here up to that size; a
    // simulated workgroup of more lanes needs more bits)
    uint32_t* place = (uint32_t*)malloc(lanes * 4);
    uint32_t* rel = (uint32_t*)malloc(3 * (n_docs + 1) * 4);
    memset(rel, 0xEE, 3 * (n_docs + 1) * 4);
    uint64_t most_searches = 0;
    TkU8rNoStream none;
    // tk_k_u8r_count
    for (uint64_t b : order_of(nb, order, 1)) {
        std::vector<TkU8rCounts> cnt(wg_lanes), ex(wg_lanes), first(wg_lanes);
        std::vector<LaneIn> ins(wg_lanes);
        for (uint64_t l : order_of(wg_lanes, order, b + 2)) {
            ins[l] = load(bytes, n, docb, (b * wg_lanes + l) * 16, &f);
            cnt[l] = TkU8rCounts{ins[l].nvalid, ins[l].nvalid, 0u};
            const uint32_t starts = ins[l].bounds & 0xFFFFu & ((2u << ins[l].nvalid) - 1u), first_i = starts ? (uint32_t)__builtin_ctz(starts) : 0u;
            first[l] = TkU8rCounts{first_i, first_i, 0u};  // the one step takes the first start's prefixes along
            if (!plain(ins[l]))
                cnt[l] = tk_u8r_lane(ins[l].lo, ins[l].hi, ins[l].nvalid, ins[l].prev, ins[l].bounds, ins[l].before, mode, none, [&](uint32_t i, const TkU8rCounts& at) {
                    if (i == first_i) first[l] = at;
                });
        }
        TkU8rCounts run{0, 0, 0};
        for (uint32_t l = 0; l < wg_lanes; ++l) {  // the two tk_block_exscan_256
            ex[l] = run;
            run.out += cnt[l].out, run.chars += cnt[l].chars, run.repl += cnt[l].repl;
        }
        sums[b] = run.out, sums[nb + b] = run.chars, sums[2 * nb + b] = run.repl;
        for (uint64_t l : order_of(wg_lanes, order, b + 3)) {
            const uint64_t lane = b * wg_lanes + l, p0 = lane * 16;
            const LaneIn& in = ins[l];
            if (p0 <= n) place[lane] = wg_lanes <= 256 ? (uint16_t)ex[l].out : ex[l].out;
            const uint32_t starts = in.bounds & 0xFFFFu & ((2u << in.nvalid) - 1u);
            if (!starts) continue;
            uint64_t searches = 0;
            auto doc = [&](uint32_t i, const TkU8rCounts& at) {
                const uint64_t p = p0 + i, k = lower_bound(off, n_docs + 1, p);
                ++searches;
                if (k <= n_docs && off[k] == p) {
                    rel[k] = ex[l].out + at.out;
                    rel[n_docs + 1 + k] = ex[l].chars + at.chars;
                    rel[2 * (n_docs + 1) + k] = ex[l].repl + at.repl;
                }
            };
            const uint32_t first_i = (uint32_t)__builtin_ctz(starts), more = starts & (starts - 1u);
            doc(first_i, first[l]);
            if (more && plain(in)) {
                for (uint32_t m = more; m; m &= m - 1u) {
                    const uint32_t i = (uint32_t)__builtin_ctz(m);
                    doc(i, TkU8rCounts{i, i, 0u});
                }
            } else if (more) {  // further starts in the lane: the step again
                (void)tk_u8r_lane(in.lo, in.hi, in.nvalid, in.prev, in.bounds, in.before, mode, none, [&](uint32_t i, const TkU8rCounts& at) {
                    if (i != first_i) doc(i, at);
                });
            }
            most_searches = std::max(most_searches, searches);
        }
    }
    // tk_k_u8r_scan
    for (uint32_t k = 0; k < 3; ++k) {
        uint64_t carry = 0;
        for (uint64_t b = 0; b < nb; ++b) {
            const uint64_t own = sums[k * nb + b];
            sums[k * nb + b] = carry;
            carry += own;
        }
        totals[k] = carry;
    }
    totals[3] = totals[2] ? 1 : 0;
    totals[4] = most_searches;
    // tk_k_u8r_docs (any order: it reads what the count pass wrote)
    for (uint64_t d : order_of(n_docs + 1, order, 5)) {
        uint64_t fst = d;  // tk_span_first_at: one search for a document behind an empty one
        if (d && off[d] == off[d - 1]) fst = lower_bound(off, n_docs + 1, off[d]);
        const uint64_t w = off[fst] / wg_bytes;
        uint64_t* out[3] = {text_off, char_off, repl_off};
        for (uint32_t k = 0; k < 3; ++k) out[k][d] = sums[k * nb + w] + rel[k * (n_docs + 1) + fst];
    }
    // tk_k_u8r_write
    const uint64_t n_text = totals[0];
    if (totals[2]) {
        uint8_t* out = (uint8_t*)malloc(n_text + 16);
        uint8_t* times = (uint8_t*)calloc(n_text + 16, 1);
        const Stores stores_c{out, n_text, times, &f};
        for (uint64_t b : order_of((n + wg_bytes - 1) / wg_bytes, order, 7)) {
            for (uint64_t l : order_of(wg_lanes, order, b + 8)) {
                const uint64_t lane = b * wg_lanes + l;
                const LaneIn in = load(bytes, n, docb, lane * 16, &f);
                if (!in.nvalid) continue;
                Stores stores = stores_c;
                TkU8rStream<Stores> stream(stores, sums[b] + place[lane]);
                if (plain(in)) {
                    uint64_t lo = in.lo, hi = in.hi;
                    for (uint32_t left = in.nvalid; left; left -= left < 4u ? left : 4u) {
                        const uint32_t nbytes = left < 4u ? left : 4u;
                        stream.put((uint32_t)lo & (nbytes < 4u ? (1u << (8u * nbytes)) - 1u : 0xFFFFFFFFu), nbytes);
                        lo = (lo >> 32) | (hi << 32);
                        hi >>= 32;
                    }
                } else {
                    (void)tk_u8r_lane(in.lo, in.hi, in.nvalid, in.prev, in.bounds, in.before, mode, stream, TkU8rNoDocs());
                }
                stream.finish();
            }
        }
        for (uint64_t i = 0; i < n_text; ++i)
            if (times[i] != 1) f.set(times[i] ? 3 : 5);
        memcpy(text, out, n_text);
        free(out), free(times);
    } else if (n) {
        memcpy(text, bytes, n);
    }
    free(bm), free(place), free(rel);
    return f.code;
}
}
