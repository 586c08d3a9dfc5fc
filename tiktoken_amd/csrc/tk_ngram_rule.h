// Token n-gram sets: the parts of the device passes of tk_ngram.h that are plain C++ -- which positions of a document start an n-gram,
// an n-gram's key, the shape of a set, where a key's probe starts and which bit of the filter is its, the probe and the insert over a
// table (the insert's compare-and-swap is the caller's), the smear of hit words into covered words, the counts over a range of bits, and
// what one lane does with a range of positions in the key step (tk_ng_seg_keys) and in the count step (tk_ng_seg_count).  The rule is
// stated in include/tiktoken_amd.h.  Compiles for the host too: tests/test_ngram_sim.py drives the steps on the CPU at tiles of 8 and 64
// positions and at the shipped one.
//
// A tile is TK_NG_TILE positions of `tokens`, [g0, g0 + T).  Its bits -- one per position, hit or covered -- lie in 64-bit words; bit
// index g - g0 + TK_NG_LEFT, so word 0 is the left halo (ngram - 1 < 64 positions before the tile, whose hits cover tokens of the tile)
// and word 1 starts at g0.  T is a multiple of 64 times the segments of a tile, so a segment is whole words.
//
// Why T = 1024 with 256 lanes: a tile keeps 8 (T + 64) bytes of keys and 4 (T + 64) bytes of ids in LDS, 13 KiB, so eight workgroups --
// every wavefront slot of a CU -- are resident, which is what a pass of dependent HBM loads needs most; the halo that is hashed twice is
// (k - 1) / T, 1.2 % at k = 13 and 3 % at k = 32; a tile of 2048 positions would halve that and leave six workgroups resident.
#pragma once
#include <stdint.h>

#include "tk_fingerprint_rule.h"  // tk_fp_hash, tk_fp_walk, TK_FP_MAX_NGRAM

#define TK_NG_TILE 1024u    // token positions per workgroup
#define TK_NG_THREADS 256u  // its lanes
#define TK_NG_SEGS 4u       // segments of a tile: one per wavefront
#define TK_NG_LEFT 64u      // bits before the tile's first position: one word
#define TK_NG_HALO 32u      // staged ids before the tile's first position, and behind its last
#define TK_NG_NONE 0xFFFFFFFFFFFFFFFFull  // first_hit of a document without a hit
#define TK_NG_MAX_CAPACITY (1ull << 30)

struct TkNg {
    uint32_t k;
    uint64_t seed, S;  // S: slots of the table, a power of two >= 2 capacity; the filter has 4 S bits
    uint64_t n_tokens, n_docs;
};

// The shape of a set.  0, or why it is refused: 1 ngram, 2 capacity.
TK_HD int tk_ng_shape(uint32_t ngram, uint64_t seed, uint64_t capacity, TkNg* p) {
    if (ngram < 1 || ngram > TK_FP_MAX_NGRAM) return 1;
    if (capacity < 1 || capacity > TK_NG_MAX_CAPACITY) return 2;
    uint64_t S = 2;
    while (S < 2 * capacity) S <<= 1;
    p->k = ngram, p->seed = seed, p->S = S, p->n_tokens = 0, p->n_docs = 0;
    return 0;
}
TK_HD uint64_t tk_ng_filter_words(uint64_t S) { return S < 8 ? 1 : S / 8; }  // uint32 words of the filter: 4 S bits, S / 2 bytes

// The n-grams of the document [s, e) start at [s, result): none when it is shorter than k
TK_HD uint64_t tk_ng_starts_end(uint64_t s, uint64_t e, uint32_t k) { return e - s >= k ? e - k + 1 : s; }
// ids[at .. at + k): an n-gram's key (never 0: 0 is the empty slot)
template <class Ids>
TK_HD uint64_t tk_ng_key(const Ids& ids, uint64_t at, uint32_t k, uint64_t seed) {
    const uint64_t h = tk_fp_hash(ids, at, k, seed);
    return h ? h : 1;
}
TK_HD uint64_t tk_ng_slot(uint64_t key, uint64_t S) { return key & (S - 1); }
TK_HD uint64_t tk_ng_filter_bit(uint64_t key, uint64_t S) { return (key >> 31) & (4 * S - 1); }  // (the bits the slot does not use first)

// Is `key` in the table?  The walk ends at the key or at an empty slot; a set holds at most S / 2 keys, so there is one.
template <class Table>
TK_HD bool tk_ng_probe(const Table& table, uint64_t S, uint64_t key) {
    uint64_t i = tk_ng_slot(key, S);
    for (uint64_t n = 0; n < S; ++n, i = (i + 1) & (S - 1)) {
        const uint64_t v = table[i];
        if (v == key) return true;
        if (v == 0) return false;
    }
    return false;
}
template <class Filter>
TK_HD bool tk_ng_filter_has(const Filter& filter, uint64_t S, uint64_t key) {
    const uint64_t b = tk_ng_filter_bit(key, S);
    return (filter[b >> 5] >> (b & 31)) & 1u;
}
// `key` into the table: cas(i, key) claims slot i if it is empty and returns what it held before.  True: this call claimed a slot
// (the key was not there).  At most S steps (a table without an empty slot: nothing is written).
template <class Table, class Cas>
TK_HD bool tk_ng_insert(const Table& table, uint64_t S, uint64_t key, Cas&& cas) {
    uint64_t i = tk_ng_slot(key, S);
    for (uint64_t n = 0; n < S; ++n, i = (i + 1) & (S - 1)) {
        uint64_t v = table[i];
        if (v == 0) v = cas(i, key);
        if (v == 0) return true;
        if (v == key) return false;
    }
    return false;
}

// Hit words -> a covered word: bit b of the result is set when a bit of [b - k + 1, b] of the 128-bit (lo, hi) is: hi smeared upwards by k
// positions, doubling, the carry from lo (k <= 32: one word back is enough).
TK_HD uint64_t tk_ng_smear(uint64_t lo, uint64_t hi, uint32_t k) {
    uint32_t w = 1;
    for (; 2 * w <= k; w *= 2) {
        hi |= (hi << w) | (lo >> (64 - w));
        lo |= lo << w;
    }
    const uint32_t r = k - w;  // (r <= w)
    if (r) hi |= (hi << r) | (lo >> (64 - r));
    return hi;
}
// the bits [lo, hi) of a word (lo < hi <= 64)
TK_HD uint64_t tk_ng_bits(uint32_t lo, uint32_t hi) { return (hi >= 64 ? ~0ull : (1ull << hi) - 1) & ~((1ull << lo) - 1); }
TK_HD uint32_t tk_ng_popc(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popcll(x);
#else
    return (uint32_t)__builtin_popcountll(x);
#endif
}
TK_HD uint32_t tk_ng_ctz(uint64_t x) {  // x != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__ffsll((unsigned long long)x) - 1;
#else
    return (uint32_t)__builtin_ctzll(x);
#endif
}

// The key step, one lane of the `n_lanes` that share the positions [c0, c1) of the tile that starts at g0 (ids: the staged ids,
// ids[g - g0 + TK_NG_HALO] = tokens[g], zeros outside the batch): f(g, key) for every g of the range, key 0 where g starts no n-gram.
template <class Off, class Ids, class F>
TK_HD void tk_ng_seg_keys(const TkNg& p, const Off& tok_off, const Ids& ids, uint64_t g0, uint64_t c0, uint64_t c1, uint32_t lane, uint32_t n_lanes, F&& f) {
    tk_fp_walk(tok_off, p.n_docs, c0, c1, [&](uint64_t, uint64_t s, uint64_t e, uint64_t a, uint64_t b) {
        const uint64_t v1 = tk_ng_starts_end(s, e, p.k);
        for (uint64_t g = a + lane; g < b; g += n_lanes) f(g, g < v1 ? tk_ng_key(ids, g - g0 + TK_NG_HALO, p.k, p.seed) : 0ull);
    });
}
// The count step, lane `lane` of those that share the segment [c0, c1) of the tile at g0 (c0 - g0 a multiple of 64; the lane takes the
// segment's word `lane` and nothing if the segment has fewer): per document that owns a position of the segment, this lane's share of
// its hits, covered tokens and lowest hit start, to the sink:
//   sink.counts(d, whole, n_hit, n_covered, first)   whole: the document lies inside the segment; first relative to the document
template <class Off, class Words, class Sink>
TK_HD void tk_ng_seg_count(const TkNg& p, const Off& tok_off, const Words& hit, const Words& cov, uint64_t g0, uint64_t c0, uint64_t c1, uint32_t lane, Sink& sink) {
    const uint64_t w0 = c0 + 64ull * lane, w1 = w0 + 64;  // this lane's word, as positions
    const uint64_t word = (w0 - g0 + TK_NG_LEFT) / 64;
    tk_fp_walk(tok_off, p.n_docs, c0, c1, [&](uint64_t d, uint64_t s, uint64_t e, uint64_t a, uint64_t b) {
        const uint64_t lo = a > w0 ? a : w0, hi = b < w1 ? b : w1;
        uint64_t nh = 0, nc = 0, first = TK_NG_NONE;
        if (lo < hi) {
            const uint64_t m = tk_ng_bits((uint32_t)(lo - w0), (uint32_t)(hi - w0)), h = hit[word] & m;
            nh = tk_ng_popc(h), nc = tk_ng_popc(cov[word] & m);
            if (h) first = w0 + tk_ng_ctz(h) - s;
        }
        sink.counts(d, s >= c0 && e <= c1, nh, nc, first);
    });
}
