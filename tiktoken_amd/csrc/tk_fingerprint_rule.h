// Near-duplicate fingerprints of a packed batch: the parts of the device passes of tk_fingerprint.h that are plain C++ -- the mix, the
// shape of a call, which positions of a document start a shingle, a shingle's hash, a permutation and its value, the exact hash's terms,
// a band key, the walk over the documents that meet a range of positions, and what one lane does with such a range in the hash step
// (tk_fp_seg_hash) and in the signature step (tk_fp_slice_sig).  The rule is stated in include/tiktoken_amd.h.  Compiles for the host
// too: tests/test_fingerprint_sim.py drives the steps lane by lane on the CPU, at the shipped tile and at tiles of 8 and 64 positions.
//
// A tile is TK_FP_TILE positions of `tokens`.  The hash step cuts it into TK_FP_WAVES segments, one per wavefront; the signature step
// cuts it into slices of lanes_for(P) lanes each, every lane one permutation.  Segment or slice, the part of a document inside it is
// flushed with a plain store when the whole document lies inside and with an atomic otherwise -- minimum and sum are commutative, so the
// result is a function of (tokens, tok_off, spec) alone, whatever the tile and however the blocks are scheduled.
#pragma once
#include <stdint.h>

#include "tk_rows_rule.h"  // tk_last_le

#define TK_FP_TILE 1024u      // token positions per workgroup
#define TK_FP_THREADS 256u    // its lanes
#define TK_FP_MAX_NGRAM 32u
#define TK_FP_MAX_PERM 256u
#define TK_FP_NONE 0xFFFFFFFFu  // the signature of a document without a shingle
#define TK_FP_BAND_SALT 0x42414E4400000000ull

struct TkFp {
    uint32_t k, P, B, r;  // ngram, n_perm, bands, rows of a band
    uint64_t seed, n_tokens, n_docs;
};

TK_HD uint64_t tk_fp_mix(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// The shape of a call.  0, or why it is refused: 1 ngram, 2 n_perm, 3 bands.
TK_HD int tk_fp_shape(uint32_t ngram, uint32_t n_perm, uint32_t bands, uint64_t seed, uint64_t n_tokens, uint64_t n_docs, TkFp* p) {
    if (ngram < 1 || ngram > TK_FP_MAX_NGRAM) return 1;
    if (n_perm < 1 || n_perm > TK_FP_MAX_PERM) return 2;
    if (bands < 1 || bands > n_perm || n_perm % bands) return 3;
    p->k = ngram, p->P = n_perm, p->B = bands, p->r = n_perm / bands;
    p->seed = seed, p->n_tokens = n_tokens, p->n_docs = n_docs;
    return 0;
}
// Lanes of a slice of the signature step: a whole number of wavefronts that holds every permutation
TK_HD uint32_t tk_fp_slice_lanes(uint32_t P) { return P <= 64 ? 64u : P <= 128 ? 128u : 256u; }

// The shingles of the document [s, e): they start at [s, *v1), each over *m ids (none: *v1 == s)
TK_HD void tk_fp_shingles(uint64_t s, uint64_t e, uint32_t k, uint64_t* v1, uint32_t* m) {
    const uint64_t L = e - s;
    *m = L < k ? (uint32_t)L : k;
    *v1 = L == 0 ? s : L < k ? s + 1 : e - k + 1;
}
// ids[at .. at + m): a shingle's hash
template <class Ids>
TK_HD uint64_t tk_fp_hash(const Ids& ids, uint64_t at, uint32_t m, uint64_t seed) {
    uint64_t x = tk_fp_mix(seed ^ m);
    for (uint32_t j = 0; j < m; ++j) x = tk_fp_mix(x ^ (uint64_t)(uint32_t)ids[at + j]);
    return x;
}
TK_HD void tk_fp_perm(uint64_t seed, uint32_t p, uint64_t* a, uint64_t* b) {
    *a = tk_fp_mix(seed + 2ull * p + 1) | 1ull;
    *b = tk_fp_mix(seed + 2ull * p + 2);
}
TK_HD uint32_t tk_fp_value(uint64_t a, uint64_t b, uint64_t h) { return (uint32_t)((a * h + b) >> 32); }
// token i of its document, id t: its term of the exact hash's sum; the hash of a document of L tokens
TK_HD uint64_t tk_fp_exact_term(uint64_t seed, uint64_t i, uint32_t t) { return tk_fp_mix(seed ^ ((i + 1) << 32) ^ (uint64_t)t); }
TK_HD uint64_t tk_fp_exact_done(uint64_t L, uint64_t sum) { return tk_fp_mix(L ^ sum); }
// band j of a signature (sig: its P values)
template <class Sig>
TK_HD uint64_t tk_fp_band_key(uint64_t seed, uint32_t j, uint32_t r, const Sig& sig) {
    uint64_t x = tk_fp_mix(seed ^ TK_FP_BAND_SALT ^ (uint64_t)j);
    for (uint32_t i = 0; i < r; ++i) x = tk_fp_mix(x ^ (uint64_t)(uint32_t)sig[(uint64_t)j * r + i]);
    return x;
}

// The documents that own a position of [c0, c1) (c0 < c1 <= n_tokens), in order: f(d, s, e, a, b), [s, e) the document, [a, b) its part
// in the range.  Empty documents own nothing and are stepped over -- by the search where more than one follows.  Whatever tok_off holds,
// a <  b, both inside the range, d < n_docs, and the walk ends: an array that does not ascend from 0 to n_tokens gives values nobody
// has defined, never an access outside tok_off[0 .. n_docs] or outside the range.
template <class Off, class F>
TK_HD void tk_fp_walk(const Off& tok_off, uint64_t n_docs, uint64_t c0, uint64_t c1, F&& f) {
    if (!n_docs) return;
    uint64_t d = tk_last_le(tok_off, 0, n_docs, c0), cur = c0;
    while (cur < c1) {
        const uint64_t s = tok_off[d], e = tok_off[d + 1];
        uint64_t nx = e < c1 ? e : c1;
        if (nx <= cur) nx = cur + 1;  // (an array that does not ascend)
        f(d, s, e, cur, nx);
        cur = nx;
        if (cur >= c1 || d + 1 >= n_docs) break;
        d = d + 1;
        if (d + 1 < n_docs && tok_off[d + 1] <= cur) d = tk_last_le(tok_off, d + 1, n_docs, cur);
    }
}

// The hash step, one lane of the `n_lanes` that share the segment [c0, c1) of the tile that starts at g0 (ids: the tile's ids and the
// TK_FP_MAX_NGRAM - 1 that follow, ids[0] = tokens[g0], zeros behind n_tokens): hash[g - g0] of every g of the segment that starts a
// shingle; per document, this lane's share of the exact hash's sum, and the document's shingles in the segment, to the sink:
//   sink.sums(d, whole, exact_part, n_shingles_part)   whole: the document lies inside the segment; every lane calls, lane 0 counts
template <class Off, class Ids, class Hash, class Sink>
TK_HD void tk_fp_seg_hash(const TkFp& p, const Off& tok_off, const Ids& ids, uint64_t g0, uint64_t c0, uint64_t c1, uint32_t lane, uint32_t n_lanes, Hash& hash, Sink& sink) {
    tk_fp_walk(tok_off, p.n_docs, c0, c1, [&](uint64_t d, uint64_t s, uint64_t e, uint64_t a, uint64_t b) {
        uint64_t v1, sum = 0;
        uint32_t m;
        tk_fp_shingles(s, e, p.k, &v1, &m);
        const uint64_t vb = v1 < b ? v1 : b;  // shingle starts in [a, vb)
        for (uint64_t g = a + lane; g < vb; g += n_lanes) hash[g - g0] = tk_fp_hash(ids, g - g0, m, p.seed);
        for (uint64_t g = a + lane; g < b; g += n_lanes) sum += tk_fp_exact_term(p.seed, g - s, (uint32_t)ids[g - g0]);
        sink.sums(d, s >= c0 && e <= c1, sum, vb > a ? vb - a : 0);
    });
}
// The signature step, the lane of permutation `perm` on the slice [c0, c1) of the tile that starts at g0: the minimum of the
// permutation over the hashes of every document's shingles in the slice, to the sink:
//   sink.sig(d, whole, perm, value)   value TK_FP_NONE: the document has no shingle in the slice (an atomic may be left out)
template <class Off, class Hash, class Sink>
TK_HD void tk_fp_slice_sig(const TkFp& p, const Off& tok_off, const Hash& hash, uint64_t g0, uint64_t c0, uint64_t c1, uint32_t perm, Sink& sink) {
    uint64_t pa, pb;
    tk_fp_perm(p.seed, perm, &pa, &pb);
    tk_fp_walk(tok_off, p.n_docs, c0, c1, [&](uint64_t d, uint64_t s, uint64_t e, uint64_t a, uint64_t b) {
        uint64_t v1;
        uint32_t m, mn = TK_FP_NONE;
        tk_fp_shingles(s, e, p.k, &v1, &m);
        const uint64_t vb = v1 < b ? v1 : b;
        for (uint64_t g = a; g < vb; ++g) {
            const uint32_t v = tk_fp_value(pa, pb, hash[g - g0]);
            mn = v < mn ? v : mn;
        }
        sink.sig(d, s >= c0 && e <= c1, perm, mn);
    });
}
// The finish step of (document d, band j): the band key from the finished signature; band 0 closes the exact hash (sum -> hash)
template <class Off>
TK_HD void tk_fp_finish(const TkFp& p, const Off& tok_off, uint64_t d, uint32_t j, const uint32_t* sig, uint64_t* band, uint64_t* exact) {
    if (band) band[d * p.B + j] = tk_fp_band_key(p.seed, j, p.r, sig + d * p.P);
    if (exact && j == 0) exact[d] = tk_fp_exact_done(tok_off[d + 1] - tok_off[d], exact[d]);
}
