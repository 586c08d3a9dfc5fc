// Training rows from a packed batch: the parts of the device passes of tk_rows.h that are plain C++ -- the shape of the result, what a
// tok_off entry must satisfy, which document a stream position belongs to, where a stream element comes from (bos, body, eos or pad), the
// pos rule, what counts as a segment start, and a whole lane of the write pass (tk_rows_lane).  Compiles for the host too:
// tests/test_rows_sim.py drives them lane by lane on the CPU.
//
// The stream: for every document d, in order, [bos] tokens[tok_off[d] .. tok_off[d + 1]) [eos]; k = how many of bos / eos there are, so
// document d starts at out_off(d) = tok_off[d] + d * k and the stream has S = T + n_docs * k elements.  It is cut into R rows of L; M
// positions are written (R * L padded with pad_id, or -- drop_last -- the S of the stream: R whole rows, then the tail).
#pragma once
#include <stdint.h>

#include "tk_common.h"

#define TK_ROWS_NONE 0xFFFFFFFFu  // no bos / eos; the `doc` of padding

struct TkRows {
    uint64_t n_tokens, n_docs;     // T, the documents
    uint32_t seq_len, bos, eos, pad;
    uint32_t k, has_bos;           // elements added per document; 1 when one of them goes in front
    uint64_t S, R, M;              // stream length, rows, positions written
};

// The shape of a call.  0, or why it is refused: 1 seq_len == 0, 2 the outputs are 32-bit (positions), 3 ... (document indices).
TK_HD int tk_rows_shape(uint64_t n_tokens, uint64_t n_docs, uint32_t seq_len, uint32_t bos, uint32_t eos, uint32_t pad, bool drop_last, TkRows* r) {
    if (!seq_len) return 1;
    if (n_docs >= 0xFFFFFFFFull) return 3;
    if (n_tokens >> 32) return 2;
    r->n_tokens = n_tokens;
    r->n_docs = n_docs;
    r->seq_len = seq_len;
    r->bos = bos;
    r->eos = eos;
    r->pad = pad;
    r->has_bos = bos != TK_ROWS_NONE ? 1u : 0u;
    r->k = r->has_bos + (eos != TK_ROWS_NONE ? 1u : 0u);
    r->S = n_tokens + n_docs * r->k;  // (below 2^34)
    r->R = drop_last ? r->S / seq_len : (r->S + seq_len - 1) / seq_len;
    r->M = drop_last ? r->S : r->R * seq_len;
    if ((r->S > r->M ? r->S : r->M) >> 32) return 2;
    return 0;
}

TK_HD uint64_t tk_rows_out_off(uint64_t tok_off_d, uint64_t d, uint32_t k) { return tok_off_d + d * k; }

// What entry d of tok_off (a = tok_off[d]; b = tok_off[d + 1], or n_tokens for d == n_docs) must satisfy.  0, or 1: tok_off[0] != 0,
// 2: document d ends before it starts, 3: the last entry is not n_tokens.  Entries that all pass ascend from 0 to n_tokens.
TK_HD uint32_t tk_rows_off_error(uint64_t a, uint64_t b, uint64_t d, uint64_t n_docs) {
    if (d == 0 && a != 0) return 1u;
    if (d == n_docs) return a != b ? 3u : 0u;
    return a > b ? 2u : 0u;
}
// the word an offending entry is reported in: the lowest key is the first offending document (entry n_docs speaks for the last document)
TK_HD uint64_t tk_rows_bad_key(uint64_t d, uint64_t n_docs, uint32_t why) { return ((d == n_docs && d ? d - 1 : d) << 2) | why; }
// A report word that keeps the lowest value it is handed: on the device a word every thread shares (all ones = none), on the CPU a plain variable
TK_HD void tk_report_min(unsigned long long* word, unsigned long long v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(word, v);
#else
    *word = v < *word ? v : *word;
#endif
}
// The head of a pass over the entries of an offsets array (tok_off in the row, padded and samples passes; sample_off): *a = entry d, *b =
// the next one (n_tokens behind the last), and what tk_rows_off_error says about them.  An offending entry's key goes into *bad, the report
// word TK_BAD_OFF, which keeps the lowest.  `tok_off` is indexed with []: the device passes the caller's array, a CPU simulation may pass
// one that checks every index.
enum { TK_BAD_OFF = 0 };
template <class Off>
TK_HD uint32_t tk_rows_off_check(Off tok_off, uint64_t d, uint64_t n_docs, uint64_t n_tokens, uint64_t* a, uint64_t* b, unsigned long long* bad) {
    *a = tok_off[d];
    *b = d < n_docs ? tok_off[d + 1] : n_tokens;
    const uint32_t why = tk_rows_off_error(*a, *b, d, n_docs);
    if (why) tk_report_min(bad, tk_rows_bad_key(d, n_docs, why));
    return why;
}
// The stream position entry d marks, or all ones: the start of a document that owns a position (with k == 0 an empty document owns none),
// and -- entry n_docs -- the start of the padding.  Guarded by a <= n_tokens: whatever tok_off holds, a mark lies below M.
TK_HD uint64_t tk_rows_mark_at(uint64_t a, uint64_t b, uint64_t d, const TkRows& r) {
    if (a > r.n_tokens) return ~0ull;
    const uint64_t p = tk_rows_out_off(a, d, r.k);
    if (d == r.n_docs) return a == r.n_tokens && p < r.M ? p : ~0ull;
    return (r.k || b > a) && p < r.M ? p : ~0ull;
}

// The one search of the row, padded and samples passes: the last index in [lo, hi) whose key is <= x, lo if there is none.  key[mid] is
// the key of entry mid (doc_row, pstart, or a reader that computes it); the keys do not descend.  Among entries with one key -- a run of
// empty documents, of empty parts -- that is the last: the one that is not empty, the one that owns the position.
template <class Key>
TK_HD uint64_t tk_last_le(Key key, uint64_t lo, uint64_t hi, uint64_t x) {
    uint64_t a = lo, b = hi;  // first index with key > x
    while (a < b) {
        const uint64_t mid = (a + b) >> 1;
        if (key[mid] <= x) a = mid + 1;
        else b = mid;
    }
    return a > lo ? a - 1 : lo;
}
// The document a stream position j < S belongs to, searched in [lo, hi): the last d there with out_off(d) <= j (out_off(lo) <= j)
template <class Off>
struct TkRowsOutOff {
    Off tok_off;
    uint32_t k;
    TK_HD uint64_t operator[](uint64_t d) const { return tk_rows_out_off(tok_off[d], d, k); }
};
template <class Off>
TK_HD uint64_t tk_rows_last_doc(Off tok_off, uint64_t lo, uint64_t hi, uint32_t k, uint64_t j) { return tk_last_le(TkRowsOutOff<Off>{tok_off, k}, lo, hi, j); }
// The width of padded rows (tk_pad_size, tk_smp_size): the longest rounded up to a multiple of width_multiple, at most max_len (0: max_len)
TK_HD uint32_t tk_row_width(uint32_t max_len, uint32_t width_multiple, uint32_t longest) {
    if (!width_multiple) return max_len;
    const uint64_t w = ((uint64_t)longest + width_multiple - 1) / width_multiple * width_multiple;
    return w < max_len ? (uint32_t)w : max_len;
}

// Where the element at position p of document d (stream range [start, next)) comes from: TK_ROWS_BOS, TK_ROWS_EOS, or the body -- then
// *tok is the index into tokens.
enum { TK_ROWS_BODY = 0, TK_ROWS_BOS, TK_ROWS_EOS };
TK_HD int tk_rows_source(const TkRows& r, uint64_t d, uint64_t start, uint64_t next, uint64_t p, uint64_t* tok) {
    if (r.has_bos && p == start) return TK_ROWS_BOS;
    if (r.k > r.has_bos && p + 1 == next) return TK_ROWS_EOS;
    *tok = p - d * r.k - r.has_bos;  // = tok_off[d] + (p - start) - has_bos
    return TK_ROWS_BODY;
}

// pos restarts at a document's start (the padding's: S) and at a row's start; a segment starts where it is 0
TK_HD uint32_t tk_rows_pos(uint64_t p, uint64_t start, uint64_t row_start) { return (uint32_t)(p - (start > row_start ? start : row_start)); }

// Eight positions from i0 on (a multiple of 8, below M): which of them are written, which are row starts (rem = i0 % L)
TK_HD uint32_t tk_rows_valid_bits(uint64_t i0, uint64_t M) { return M - i0 >= 8u ? 0xFFu : (1u << (uint32_t)(M - i0)) - 1u; }
TK_HD uint32_t tk_rows_row_bits(uint32_t rem, uint32_t L) {
    uint32_t bits = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t j = 0; j < 8u; ++j) {
        bits |= (rem == 0u ? 1u : 0u) << j;
        if (++rem == L) rem = 0u;
    }
    return bits;
}
// segment starts among them: marked positions (document starts, the padding's start) and row starts, a coincidence counted once
TK_HD uint32_t tk_rows_seg_bits(uint32_t marks, uint32_t rows, uint32_t valid) { return (marks | rows) & valid; }

// The documents a workgroup's lanes search between: those of its first stream position b0 and of its last (none where b0 lies in the padding)
template <class Off>
TK_HD void tk_rows_block_docs(const TkRows& r, Off tok_off, uint64_t b0, uint64_t block, uint64_t* d_lo, uint64_t* d_hi) {
    *d_lo = *d_hi = 0;
    if (b0 < r.S) {
        const uint64_t last = b0 + block <= r.S ? b0 + block - 1 : r.S - 1;
        *d_lo = tk_rows_last_doc(tok_off, 0, r.n_docs, r.k, b0);
        *d_hi = tk_rows_last_doc(tok_off, *d_lo, r.n_docs, r.k, last) + 1;
    }
}
// A lane of the write pass: ids, documents and positions of the eight stream positions from i0 < M on (i0 a multiple of 8; positions at and
// past M left as padding), and as bits which of them start a segment and which a row.  The lane's first position belongs to a document in
// [d_lo, d_hi); from there it walks along the documents: a position at or beyond the current document's end moves on to the next one that
// owns a position.  `tok` fetches body tokens: tok.one(i) is tokens[i], and tok.eight(i, out) fetches tokens[i .. i + 8) as two 16-byte
// words where their address allows it and says whether it did -- asked only where the stream is the token array (k == 0) and all eight
// exist.  The device passes the caller's arrays, the CPU simulation ones that check every index.
template <class Tok, class Off>
TK_HD void tk_rows_lane(const TkRows& r, const Tok& tok, Off tok_off, uint64_t d_lo, uint64_t d_hi, uint64_t i0, uint32_t id[8], uint32_t dc[8], uint32_t ps[8],
                        uint32_t* seg_out, uint32_t* rows_out) {
    uint64_t d = 0, start = r.S, next = r.S;  // (beyond the stream: the padding, one segment from S on)
    if (i0 < r.S) {
        d = tk_rows_last_doc(tok_off, d_lo, d_hi, r.k, i0);
        start = tk_rows_out_off(tok_off[d], d, r.k);
        next = tk_rows_out_off(tok_off[d + 1], d + 1, r.k);
    }
    uint32_t tw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const bool wide = r.k == 0 && i0 + 8 <= r.n_tokens && tok.eight(i0, tw);
    uint32_t rem = (uint32_t)i0 % r.seq_len, seg = 0, rows = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < 8; ++j) {
        const uint64_t p = i0 + j;
        id[j] = r.pad;
        dc[j] = TK_ROWS_NONE;
        ps[j] = 0;
        if (p < r.M) {
            if (p < r.S) {
                if (p >= next) {  // the next document that owns a position: the one after, unless that one is empty
                    ++d;
                    if (tk_rows_out_off(tok_off[d + 1], d + 1, r.k) <= p) d = tk_rows_last_doc(tok_off, d + 1, d_hi, r.k, p);
                    start = tk_rows_out_off(tok_off[d], d, r.k);
                    next = tk_rows_out_off(tok_off[d + 1], d + 1, r.k);
                }
                uint64_t t = 0;
                const int src = tk_rows_source(r, d, start, next, p, &t);
                id[j] = src == TK_ROWS_BOS ? r.bos : src == TK_ROWS_EOS ? r.eos : wide ? tw[j] : tok.one(t);
                dc[j] = (uint32_t)d;
            } else {
                start = r.S;
            }
            ps[j] = tk_rows_pos(p, start, p - rem);
            seg |= (ps[j] == 0u ? 1u : 0u) << j;
            rows |= (rem == 0u ? 1u : 0u) << j;
        }
        if (++rem == r.seq_len) rem = 0u;
    }
    *seg_out = seg;
    *rows_out = rows;
}
