// Training rows from a packed batch: the parts of the device passes of tk_rows.h that are plain C++ -- the shape of the result, what a
// tok_off entry must satisfy, which document a stream position belongs to, where a stream element comes from (bos, body, eos or pad), the
// pos rule and what counts as a segment start.  Compiles for the host too: tests/test_rows_sim.py drives them lane by lane on the CPU.
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
// The stream position entry d marks, or all ones: the start of a document that owns a position (with k == 0 an empty document owns none),
// and -- entry n_docs -- the start of the padding.  Guarded by a <= n_tokens: whatever tok_off holds, a mark lies below M.
TK_HD uint64_t tk_rows_mark_at(uint64_t a, uint64_t b, uint64_t d, const TkRows& r) {
    if (a > r.n_tokens) return ~0ull;
    const uint64_t p = tk_rows_out_off(a, d, r.k);
    if (d == r.n_docs) return a == r.n_tokens && p < r.M ? p : ~0ull;
    return (r.k || b > a) && p < r.M ? p : ~0ull;
}

// The document a stream position j < S belongs to, searched in [lo, hi): the last d there with out_off(d) <= j (out_off(lo) <= j).  Behind a
// run of empty documents with k == 0 that is the one that is not empty -- the last of those that start at one position.
TK_HD uint64_t tk_rows_last_doc(const uint64_t* tok_off, uint64_t lo, uint64_t hi, uint32_t k, uint64_t j) {
    uint64_t a = lo, b = hi;  // first index with out_off > j
    while (a < b) {
        const uint64_t mid = (a + b) >> 1;
        if (tk_rows_out_off(tok_off[mid], mid, k) <= j) a = mid + 1;
        else b = mid;
    }
    return a > lo ? a - 1 : lo;
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
