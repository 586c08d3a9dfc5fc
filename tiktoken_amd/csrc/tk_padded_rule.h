// Padded model inputs from a packed batch: the parts of the device passes of tk_padded.h that are plain C++ -- what a tk_pad_spec may say,
// how many rows a document owns and how long its longest one is, the width, which body tokens a row holds, which document a row belongs
// to, and where the element in a column comes from (bos, body, eos or padding).  Compiles for the host too: tests/test_padded_sim.py drives
// them lane by lane on the CPU.  The rule itself is stated in include/tiktoken_amd.h (tk_pad_batch_device).
#pragma once
#include <stdint.h>

#include "tk_rows_rule.h"  // TK_ROWS_NONE, tk_rows_off_check, tk_last_le, tk_row_width

#define TK_PADF_WINDOWS 1u  // (= TK_PAD_WINDOWS .. TK_PAD_IDS16 of the C ABI; tk_api.hip asserts it)
#define TK_PADF_KEEP_TAIL 2u
#define TK_PADF_LEFT 4u
#define TK_PADF_IDS16 8u

struct TkPad {
    uint64_t n_tokens, n_docs;  // T, the documents
    uint32_t max_len, stride, width_multiple, bos, eos, pad, flags;
    uint32_t k, has_bos, has_eos;  // elements added per row; 1 when there is a bos / an eos
    uint32_t c, step;              // body capacity of a row; with WINDOWS the distance between the starts of consecutive rows
    uint64_t R;                    // rows (tk_pad_size: known after the count)
    uint32_t W;                    // width
};

// What the spec and the figures of a call alone decide.  0, or why it is refused: 1 max_len == 0 or no room for a body token, 2 stride >= c,
// 3 stride without WINDOWS, 4 KEEP_TAIL with WINDOWS, 5 too many documents (doc_row and row_doc are 32-bit), 6 too many tokens.
TK_HD int tk_pad_shape(uint64_t n_tokens, uint64_t n_docs, uint32_t max_len, uint32_t stride, uint32_t width_multiple, uint32_t bos, uint32_t eos, uint32_t pad,
                       uint32_t flags, TkPad* p) {
    p->n_tokens = n_tokens;
    p->n_docs = n_docs;
    p->max_len = max_len;
    p->stride = stride;
    p->width_multiple = width_multiple;
    p->bos = bos;
    p->eos = eos;
    p->pad = pad;
    p->flags = flags;
    p->has_bos = bos != TK_ROWS_NONE ? 1u : 0u;
    p->has_eos = eos != TK_ROWS_NONE ? 1u : 0u;
    p->k = p->has_bos + p->has_eos;
    p->R = 0;
    p->W = 0;
    if (max_len <= p->k) return 1;
    p->c = max_len - p->k;
    if (stride >= p->c) return 2;
    p->step = p->c - stride;
    if (stride && !(flags & TK_PADF_WINDOWS)) return 3;
    if ((flags & TK_PADF_KEEP_TAIL) && (flags & TK_PADF_WINDOWS)) return 4;
    if (n_docs >= 0xFFFFFFFFull) return 5;
    if (n_tokens >> 32) return 6;
    return 0;
}

// The rows document d owns (n = its body tokens): one, or with WINDOWS 1 + ceil((n - c) / step) when it does not fit
TK_HD uint64_t tk_pad_windows(const TkPad& p, uint64_t n) {
    if (!(p.flags & TK_PADF_WINDOWS) || n <= p.c) return 1;
    return 1 + (n - p.c + p.step - 1) / p.step;
}
// len of its longest row: the first one
TK_HD uint32_t tk_pad_longest(const TkPad& p, uint64_t n) { return p.k + (uint32_t)(n < p.c ? n : p.c); }

// R and W once the count is known.  0, or why it is refused: 7 R >= 2^32, 8 R * W >= 2^32.
TK_HD int tk_pad_size(TkPad* p, uint64_t R, uint32_t longest) {
    p->R = R;
    p->W = tk_row_width(p->max_len, p->width_multiple, longest);
    if (R >> 32) return 7;
    if ((R * p->W) >> 32) return 8;
    return 0;
}

// Row j of a document of n body tokens: *tok = its first body token (an index inside the document), returns how many it holds
TK_HD uint32_t tk_pad_row(const TkPad& p, uint64_t n, uint64_t j, uint64_t* tok) {
    if (p.flags & TK_PADF_WINDOWS) {
        const uint64_t t = n <= p.c ? 0 : j * p.step;  // (j == 0 when the document fits)
        *tok = t;
        return (uint32_t)(n - t < p.c ? n - t : p.c);
    }
    *tok = (p.flags & TK_PADF_KEEP_TAIL) && n > p.c ? n - p.c : 0;
    return (uint32_t)(n < p.c ? n : p.c);
}

// Entry d <= n_docs of the count pass (tk_k_pad_count): the entry of tok_off is checked (nothing is indexed with it) and, for a document,
// doc_row[d] = the rows it owns (one where its entry offends).  Returns the len of the document's longest row, 0 for entry n_docs.
template <class Off>
TK_HD uint32_t tk_pad_count_entry(const TkPad& p, Off tok_off, uint64_t d, uint32_t* doc_row, unsigned long long* words) {
    uint64_t a, b;
    const uint32_t why = tk_rows_off_check(tok_off, d, p.n_docs, p.n_tokens, &a, &b, words + TK_BAD_OFF);
    if (d >= p.n_docs) return 0u;
    const uint64_t n = why ? 0 : b - a;           // (no error here: a <= b)
    doc_row[d] = (uint32_t)tk_pad_windows(p, n);  // (at most n, and n < 2^32 unless another entry is reported)
    return tk_pad_longest(p, n);
}

// The document row r < R belongs to, searched in [lo, hi) (doc_row[lo] <= r): every document owns a row, so doc_row ascends strictly
template <class Rows>
TK_HD uint64_t tk_pad_doc_of_row(Rows doc_row, uint64_t lo, uint64_t hi, uint64_t r) { return tk_last_le(doc_row, lo, hi, r); }

// A row as the write pass carries it from column to column: its document, the rows of that document, where its body lies in tokens
struct TkPadRow {
    uint64_t d, first, next_first;  // the document; its first row, the next document's
    uint64_t off, n;                // tok_off[d], the document's body tokens
    uint64_t src;                   // index into tokens of the row's first body token
    uint64_t tok;                   // the same inside the document (row_tok)
    uint32_t len;                   // k + body tokens held
};
TK_HD void tk_pad_row_set(const TkPad& p, uint64_t r, TkPadRow* w) {
    w->len = p.k + tk_pad_row(p, w->n, r - w->first, &w->tok);
    w->src = w->off + w->tok;
}
// row r of document d (doc_row[d] <= r < doc_row[d + 1]; d < n_docs, so entry d + 1 of both arrays exists)
template <class Off, class Rows>
TK_HD void tk_pad_row_load(const TkPad& p, Off tok_off, Rows doc_row, uint64_t d, uint64_t r, TkPadRow* w) {
    w->d = d;
    w->first = doc_row[d];
    w->next_first = doc_row[d + 1];
    w->off = tok_off[d];
    w->n = tok_off[d + 1] - w->off;
    tk_pad_row_set(p, r, w);
}
// from row r - 1 to row r < R: the same document's next window, or the first row of the next document
template <class Off, class Rows>
TK_HD void tk_pad_row_next(const TkPad& p, Off tok_off, Rows doc_row, uint64_t r, TkPadRow* w) {
    if (r >= w->next_first) tk_pad_row_load(p, tok_off, doc_row, w->d + 1, r, w);
    else tk_pad_row_set(p, r, w);
}
// Row r < R of the per-row pass (tk_k_pad_rows): its len, its document and its first body token (inside the document)
template <class Off, class Rows>
TK_HD void tk_pad_row_entry(const TkPad& p, Off tok_off, Rows doc_row, uint64_t r, uint32_t* len, uint32_t* row_doc, uint32_t* row_tok) {
    TkPadRow w;
    tk_pad_row_load(p, tok_off, doc_row, tk_pad_doc_of_row(doc_row, 0, p.n_docs, r), r, &w);
    len[r] = w.len;
    row_doc[r] = (uint32_t)w.d;
    row_tok[r] = (uint32_t)w.tok;
}

// Where the element in column col < W of a row of `len` elements comes from; for the body *t is the index of the token inside the row's body
enum { TK_PAD_SRC_PAD = 0, TK_PAD_SRC_BOS, TK_PAD_SRC_EOS, TK_PAD_SRC_BODY };
TK_HD int tk_pad_source(const TkPad& p, uint32_t len, uint32_t col, uint32_t* t) {
    uint32_t e = col;
    if (p.flags & TK_PADF_LEFT) {
        if (col < p.W - len) return TK_PAD_SRC_PAD;
        e = col - (p.W - len);
    } else if (col >= len) {
        return TK_PAD_SRC_PAD;
    }
    if (p.has_bos && e == 0) return TK_PAD_SRC_BOS;
    if (p.has_eos && e + 1 == len) return TK_PAD_SRC_EOS;
    *t = e - p.has_bos;
    return TK_PAD_SRC_BODY;
}
// Eight columns from col on lie in one row and are all body tokens: *t = the first one's index inside the row's body
TK_HD bool tk_pad_all_body(const TkPad& p, uint32_t len, uint32_t col, uint32_t* t) {
    if ((uint64_t)col + 8 > p.W) return false;
    const uint32_t lead = (p.flags & TK_PADF_LEFT) ? p.W - len : 0u;  // columns in front of the elements
    if (col < lead + p.has_bos) return false;
    if ((uint64_t)col + 8 > (uint64_t)lead + len - p.has_eos) return false;
    *t = col - lead - p.has_bos;
    return true;
}

// A lane of the write pass: the ids and the mask bytes (byte j = 1 on an element) of the eight positions from i0 < N = R * W on, positions
// at and past N left as padding.  The lane's first row belongs to a document in [d_lo, d_hi) (doc_row[d_lo] <= i0 / W); from there it steps
// from row to row.  N is below 2^32, so positions, rows and columns are 32-bit.  `tok` fetches body tokens: tok.one(i) is tokens[i], and
// tok.eight(i, out) fetches tokens[i .. i + 8) as two 16-byte words where their address allows it and says whether it did -- the device
// passes the caller's arrays, the CPU simulation ones that check every index (tok_off and doc_row, indexed with [], too).
template <class Tok, class Off, class Rows>
TK_HD void tk_pad_lane(const TkPad& p, const Tok& tok, Off tok_off, Rows doc_row, uint64_t d_lo, uint64_t d_hi, uint32_t i0, uint32_t N,
                       uint32_t id[8], uint64_t* mask_out) {
    uint32_t r = i0 / p.W, col = i0 - r * p.W;
    TkPadRow w;
    tk_pad_row_load(p, tok_off, doc_row, tk_pad_doc_of_row(doc_row, d_lo, d_hi, r), r, &w);
    uint32_t t0 = 0, tw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const bool wide = tk_pad_all_body(p, w.len, col, &t0) && tok.eight(w.src + t0, tw);
    uint64_t mask = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < 8; ++j) {
        id[j] = p.pad;
        if (N - i0 > (uint32_t)j) {
            uint32_t t = 0;
            const int src = tk_pad_source(p, w.len, col, &t);
            if (src != TK_PAD_SRC_PAD) {
                id[j] = src == TK_PAD_SRC_BOS ? p.bos : src == TK_PAD_SRC_EOS ? p.eos : wide ? tw[j] : tok.one(w.src + t);
                mask |= 1ull << (8 * j);
            }
            if (++col == p.W) {
                col = 0u;
                if (++r < p.R) tk_pad_row_next(p, tok_off, doc_row, r, &w);
            }
        }
    }
    *mask_out = mask;
}
// The documents a workgroup's lanes search between: those of the rows of its first position b0 < N and of its last
template <class Rows>
TK_HD void tk_pad_block_docs(const TkPad& p, Rows doc_row, uint32_t b0, uint32_t block, uint32_t N, uint64_t* d_lo, uint64_t* d_hi) {
    const uint32_t last = N - b0 > block ? b0 + block - 1 : N - 1;
    *d_lo = tk_pad_doc_of_row(doc_row, 0, p.n_docs, b0 / p.W);
    *d_hi = tk_pad_doc_of_row(doc_row, *d_lo, p.n_docs, last / p.W) + 1;
}
