// The padded passes (tiktoken_amd/csrc/tk_padded.h) on the CPU: the plain C++ they are made of -- tk_padded_rule.h: what a spec may say, the
// rows of a document, the width, a row's body, the document of a row, where a column's element comes from -- compiled for the host and
// driven the way the kernels drive it: lanes of eight positions, workgroups of `block` positions.  Test infrastructure only
// (tests/test_padded_sim.py builds it).
#include <stdint.h>

#include "../../tiktoken_amd/csrc/tk_padded_rule.h"
#include "sim_readers.h"

extern "C" {
// The figures of a call: counts = {R, W}.  Returns 0; 1 .. 8: tk_pad_shape's / tk_pad_size's refusal; 16 + tk_rows_bad_key: tok_off is
// refused; -1: an index out of bounds.  doc_row: room for n_docs + 1.  Nothing else is written: the caller sizes the other arrays from counts and calls padded_sim.
int64_t padded_sim_count(uint64_t T, const uint64_t* tok_off, uint64_t n_docs, uint32_t max_len, uint32_t stride, uint32_t width_multiple, uint32_t bos, uint32_t eos,
                         uint32_t pad, uint32_t flags, uint32_t* doc_row, uint64_t* counts) {
    TkPad p;
    const int refused = tk_pad_shape(T, n_docs, max_len, stride, width_multiple, bos, eos, pad, flags, &p);
    if (refused) return refused;
    // tk_k_pad_count
    bool oob = false;
    const SimOffsets off{tok_off, n_docs, &oob};
    unsigned long long bad = ~0ull;
    uint32_t longest = 0;
    for (uint64_t d = 0; d <= n_docs; ++d) {
        const uint32_t l = tk_pad_count_entry(p, off, d, doc_row, &bad);
        longest = l > longest ? l : longest;
    }
    if (oob) return -1;
    // tk_k_pad_scan
    const uint64_t carry = sim_scan(doc_row, n_docs);
    doc_row[n_docs] = (uint32_t)carry;
    // the host
    if (bad != ~0ull) return 16 + (int64_t)bad;
    const int too_big = tk_pad_size(&p, carry, longest);
    counts[0] = p.R;
    counts[1] = p.W;
    return too_big;
}

// tk_k_pad_rows and tk_k_pad_write after padded_sim_count has accepted the call and left doc_row: through tk_pad_row_entry,
// tk_pad_block_docs and tk_pad_lane -- the functions the kernels themselves call -- with the kernels' stores.  ids / mask: room for R * W,
// len / row_doc / row_tok: R.  tok_off holds off_len entries and doc_row row_len (n_docs + 1 each, unless a test hands in less): -1 if an
// index into them or into tokens lies out of bounds.
int64_t padded_sim(const uint32_t* tokens, uint64_t T, const uint64_t* tok_off_in, uint64_t off_len, uint64_t n_docs, uint32_t max_len, uint32_t stride, uint32_t width_multiple,
                   uint32_t bos, uint32_t eos, uint32_t pad, uint32_t flags, uint32_t block, const uint32_t* doc_row_in, uint64_t row_len, uint64_t R, uint32_t W,
                   uint32_t* ids_out, uint8_t* mask_out, uint32_t* len, uint32_t* row_doc, uint32_t* row_tok) {
    TkPad p;
    if (tk_pad_shape(T, n_docs, max_len, stride, width_multiple, bos, eos, pad, flags, &p)) return -3;
    p.R = R;
    p.W = W;  // (what padded_sim_count settled)
    bool oob = false;
    if (!off_len) return -1;
    const SimOffsets tok_off{tok_off_in, off_len - 1, &oob};  // (entries [0, off_len - 1])
    const SimArray<uint32_t> doc_row{doc_row_in, row_len, &oob};
    const SimTokens tok{tokens, T, &oob};
    // tk_k_pad_rows
    for (uint64_t r = 0; r < p.R; ++r) tk_pad_row_entry(p, tok_off, doc_row, r, len, row_doc, row_tok);
    if (oob) return -1;  // (nothing further is computed from what was not read)
    // tk_k_pad_write
    const uint32_t N = (uint32_t)(p.R * p.W), nb = (uint32_t)(((uint64_t)N + block - 1) / block);
    for (uint32_t blk = 0; blk < nb; ++blk) {
        const uint32_t b0 = blk * block;
        uint64_t lo = 0, hi = 0;
        tk_pad_block_docs(p, doc_row, b0, block, N, &lo, &hi);
        if (hi > n_docs) return -1;
        for (uint32_t t = 0; t < block / 8; ++t) {
            if (N - b0 <= t * 8u) continue;
            const uint32_t i0 = b0 + t * 8u;
            uint32_t id[8];
            uint64_t mask;
            tk_pad_lane(p, tok, tok_off, doc_row, lo, hi, i0, N, id, &mask);
            for (uint32_t j = 0; j < 8; ++j)
                if (N - i0 > j) {
                    ids_out[i0 + j] = id[j];
                    mask_out[i0 + j] = (uint8_t)(mask >> (8 * j));
                }
        }
    }
    return oob ? -1 : 0;
}
}
