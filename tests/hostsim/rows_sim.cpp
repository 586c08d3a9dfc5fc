// The row passes (tiktoken_amd/csrc/tk_rows.h) on the CPU: the plain C++ they are made of -- tk_rows_rule.h: the shape, the check of tok_off,
// the documents of a workgroup, a lane of the write pass -- compiled for the host and driven the way the kernels drive it: lanes of eight
// positions, workgroups of `block` positions.  The write pass runs through tk_rows_block_docs and tk_rows_lane, the functions the kernel
// itself calls.  Test infrastructure only (tests/test_rows_sim.py builds it).
#include <stdint.h>

#include <vector>

#include "../../tiktoken_amd/csrc/tk_rows_rule.h"
#include "sim_readers.h"

extern "C" {
// The search every pass shares (tk_last_le) over `n` keys, and the width rule of the padded and the samples passes, each on its own
int64_t rows_sim_last_le(const uint64_t* keys, uint64_t n, uint64_t lo, uint64_t hi, uint64_t x) {
    bool oob = false;
    const SimArray<uint64_t> k{keys, n, &oob};
    const uint64_t at = tk_last_le(k, lo, hi, x);
    return oob ? -1 : (int64_t)at;
}
uint32_t rows_sim_row_width(uint32_t max_len, uint32_t width_multiple, uint32_t longest) { return tk_row_width(max_len, width_multiple, longest); }

// The passes in the kernels' order, with the kernels' stores.  ids / doc / pos: room for M (+ 8), cu: n_docs + R + 4, row_seg: R + 1;
// counts: {R, n_segs, S, n_tail, M}.  Every access to tokens and tok_off is checked here: -1 if one lies out of bounds.
// Returns 0; 1 .. 3: tk_rows_shape's refusal; 16 + tk_rows_bad_key: tok_off is refused.
int64_t rows_sim(const uint32_t* tokens_in, uint64_t T, const uint64_t* tok_off_in, uint64_t n_docs, uint32_t L, uint32_t bos, uint32_t eos, uint32_t pad, int drop_last,
                 uint32_t block, uint32_t* ids_out, uint32_t* doc_out, uint32_t* pos_out, uint32_t* cu, uint32_t* row_seg, uint64_t* counts) {
    TkRows r;
    const int refused = tk_rows_shape(T, n_docs, L, bos, eos, pad, drop_last != 0, &r);
    if (refused) return refused;
    bool oob = false;
    const SimOffsets tok_off{tok_off_in, n_docs, &oob};
    const SimTokens tok{tokens_in, T, &oob};
    // tk_k_rows_mark
    std::vector<uint32_t> bm(r.M / 32 + 4, 0u);
    unsigned long long bad = ~0ull;
    for (uint64_t d = 0; d <= n_docs; ++d) {
        uint64_t a, b;
        tk_rows_off_check(tok_off, d, r.n_docs, r.n_tokens, &a, &b, &bad);
        const uint64_t p = tk_rows_mark_at(a, b, d, r);
        if (p != ~0ull) {
            if ((p >> 5) >= bm.size()) return -1;
            bm[p >> 5] |= 1u << (p & 31u);
        }
    }
    const uint8_t* marks = (const uint8_t*)bm.data();  // (little endian, as the device)
    const uint32_t lanes = block / 8;
    const uint64_t nb = (r.M + block - 1) / block;
    // tk_k_rows_count
    std::vector<uint64_t> cnt(nb + 1, 0);
    for (uint64_t blk = 0; blk < nb; ++blk)
        for (uint32_t l = 0; l < lanes; ++l) {
            const uint64_t i0 = blk * block + l * 8ull;
            uint32_t bits = 0;
            if (i0 < r.M) bits = tk_rows_seg_bits(marks[i0 >> 3], tk_rows_row_bits((uint32_t)i0 % r.seq_len, r.seq_len), tk_rows_valid_bits(i0, r.M));
            cnt[blk] += (uint32_t)__builtin_popcount(bits);
        }
    // tk_k_rows_scan
    const uint64_t carry = sim_scan(cnt.data(), nb);
    if (carry > n_docs + r.R + 3) return -1;
    cu[carry] = (uint32_t)r.M;
    if (r.R * r.seq_len == r.M) row_seg[r.R] = (uint32_t)carry;
    counts[0] = r.R;
    counts[1] = carry;
    counts[2] = r.S;
    counts[3] = drop_last ? r.S - r.R * r.seq_len : 0;
    counts[4] = r.M;
    // tk_k_rows_write
    if (bad != ~0ull) return 16 + (int64_t)bad;
    for (uint64_t blk = 0; blk < nb; ++blk) {
        const uint64_t b0 = blk * block;
        uint64_t d_lo = 0, d_hi = 0;
        tk_rows_block_docs(r, tok_off, b0, block, &d_lo, &d_hi);
        if (d_hi > n_docs) return -1;
        uint64_t at = cnt[blk];  // (the lanes in order: the exclusive scan of their counts)
        for (uint32_t l = 0; l < lanes; ++l) {
            const uint64_t i0 = b0 + l * 8ull;
            uint32_t seg = 0, rows = 0;
            if (i0 < r.M) {
                uint32_t id[8], dc[8], ps[8];
                tk_rows_lane(r, tok, tok_off, d_lo, d_hi, i0, id, dc, ps, &seg, &rows);
                for (uint32_t j = 0; j < 8; ++j)
                    if (i0 + j < r.M) {
                        ids_out[i0 + j] = id[j];
                        doc_out[i0 + j] = dc[j];
                        pos_out[i0 + j] = ps[j];
                    }
            }
            while (seg) {
                const uint32_t j = (uint32_t)__builtin_ctz(seg);
                seg &= seg - 1u;
                if (at > n_docs + r.R + 3 || (i0 + j) / r.seq_len > r.R) return -1;
                cu[at] = (uint32_t)(i0 + j);
                if ((rows >> j) & 1u) row_seg[(uint32_t)(i0 + j) / r.seq_len] = (uint32_t)at;
                ++at;
            }
        }
        if (blk + 1 < nb ? at != cnt[blk + 1] : at != carry) return -2;  // (the count pass and the write pass agree on what a segment start is)
    }
    return oob ? -1 : 0;
}
}
