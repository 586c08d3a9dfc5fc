// The row passes (tiktoken_amd/csrc/tk_rows.h) on the CPU: the plain C++ they are made of -- tk_rows_rule.h: the shape, the check of tok_off,
// the document of a position, where an element comes from, the pos rule, what counts as a segment start -- compiled for the host and
// driven the way the kernels drive it: lanes of eight positions, workgroups of `block` positions.  Test infrastructure only
// (tests/test_rows_sim.py builds it).
#include <stdint.h>

#include <vector>

#include "../../tiktoken_amd/csrc/tk_rows_rule.h"

extern "C" {
// Statement by statement what the kernels do with the shared rule.  ids / doc / pos: room for M (+ 8), cu: n_docs + R + 4, row_seg: R + 1;
// counts: {R, n_segs, S, n_tail, M}.  Every access to tokens and tok_off is checked here: -1 if one lies out of bounds.
// Returns 0; 1 .. 3: tk_rows_shape's refusal; 16 + tk_rows_bad_key: tok_off is refused.
int64_t rows_sim(const uint32_t* tokens_in, uint64_t T, const uint64_t* tok_off_in, uint64_t n_docs, uint32_t L, uint32_t bos, uint32_t eos, uint32_t pad, int drop_last,
                 uint32_t block, uint32_t* ids_out, uint32_t* doc_out, uint32_t* pos_out, uint32_t* cu, uint32_t* row_seg, uint64_t* counts) {
    TkRows r;
    const int refused = tk_rows_shape(T, n_docs, L, bos, eos, pad, drop_last != 0, &r);
    if (refused) return refused;
    bool oob = false;
    std::vector<uint64_t> off_copy(tok_off_in, tok_off_in + n_docs + 1);
    const uint64_t* tok_off = off_copy.data();
    auto off_at = [&](uint64_t d) -> uint64_t {
        if (d > n_docs) {
            oob = true;
            return 0;
        }
        return tok_off[d];
    };
    auto token_at = [&](uint64_t t) -> uint32_t {
        if (t >= T) {
            oob = true;
            return 0;
        }
        return tokens_in[t];
    };
    // tk_k_rows_mark
    std::vector<uint32_t> bm(r.M / 32 + 4, 0u);
    uint64_t bad = ~0ull;
    for (uint64_t d = 0; d <= n_docs; ++d) {
        const uint64_t a = off_at(d), b = d < n_docs ? off_at(d + 1) : r.n_tokens;
        const uint32_t why = tk_rows_off_error(a, b, d, r.n_docs);
        if (why) {
            const uint64_t key = tk_rows_bad_key(d, r.n_docs, why);
            bad = key < bad ? key : bad;
        }
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
    uint64_t carry = 0;
    for (uint64_t blk = 0; blk < nb; ++blk) {
        const uint64_t at = carry;
        carry += cnt[blk];
        cnt[blk] = at;
    }
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
        if (b0 < r.S) {
            const uint64_t last = b0 + block <= r.S ? b0 + block - 1 : r.S - 1;
            d_lo = tk_rows_last_doc(tok_off, 0, r.n_docs, r.k, b0);
            d_hi = tk_rows_last_doc(tok_off, d_lo, r.n_docs, r.k, last) + 1;
        }
        uint64_t at = cnt[blk];  // (the lanes in order: the exclusive scan of their counts)
        for (uint32_t l = 0; l < lanes; ++l) {
            const uint64_t i0 = b0 + l * 8ull;
            uint32_t seg = 0, rows = 0;
            if (i0 < r.M) {
                uint64_t d = 0, start = r.S, next = r.S;
                if (i0 < r.S) {
                    d = tk_rows_last_doc(tok_off, d_lo, d_hi, r.k, i0);
                    start = tk_rows_out_off(off_at(d), d, r.k);
                    next = tk_rows_out_off(off_at(d + 1), d + 1, r.k);
                }
                uint32_t rem = (uint32_t)i0 % r.seq_len;
                for (int j = 0; j < 8; ++j) {
                    const uint64_t p = i0 + j;
                    uint32_t id = r.pad, dc = TK_ROWS_NONE, ps = 0;
                    if (p < r.M) {
                        if (p < r.S) {
                            if (p >= next) {
                                ++d;
                                if (tk_rows_out_off(off_at(d + 1), d + 1, r.k) <= p) d = tk_rows_last_doc(tok_off, d + 1, d_hi, r.k, p);
                                start = tk_rows_out_off(off_at(d), d, r.k);
                                next = tk_rows_out_off(off_at(d + 1), d + 1, r.k);
                            }
                            uint64_t t = 0;
                            const int src = tk_rows_source(r, d, start, next, p, &t);
                            id = src == TK_ROWS_BOS ? r.bos : src == TK_ROWS_EOS ? r.eos : token_at(t);
                            dc = (uint32_t)d;
                        } else {
                            start = r.S;
                        }
                        ps = tk_rows_pos(p, start, p - rem);
                        seg |= (ps == 0u ? 1u : 0u) << j;
                        rows |= (rem == 0u ? 1u : 0u) << j;
                        ids_out[p] = id;
                        doc_out[p] = dc;
                        pos_out[p] = ps;
                    }
                    if (++rem == r.seq_len) rem = 0u;
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
