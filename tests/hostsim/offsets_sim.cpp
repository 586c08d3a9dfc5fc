// The token-span passes (tiktoken_amd/csrc/tk_offsets.h) on the CPU: the plain C++ they are made of -- tk_span_rule.h: the per-id char word,
// the keys a document start travels in, the clamp, the lane body of the strict UTF-8 check -- compiled for the host and driven the way the kernels
// drive it: lanes of eight tokens, workgroups of `block` tokens, the batch; sixteen bytes per lane of the UTF-8 check, lanes in any order.
// Test infrastructure only (tests/test_offsets_sim.py builds it).
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../tiktoken_amd/csrc/tk_span_rule.h"

extern "C" {
uint32_t ofs_char_word(const uint8_t* b, uint32_t len) { return tk_char_word(b, len); }

// The span passes over a packed batch: lens / words per token (the two tables' entries), tok_off[n_docs + 1]; the batch runs in ranges of
// `range` tokens (a multiple of `block`; 0: one range), workgroups of `block` tokens, lanes of eight.  Statement by statement what the
// kernels do with the shared rule: tk_k_span_len (a lane's sums and its last document start; tk_span_key, the workgroup's maximum),
// tk_k_span_scan (the bases; tk_span_mark_at through a running maximum; the carry words between ranges), tk_k_span_write (the key of the
// lanes before, or the workgroup's doc_b / doc_c; the first document at a position gets its offsets), tk_k_span_docs (the other
// documents at that position).  Returns 0, or 1 + the first document of 4 GiB or more.
uint64_t ofs_spans(const uint32_t* lens, const uint32_t* words, uint64_t n, const uint64_t* tok_off, uint64_t n_docs, uint32_t block, uint64_t range,
                   uint32_t* byte_start, uint32_t* char_start, uint64_t* byte_off, uint64_t* char_off) {
    std::vector<uint8_t> mark(n + 9 + block, 0);
    for (uint64_t d = 0; d <= n_docs; ++d)
        if (tok_off[d] <= n) mark[tok_off[d]] = 1;
    if (!range) range = n ? n : 1;
    uint64_t carry[4] = {0, 0, 0, 0};  // TK_SPAN_BYTES, _CHARS, _MARK_B, _MARK_C
    const uint32_t lanes = block / 8;
    for (uint64_t a = 0; a < n || a == 0; a += range) {
        const uint64_t cnt = a + range < n ? range : n - a, end = a + cnt == n ? 1 : 0;
        const uint64_t nb = (cnt + end + block - 1) / block;
        auto len_at = [&](uint64_t i) { return i < cnt ? lens[a + i] : 0u; };
        auto word_at = [&](uint64_t i) { return i < cnt ? words[a + i] : 0u; };
        // a lane's sums and last mark, the lanes' exclusive prefixes, the keys: shared by tk_k_span_len and tk_k_span_write
        struct Lane { uint32_t sum, chars, mark_b, mark_c, ex_b, ex_c; uint64_t key; bool mk; };
        auto lanes_of = [&](uint64_t b, std::vector<Lane>& L) {
            uint32_t run_b = 0, run_c = 0;
            for (uint32_t l = 0; l < lanes; ++l) {
                Lane x{0, 0, 0, 0, run_b, run_c, 0, false};
                const uint64_t i0 = b * block + l * 8ull;
                for (int j = 0; j < 8; ++j) {
                    const uint64_t i = i0 + j;
                    if (i0 < cnt + end && mark[a + i]) x.mark_b = x.sum, x.mark_c = x.chars, x.mk = true;
                    x.sum += len_at(i);
                    x.chars += word_at(i) & ~TK_SPAN_CONT;
                }
                x.key = x.mk ? tk_span_key(x.ex_b + x.mark_b, x.ex_c + x.mark_c) : 0;
                run_b += x.sum;
                run_c += x.chars;
                L[l] = x;
            }
        };
        std::vector<uint64_t> bsum(nb), csum(nb), mkey(nb), doc_b(nb), doc_c(nb);
        std::vector<Lane> L(lanes);
        for (uint64_t b = 0; b < nb; ++b) {  // tk_k_span_len
            lanes_of(b, L);
            bsum[b] = L[lanes - 1].ex_b + L[lanes - 1].sum;
            csum[b] = L[lanes - 1].ex_c + L[lanes - 1].chars;
            mkey[b] = 0;
            for (const Lane& x : L) mkey[b] = x.key > mkey[b] ? x.key : mkey[b];
        }
        for (uint64_t b = 0; b < nb; ++b) {  // tk_k_span_scan
            const uint64_t at_b = carry[0], at_c = carry[1];
            doc_b[b] = carry[2] ? carry[2] - 1 : 0;
            doc_c[b] = carry[3] ? carry[3] - 1 : 0;
            const uint64_t mb = tk_span_mark_at(at_b, mkey[b], true), mc = tk_span_mark_at(at_c, mkey[b], false);
            carry[0] += bsum[b];
            carry[1] += csum[b];
            carry[2] = mb > carry[2] ? mb : carry[2];
            carry[3] = mc > carry[3] ? mc : carry[3];
            bsum[b] = at_b;
            csum[b] = at_c;
        }
        for (uint64_t b = 0; b < nb; ++b) {  // tk_k_span_write
            lanes_of(b, L);
            uint64_t before = 0;
            for (uint32_t l = 0; l < lanes; ++l) {
                uint64_t base_b = before ? bsum[b] + tk_span_key_bytes(before) : doc_b[b], base_c = before ? csum[b] + tk_span_key_chars(before) : doc_c[b];
                uint64_t at_b = bsum[b] + L[l].ex_b, at_c = csum[b] + L[l].ex_c;
                for (int j = 0; j < 8; ++j) {
                    const uint64_t i = b * block + l * 8ull + j;
                    if (i >= cnt + end) break;
                    if (mark[a + i] || i == cnt) {
                        base_b = at_b;
                        base_c = at_c;
                        uint64_t lo = 0, hi = n_docs + 1;
                        while (lo < hi) {
                            const uint64_t mid = (lo + hi) / 2;
                            if (tok_off[mid] < a + i) lo = mid + 1;
                            else hi = mid;
                        }
                        if (lo <= n_docs && tok_off[lo] == a + i) byte_off[lo] = at_b, char_off[lo] = at_c;
                    }
                    if (i < cnt) {
                        byte_start[a + i] = (uint32_t)(at_b - base_b);
                        char_start[a + i] = tk_span_char_start(at_c - base_c, words[a + i]);
                    }
                    at_b += len_at(i);
                    at_c += word_at(i) & ~TK_SPAN_CONT;
                }
                before = L[l].key > before ? L[l].key : before;
            }
        }
        if (end) break;
    }
    auto first_at = [&](uint64_t d) {
        if (!d || tok_off[d] != tok_off[d - 1]) return d;
        uint64_t lo = 0, hi = n_docs + 1;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) / 2;
            if (tok_off[mid] < tok_off[d]) lo = mid + 1;
            else hi = mid;
        }
        return lo;
    };
    uint64_t big = 0;
    for (uint64_t d = n_docs + 1; d-- > 0;) {  // tk_k_span_docs (any order: it reads only what tk_k_span_write wrote)
        const uint64_t f = first_at(d);
        if (f != d) byte_off[d] = byte_off[f], char_off[d] = char_off[f];
    }
    for (uint64_t d = 0; d < n_docs; ++d)
        if ((byte_off[d + 1] - byte_off[d]) >> 32 && !big) big = d + 1;
    return big;
}

// tk_k_utf8_docs lane by lane: text[0, n), documents at byte_off[0 .. n_docs]; lanes in the order lane_order gives (null: ascending).
// Returns the first document that is not well-formed, or all ones.
uint64_t ofs_utf8_first_invalid(const uint8_t* text_in, uint64_t n, const uint64_t* byte_off, uint64_t n_docs, const uint64_t* lane_order) {
    std::vector<uint32_t> store((n + 16 + 3) / 4 + 4, 0xA5A5A5A5u);  // (what lies behind the text is not zero on the device either)
    uint8_t* text = (uint8_t*)store.data();
    if (n) memcpy(text, text_in, n);
    std::vector<uint32_t> docb(n / 32 + 4, 0u);
    for (uint64_t d = 0; d <= n_docs; ++d)
        if (byte_off[d] <= n) docb[byte_off[d] >> 5] |= 1u << (byte_off[d] & 31);
    uint64_t first = ~0ull;
    const uint64_t lanes = (n + 15) / 16;
    for (uint64_t k = 0; k < lanes; ++k) {
        const uint64_t p0 = (lane_order ? lane_order[k] : k) * 16;
        const uint32_t nvalid = n - p0 < 16 ? (uint32_t)(n - p0) : 16u;
        uint32_t w[4], prev = 0;
        memcpy(w, text + p0, 16);
        if (p0) memcpy(&prev, text + p0 - 4, 4);
        for (uint32_t j = 0; j < 4; ++j) {
            if (nvalid <= 4u * j) w[j] = 0u;
            else if (nvalid < 4u * j + 4u) w[j] &= (1u << (8u * (nvalid - 4u * j))) - 1u;
        }
        const uint32_t bw = docb[p0 >> 5], sh = (uint32_t)(p0 & 31u);
        const uint32_t bounds = ((bw >> sh) & 0xFFFFu) | ((sh ? (docb[(p0 >> 5) + 1] & 1u) : ((bw >> 16) & 1u)) << 16);
        const uint32_t err = tk_utf8_lane_errors(w, prev >> 8, bounds, nvalid);
        if (!err) continue;
        const uint64_t q = p0 + (uint32_t)__builtin_ctz(err);
        uint64_t lo = 0, hi = n_docs + 1;  // the last document that starts at or before q
        while (lo < hi) {
            const uint64_t mid = (lo + hi) / 2;
            if (byte_off[mid] <= q) lo = mid + 1;
            else hi = mid;
        }
        const uint64_t d = lo ? lo - 1 : 0;
        if (d < first) first = d;
    }
    return first;
}
}
