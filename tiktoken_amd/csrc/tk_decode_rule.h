// Decode (reference CoreBPE::decode_bytes, src/lib.rs:345-358): the parts of the device passes of tk_decode.h that are plain C++ -- the
// length of an id from the id -> {offset, length} table, the stream of a lane of the copy pass with every store it makes, and the entry
// of the per-document pass.  Compiles for the host too: tests/test_decode_sim.py drives them lane by lane on the CPU, with a writer that
// checks and counts every store.
#pragma once
#include <stdint.h>

#include "tk_device.h"  // tk_load8, tk_mask_low_bytes

#define TK_DEC_SPEC 0x80000000u  // entry.x bit: the bytes live in the special-token blob
#define TK_DEC_BLOCK 2048        // tokens per workgroup of the scan passes (256 threads x 8)

// Length of id t: dec holds n_ids entries {x = offset into a blob | TK_DEC_SPEC, y = length}; 0 = no entry (every real token has at least
// one byte), for an id beyond the table as for a hole in it.  Nothing is read from dec at or beyond n_ids.
template <class Dec>
TK_HD uint32_t tk_dec_len_of(Dec dec, uint32_t n_ids, uint32_t t) {
    return t < n_ids ? dec[t].y : 0u;
}

// The stores of the kernel: straight to the output
struct TkDecStores {
    uint8_t* __restrict__ out;
    TK_HD void word(unsigned long long off /* a multiple of 8 */, uint64_t v) const { *(uint64_t*)(out + off) = v; }
    TK_HD void byte(unsigned long long off, uint8_t v) const { out[off] = v; }
};

// A lane of the copy pass: the tokens i0 .. i0 + 7 (those below n), whose bytes are one contiguous stretch of the output from byte `at`
// on; len[j] = the length of token i0 + j (0 at and past n).  They stream through a 64-bit register aligned with the destination: `acc`
// holds the bytes of the aligned word at `word` from byte `fill` on (bytes below `first_lo` of the first word are a neighbour's).  One
// aligned 8-byte store per eight bytes -- out.word --; the first and the last word of the stretch, shared with the neighbours, go out byte
// by byte -- out.byte.  Sources are read as aligned words and shifted (tk_load8: the blobs are readable 16 bytes past their ends).
// tok_byte_off (may be null): entry i = off_base + the byte offset of token i.
template <class Tok, class Dec, class Out>
TK_HD void tk_dec_lane(Tok tokens, uint64_t i0, uint64_t n, const uint32_t len[8], unsigned long long at, Dec dec, const uint8_t* __restrict__ tok_bytes,
                       const uint8_t* __restrict__ spec_bytes, Out& out, unsigned long long* __restrict__ tok_byte_off, unsigned long long off_base) {
    unsigned long long word = at & ~7ull;
    const uint32_t first_lo = (uint32_t)(at & 7ull);
    uint32_t fill = first_lo;
    uint64_t acc = 0;
    bool first = true;
    auto flush = [&](uint32_t upto /* bytes of the word that are valid: fill */) {
        if (!first && upto == 8u) {
            out.word(word, acc);
        } else {
            for (uint32_t b = first ? first_lo : 0u; b < upto; ++b) out.byte(word + b, (uint8_t)(acc >> (8u * b)));
        }
        first = false;
    };
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < 8; ++j) {
        const uint64_t i = i0 + j;
        if (i < n) {
            if (tok_byte_off) tok_byte_off[i] = off_base + at;
            const auto e = dec[tokens[i]];
            const uint8_t* src = ((e.x & TK_DEC_SPEC) ? spec_bytes : tok_bytes);
            const uint64_t so = e.x & ~TK_DEC_SPEC;
            for (uint32_t b = 0; b < len[j]; b += 8u) {
                const uint32_t nb = len[j] - b < 8u ? len[j] - b : 8u;
                const uint64_t w = tk_mask_low_bytes(tk_load8(src, so + b), nb);
                acc |= w << (8u * fill);
                if (fill + nb >= 8u) {
                    flush(8u);
                    acc = fill ? (w >> (8u * (8u - fill))) : 0ull;
                    word += 8ull;
                    fill = fill + nb - 8u;
                } else {
                    fill += nb;
                }
            }
            at += len[j];
        }
    }
    if (fill > (first ? first_lo : 0u)) flush(fill);
}

// Entry d <= n_docs of the per-document pass: the byte offset of the first token of document d -- that of token tok_off[d], or the total
// where the document starts at the batch's end (tok_off: n_docs + 1 token offsets, non-decreasing)
template <class Off, class ByteOff>
TK_HD uint64_t tk_dec_doc_off(Off tok_off, uint64_t d, uint64_t n, ByteOff tok_byte_off, const unsigned long long* __restrict__ total) {
    const uint64_t t = tok_off[d];
    return t < n ? tok_byte_off[t] : total[0];
}
