// Token spans (reference Encoding.decode_with_offsets, tiktoken/core.py:312-335): the parts of the device passes of tk_offsets.h that are
// plain C++ -- the word a token contributes to the char count, how runs of tokens join, the clamp, and the lane body of the strict UTF-8
// check.  Compiles for the host too: tests/test_offsets_sim.py drives them lane by lane on the CPU.
#pragma once
#include <stdint.h>

#include "tk_common.h"

#define TK_SPAN_CONT 0x80000000u  // bit of a token's char word: its first byte is a continuation byte (0x80 .. 0xBF)

// The per-id char word: low 31 bits = bytes of the token outside 0x80 .. 0xBF (each starts a char), bit 31 = the first byte is inside.
TK_HD uint32_t tk_char_word(const uint8_t* b, uint32_t len) {
    uint32_t n = 0;
    for (uint32_t i = 0; i < len; ++i) n += (b[i] & 0xC0u) != 0x80u;
    return n | ((len && (b[0] & 0xC0u) == 0x80u) ? TK_SPAN_CONT : 0u);
}

// core.py:330: a token that starts inside a char belongs to the char before; `rel` = chars of the document before the token
TK_HD uint32_t tk_span_char_start(uint64_t rel, uint32_t word) { return (uint32_t)((word & TK_SPAN_CONT) && rel ? rel - 1 : rel); }

// How a token learns where its document starts.  The position of the LAST document start of a run of tokens travels with the run's sums:
// inside a workgroup as ONE word through a max-scan -- {bytes + 1, chars} from the workgroup's first token; bytes and chars grow
// together along the tokens, so the larger key is the later start; 0 = no document starts in the run --, across workgroups as the
// start's offset in the batch + 1 (tk_span_mark_at; 0 = none), again through max-scans.
TK_HD uint64_t tk_span_key(uint32_t mark_bytes, uint32_t mark_chars) { return (((uint64_t)mark_bytes + 1u) << 32) | mark_chars; }
TK_HD uint32_t tk_span_key_bytes(uint64_t key) { return (uint32_t)(key >> 32) - 1u; }
TK_HD uint32_t tk_span_key_chars(uint64_t key) { return (uint32_t)key; }
// `at`: bytes (chars) of the batch before the workgroup; key: the workgroup's
TK_HD uint64_t tk_span_mark_at(uint64_t at, uint64_t key, bool bytes) { return key ? at + (bytes ? tk_span_key_bytes(key) : tk_span_key_chars(key)) + 1u : 0u; }

// ------------------------------------------------------------------------------------------
// Strict UTF-8, sixteen bytes per lane.  A byte is judged by the three bytes before it (Python's decoder, bytes.decode("utf-8", "strict"):
// no overlong forms, no surrogates ED A0..BF, nothing above F4 8F BF BF, no truncated and no stray continuation):
//   it must be a continuation byte exactly when one of them opened a sequence that is still running,
//   C0, C1 and F5 .. FF are never valid, and the byte after E0 / ED / F0 / F4 has a narrower range.
// Documents never share a sequence: the bytes before a document's start count as absent, and at a document's end no sequence may be
// running -- so a sequence cut by a boundary makes both documents invalid.
//   w[4]     the lane's bytes (little endian words); `nvalid` (1 .. 16) of them are text
//   prev     the three bytes before the lane: byte -3 in bits 0..7, -2 in 8..15, -1 in 16..23 (the neighbour lane's last word >> 8; 0 at the text's start)
//   bounds   bit i (0 .. 16): a document starts at the lane's byte i (bit `nvalid` of the last lane: the text ends there)
// Returns the lane's bytes in error, bit i for byte i; an unfinished sequence is charged to the document's last byte.
// ------------------------------------------------------------------------------------------
TK_HD bool tk_utf8_open(uint32_t p1, uint32_t p2, uint32_t p3) { return p1 >= 0xC0u || p2 >= 0xE0u || p3 >= 0xF0u; }
TK_HD uint32_t tk_utf8_lane_errors(const uint32_t w[4], uint32_t prev, uint32_t bounds, uint32_t nvalid) {
    uint32_t p3 = prev & 0xFFu, p2 = (prev >> 8) & 0xFFu, p1 = (prev >> 16) & 0xFFu;
    const uint32_t any = w[0] | w[1] | w[2] | w[3];
    if (!(any & 0x80808080u) && !tk_utf8_open(p1, p2, p3)) return 0u;  // ASCII behind a finished sequence (bytes past nvalid are zero)
    uint32_t err = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < 16u; ++i) {
        if (i < nvalid) {
            if ((bounds >> i) & 1u) p1 = p2 = p3 = 0u;
            const uint32_t b = (w[i >> 2] >> (8u * (i & 3u))) & 0xFFu;
            const bool cont = (b & 0xC0u) == 0x80u;
            bool bad = tk_utf8_open(p1, p2, p3) != cont;
            bad |= b == 0xC0u || b == 0xC1u || b >= 0xF5u;
            bad |= (p1 == 0xE0u && b < 0xA0u) || (p1 == 0xEDu && b > 0x9Fu) || (p1 == 0xF0u && b < 0x90u) || (p1 == 0xF4u && b > 0x8Fu);
            p3 = p2;
            p2 = p1;
            p1 = b;
            if ((bounds >> (i + 1u)) & 1u) bad |= tk_utf8_open(p1, p2, p3);
            err |= (bad ? 1u : 0u) << i;
        }
    }
    return err;
}
