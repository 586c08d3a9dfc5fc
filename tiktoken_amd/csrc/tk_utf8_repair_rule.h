// UTF-8 repair (bytes.decode("utf-8", "replace" / "ignore") per document; the rule: include/tiktoken_amd.h): the parts of the device passes of
// tk_utf8_repair.h that are plain C++ -- the state a lane starts in, the step over its sixteen bytes with everything it emits, and the
// stream its output leaves through.  Compiles for the host too: tests/test_utf8_repair_sim.py drives them lane by lane on the CPU, with a
// reader that refuses what the contract does not allow and a writer that checks and counts every store.
#pragma once
#include <stdint.h>

#include "tk_decode_rule.h"  // TkDecStores: the kernel's stores

#define TK_U8R_REPLACE 0u  // == TK_U8_REPLACE
#define TK_U8R_IGNORE 1u   // == TK_U8_IGNORE
#define TK_U8R_BLOCK 4096  // bytes per workgroup (256 lanes x 16)
#define TK_U8R_FFFD 0xBDBFEFu  // EF BF BD as the stream takes it: little endian

// the length a lead byte declares (0: no lead -- ASCII, a continuation byte, C0, C1, F5 .. FF)
TK_HD uint32_t tk_u8r_lead_len(uint32_t b) { return b < 0xC2u ? 0u : b < 0xE0u ? 2u : b < 0xF0u ? 3u : b < 0xF5u ? 4u : 0u; }
TK_HD bool tk_u8r_cont(uint32_t b) { return (b & 0xC0u) == 0x80u; }
// the first byte a lead accepts (a continuation byte): narrower after E0, ED, F0 and F4
TK_HD bool tk_u8r_first_ok(uint32_t lead, uint32_t b) {
    return !((lead == 0xE0u && b < 0xA0u) || (lead == 0xEDu && b > 0x9Fu) || (lead == 0xF0u && b < 0x90u) || (lead == 0xF4u && b > 0x8Fu));
}

// What a lane leaves: bytes out, chars out (a replacement is one), units replaced or dropped
struct TkU8rCounts {
    uint32_t out, chars, repl;
};

// The sequence that is running: `len` what its lead declared, `need` the continuation bytes it still waits for (0: none is running)
struct TkU8rState {
    uint32_t len, need;
};
// ... behind the three bytes p3 p2 p1 (p1 the last; a byte that is absent -- before the document's start -- is passed as 0).  A lead is
// never swallowed by another unit, so three bytes decide it.
TK_HD TkU8rState tk_u8r_state_behind(uint32_t p1, uint32_t p2, uint32_t p3) {
    TkU8rState s{0u, 0u};
    if (tk_u8r_lead_len(p1)) {
        s.len = tk_u8r_lead_len(p1);
        s.need = s.len - 1u;
    } else if (tk_u8r_cont(p1)) {
        if (tk_u8r_lead_len(p2) >= 3u && tk_u8r_first_ok(p2, p1)) {
            s.len = tk_u8r_lead_len(p2);
            s.need = s.len - 2u;
        } else if (tk_u8r_cont(p2) && tk_u8r_lead_len(p3) == 4u && tk_u8r_first_ok(p3, p2)) {
            s.len = 4u;
            s.need = 1u;
        }
    }
    return s;
}

// A lane's output on its way to memory: one contiguous stretch from byte `at` on, streamed through a 64-bit register aligned with the
// destination as tk_dec_lane streams a lane's tokens -- one aligned 8-byte store per eight bytes (st.word); the first and the last word of
// the stretch, shared with the neighbour lanes, go out byte by byte (st.byte).
template <class Stores>
struct TkU8rStream {
    Stores& st;
    unsigned long long word;
    uint64_t acc;
    uint32_t first_lo, fill;
    bool first;
    TK_HD TkU8rStream(Stores& stores, unsigned long long at) : st(stores), word(at & ~7ull), acc(0), first_lo((uint32_t)(at & 7ull)), fill((uint32_t)(at & 7ull)), first(true) {}
    TK_HD void flush(uint32_t upto) {
        if (!first && upto == 8u) {
            st.word(word, acc);
        } else {
            for (uint32_t b = first ? first_lo : 0u; b < upto; ++b) st.byte(word + b, (uint8_t)(acc >> (8u * b)));
        }
        first = false;
    }
    // nb (1 .. 4) bytes, the first in v's low byte; the bytes of v above them are zero
    TK_HD void put(uint32_t v, uint32_t nb) {
        acc |= (uint64_t)v << (8u * fill);
        if (fill + nb >= 8u) {
            flush(8u);
            acc = (uint64_t)v >> (8u * (8u - fill));  // (fill >= 4 here: a shift of 8 .. 32)
            word += 8ull;
            fill = fill + nb - 8u;
        } else {
            fill += nb;
        }
    }
    TK_HD void finish() {
        if (fill > (first ? first_lo : 0u)) flush(fill);
    }
};
// the stream of the passes that only count
struct TkU8rNoStream {
    TK_HD void put(uint32_t, uint32_t) const {}
};
struct TkU8rNoDocs {
    TK_HD void operator()(uint32_t, const TkU8rCounts&) const {}
};

// ------------------------------------------------------------------------------------------
// A lane: sixteen bytes of the packed text, `nvalid` (0 .. 16) of them text.
//   lo, hi   the bytes, little endian (byte 0 in lo's low byte)
//   prev     the three bytes before the lane: byte -3 in bits 0..7, -2 in 8..15, -1 in 16..23 (0 at the text's start)
//   bounds   bit i (0 .. 16): a document starts at the lane's byte i (the text's end is the start of what lies behind it)
//   before   bit 0: a document starts at byte -2, bit 1: at byte -1
// A unit's output is charged to the byte at which its fate is known, so nothing is looked at that lies ahead: a well-formed sequence at
// its last byte, a broken one at the first byte that does not continue it, a sequence that its document's end cuts at the document's last
// byte.  Output comes in the order of the input.  out.put(v, nb) takes every emitted piece; docs(i, counts) is called for every i < 16
// with bit i of `bounds`, and for i == nvalid with it, before byte i is looked at: `counts` is what the lane's bytes before i were charged.
// ------------------------------------------------------------------------------------------
template <class Out, class Docs>
TK_HD TkU8rCounts tk_u8r_lane(uint64_t lo, uint64_t hi, uint32_t nvalid, uint32_t prev, uint32_t bounds, uint32_t before, uint32_t mode, Out& out, Docs&& docs) {
    if (bounds & 1u) prev = 0u;
    else if (before & 2u) prev &= 0xFF0000u;
    else if (before & 1u) prev &= 0xFFFF00u;
    TkU8rState s = tk_u8r_state_behind((prev >> 16) & 0xFFu, (prev >> 8) & 0xFFu, prev & 0xFFu);
    TkU8rCounts c{0u, 0u, 0u};
    const uint32_t rlen = mode == TK_U8R_REPLACE ? 3u : 0u;
    auto replace = [&]() {
        if (rlen) out.put(TK_U8R_FFFD, 3u);
        c.out += rlen;
        c.chars += rlen ? 1u : 0u;
        c.repl += 1u;
    };
    for (uint32_t i = 0; i < 16u; ++i) {
        if ((bounds >> i) & 1u) {
            if (i <= nvalid) docs(i, c);
            prev = 0u;
            s.need = 0u;
        }
        if (i >= nvalid) break;
        const uint32_t b = (uint32_t)lo & 0xFFu;
        lo = (lo >> 8) | (hi << 56);
        hi >>= 8;
        const uint32_t q = prev | (b << 24);  // the last four bytes in memory order
        bool taken = false;
        if (s.need && tk_u8r_cont(b)) taken = s.need + 1u != s.len || tk_u8r_first_ok((prev >> 16) & 0xFFu, b);
        if (taken) {
            if (--s.need == 0u) {
                out.put(q >> (8u * (4u - s.len)), s.len);
                c.out += s.len;
                c.chars += 1u;
            }
        } else {
            if (s.need) replace();  // the lead and what it accepted: the maximal subpart
            s.need = 0u;
            const uint32_t len = tk_u8r_lead_len(b);
            if (b < 0x80u) {
                out.put(b, 1u);
                c.out += 1u;
                c.chars += 1u;
            } else if (len) {
                s.len = len;
                s.need = len - 1u;
            } else {
                replace();
            }
        }
        prev = q >> 8;
        if (s.need && ((bounds >> (i + 1u)) & 1u)) {  // the document ends inside the sequence
            replace();
            s.need = 0u;
        }
    }
    return c;
}

// the bounds of a lane at byte p0 (a multiple of 16) from the bitmap over the bytes (bit p: a document starts at byte p), as tk_k_utf8_docs
// takes them: bits 0 .. 16; and the two bits before.  Reads the word of bit p0, the next one where the lane ends a word, the one before
// where it starts one.
template <class Bits>
TK_HD uint32_t tk_u8r_bounds(Bits docb, uint64_t p0, uint32_t* before) {
    const uint32_t bw = docb[p0 >> 5], sh = (uint32_t)(p0 & 31u);
    *before = !p0 ? 0u : sh ? (bw >> 14) & 3u : docb[(p0 >> 5) - 1] >> 30;
    return ((bw >> sh) & 0xFFFFu) | ((sh ? (docb[(p0 >> 5) + 1] & 1u) : ((bw >> 16) & 1u)) << 16);
}
