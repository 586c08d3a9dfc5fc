// Stop strings (the rule: include/tiktoken_amd.h, tk_stop_text_device): the parts of the device passes of tk_stop_text.h that are plain
// C++ -- the stop set as the kernels read it, a lane of the search over its sixteen start positions, a document's kept length from its
// word, a lane of the cut with every store it makes, and a row's token count.  Compiles for the host too: tests/test_stop_text_sim.py
// drives them lane by lane on the CPU, with a reader that refuses what the contract does not allow and a writer that counts every store.
#pragma once
#include <stdint.h>

#include "tk_device.h"  // TK_HD

#define TK_STOPS_MAX 16      // strings in a stop set
#define TK_STOPS_MAXLEN 64   // bytes in a string
#define TK_STOPS_BLOCK 4096  // bytes per workgroup of the search (256 lanes x 16)
#define TK_STOPS_TAIL 64     // bytes staged behind a workgroup's own (a match may start at its last byte: 63 more, rounded to a 16-byte load)
#define TK_STOPSF_KEEP 1u    // == TK_STOPS_KEEP
#define TK_STOPS_NO_HIT 0xFFFFFFFFu

// The stop set as it travels to the device and lies in LDS: the strings back to back, their offsets, and the bitmap of their first bytes.
struct TkStopSet {
    uint32_t n, flags;
    uint32_t off[TK_STOPS_MAX + 1];
    uint32_t mask[8];  // bit b: some string starts with byte b
    uint8_t blob[TK_STOPS_MAX * TK_STOPS_MAXLEN];
};
#define TK_STOPS_SET_WORDS (sizeof(TkStopSet) / 4)

// What can be refused on the host: 0 fine, 1 more than 16 strings, 2 an empty string, 3 a string over 64 bytes, 4 offsets that do not
// ascend from 0, 5 an unknown flag.  Fills *set when fine.
inline int tk_stops_make(uint32_t n, const uint8_t* blob, const uint32_t* off, uint32_t flags, TkStopSet* set) {
    if (flags & ~TK_STOPSF_KEEP) return 5;
    if (n > TK_STOPS_MAX) return 1;
    if (n && off[0] != 0u) return 4;
    for (uint32_t k = 0; k < n; ++k) {
        if (off[k + 1] < off[k]) return 4;
        if (off[k + 1] == off[k]) return 2;
        if (off[k + 1] - off[k] > TK_STOPS_MAXLEN) return 3;
    }
    *set = TkStopSet();
    set->n = n;
    set->flags = flags;
    for (uint32_t k = 0; k <= TK_STOPS_MAX; ++k) set->off[k] = n ? off[k < n ? k : n] : 0u;
    for (uint32_t i = 0; n && i < off[n]; ++i) set->blob[i] = blob[i];
    for (uint32_t k = 0; k < n; ++k) set->mask[blob[off[k]] >> 5] |= 1u << (blob[off[k]] & 31u);
    return 0;
}

// the document of byte p < off[n_docs]: the d with off[d] <= p < off[d + 1].  Indexes off with indices only: whatever the offsets hold
// (they are checked beside this pass, not before it), the answer lies in [0, n_docs).  n_docs >= 1.
template <class Off>
TK_HD uint64_t tk_stops_doc_of(Off off, uint64_t n_docs, uint64_t p) {
    uint64_t lo = 0, hi = n_docs;  // first d in [0, n_docs) with off[d + 1] > p
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (off[mid + 1] <= p) lo = mid + 1;
        else hi = mid;
    }
    return lo < n_docs ? lo : n_docs - 1;
}

// A lane of the search: the start positions p0 .. p0 + 15 below n.  tile(i): the byte at text position i, staged by the lane's workgroup
// (its own bytes and TK_STOPS_TAIL behind them, never at or past n + 16); set: the stop set (LDS).  A position survives when its byte is
// in the mask; it is then compared, in list order, with the strings that start with that byte, and a string matches only where it ends
// at or before its document's end and the text's.  hit(d, key) takes key = (p - off[d]) * 16 + k for the lane's first match in every
// document -- later ones in the same document have larger keys.  One search of off per lane, one more per document boundary that a
// surviving position lies behind.
template <class Tile, class Off, class Hit>
TK_HD void tk_stops_lane(const Tile& tile, const TkStopSet& set, Off off, uint64_t n_docs, uint64_t n, uint64_t p0, Hit&& hit) {
    uint64_t d = 0, d_begin = 0, d_end = 0;  // the document of the last surviving position: [d_begin, d_end); none yet
    bool found = false;                      // ... and it has its match
    for (uint32_t j = 0; j < 16u; ++j) {
        const uint64_t p = p0 + j;
        if (p >= n) break;
        const uint32_t b = tile(p);
        if (!((set.mask[b >> 5] >> (b & 31u)) & 1u)) continue;
        if (p >= d_end) {
            d = tk_stops_doc_of(off, n_docs, p);
            d_begin = off[d];
            d_end = off[d + 1];
            found = false;
            if (p < d_begin || p >= d_end) {  // (offsets that do not ascend: the call is refused; nothing is compared beyond this lane)
                d_end = 0;
                continue;
            }
        }
        if (found) continue;
        const uint64_t limit = d_end < n ? d_end : n;
        for (uint32_t k = 0; k < set.n; ++k) {
            const uint32_t a = set.off[k], len = set.off[k + 1] - a;
            if (set.blob[a] != b || p + len > limit) continue;
            uint32_t i = 1;
            while (i < len && tile(p + i) == set.blob[a + i]) ++i;
            if (i == len) {
                hit(d, (unsigned long long)(p - d_begin) * TK_STOPS_MAX + k);
                found = true;
                break;
            }
        }
    }
}

// A document's kept length and hit from its word (all ones: no hit) and its length
TK_HD uint64_t tk_stops_kept(unsigned long long word, uint64_t doc_len, const TkStopSet& set, uint32_t* hit) {
    if (word == ~0ull) {
        *hit = TK_STOPS_NO_HIT;
        return doc_len;
    }
    const uint32_t k = (uint32_t)(word % TK_STOPS_MAX);
    *hit = k;
    return word / TK_STOPS_MAX + ((set.flags & TK_STOPSF_KEEP) ? set.off[k + 1] - set.off[k] : 0u);
}

// sixteen bytes from byte `sh` (0 .. 15) of the 32 bytes a0 a1 b0 b1 (little endian words)
TK_HD void tk_stops_shift16(uint64_t a0, uint64_t a1, uint64_t b0, uint64_t b1, uint32_t sh, uint64_t* lo, uint64_t* hi) {
    const bool up = sh >= 8u;
    const uint64_t w0 = up ? a1 : a0, w1 = up ? b0 : a1, w2 = up ? b1 : b0;
    const uint32_t s = 8u * (sh & 7u);
    *lo = s ? (w0 >> s) | (w1 << (64u - s)) : w0;
    *hi = s ? (w1 >> s) | (w2 << (64u - s)) : w1;
}

// A lane of the cut: the output bytes q0 .. q0 + 15 below n_text (q0 a multiple of 16).  Output byte q of document d comes from input byte
// byte_off[d] + (q - text_off[d]).  src.load16(pos, &lo, &hi): the sixteen bytes at the 16-byte aligned input position pos; src.byte(pos).
// st.store16(q, lo, hi): an aligned 16-byte store; st.byte(q, v).  A lane whose sixteen bytes lie in one document takes them with two
// aligned loads and one aligned store; a lane with a boundary inside, and the text's last lane, go byte by byte.  Every output byte is
// stored exactly once; nothing is read at or past the end of a document's kept bytes, except inside the aligned 16 bytes around them.
template <class Src, class Off, class Stores>
TK_HD void tk_stops_cut_lane(const Src& src, Off byte_off, Off text_off, uint64_t n_docs, uint64_t n_text, uint64_t q0, Stores& st) {
    if (q0 >= n_text) return;
    uint64_t d = tk_stops_doc_of(text_off, n_docs, q0);
    uint64_t t_begin = text_off[d], t_end = text_off[d + 1], from = byte_off[d];
    if (q0 + 16u <= t_end) {
        const uint64_t s = from + (q0 - t_begin), aligned = s & ~15ull;
        const uint32_t sh = (uint32_t)(s & 15ull);
        uint64_t a0, a1, b0 = 0, b1 = 0, lo, hi;
        src.load16(aligned, &a0, &a1);
        if (sh) src.load16(aligned + 16u, &b0, &b1);
        tk_stops_shift16(a0, a1, b0, b1, sh, &lo, &hi);
        st.store16(q0, lo, hi);
        return;
    }
    const uint64_t q_end = q0 + 16u < n_text ? q0 + 16u : n_text;
    for (uint64_t q = q0; q < q_end; ++q) {
        while (q >= t_end) {  // (q < n_text == text_off[n_docs]: the walk ends at a document that holds q)
            ++d;
            t_begin = t_end;
            t_end = text_off[d + 1];
            from = byte_off[d];
        }
        st.byte(q, src.byte(from + (q - t_begin)));
    }
}

// A row's token count: the tokens [t0, t1) of the row start at the ascending byte positions tok_byte[t0 .. t1) of the decoded bytes; the
// row's kept text ends at byte position `kept_end`.  The number of tokens whose first byte lies before it.
template <class TokByte>
TK_HD uint32_t tk_stops_ntok(TokByte tok_byte, uint64_t t0, uint64_t t1, uint64_t kept_end) {
    uint64_t lo = t0, hi = t1;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (tok_byte[mid] < kept_end) lo = mid + 1;
        else hi = mid;
    }
    return (uint32_t)(lo - t0);
}
