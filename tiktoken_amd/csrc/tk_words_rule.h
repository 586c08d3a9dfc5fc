// Word statistics per document of packed text: the parts of the device passes of tk_words.h that are plain C++ -- the white-space
// patterns, the masks of a lane's 16 bytes, the element the scans carry and its join, a stretch of a lane as such an element, the stop
// words of a call and the shape of a call.  The rule is stated in include/tiktoken_amd.h.  Compiles for the host.
//
// Words.  A byte is WHITE SPACE when it lies in one of the byte sequences of the 29 chars of str.isspace() and that sequence lies wholly
// inside one document; every other byte below N is CONTENT.  A position is a CUT when a document starts there or its byte is no content
// (position N is one).  A word is a maximal run of content; it is handed out at the cut that ends it, by the lane whose 16 bytes hold the
// cut; the tiles cover [0, N] inclusive.  What is known of a run is exact and small: its bytes, its chars, whether a letter is among them,
// and its first 8 bytes packed little-endian -- so "equals one of a few short strings" is a comparison of 64 bits and a length, and two
// runs join without a multiplication: l.packed | r.packed << 8 l.bytes while l.bytes < 8.
// Dots.  A maximal run of r '.' inside a document counts r / 3 ellipses.  Wherever the run is split, the triples that end in a part are
// (m + len) / 3, m the dots before the part modulo 3: so the scans carry the length of the open run modulo 3 and nothing else.
#pragma once
#include <stdint.h>

#include "tk_lines_rule.h"  // tk_ln_cont_mask, tk_last_le

#define TK_WD_TILE 4096u      // bytes of text per workgroup
#define TK_WD_THREADS 256u    // its lanes
#define TK_WD_LANE 16u        // bytes per lane: one 16-byte load
#define TK_WD_WAVE 1024u      // bytes per wavefront
#define TK_WD_DOCS 256u       // documents of a tile whose sums are gathered in LDS; the rest add to HBM directly
#define TK_WD_MAX_BYTES 0xFFFF0000ull
#define TK_WD_MAX_STOP 32u
#define TK_WD_MAX_STOP_BYTES 8u
#define TK_WD_MAX_TERMINAL 16u
#ifndef TK_WD_ASCII_PATH
#define TK_WD_ASCII_PATH 1  // 0 (experiments, tools/build_variant.sh): no lane is done by SWAR alone; every lead byte goes through the class table
#endif
// the sums of a document, uint64[TK_WD_SUMS][n_docs], in the order of the outputs
enum { TK_WD_S_WORDS = 0, TK_WD_S_CHARS, TK_WD_S_ALPHA, TK_WD_S_STOP, TK_WD_S_HASH, TK_WD_S_ELLIPSIS, TK_WD_S_LINES, TK_WD_S_PUNCT, TK_WD_SUMS };

struct TkWd {
    uint64_t n_bytes, n_docs;
    uint64_t stop[TK_WD_MAX_STOP];  // the stop words' bytes, packed little-endian
    uint32_t n_tiles, n_stop;
    uint32_t terminal[4];           // bit b: the ASCII byte b ends a punctuated line
    uint8_t stop_len[TK_WD_MAX_STOP];
};

// The length of the white-space char that starts with the bytes b0 b1 b2 (bytes behind the text: 0), 0 if there is none.
TK_HD uint32_t tk_wd_ws_len(uint32_t b0, uint32_t b1, uint32_t b2) {
    if (b0 < 0x80u) return ((b0 >= 0x09u && b0 <= 0x0Du) || (b0 >= 0x1Cu && b0 <= 0x20u)) ? 1u : 0u;
    if (b0 == 0xC2u) return (b1 == 0x85u || b1 == 0xA0u) ? 2u : 0u;
    if (b0 == 0xE1u) return (b1 == 0x9Au && b2 == 0x80u) ? 3u : 0u;
    if (b0 == 0xE2u) {
        if (b1 == 0x80u) return ((b2 >= 0x80u && b2 <= 0x8Au) || b2 == 0xA8u || b2 == 0xA9u || b2 == 0xAFu) ? 3u : 0u;
        return (b1 == 0x81u && b2 == 0x9Fu) ? 3u : 0u;
    }
    if (b0 == 0xE3u) return (b1 == 0x80u && b2 == 0x80u) ? 3u : 0u;
    return 0u;
}

// The shape of a call.  0, or why it is refused: 1 n_bytes; 2 more than 32 stop words; 3 a stop word that is empty or longer than 8
// bytes; 4 one that holds white space; 5 one that is repeated; 6 more than 16 terminal bytes; 7 a terminal byte >= 0x80.
TK_HD int tk_wd_shape(uint64_t n_bytes, uint64_t n_docs, const uint8_t* stop_bytes, const uint64_t* stop_off, uint64_t n_stop, const uint8_t* terminal, uint64_t n_terminal,
                      TkWd* p) {
    if (n_bytes > TK_WD_MAX_BYTES) return 1;
    if (n_stop > TK_WD_MAX_STOP) return 2;
    if (n_terminal > TK_WD_MAX_TERMINAL) return 6;
    p->n_bytes = n_bytes, p->n_docs = n_docs, p->n_stop = (uint32_t)n_stop;
    p->n_tiles = (uint32_t)(n_bytes / TK_WD_TILE + 1);  // (position N lies in a tile)
    for (uint32_t i = 0; i < TK_WD_MAX_STOP; ++i) p->stop[i] = 0, p->stop_len[i] = 0;
    for (uint64_t i = 0; i < n_stop; ++i) {
        const uint64_t a = stop_off[i], b = stop_off[i + 1];
        if (b <= a || b - a > TK_WD_MAX_STOP_BYTES) return 3;
        const uint32_t n = (uint32_t)(b - a);
        uint64_t packed = 0;
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t len = tk_wd_ws_len(stop_bytes[a + j], j + 1 < n ? stop_bytes[a + j + 1] : 0u, j + 2 < n ? stop_bytes[a + j + 2] : 0u);
            if (len && j + len <= n) return 4;
            packed |= (uint64_t)stop_bytes[a + j] << (8 * j);
        }
        for (uint64_t k = 0; k < i; ++k)
            if (p->stop_len[k] == n && p->stop[k] == packed) return 5;
        p->stop[i] = packed, p->stop_len[i] = (uint8_t)n;
    }
    for (uint32_t i = 0; i < 4; ++i) p->terminal[i] = 0;
    for (uint64_t i = 0; i < n_terminal; ++i) {
        if (terminal[i] >= 0x80u) return 7;
        p->terminal[terminal[i] >> 5] |= 1u << (terminal[i] & 31u);
    }
    return 0;
}
TK_HD bool tk_wd_is_terminal(const TkWd& p, uint32_t byte) {
    const uint32_t w = byte >> 5, t = w == 0 ? p.terminal[0] : w == 1 ? p.terminal[1] : w == 2 ? p.terminal[2] : p.terminal[3];
    return byte < 0x80u && ((t >> (byte & 31u)) & 1u);
}

// What the scans carry: the word that is open at a range's end -- the run behind its last word cut -- and the dots that are open there,
// modulo 3, each with whether a cut of its kind lies in the range.  The identity is all zero.
struct TkWdRun {
    uint64_t packed;        // the first 8 bytes
    uint32_t bytes, chars;
    uint32_t flags;         // TK_WD_F_*
};
enum { TK_WD_F_ALPHA = 1u, TK_WD_F_CUT = 2u, TK_WD_F_DOTS = 12u, TK_WD_F_DOTS_SHIFT = 2, TK_WD_F_DOT_CUT = 16u };
TK_HD TkWdRun tk_wd_empty() { return TkWdRun{0, 0, 0, 0}; }
TK_HD uint32_t tk_wd_dots(const TkWdRun& r) { return (r.flags & TK_WD_F_DOTS) >> TK_WD_F_DOTS_SHIFT; }
TK_HD TkWdRun tk_wd_join(const TkWdRun& l, const TkWdRun& r) {
    TkWdRun o;
    if (r.flags & TK_WD_F_CUT) {
        o.packed = r.packed, o.bytes = r.bytes, o.chars = r.chars, o.flags = r.flags & (TK_WD_F_ALPHA | TK_WD_F_CUT);
    } else {
        o.packed = l.packed | (l.bytes < 8u ? r.packed << (8u * l.bytes) : 0ull);
        o.bytes = l.bytes + r.bytes, o.chars = l.chars + r.chars;
        o.flags = ((l.flags | r.flags) & TK_WD_F_ALPHA) | (l.flags & TK_WD_F_CUT);
    }
    if (r.flags & TK_WD_F_DOT_CUT) o.flags |= r.flags & (TK_WD_F_DOTS | TK_WD_F_DOT_CUT);
    else o.flags |= (((tk_wd_dots(l) + tk_wd_dots(r)) % 3u) << TK_WD_F_DOTS_SHIFT) | (l.flags & TK_WD_F_DOT_CUT);
    return o;
}

// SWAR over 8 bytes: 0x80 in every byte of w that is below 0x80 and in [a, b] (a <= b < 0x80; no carry crosses a byte)
TK_HD uint64_t tk_wd_in(uint64_t w, uint32_t a, uint32_t b) {
    const uint64_t ones = 0x0101010101010101ull, y = w & 0x7F7F7F7F7F7F7F7Full;
    return (y + ones * (0x80u - a)) & ~(y + ones * (0x7Fu - b)) & ~w & 0x8080808080808080ull;
}
// the sixteen 0x80 flags of two such words as 16 bits
TK_HD uint32_t tk_wd_gather(uint64_t flo, uint64_t fhi) {
    return (uint32_t)(((flo >> 7) * 0x0102040810204080ull) >> 56) | ((uint32_t)(((fhi >> 7) * 0x0102040810204080ull) >> 56) << 8);
}

struct TkWdLane {  // what a lane knows of its 16 bytes; masks of 16 bits, bit j: byte j
    uint64_t lo, hi;
    uint32_t pos;      // of its first byte, from the tile's start
    uint32_t brk;      // bit j: a document starts at byte j; 17 bits
    uint32_t rank;     // document starts at the tile's positions before the lane
    uint32_t content;  // a byte of a word
    uint32_t cut;      // a word ends before byte j: brk | ~content
    uint32_t lead;     // a byte below N that is not 0b10xxxxxx
    uint32_t letter;   // a lead byte that is a letter
    uint32_t dot, hash;
    uint32_t ell;      // the E2 of an E2 80 A6 inside one document
    uint32_t lend;     // the last byte of a line
    TK_HD uint32_t byte(uint32_t j) const { return (uint32_t)((j < 8 ? lo >> (8 * j) : hi >> (8 * (j - 8))) & 0xFFu); }
    TK_HD uint32_t dot_cut() const { return (brk | ~dot) & 0xFFFFu; }
    // the local document a word that ends before byte j belongs to (that of byte j - 1), and the one of byte j
    TK_HD uint32_t doc_before(uint32_t j) const { return rank + (uint32_t)__builtin_popcount(brk & ((1u << j) - 1u)); }
    TK_HD uint32_t doc(uint32_t j) const { return rank + (uint32_t)__builtin_popcount(brk & ((2u << j) - 1u)); }
};

// The masks of a lane.  In: its bytes (zeros behind the text), n_left = min(N - its first position, 17) (0 for a lane behind the text),
// B: bit k is set when a document starts at the lane's byte k - 2 (k < 32), at(k): the byte at the lane's position k, -2 <= k < 19, 0
// outside the text; is_letter(cp): the class of the code point is in TK_M_L.  Lanes without a byte >= 0x80 never call at or is_letter.
template <class At, class IsLetter>
TK_HD void tk_wd_lane_masks(uint64_t lo, uint64_t hi, uint32_t n_left, uint32_t B, uint32_t next_byte, At&& at, IsLetter&& is_letter, TkWdLane* L) {
    const uint32_t valid = n_left >= 16u ? 0xFFFFu : (1u << n_left) - 1u;
    const uint32_t high = tk_wd_gather(lo & 0x8080808080808080ull, hi & 0x8080808080808080ull);
    uint32_t ws = tk_wd_gather(tk_wd_in(lo, 0x09, 0x0D) | tk_wd_in(lo, 0x1C, 0x20), tk_wd_in(hi, 0x09, 0x0D) | tk_wd_in(hi, 0x1C, 0x20));
    const uint32_t nl = tk_wd_gather(tk_wd_in(lo, '\n', '\n'), tk_wd_in(hi, '\n', '\n'));
    L->lo = lo, L->hi = hi;
    L->brk = (B >> 2) & 0x1FFFFu;
    L->dot = tk_wd_gather(tk_wd_in(lo, '.', '.'), tk_wd_in(hi, '.', '.'));
    L->hash = tk_wd_gather(tk_wd_in(lo, '#', '#'), tk_wd_in(hi, '#', '#'));
    L->letter = TK_WD_ASCII_PATH ? tk_wd_gather(tk_wd_in(lo, 'A', 'Z') | tk_wd_in(lo, 'a', 'z'), tk_wd_in(hi, 'A', 'Z') | tk_wd_in(hi, 'a', 'z')) : 0u;
    L->lead = valid & ~tk_ln_cont_mask(lo, hi);
    L->ell = 0;
    if (high || !TK_WD_ASCII_PATH) {
        // a char of k bytes that starts at byte j lies inside one document when no document starts at j + 1 .. j + k - 1
        auto inside = [&](int j, uint32_t k) { return !((B >> (j + 3)) & ((1u << (k - 1u)) - 1u)); };
        for (int j = -2; j < 0; ++j) {  // white space that starts before the lane and reaches into it
            const uint32_t k = tk_wd_ws_len(at(j), at(j + 1), at(j + 2));
            if (k > 1u && inside(j, k)) ws |= ((1u << k) - 1u) >> -j;
        }
        for (uint32_t m = TK_WD_ASCII_PATH ? high & L->lead : L->lead; m; m &= m - 1u) {
            const int j = __builtin_ctz(m);
            const uint32_t b0 = at(j), b1 = at(j + 1), b2 = at(j + 2);
            if (b0 < 0x80u) {  // (only without the ASCII path)
                if (is_letter(b0)) L->letter |= 1u << j;
                continue;
            }
            const uint32_t k = tk_wd_ws_len(b0, b1, b2);
            if (k > 1u && inside(j, k)) ws |= (((1u << k) - 1u) << j) & 0xFFFFu;
            if (b0 == 0xE2u && b1 == 0x80u && b2 == 0xA6u && inside(j, 3u)) L->ell |= 1u << j;
            const uint32_t len = b0 >= 0xF0u ? 4u : b0 >= 0xE0u ? 3u : 2u;  // (as tk_classify_text)
            const uint32_t b3 = len == 4u ? at(j + 3) : 0x80u;
            if ((b1 & 0xC0u) != 0x80u || (len > 2u && (b2 & 0xC0u) != 0x80u) || (b3 & 0xC0u) != 0x80u || !inside(j, len)) continue;
            const uint32_t cp = len == 2u   ? ((b0 & 0x1Fu) << 6) | (b1 & 0x3Fu)
                                : len == 3u ? ((b0 & 0x0Fu) << 12) | ((b1 & 0x3Fu) << 6) | (b2 & 0x3Fu)
                                            : ((b0 & 0x07u) << 18) | ((b1 & 0x3Fu) << 12) | ((b2 & 0x3Fu) << 6) | (b3 & 0x3Fu);
            if (is_letter(cp)) L->letter |= 1u << j;
        }
    }
    L->content = valid & ~ws;
    L->cut = (L->brk | ~L->content) & 0xFFFFu;
    L->letter &= L->content;
    const uint32_t nonl = (valid & ~nl) | ((n_left > 16u && next_byte != '\n') ? 0x10000u : 0u);
    L->lend = nonl & ((L->brk >> 1) | ~(nonl >> 1)) & 0xFFFFu;
}

// Bytes [s, e) of a lane, all of them content, as a run (flags: TK_WD_F_ALPHA alone); s <= e <= 16
TK_HD TkWdRun tk_wd_part(const TkWdLane& L, uint32_t s, uint32_t e) {
    const uint32_t n = e - s, R = ((1u << e) - 1u) & ~((1u << s) - 1u);
    uint64_t v = s == 0 ? L.lo : s < 8u ? (L.lo >> (8u * s)) | (L.hi << (64u - 8u * s)) : s < 16u ? L.hi >> (8u * (s - 8u)) : 0ull;
    if (n < 8u) v &= (1ull << (8u * n)) - 1ull;
    return TkWdRun{v, n, (uint32_t)__builtin_popcount(L.lead & R), (L.letter & R) ? (uint32_t)TK_WD_F_ALPHA : 0u};
}
// where the run starts that ends before byte j, given the highest cut l below j: at l when a document starts on content there, else behind it
TK_HD uint32_t tk_wd_start(uint32_t content, uint32_t l) { return l + (((content >> l) & 1u) ^ 1u); }
// The lane as the scans see it: the word behind its last cut and the dots behind its last dot cut
TK_HD TkWdRun tk_wd_lane_tail(const TkWdLane& L) {
    TkWdRun r = L.cut ? tk_wd_part(L, tk_wd_start(L.content, 31u - (uint32_t)__builtin_clz(L.cut)), TK_WD_LANE) : tk_wd_part(L, 0, TK_WD_LANE);
    if (L.cut) r.flags |= TK_WD_F_CUT;
    const uint32_t dc = L.dot_cut();
    const uint32_t from = dc ? tk_wd_start(L.dot, 31u - (uint32_t)__builtin_clz(dc)) : 0u;
    r.flags |= (((TK_WD_LANE - from) % 3u) << TK_WD_F_DOTS_SHIFT) | (dc ? (uint32_t)TK_WD_F_DOT_CUT : 0u);
    return r;
}
// bit j: a word ends before byte j of the lane; `before`: the run that is open at the lane's start
TK_HD uint32_t tk_wd_ends(const TkWdLane& L, const TkWdRun& before) { return L.cut & ((L.content << 1) | (before.bytes ? 1u : 0u)); }
// ... that word
TK_HD TkWdRun tk_wd_word(const TkWdLane& L, const TkWdRun& before, uint32_t j) {
    const uint32_t low = L.cut & ((1u << j) - 1u);
    if (low) return tk_wd_part(L, tk_wd_start(L.content, 31u - (uint32_t)__builtin_clz(low)), j);
    TkWdRun l = before;
    l.flags &= TK_WD_F_ALPHA;
    return tk_wd_join(l, tk_wd_part(L, 0, j));
}
// bit i: the word equals stop word i
TK_HD uint32_t tk_wd_stop_bits(const TkWd& p, const TkWdRun& w) {
    uint32_t m = 0;
    if (w.bytes <= TK_WD_MAX_STOP_BYTES)
        for (uint32_t i = 0; i < p.n_stop; ++i)
            if (p.stop_len[i] == w.bytes && p.stop[i] == w.packed) m |= 1u << i;
    return m;
}
// bit j: a run of dots starts at byte j of the lane (at byte 0: or goes on); the ellipses that END in the part of the run that starts at s
TK_HD uint32_t tk_wd_dot_starts(const TkWdLane& L) { return L.dot & (~(L.dot << 1) | L.brk) & 0xFFFFu; }
TK_HD uint32_t tk_wd_dot_triples(const TkWdLane& L, const TkWdRun& before, uint32_t s) {
    const uint32_t rest = L.dot_cut() & ~((2u << s) - 1u), e = rest ? (uint32_t)__builtin_ctz(rest) : TK_WD_LANE;
    return ((s == 0 && !(L.brk & 1u) ? tk_wd_dots(before) : 0u) + e - s) / 3u;
}
