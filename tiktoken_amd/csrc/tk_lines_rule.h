// Duplicate lines and paragraphs per document of packed text: the parts of the device passes of tk_lines.h that are plain C++ -- the
// arithmetic modulo 2^61 - 1, the two bases, the element of the monoid and its combine, a run of bytes appended to an element, the key
// of a finished line or paragraph, the masks of 16 bytes (newlines, chars, the content of the two segmentations), the bullet and
// ellipsis tests, the shape of a call and the size of its table.  The rule is stated in include/tiktoken_amd.h.  Compiles for the host.
//
// Segments.  Lines and paragraphs are both maximal runs of CONTENT bytes inside one document; the two segmentations differ in which
// newlines are content (none for lines; for paragraphs a newline that is neither first nor last in its document and has no newline
// beside it).  A position is a CUT when a document starts there or its byte is no content.  A segment is handed out at the cut that
// ends it, by the lane whose 16 bytes hold the cut; the tiles cover [0, N] inclusive, so position N -- no content -- cuts the last one.
//
// The hash.  h(s) = sum (s[i] + 1) B^(|s| - 1 - i) mod p, p = 2^61 - 1, under two bases B1, B2 in [257, p) drawn from `seed`; so
// h(ab) = h(a) B^|b| + h(b), which is what lets lanes, wavefronts and tiles hash their own bytes and be combined in any grouping.
// Two different runs of the same length L agree in one hash for at most L - 1 of the p - 257 bases, in both with probability below
// (L / 2^61)^2 = L^2 / 2^122; the key then mixes (h1, h2, L, document, kind) into 64 bits, where two different tuples meet with 2^-64.
// Runs of different length never have the same tuple.  So two different lines of a document are confused with about 2^-64 + L^2 / 2^122
// per pair -- a hash DECIDES here, unlike in tk_repeat_rule.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "tk_fingerprint_rule.h"  // tk_fp_mix, tk_last_le

#define TK_LN_TILE 4096u      // bytes of text per workgroup
#define TK_LN_THREADS 256u    // its lanes
#define TK_LN_LANE 16u        // bytes per lane: one 16-byte load
#define TK_LN_WAVE 1024u      // bytes per wavefront
#define TK_LN_DOCS 256u       // documents of a tile whose sums are gathered in LDS: one per lane at the flush; the rest add to HBM directly
#define TK_LN_MAX_BYTES 0xFFFF0000ull
#define TK_LN_P 0x1FFFFFFFFFFFFFFFull
#define TK_LN_LINE 0u
#define TK_LN_PARA 1u
#define TK_LN_SALT_B1 0x4C4E423100000000ull
#define TK_LN_SALT_B2 0x4C4E423200000000ull
#define TK_LN_SALT_KIND 0x4C4E4B4900000000ull
// the sums of a document, uint64[TK_LN_SUMS][n_docs]: chars; then per kind: segments, their chars, distinct ones, chars of one per class
enum { TK_LN_S_CHARS = 0, TK_LN_S_SEG = 1, TK_LN_S_SEGCH = 2, TK_LN_S_DIST = 3, TK_LN_S_DISTCH = 4, TK_LN_S_BULLET = 9, TK_LN_S_ELLIPSIS = 10, TK_LN_SUMS = 11 };
enum { TK_LN_W_SEGS = 0, TK_LN_W_BAD = 1, TK_LN_WORDS = 2 };  // report words: segments of both kinds; doc_off does not ascend from 0 to N

struct TkLn {
    uint64_t B1, B2, seed, n_bytes, n_docs;
    uint32_t n_tiles;
    uint32_t norm;  // TK_LN_N_* of a normalising line set; 0 everywhere else
};
// The shape of a call.  0, or why it is refused: 1 n_bytes.
TK_HD uint64_t tk_ln_base(uint64_t seed, uint64_t salt) { return 257 + tk_fp_mix(seed ^ salt) % (TK_LN_P - 257); }
TK_HD int tk_ln_shape(uint64_t n_bytes, uint64_t n_docs, uint64_t seed, TkLn* p) {
    if (n_bytes > TK_LN_MAX_BYTES) return 1;
    p->B1 = tk_ln_base(seed, TK_LN_SALT_B1), p->B2 = tk_ln_base(seed, TK_LN_SALT_B2);
    p->seed = seed, p->n_bytes = n_bytes, p->n_docs = n_docs;
    p->n_tiles = (uint32_t)(n_bytes / TK_LN_TILE + 1);  // (position N lies in a tile)
    p->norm = 0;
    return 0;
}
// slots of the table for `segs` lines and paragraphs: the power of two >= 2 segs
TK_HD uint64_t tk_ln_slots(uint64_t segs) {
    uint64_t S = 2;
    while (S < 2 * segs) S <<= 1;
    return S;
}

TK_HD uint64_t tk_ln_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}
// a b mod p for a, b < 2^61: the 122-bit product is (hi 2^3 + lo >> 61) 2^61 + (lo & p), and 2^61 = 1
TK_HD uint64_t tk_ln_mulmod(uint64_t a, uint64_t b) {
    const uint64_t lo = a * b, hi = tk_ln_mulhi(a, b);
    uint64_t s = (lo & TK_LN_P) + ((hi << 3) | (lo >> 61));
    s = (s & TK_LN_P) + (s >> 61);
    return s >= TK_LN_P ? s - TK_LN_P : s;
}
TK_HD uint64_t tk_ln_addmod(uint64_t a, uint64_t b) {  // a, b < p
    const uint64_t s = a + b;
    return s >= TK_LN_P ? s - TK_LN_P : s;
}

struct TkLnEl {  // a run of bytes: the identity is the empty run
    uint64_t h1, w1, h2, w2;  // the two hashes and B1^bytes, B2^bytes
    uint32_t bytes, chars;
};
TK_HD TkLnEl tk_ln_empty() { return TkLnEl{0, 1, 0, 1, 0, 0}; }
TK_HD TkLnEl tk_ln_join(const TkLnEl& l, const TkLnEl& r) {
    return TkLnEl{tk_ln_addmod(tk_ln_mulmod(l.h1, r.w1), r.h1), tk_ln_mulmod(l.w1, r.w1), tk_ln_addmod(tk_ln_mulmod(l.h2, r.w2), r.h2), tk_ln_mulmod(l.w2, r.w2),
                  l.bytes + r.bytes, l.chars + r.chars};
}
// a run and whether a cut lies before its open end: what the scans carry.  (cut, run) of a range is the run behind its last cut.
struct TkLnSeg {
    TkLnEl e;
    uint32_t cut;
};
TK_HD TkLnSeg tk_ln_seg_join(const TkLnSeg& l, const TkLnSeg& r) { return r.cut ? r : TkLnSeg{tk_ln_join(l.e, r.e), l.cut}; }
// one byte behind a run whose powers nobody needs (h1, h2, bytes, chars only)
TK_HD void tk_ln_push(const TkLn& p, TkLnEl& e, uint32_t byte) {
    e.h1 = tk_ln_addmod(tk_ln_mulmod(e.h1, p.B1), byte + 1), e.h2 = tk_ln_addmod(tk_ln_mulmod(e.h2, p.B2), byte + 1);
    e.bytes += 1, e.chars += (byte & 0xC0u) != 0x80u;
}
// the key of a finished segment of document d (never 0: 0 is the empty slot)
TK_HD uint64_t tk_ln_key(const TkLn& p, uint32_t kind, uint64_t d, const TkLnEl& e) {
    uint64_t x = tk_fp_mix(p.seed ^ TK_LN_SALT_KIND ^ kind);
    x = tk_fp_mix(x ^ e.h1), x = tk_fp_mix(x ^ e.h2), x = tk_fp_mix(x ^ e.bytes), x = tk_fp_mix(x ^ d);
    return x ? x : 1;
}

// 16 bytes as two words, byte j at bits 8 (j & 7) of w[j >> 3]: bit j of the result is set where byte j == c (SWAR: no carry crosses a byte)
TK_HD uint32_t tk_ln_eq_mask(uint64_t lo, uint64_t hi, uint8_t c) {
    uint32_t m = 0;
    const uint64_t w[2] = {lo, hi};
    for (int i = 0; i < 2; ++i) {
        const uint64_t x = w[i] ^ (0x0101010101010101ull * c);
        const uint64_t z = ~(((x & 0x7F7F7F7F7F7F7F7Full) + 0x7F7F7F7F7F7F7F7Full) | x) & 0x8080808080808080ull;  // 0x80 where the byte is 0
        m |= (uint32_t)((z * 0x0002040810204081ull) >> 56) << (8 * i);                                             // the eight flags gathered
    }
    return m;
}
// ... where byte j is a continuation byte 0b10xxxxxx
TK_HD uint32_t tk_ln_cont_mask(uint64_t lo, uint64_t hi) {
    uint32_t m = 0;
    const uint64_t w[2] = {lo, hi};
    for (int i = 0; i < 2; ++i) {
        const uint64_t z = w[i] & ~(w[i] << 1) & 0x8080808080808080ull;
        m |= (uint32_t)((z * 0x0002040810204081ull) >> 56) << (8 * i);
    }
    return m;
}
// The masks of a lane, 16 bits each.  In: nl the newlines, valid the bytes below N, brk bit j: a document starts at byte j (17 bits: bit 16
// is the byte behind the lane), nl_before / nl_after: the bytes beside the lane are newlines (false outside the text).
//   content[TK_LN_LINE], content[TK_LN_PARA]; cut[kind] = brk | ~content: a segment ends before byte j
TK_HD void tk_ln_masks(uint32_t nl, uint32_t valid, uint32_t brk, bool nl_before, bool nl_after, uint32_t content[2], uint32_t cut[2]) {
    const uint32_t left = (nl << 1) | (nl_before ? 1u : 0u), right = (nl >> 1) | (nl_after ? 0x8000u : 0u);
    const uint32_t inner = nl & ~brk & ~(brk >> 1) & ~left & ~right;  // neither first nor last of its document, no newline beside it
    content[TK_LN_LINE] = valid & ~nl, content[TK_LN_PARA] = valid & (~nl | inner);
    cut[TK_LN_LINE] = (brk | ~content[TK_LN_LINE]) & 0xFFFFu, cut[TK_LN_PARA] = (brk | ~content[TK_LN_PARA]) & 0xFFFFu;
}
// A line of n bytes, at(i) its byte i: does it start with - * U+2022 U+25CF; does it end with ... or U+2026
template <class At>
TK_HD bool tk_ln_bullet(uint32_t n, At&& at) {
    const uint32_t a = at(0);
    if (a == '-' || a == '*') return true;
    return n >= 3 && a == 0xE2 && ((at(1) == 0x80 && at(2) == 0xA2) || (at(1) == 0x97 && at(2) == 0x8F));
}
template <class At>
TK_HD bool tk_ln_ellipsis(uint32_t n, At&& at) {
    if (n < 3) return false;
    const uint32_t a = at(n - 3), b = at(n - 2), c = at(n - 1);
    return (a == '.' && b == '.' && c == '.') || (a == 0xE2 && b == 0x80 && c == 0xA6);
}

// ------------------------------------------------------------------------------------------
// The normal form of a line: what a line set made with a `normalize` mask hashes in place of the line's bytes.  With TK_LN_N_PUNCT the
// 32 bytes of Python's string.punctuation are deleted, first; with TK_LN_N_CASE 'A'..'Z' become 'a'..'z'; with TK_LN_N_DIGITS '0'..'9'
// become '0'; with TK_LN_N_SPACE every maximal run of 0x09 0x0B 0x0C 0x0D 0x20 becomes one 0x20 and the runs at the line's ends vanish
// (b" ".join(x.split()) on a line, which holds no '\n').  Bytes >= 0x80 are never touched.
//
// The normal form composes as the hash does.  A scan value is the BODY of the bytes seen so far -- their normal form without the blanks
// at its ends: the two hashes, the powers, its length -- with the raw byte count, and flags beside the cut bit: LEAD, a body exists and
// white space precedes it; TRAIL, a body exists and white space follows it; WS, no body and white space was seen.  Two bodies join with
// one blank between them when the left has TRAIL or the right has LEAD -- a multiply by B and an add per hash, a multiply on the
// power --; a value without a body hands its white space to the near flag of the other; deleted bytes leave no trace but the raw count.
// The value has the size and the layout of TkLnSeg, with the body's length where the raw runs keep their chars: the passes that read
// only the raw count of the run that enters a tile (tk_k_ls_keep, tk_k_ls_write) read either.
// ------------------------------------------------------------------------------------------
#define TK_LN_N_CASE 1u
#define TK_LN_N_DIGITS 2u
#define TK_LN_N_SPACE 4u
#define TK_LN_N_PUNCT 8u
#define TK_LN_N_ALL 15u
#define TK_LN_NF_CUT 1u
#define TK_LN_NF_LEAD 2u
#define TK_LN_NF_TRAIL 4u
#define TK_LN_NF_WS 8u

struct TkLnNEl {
    uint64_t h1, w1, h2, w2;  // of the body
    uint32_t bytes, len;      // raw bytes; bytes of the body
};
struct TkLnNSeg {
    TkLnNEl e;
    uint32_t cut;  // TK_LN_NF_*
};
static_assert(sizeof(TkLnNSeg) == sizeof(TkLnSeg) && offsetof(TkLnNSeg, e.bytes) == offsetof(TkLnSeg, e.bytes), "the raw count of either scan value lies at one place");
TK_HD TkLnNSeg tk_lnn_empty() { return TkLnNSeg{TkLnNEl{0, 1, 0, 1, 0, 0}, 0u}; }
// a blank behind a body: hashes and powers
TK_HD void tk_lnn_blank(const TkLn& p, TkLnNEl& e) {
    e.h1 = tk_ln_addmod(tk_ln_mulmod(e.h1, p.B1), 0x21), e.h2 = tk_ln_addmod(tk_ln_mulmod(e.h2, p.B2), 0x21);
    e.w1 = tk_ln_mulmod(e.w1, p.B1), e.w2 = tk_ln_mulmod(e.w2, p.B2), e.len += 1;
}
// l then r, no cut between them: the cut bit is l's
TK_HD TkLnNSeg tk_lnn_join(const TkLn& p, const TkLnNSeg& l, const TkLnNSeg& r) {
    const bool lb = l.e.len != 0, rb = r.e.len != 0;
    TkLnNEl a = l.e;
    if (lb && rb && ((l.cut & TK_LN_NF_TRAIL) || (r.cut & TK_LN_NF_LEAD))) tk_lnn_blank(p, a);
    uint32_t f = l.cut & TK_LN_NF_CUT;
    if (lb) f |= l.cut & TK_LN_NF_LEAD;
    else if (rb) f |= (r.cut & TK_LN_NF_LEAD) | ((l.cut & TK_LN_NF_WS) ? TK_LN_NF_LEAD : 0u);
    if (rb) f |= r.cut & TK_LN_NF_TRAIL;
    else if (lb) f |= (l.cut & TK_LN_NF_TRAIL) | ((r.cut & TK_LN_NF_WS) ? TK_LN_NF_TRAIL : 0u);
    if (!lb && !rb) f |= (l.cut | r.cut) & TK_LN_NF_WS;
    return TkLnNSeg{TkLnNEl{tk_ln_addmod(tk_ln_mulmod(a.h1, r.e.w1), r.e.h1), tk_ln_mulmod(a.w1, r.e.w1), tk_ln_addmod(tk_ln_mulmod(a.h2, r.e.w2), r.e.h2),
                            tk_ln_mulmod(a.w2, r.e.w2), l.e.bytes + r.e.bytes, a.len + r.e.len},
                    f};
}
TK_HD TkLnNSeg tk_lnn_seg_join(const TkLn& p, const TkLnNSeg& l, const TkLnNSeg& r) { return (r.cut & TK_LN_NF_CUT) ? r : tk_lnn_join(p, l, r); }

// 8 bytes: 0x80 where lo <= byte <= hi, for 1 <= lo <= hi < 0x80 (SWAR: the sums stay below 0x100, no carry crosses a byte)
TK_HD uint64_t tk_ln_in_range(uint64_t w, uint8_t lo, uint8_t hi) {
    const uint64_t ones = 0x0101010101010101ull, x = w & (0x7Full * ones);
    return (x + (0x80u - lo) * ones) & ~(x + (0x7Fu - hi) * ones) & ~w & (0x80ull * ones);
}
TK_HD uint32_t tk_ln_gather(uint64_t z) { return (uint32_t)((z * 0x0002040810204081ull) >> 56); }  // the eight 0x80 flags of z as bits 0 .. 7
// A lane's 16 bytes under the mask `norm`: the bytes with case and digits mapped; bit j of del: byte j is deleted; of ws: it is white space
struct TkLnNLane {
    uint64_t lo, hi;
    uint32_t del, ws;
    TK_HD uint32_t byte(uint32_t j) const { return (uint32_t)((j < 8 ? lo >> (8 * j) : hi >> (8 * (j - 8))) & 0xFFu); }
};
TK_HD uint64_t tk_lnn_word(uint64_t x, uint32_t norm, uint32_t shift, uint32_t& del, uint32_t& ws) {
    const uint64_t upper = tk_ln_in_range(x, 'A', 'Z'), digit = tk_ln_in_range(x, '0', '9');
    const uint64_t space = tk_ln_in_range(x, 0x0B, 0x0D) | tk_ln_in_range(x, 0x09, 0x09) | tk_ln_in_range(x, 0x20, 0x20);
    const uint64_t punct = tk_ln_in_range(x, 0x21, 0x2F) | tk_ln_in_range(x, 0x3A, 0x40) | tk_ln_in_range(x, 0x5B, 0x60) | tk_ln_in_range(x, 0x7B, 0x7E);
    if (norm & TK_LN_N_SPACE) ws |= tk_ln_gather(space) << shift;
    if (norm & TK_LN_N_PUNCT) del |= tk_ln_gather(punct) << shift;
    if (norm & TK_LN_N_CASE) x |= upper >> 2;                   // + 0x20
    if (norm & TK_LN_N_DIGITS) x &= ~((digit >> 7) * 0x0Full);  // the low nibble to 0
    return x;
}
TK_HD TkLnNLane tk_lnn_lane(uint64_t lo, uint64_t hi, uint32_t norm) {
    TkLnNLane c{0, 0, 0u, 0u};
    c.lo = tk_lnn_word(lo, norm, 0u, c.del, c.ws), c.hi = tk_lnn_word(hi, norm, 8u, c.del, c.ws);
    return c;
}
// one byte that is not deleted behind a run whose powers and raw count nobody needs here; ws: it is white space
TK_HD void tk_lnn_push(const TkLn& p, TkLnNSeg& s, uint32_t byte, bool ws) {
    if (ws) {
        s.cut |= s.e.len ? TK_LN_NF_TRAIL : TK_LN_NF_WS;
        return;
    }
    if (s.cut & TK_LN_NF_TRAIL) {
        s.e.h1 = tk_ln_addmod(tk_ln_mulmod(s.e.h1, p.B1), 0x21), s.e.h2 = tk_ln_addmod(tk_ln_mulmod(s.e.h2, p.B2), 0x21);
        s.e.len += 1, s.cut &= ~TK_LN_NF_TRAIL;
    } else if (s.cut & TK_LN_NF_WS) {
        s.cut ^= TK_LN_NF_WS | TK_LN_NF_LEAD;
    }
    s.e.h1 = tk_ln_addmod(tk_ln_mulmod(s.e.h1, p.B1), byte + 1), s.e.h2 = tk_ln_addmod(tk_ln_mulmod(s.e.h2, p.B2), byte + 1);
    s.e.len += 1;
}
// the bytes [from, to) of a lane behind a run, the raw count with them: only the bytes that reach the body cost a multiply
TK_HD void tk_lnn_append(const TkLn& p, const TkLnNLane& c, uint32_t from, uint32_t to, TkLnNSeg& s) {
    s.e.bytes += to - from;
    for (uint32_t m = ~c.del & ((1u << to) - (1u << from)); m; m &= m - 1u) {
        const uint32_t j = (uint32_t)__builtin_ctz(m);
        tk_lnn_push(p, s, c.byte(j), (c.ws >> j) & 1u);
    }
}
