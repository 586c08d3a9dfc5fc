// Cleaning packed text line by line: the parts of the device passes of tk_clean.h that are plain C++ -- the fold, the phrase table and
// its first-byte set, the shape of a call, the masks of a lane beside the word rule's, the element the scans carry and its join, a
// stretch of a lane as such an element, the line that closes at a cut, its verdict, and the bytes of dropped documents.  The rule is
// stated in include/tiktoken_amd.h.  Compiles for the host.
//
// Lines.  A position is a LINE CUT when a document starts there or its byte is '\n' or lies behind the text (position N is one); a line
// is a maximal run of other bytes and is handed out at the cut that ends it, by the lane whose 16 bytes hold the cut.  Words are the
// word rule's (tk_words_rule.h): inside a line only a white-space byte ends one, for '\n' is white space and a document start is a cut.
// The element.  TkClSt describes the line that is open at a range's end, from the range's last line cut on: where it starts; the words
// that lie between two white-space bytes of the range, and the longest of them; the chars before the range's first white-space byte
// (`head`) and behind its last one (`open`) -- a range without white space has `open` alone, the word that runs through it --, so a
// word that a lane, wavefront or tile edge cuts is head + open of its two sides and measured once; a flag each that a word's BYTES lie
// there, for a word of continuation bytes alone is a word of no char and counts; whether a line phrase occurs; and the
// position behind the line's last byte that is not blank, from which the verdict reads the end's last three bytes.  Sums, maxima and
// ORs: two ranges join without a multiplication, and a range with a line cut hands on only what lies behind it.
#pragma once
#include <stdint.h>

#include "tk_line_set_rule.h"  // tk_ls_open_start, tk_ls_keep_mask, tk_ls_bitmap_words
#include "tk_words_rule.h"     // the white-space patterns: tk_wd_lane_masks, TkWdLane; tk_wd_in, tk_wd_gather

#define TK_CL_TILE 4096u     // bytes of text per workgroup
#define TK_CL_THREADS 256u   // its lanes
#define TK_CL_LANE 16u       // bytes per lane: one 16-byte load
#define TK_CL_WAVE 1024u     // bytes per wavefront
#define TK_CL_DOCS 256u      // documents of a tile whose sums are gathered in LDS; the rest add to HBM directly
#define TK_CL_MAX_BYTES 0xFFFF0000ull
#define TK_CL_MAX_PHRASES 16u       // of a list
#define TK_CL_MAX_PHRASE_BYTES 32u
#define TK_CL_MAX_TERMINAL 16u
#define TK_CL_SLOTS (2u * TK_CL_MAX_PHRASES)  // line phrase i in slot i, document phrase i in slot 16 + i
#define TK_CL_ELLIPSIS 1u                     // spec flag: TK_CLEAN_ELLIPSIS
// the sums of a document, uint64[TK_CL_SUMS][n_docs]
enum { TK_CL_S_LINES = 0, TK_CL_S_DROPPED, TK_CL_S_SHORT, TK_CL_S_LONG, TK_CL_S_NO_END, TK_CL_S_ELLIPSIS, TK_CL_S_PHRASE, TK_CL_S_HIT, TK_CL_SUMS };
enum { TK_CL_R_SHORT = 1u, TK_CL_R_LONG = 2u, TK_CL_R_NO_END = 4u, TK_CL_R_ELLIPSIS = 8u, TK_CL_R_PHRASE = 16u };  // the rules that hold for a line

struct TkCl {
    uint64_t n_bytes, n_docs, min_words, max_word_chars;
    uint32_t n_tiles, flags, n_line, n_doc, n_terminal;
    uint32_t terminal[4];                                       // bit b: the ASCII byte b is terminal
    uint32_t first[8];                                          // bit b: a phrase starts with the folded byte b
    uint32_t ph[TK_CL_SLOTS][TK_CL_MAX_PHRASE_BYTES / 4];  // the folded bytes of a slot's phrase, little-endian
    uint8_t len[TK_CL_SLOTS];                                   // 0: the slot is empty
};

TK_HD uint32_t tk_cl_fold(uint32_t b) { return b - 0x41u < 26u ? b + 0x20u : b; }
TK_HD uint64_t tk_cl_fold8(uint64_t w) { return w + (tk_wd_in(w, 'A', 'Z') >> 2); }  // eight bytes at once: 0x80 >> 2 is 0x20, no carry
TK_HD uint32_t tk_cl_ph_byte(const uint32_t* ph, uint32_t k) { return (ph[k >> 2] >> (8u * (k & 3u))) & 0xFFu; }

// The shape of a call.  0, or why it is refused: 1 n_bytes; 2 more than 16 phrases in a list; 3 a phrase that is empty or longer than
// 32 bytes; 4 a line phrase with '\n'; 5 more than 16 terminal bytes; 6 a terminal byte >= 0x80.
TK_HD int tk_cl_shape(uint64_t n_bytes, uint64_t n_docs, uint64_t min_words, uint64_t max_word_chars, uint32_t flags, const uint8_t* terminal, uint64_t n_terminal,
                      const uint8_t* line_bytes, const uint64_t* line_off, uint64_t n_line, const uint8_t* doc_bytes, const uint64_t* doc_off, uint64_t n_doc, TkCl* p) {
    if (n_bytes > TK_CL_MAX_BYTES) return 1;
    if (n_line > TK_CL_MAX_PHRASES || n_doc > TK_CL_MAX_PHRASES) return 2;
    if (n_terminal > TK_CL_MAX_TERMINAL) return 5;
    p->n_bytes = n_bytes, p->n_docs = n_docs, p->min_words = min_words, p->max_word_chars = max_word_chars;
    p->n_tiles = (uint32_t)(n_bytes / TK_CL_TILE + 1);  // (position N lies in a tile)
    p->flags = flags, p->n_line = (uint32_t)n_line, p->n_doc = (uint32_t)n_doc, p->n_terminal = (uint32_t)n_terminal;
    for (uint32_t i = 0; i < 8; ++i) p->first[i] = 0;
    for (uint32_t s = 0; s < TK_CL_SLOTS; ++s) {
        p->len[s] = 0;
        for (uint32_t k = 0; k < TK_CL_MAX_PHRASE_BYTES / 4; ++k) p->ph[s][k] = 0;
        const bool line = s < TK_CL_MAX_PHRASES;
        const uint64_t i = line ? s : s - TK_CL_MAX_PHRASES;
        if (i >= (line ? n_line : n_doc)) continue;
        const uint8_t* bytes = line ? line_bytes : doc_bytes;
        const uint64_t a = (line ? line_off : doc_off)[i], b = (line ? line_off : doc_off)[i + 1];
        if (b <= a || b - a > TK_CL_MAX_PHRASE_BYTES) return 3;
        for (uint32_t k = 0; k < (uint32_t)(b - a); ++k) {
            if (line && bytes[a + k] == '\n') return 4;
            p->ph[s][k >> 2] |= tk_cl_fold(bytes[a + k]) << (8u * (k & 3u));
        }
        p->len[s] = (uint8_t)(b - a);
        const uint32_t f = tk_cl_ph_byte(p->ph[s], 0);
        p->first[f >> 5] |= 1u << (f & 31u);
    }
    for (uint32_t i = 0; i < 4; ++i) p->terminal[i] = 0;
    for (uint64_t i = 0; i < n_terminal; ++i) {
        if (terminal[i] >= 0x80u) return 6;
        p->terminal[terminal[i] >> 5] |= 1u << (terminal[i] & 31u);
    }
    return 0;
}
TK_HD bool tk_cl_is_terminal(const TkCl& q, uint32_t byte) {
    const uint32_t w = byte >> 5, t = w == 0 ? q.terminal[0] : w == 1 ? q.terminal[1] : w == 2 ? q.terminal[2] : q.terminal[3];
    return byte < 0x80u && ((t >> (byte & 31u)) & 1u);
}
// Does the phrase `ph` of `len` bytes occur where the folded bytes are at(0), at(1), ...?  room: the bytes from there to the end of the
// document (and of the text).  (The device has compared at(0), and at(1) of a longer phrase, before it comes here; again is cheap.)
template <class At>
TK_HD bool tk_cl_occurs(const uint32_t* ph, uint32_t len, uint32_t room, At&& at) {
    if (!len || len > room) return false;
    for (uint32_t k = 0; k < len; ++k)
        if (at(k) != tk_cl_ph_byte(ph, k)) return false;
    return true;
}

struct TkClLane {  // what a lane knows of its 16 bytes beside the word rule's view; masks of 16 bits, bit j: byte j
    TkWdLane w;
    uint32_t at;        // the position of its first byte in the text
    uint32_t valid;     // a byte below N
    uint32_t lcontent;  // a byte of a line: valid and not '\n'
    uint32_t lcut;      // a line ends before byte j: a document start, a '\n', a byte behind the text
    uint32_t nonblank;  // a byte of a line that is not 0x20, 0x09, 0x0D
    uint32_t lhit;      // a line phrase occurs at byte j
};
// ... from the word rule's view: n_left as for tk_wd_lane_masks
TK_HD void tk_cl_lane_masks(uint32_t at, uint32_t n_left, TkClLane* L) {
    const uint64_t lo = L->w.lo, hi = L->w.hi;
    L->at = at, L->valid = n_left >= 16u ? 0xFFFFu : (1u << n_left) - 1u;
    const uint32_t nl = tk_wd_gather(tk_wd_in(lo, '\n', '\n'), tk_wd_in(hi, '\n', '\n'));
    const uint32_t blank = tk_wd_gather(tk_wd_in(lo, ' ', ' ') | tk_wd_in(lo, '\t', '\t') | tk_wd_in(lo, '\r', '\r'), tk_wd_in(hi, ' ', ' ') | tk_wd_in(hi, '\t', '\t') | tk_wd_in(hi, '\r', '\r'));
    L->lcontent = L->valid & ~nl;
    L->lcut = (L->w.brk | ~L->lcontent) & 0xFFFFu;
    L->nonblank = L->lcontent & ~blank;
    L->lhit = 0;
}

// What the scans carry.  The identity is all zero.
struct TkClSt {
    uint32_t start;           // where the open line starts (with TK_CL_F_LCUT; a range without a line cut leaves it to the range before it)
    uint32_t words, longest;  // the words between two white-space bytes, and the chars of the longest
    uint32_t head, open;      // the chars before the first white-space byte (0 without one) and behind the last one
    uint32_t end;             // 1 + the position of the last byte that is not blank; 0: there is none
    uint32_t flags;           // TK_CL_F_*
};
// LCUT: the range holds a line cut; WCUT: a white-space byte behind it; HEADW, OPENW: a word's bytes lie before the first / behind the last
// white-space byte (without one: OPENW, in the range) -- apart from `head` and `open`, for a word of continuation bytes alone has no char
enum { TK_CL_F_LCUT = 1u, TK_CL_F_WCUT = 2u, TK_CL_F_PHRASE = 4u, TK_CL_F_HEADW = 8u, TK_CL_F_OPENW = 16u };
TK_HD TkClSt tk_cl_empty() { return TkClSt{0, 0, 0, 0, 0, 0, 0}; }
TK_HD uint32_t tk_cl_max(uint32_t a, uint32_t b) { return a > b ? a : b; }
TK_HD TkClSt tk_cl_join(const TkClSt& l, const TkClSt& r) {
    if (r.flags & TK_CL_F_LCUT) return r;
    TkClSt o = l;
    if (r.end) o.end = r.end;
    if (!(r.flags & TK_CL_F_WCUT)) {  // (r has neither head nor TK_CL_F_HEADW)
        o.open = l.open + r.open, o.flags |= r.flags;
        return o;
    }
    const uint32_t mid = l.open + r.head;  // the word that the edge cuts, if there is one: it may have bytes and no char
    const uint32_t midw = ((l.flags & TK_CL_F_OPENW) || (r.flags & TK_CL_F_HEADW)) ? 1u : 0u;
    o.open = r.open;
    o.flags = ((l.flags | r.flags) & ~(uint32_t)(TK_CL_F_HEADW | TK_CL_F_OPENW)) | (r.flags & TK_CL_F_OPENW);
    if (l.flags & TK_CL_F_WCUT) o.words = l.words + r.words + midw, o.longest = tk_cl_max(tk_cl_max(l.longest, r.longest), mid), o.flags |= l.flags & TK_CL_F_HEADW;
    else o.head = mid, o.words = r.words, o.longest = r.longest, o.flags |= midw ? (uint32_t)TK_CL_F_HEADW : 0u;
    return o;
}

TK_HD uint32_t tk_cl_bits(uint32_t s, uint32_t e) { return ((1u << e) - 1u) & ~((1u << s) - 1u); }  // s <= e <= 16
TK_HD uint32_t tk_cl_top(uint32_t m) { return 31u - (uint32_t)__builtin_clz(m); }                    // m != 0
// Bytes [s, e) of a lane, with no line cut among them but a document start at s, as an element (neither start nor TK_CL_F_LCUT)
TK_HD TkClSt tk_cl_part(const TkClLane& L, uint32_t s, uint32_t e) {
    const uint32_t R = tk_cl_bits(s, e), ws = ~L.w.content & R, nb = L.nonblank & R;
    TkClSt o = tk_cl_empty();
    if (nb) o.end = L.at + tk_cl_top(nb) + 1u;
    if (L.lhit & R) o.flags |= TK_CL_F_PHRASE;
    if (!ws) {
        o.open = (uint32_t)__builtin_popcount(L.w.lead & R);
        if (L.w.content & R) o.flags |= TK_CL_F_OPENW;
        return o;
    }
    const uint32_t f = (uint32_t)__builtin_ctz(ws), g = tk_cl_top(ws);
    o.flags |= TK_CL_F_WCUT;
    o.head = (uint32_t)__builtin_popcount(L.w.lead & tk_cl_bits(s, f)), o.open = (uint32_t)__builtin_popcount(L.w.lead & tk_cl_bits(g + 1u, e));
    if (L.w.content & tk_cl_bits(s, f)) o.flags |= TK_CL_F_HEADW;
    if (L.w.content & tk_cl_bits(g + 1u, e)) o.flags |= TK_CL_F_OPENW;
    for (uint32_t m = L.w.content & tk_cl_bits(f, g); m;) {  // (bit g is clear: every word here ends at or before it)
        const uint32_t a = (uint32_t)__builtin_ctz(m), b = (uint32_t)__builtin_ctz(~m & ~((1u << a) - 1u));
        o.words += 1u, o.longest = tk_cl_max(o.longest, (uint32_t)__builtin_popcount(L.w.lead & tk_cl_bits(a, b)));
        m &= ~((1u << b) - 1u);
    }
    return o;
}
// where the line starts that a cut at byte l opens: at l when a document starts on a line byte there, else behind it
TK_HD uint32_t tk_cl_from(const TkClLane& L, uint32_t l) { return l + (((L.lcontent >> l) & 1u) ^ 1u); }
// The lane as the scans see it: the line behind its last line cut
TK_HD TkClSt tk_cl_lane_tail(const TkClLane& L) {
    if (!L.lcut) return tk_cl_part(L, 0, TK_CL_LANE);
    const uint32_t from = tk_cl_from(L, tk_cl_top(L.lcut));
    TkClSt o = tk_cl_part(L, from, TK_CL_LANE);
    o.start = L.at + from, o.flags |= TK_CL_F_LCUT;
    return o;
}
// bit j: a line ends before byte j of the lane; `before`: the scanned element that enters the lane (its line is empty when it starts here)
TK_HD uint32_t tk_cl_closes(const TkClLane& L, const TkClSt& before) { return L.lcut & ((L.lcontent << 1) | (before.start < L.at ? 1u : 0u)); }
// ... that line, whole: `start` is set
TK_HD TkClSt tk_cl_line(const TkClLane& L, const TkClSt& before, uint32_t j) {
    const uint32_t low = L.lcut & ((1u << j) - 1u);
    if (!low) return tk_cl_join(before, tk_cl_part(L, 0, j));
    const uint32_t from = tk_cl_from(L, tk_cl_top(low));
    TkClSt o = tk_cl_part(L, from, j);
    o.start = L.at + from;
    return o;
}
// The rules that hold for a whole line (TK_CL_R_*); at(pos): the byte of the text at a position of the line
template <class At>
TK_HD uint32_t tk_cl_judge(const TkCl& q, const TkClSt& s, At&& at) {
    const uint64_t words = (uint64_t)s.words + ((s.flags & TK_CL_F_HEADW) ? 1u : 0u) + ((s.flags & TK_CL_F_OPENW) ? 1u : 0u), longest = tk_cl_max(tk_cl_max(s.longest, s.head), s.open);
    uint32_t r = 0;
    if (q.min_words && words < q.min_words) r |= TK_CL_R_SHORT;
    if (q.max_word_chars && longest > q.max_word_chars) r |= TK_CL_R_LONG;
    if (q.n_terminal && (!s.end || !tk_cl_is_terminal(q, at(s.end - 1u)))) r |= TK_CL_R_NO_END;
    if ((q.flags & TK_CL_ELLIPSIS) && (uint64_t)s.end >= (uint64_t)s.start + 3u) {
        const uint32_t a = at(s.end - 3u), b = at(s.end - 2u), c = at(s.end - 1u);
        if ((a == '.' && b == '.' && c == '.') || (a == 0xE2u && b == 0x80u && c == 0xA6u)) r |= TK_CL_R_ELLIPSIS;
    }
    if (s.flags & TK_CL_F_PHRASE) r |= TK_CL_R_PHRASE;
    return r;
}
// bit j: byte j of the lane lies in a dropped document.  brk: the word rule's; li0: the local document of byte 0; dropped(li, j): the
// answer for local document li, which owns the lane's byte j.
template <class D>
TK_HD uint32_t tk_cl_doc_mask(uint32_t valid, uint32_t brk, uint32_t li0, D&& dropped) {
    uint32_t out = 0, from = 0, li = li0, rest = brk & valid & 0xFFFEu;
    while (true) {
        const uint32_t to = rest ? (uint32_t)__builtin_ctz(rest) : TK_CL_LANE, R = tk_cl_bits(from, to) & valid;
        if (R && dropped(li, from)) out |= R;
        if (!rest) break;
        rest &= rest - 1u, from = to, ++li;
    }
    return out;
}
