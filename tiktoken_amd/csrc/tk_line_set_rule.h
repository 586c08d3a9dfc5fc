// Line sets: the parts of the device passes of tk_line_set.h that are plain C++ -- the shape of a set, a line's key, the word that says
// which occurrence of a key is the first, the walk that finds a key's slot, where the run that is open at a lane's end starts, and the keep
// mask of a lane's 16 bytes.  The rule is stated in include/tiktoken_amd.h.  Compiles for the host.
//
// Key.  The two polynomial hashes of tk_lines_rule.h, under bases drawn from the set's seed, the byte length and a salt of the line
// sets, mixed into 64 bits; the document's index is NOT in it, which is the difference from tk_ln_key.  Two different lines meet with
// about 2^-64 + len^2 / 2^122 per pair, as there: a hash decides.
//
// First.  Beside every slot of the table lies a second word, all ones while the slot has never been marked.  An add call with the
// set's call counter `epoch` does an atomic minimum of (epoch << 32) | start on it for every eligible line of the key: a word of an
// earlier call is smaller and stays, among the lines of one call the lowest start wins, whoever claimed the slot.  So a line of call
// `epoch` is the kept occurrence exactly when the word equals (epoch, its start), and no pass over the table tidies up between calls.
#pragma once
#include <stdint.h>

#include "tk_lines_rule.h"

#define TK_LS_MAX_CAPACITY (1ull << 30)
#define TK_LS_SALT_KEY 0x4C53455400000000ull
#define TK_LS_FRESH 0xFFFFFFFFFFFFFFFFull  // the second word of a slot that no call has marked
#define TK_LS_MAX_EPOCH 0xFFFFFFFEu       // add calls between two clears
enum { TK_LS_W_DROPPED = 0, TK_LS_WORDS = 1 };  // the report word of a call beside the line statistics' two: the lines dropped

struct TkLs {
    TkLn ln;             // the call's text: bases and seed are the set's
    uint64_t S;          // slots of the table
    uint64_t min_bytes;  // a shorter line is never dropped and never added
    uint32_t epoch;      // of this call, 1 ..; 0 for a call that does not add
};

// The shape of a set: the slots of its table, the power of two >= 2 capacity.  0, or why it is refused: 1 min_bytes, 2 capacity.
TK_HD int tk_ls_shape(uint64_t capacity, uint64_t min_bytes, uint64_t* S) {
    if (min_bytes < 1) return 1;
    if (capacity < 1 || capacity > TK_LS_MAX_CAPACITY) return 2;
    *S = tk_ln_slots(capacity);
    return 0;
}
// the key of a finished line (never 0: 0 is the empty slot)
TK_HD uint64_t tk_ls_key(uint64_t seed, const TkLnEl& e) {
    uint64_t x = tk_fp_mix(seed ^ TK_LS_SALT_KEY);
    x = tk_fp_mix(x ^ e.h1), x = tk_fp_mix(x ^ e.h2), x = tk_fp_mix(x ^ e.bytes);
    return x ? x : 1;
}
// A normalising set (ln.norm != 0): the same key over the line's normal form -- its two hashes and ITS length; a line is eligible when
// its normal form has min_bytes bytes, so a line of blanks and deleted bytes alone, whose normal form is empty, never is.  With a mask
// of 0 the normal form is the line and both are the plain set's.
TK_HD uint64_t tk_ls_key(uint64_t seed, const TkLnNEl& e) { return tk_ls_key(seed, TkLnEl{e.h1, 1, e.h2, 1, e.len, 0}); }
TK_HD bool tk_ls_eligible(const TkLs& q, const TkLnSeg& line) { return line.e.bytes >= q.min_bytes; }
TK_HD bool tk_ls_eligible(const TkLs& q, const TkLnNSeg& line) { return line.e.len >= q.min_bytes; }
TK_HD uint64_t tk_ls_first(uint32_t epoch, uint32_t start) { return ((uint64_t)epoch << 32) | start; }
// The slot of `key`, S when it is not in the table.  The walk ends at the key or at an empty slot, as tk_ng_probe's.
template <class Table>
TK_HD uint64_t tk_ls_find(const Table& table, uint64_t S, uint64_t key) {
    uint64_t i = key & (S - 1);
    for (uint64_t n = 0; n < S; ++n, i = (i + 1) & (S - 1)) {
        const uint64_t v = table[i];
        if (v == key) return i;
        if (v == 0) break;
    }
    return S;
}
TK_HD uint64_t tk_ls_bitmap_words(uint64_t n_bytes) { return n_bytes / 64 + 1; }  // 64-bit words of a bit per position 0 .. N

// Where the run that is open at the end of a lane starts, as a position of the text; 0 when the lane has no cut (the run that entered
// it goes on).  `at`: the position of the lane's first byte.  An exclusive maximum over the lanes before a lane, begun with the start
// of the run that enters the tile, is the start of the run that enters the lane -- `at` itself when that run is empty.
TK_HD uint32_t tk_ls_open_start(uint32_t cut, uint32_t content, uint32_t at) {
    if (!cut) return 0;
    uint32_t l = 15;
    while (!((cut >> l) & 1u)) --l;
    return at + l + (((content >> l) & 1u) ^ 1u);  // (a cut by a document start: its byte opens the run)
}
// The keep mask of a lane: bit j is set when byte j goes to the output.  valid, content, cut: the lane's masks of the line kind; brk bit
// j: a document starts at byte j; at: the position of the lane's first byte; s_in: where the run that enters the lane starts;
// dropped(start): the drop bit of the line that starts there.  Kept: the content of the lines that are not dropped, and every '\n' but
// the one that directly follows a dropped line inside the same document.  A lane without a cut lies inside one line: one read.
template <class Bit>
TK_HD uint32_t tk_ls_keep_mask(uint32_t valid, uint32_t content, uint32_t cut, uint32_t brk, uint32_t at, uint32_t s_in, Bit&& dropped) {
    if (!valid) return 0;
    if (!cut) return dropped(s_in) ? 0u : valid;
    bool open = s_in < at;  // the byte before byte j is content of a line
    bool drop = open && dropped(s_in);
    uint32_t keep = 0;
    for (uint32_t j = 0; j < TK_LN_LANE && ((valid >> j) & 1u); ++j) {
        const bool starts = (brk >> j) & 1u;
        if ((content >> j) & 1u) {
            if (!open || starts) drop = dropped(at + j), open = true;
            if (!drop) keep |= 1u << j;
        } else {
            if (!(open && !starts && drop)) keep |= 1u << j;
            open = false;
        }
    }
    return keep;
}
