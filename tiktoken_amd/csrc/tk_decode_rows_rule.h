// Decoding id matrices: the parts of the device passes of tk_decode_rows.h that are plain C++ -- what a tk_drows_spec and the figures of a
// call may say, which row and which columns a tile covers, what a row's begin and end must satisfy, the stop test, the live range, which live
// ids are kept and which of them have no decode entry, and a whole lane of the stop, the count and the write pass.  Compiles for the host
// too: tests/test_decode_rows_sim.py drives them lane by lane on the CPU behind readers that check every index.  The rule itself is stated
// in include/tiktoken_amd.h (tk_decode_rows_device).
//
// An element travels as a 64-bit value whatever the matrix holds: a uint32 as it is, an int32 or int64 sign-extended, so a negative one and
// one at or above 2^32 are both "at or above 2^32": in no list, without a decode entry.
#pragma once
#include <stdint.h>

#include "tk_decode_rule.h"  // TK_DEC_SPEC, TK_DEC_BLOCK
#include "tk_rows_rule.h"    // tk_report_min

#define TK_DROWSF_KEEP_STOP 1u  // (= TK_DROWS_KEEP_STOP .. TK_DROWS_I64 of the C ABI; tk_api.hip asserts it)
#define TK_DROWSF_SKIP_SPECIAL 2u
#define TK_DROWSF_I32 4u
#define TK_DROWSF_I64 8u
#define TK_DROWS_LIST 16  // most stop ids, most skip ids

// the words the passes report in (unsigned long long each): the first row whose begin / end offend, the row-major position r * W + c of the
// first kept element without a decode entry (both start as all ones = none), the kept ids of all rows
enum { TK_DROWS_BAD_ROW = 0, TK_DROWS_BAD_ID, TK_DROWS_K, TK_DROWS_WORDS };

struct TkDrows {
    uint64_t R, ld;  // rows; elements from one row's column 0 to the next row's
    uint32_t W;      // columns
    uint32_t flags, n_stop, n_skip;
    uint32_t tiles;  // tiles of a row: at least one, so that every row has a tile 0 (its thread 0 checks begin and end) even when W == 0
    uint32_t stop[TK_DROWS_LIST], skip[TK_DROWS_LIST];
};

// What the spec and the figures of a call alone decide (`block`: columns per tile).  0, or why it is refused: 1 too many stop ids, 2 too
// many skip ids, 3 both dtype flags, 4 ld < W, 5 R >= 2^32 - 1, 6 W >= 2^32, 7 an unknown flag, 8 (R - 1) * ld + W does not fit 2^60 elements.
TK_HD int tk_drows_shape(uint64_t R, uint64_t W, uint64_t ld, uint32_t flags, uint32_t n_stop, const uint32_t* stop, uint32_t n_skip, const uint32_t* skip, uint32_t block,
                         TkDrows* p) {
    if (flags & ~(TK_DROWSF_KEEP_STOP | TK_DROWSF_SKIP_SPECIAL | TK_DROWSF_I32 | TK_DROWSF_I64)) return 7;
    if (n_stop > TK_DROWS_LIST) return 1;
    if (n_skip > TK_DROWS_LIST) return 2;
    if ((flags & TK_DROWSF_I32) && (flags & TK_DROWSF_I64)) return 3;
    if (W >> 32) return 6;
    if (ld < W) return 4;
    if (R >= 0xFFFFFFFFull) return 5;
    if (R > 1 && ld >= (1ull << 60) / (R - 1)) return 8;
    p->R = R;
    p->ld = ld;
    p->W = (uint32_t)W;
    p->flags = flags;
    p->n_stop = n_stop;
    p->n_skip = n_skip;
    p->tiles = W ? (uint32_t)((W + block - 1) / block) : 1u;
    for (uint32_t k = 0; k < TK_DROWS_LIST; ++k) {
        p->stop[k] = k < n_stop ? stop[k] : 0u;
        p->skip[k] = k < n_skip ? skip[k] : 0u;
    }
    return 0;
}
// bytes of an element
TK_HD uint32_t tk_drows_elem_size(uint32_t flags) { return (flags & TK_DROWSF_I64) ? 8u : 4u; }
// the tiles of a call (R * tiles: below 2^64, R and tiles are both below 2^32)
TK_HD uint64_t tk_drows_n_tiles(const TkDrows& p) { return p.R * p.tiles; }
// Tile t < n_tiles: its row, and its first column (a multiple of `block`; with W == 0 the one tile of a row has no column)
TK_HD void tk_drows_tile(const TkDrows& p, uint64_t t, uint32_t block, uint64_t* r, uint64_t* col0) {
    *r = t / p.tiles;
    *col0 = (t - *r * p.tiles) * block;
}

// begin and end of row r (null: 0 and W).  A row with begin > end or end > W offends: it is reported by tile 0 of the row alone (`report`),
// and every pass treats it as a row without columns, so nothing is indexed with what it says.
template <class Bounds>
TK_HD bool tk_drows_range(const TkDrows& p, Bounds begin, bool has_begin, Bounds end, bool has_end, uint64_t r, uint32_t* b, uint32_t* e) {
    *b = has_begin ? begin[r] : 0u;
    *e = has_end ? end[r] : p.W;
    if (*b > *e || *e > p.W) {
        *b = *e = 0u;
        return false;
    }
    return true;
}

// v is in a list of n <= 16 ids.  The lists are uniform over a call and arrive as kernel arguments: all sixteen entries are named by a
// constant index, so they stay in scalar registers instead of a copy of the struct in private memory.
TK_HD bool tk_drows_listed(const uint32_t (&list)[TK_DROWS_LIST], uint32_t n, uint64_t v) {
    const uint32_t low = (uint32_t)v;
    bool hit = false;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t k = 0; k < TK_DROWS_LIST; ++k) hit |= k < n && list[k] == low;
    return hit && !(v >> 32);  // (a v at or above 2^32 equals no uint32)
}

// The columns [lo, hi) of row r that fall into a lane's eight from c0 on (c0 a multiple of 8, below W): bit j = column c0 + j is one, and
// v[j] = its element.  The eight arrive at once -- ids.eight: 16-byte loads -- where all of them are columns of the row and their address
// allows it, otherwise one by one, and only those asked for: nothing is read outside row r's columns [0, W).
template <class Ids>
TK_HD uint32_t tk_drows_lane_load(const TkDrows& p, const Ids& ids, uint64_t r, uint64_t c0, uint64_t lo, uint64_t hi, uint64_t v[8]) {
    uint32_t in = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t j = 0; j < 8; ++j) {
        v[j] = 0;
        if (c0 + j >= lo && c0 + j < hi) in |= 1u << j;
    }
    if (!in) return 0u;
    const uint64_t at = r * p.ld + c0;
    if (c0 + 8 <= p.W && ids.eight(at, v)) return in;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t j = 0; j < 8; ++j)
        if ((in >> j) & 1u) v[j] = ids.one(at + j);
    return in;
}

// A lane of the stop pass: the first of its columns in [b, e) that holds a stop id, or all ones
template <class Ids>
TK_HD uint32_t tk_drows_stop_lane(const TkDrows& p, const Ids& ids, uint64_t r, uint64_t c0, uint32_t b, uint32_t e) {
    uint64_t v[8];
    const uint32_t in = tk_drows_lane_load(p, ids, r, c0, b, e, v);
    uint32_t first = 0xFFFFFFFFu;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t j = 8; j-- > 0;)
        if (((in >> j) & 1u) && tk_drows_listed(p.stop, p.n_stop, v[j])) first = (uint32_t)(c0 + j);
    return first;
}
// The word the stop pass reduces a row's stops in keeps the lowest column it is handed (all ones = none): whichever tile comes first, the
// result is the same.  On the device a word the row's tiles share, on the CPU a plain variable.
TK_HD void tk_drows_stop_min(uint32_t* word, uint32_t col) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(word, col);
#else
    *word = col < *word ? col : *word;
#endif
}

// stop_col of a row from the reduced word (`found`: a column in [b, e), or all ones), and the end of its live range [b, *live_end)
TK_HD uint32_t tk_drows_stop_col(const TkDrows& p, uint32_t found, uint32_t e, uint32_t* live_end) {
    const uint32_t s = found < e ? found : e;
    *live_end = s + (((p.flags & TK_DROWSF_KEEP_STOP) && s < e) ? 1u : 0u);
    return s;
}

// a tile of `block` columns from col0 on holds a column of the live range [b, live_end): one that does not keeps nothing and reads nothing
TK_HD bool tk_drows_tile_live(uint64_t col0, uint32_t block, uint32_t b, uint32_t live_end) { return col0 < live_end && col0 + block > b; }

// the set bits of a lane's eight
TK_HD uint32_t tk_drows_popc8(uint32_t m) {
    m = (m & 0x55u) + ((m >> 1) & 0x55u);
    m = (m & 0x33u) + ((m >> 2) & 0x33u);
    return (m & 0x0Fu) + (m >> 4);
}

// A lane of the count and of the write pass: which of its columns in the live range [b, live_end) are kept -- not in skip_ids, and with
// SKIP_SPECIAL not a special token of the decode table -- and, in *bad, which of the kept ones have no decode entry.  v[j] = the element.
// dec: the id -> {x = offset | TK_DEC_SPEC, y = length} table of n_ids entries; nothing is read from it at or beyond n_ids.
template <class Ids, class Dec>
TK_HD uint32_t tk_drows_keep_lane(const TkDrows& p, const Ids& ids, Dec dec, uint32_t n_ids, uint64_t r, uint64_t c0, uint32_t b, uint32_t live_end, uint64_t v[8],
                                  uint32_t* bad) {
    const uint32_t in = tk_drows_lane_load(p, ids, r, c0, b, live_end, v);
    uint32_t keep = 0, none = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t j = 0; j < 8; ++j) {
        if (!((in >> j) & 1u)) continue;
        if (tk_drows_listed(p.skip, p.n_skip, v[j])) continue;
        uint32_t x = 0, len = 0;
        if (v[j] < n_ids) {
            const auto entry = dec[(uint32_t)v[j]];
            x = entry.x;
            len = entry.y;
        }
        if ((p.flags & TK_DROWSF_SKIP_SPECIAL) && len && (x & TK_DEC_SPEC)) continue;
        keep |= 1u << j;
        if (!len) none |= 1u << j;
    }
    *bad = none;
    return keep;
}
// ... of the count pass: the kept columns counted, the first one without entry reported by its row-major position
template <class Ids, class Dec>
TK_HD uint32_t tk_drows_count_lane(const TkDrows& p, const Ids& ids, Dec dec, uint32_t n_ids, uint64_t r, uint64_t c0, uint32_t b, uint32_t live_end,
                                   unsigned long long* words) {
    uint64_t v[8];
    uint32_t bad;
    const uint32_t keep = tk_drows_keep_lane(p, ids, dec, n_ids, r, c0, b, live_end, v, &bad);
    if (bad) {
        uint32_t j = 0;
        while (!((bad >> j) & 1u)) ++j;
        tk_report_min(words + TK_DROWS_BAD_ID, r * p.W + c0 + j);
    }
    return tk_drows_popc8(keep);
}
// ... of the write pass, which calls tk_drows_keep_lane itself, sums tk_drows_popc8(keep) over the lanes before this one and then stores: the
// kept ids in column order to tokens[at ..), `at` = the tile's offset plus that sum.  out.put(i, id) is tokens[i] = id.
template <class Out>
TK_HD void tk_drows_store_lane(uint32_t keep, const uint64_t v[8], uint64_t at, Out& out) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t j = 0; j < 8; ++j)
        if ((keep >> j) & 1u) out.put(at++, (uint32_t)v[j]);
}

// Row r <= R of the per-row pass, run once the call is accepted: tok_off[r] = the offset of the row's tile 0 (K behind the last row), and
// for a row n_kept and stop_col.  tile_off: the scanned tile counts; found: the words of the stop pass.
template <class TileOff, class Found, class Bounds>
TK_HD void tk_drows_row_entry(const TkDrows& p, TileOff tile_off, Found found, Bounds begin, bool has_begin, Bounds end, bool has_end, uint64_t K, uint64_t r,
                              uint64_t* tok_off, uint32_t* n_kept, uint32_t* stop_col) {
    const uint64_t at = r < p.R ? tile_off[r * p.tiles] : K;
    tok_off[r] = at;
    if (r >= p.R) return;
    const uint64_t next = r + 1 < p.R ? tile_off[(r + 1) * p.tiles] : K;
    uint32_t b, e, live_end;
    tk_drows_range(p, begin, has_begin, end, has_end, r, &b, &e);
    n_kept[r] = (uint32_t)(next - at);
    stop_col[r] = tk_drows_stop_col(p, found[r], e, &live_end);
}
