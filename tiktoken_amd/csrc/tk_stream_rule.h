// Streaming decode (the rule: include/tiktoken_amd.h, tk_stream_step_device): the parts of the row kernel of tk_stream.h that are plain C++ --
// a row slot's state, what a stream's figures must satisfy, whether a column's id is kept, a lane of the search for full hits and for the
// first held-back prefix, the unit boundary at or before a position, what a row emits and keeps back, and a lane of the repair of what it
// emits.  Compiles for the host too: tests/test_stream_sim.py drives them lane by lane on the CPU behind a row buffer that refuses every
// index outside the bytes the row holds.  The row rule is tk_decode_rows_rule.h's, the stop set and its order tk_stop_text_rule.h's, the
// units tk_utf8_repair_rule.h's: nothing of them is restated here.
#pragma once
#include <stdint.h>

#include "tk_decode_rows_rule.h"
#include "tk_stop_text_rule.h"
#include "tk_utf8_repair_rule.h"

#define TK_STREAM_W_MAX 64     // columns of a step: a lane of the row's wavefront per column
#define TK_STREAM_HOLD 66      // most bytes a row holds back: 63 of a stop string that may still complete, 3 of a char in front of them
#define TK_STREAM_TAIL 72      // room for them in the slot
#define TK_STREAM_ROWS_WG 4    // rows of a workgroup of the row kernel: a wavefront each
#define TK_STREAM_ROW_LDS 16000  // most bytes of a row's buffer: four of them and the stop set fit the 64 KiB a workgroup takes
#define TK_STREAM_PACK_BLOCK 256  // rows of a workgroup of the pack pass
#define TK_STREAM_ROWS_MAX 65536u  // rows of a stream (a workgroup of the pack pass adds up the lengths of the rows before its own)
#define TK_STREAM_MODE_BYTES 2u  // == TK_U8_BYTES
#define TK_STREAM_SET_BYTES ((sizeof(TkStopSet) + 15u) & ~15u)

enum { TK_STREAM_LIVE = 0, TK_STREAM_STOP_ID = 1, TK_STREAM_STOP_TEXT = 2, TK_STREAM_FLUSHED = 3 };
enum { TK_STREAM_OP_STEP = 0, TK_STREAM_OP_FLUSH = 1, TK_STREAM_OP_RESET = 2 };
// the words a call reports in (unsigned long long each): the first row whose begin / end offend, the row-major position of the first kept
// element without a decode entry (both all ones = none), a row that outgrew its buffer (never, by the sizes checked at create), and -- written
// by the pack pass of a call that is accepted -- the bytes and chars the call emitted
enum { TK_STREAM_BAD_ROW = 0, TK_STREAM_BAD_ID, TK_STREAM_OVERFLOW, TK_STREAM_N_TEXT, TK_STREAM_N_CHARS, TK_STREAM_WORDS };

// A row slot.  tail[0, tail_len): kept, decoded bytes that are not emitted yet; they begin on a unit boundary of the row's text.
struct TkStreamRow {
    uint32_t state, hit, tail_len, pad;
    uint64_t n_kept, n_text, n_chars;
    uint8_t tail[TK_STREAM_TAIL];
};

// the bytes of a row's buffer for steps of up to w columns over tokens of up to max_tok bytes; of its scratch slot (a multiple of 16)
TK_HD uint64_t tk_stream_cap(uint64_t w, uint64_t max_tok) { return TK_STREAM_HOLD + w * max_tok; }
TK_HD uint64_t tk_stream_slot(uint64_t cap, uint32_t mode) { return ((mode == TK_U8R_REPLACE ? 3u : 1u) * cap + 15u) & ~15ull; }
// What the figures of a stream alone decide: 0, or 1 w_max outside 1 .. 64, 2 more than TK_STREAM_ROWS_MAX rows, 3 a row buffer over
// TK_STREAM_ROW_LDS, 5 an unknown mode.  All the slots together stay below 2^32 bytes: the pack pass adds lengths up in 32 bits.
static_assert(3ull * (TK_STREAM_ROW_LDS + 16) * TK_STREAM_ROWS_MAX < (1ull << 32), "the slots of a stream");
TK_HD int tk_stream_shape(uint64_t n_rows, uint64_t w_max, uint64_t max_tok, uint32_t mode) {
    if (mode > TK_STREAM_MODE_BYTES) return 5;
    if (w_max < 1 || w_max > TK_STREAM_W_MAX) return 1;
    if (n_rows > TK_STREAM_ROWS_MAX) return 2;
    if (tk_stream_cap(w_max, max_tok) > TK_STREAM_ROW_LDS) return 3;
    return 0;
}

// A live column's element v: kept (tk_drows_keep_lane's test for one column); *len = the bytes of its token, 0 for a kept id without a
// decode entry; *x = where they lie.  Nothing is read from dec at or beyond n_ids.
template <class Dec>
TK_HD bool tk_stream_keep(const TkDrows& p, uint64_t v, Dec dec, uint32_t n_ids, uint32_t* x, uint32_t* len) {
    *x = *len = 0u;
    if (tk_drows_listed(p.skip, p.n_skip, v)) return false;
    if (v < n_ids) {
        const auto entry = dec[(uint32_t)v];
        *x = entry.x;
        *len = entry.y;
    }
    return !((p.flags & TK_DROWSF_SKIP_SPECIAL) && *len && (*x & TK_DEC_SPEC));
}

// A lane of the search over the row's bytes B[0, L) (B(i): byte i < L): the start positions p0, p0 + step, ...  A position survives when
// its byte is in the mask; it is then compared, in list order, with the strings that start with that byte.  *best: the least key p * 16 + k
// of a string that lies wholly inside B (tk_stops_lane's key, B the document); *e0: the least p at which B[p:] is a proper prefix of a
// string.  Both keep what they hold when the lane finds nothing less.
template <class Buf>
TK_HD void tk_stream_find_lane(const Buf& B, uint32_t L, const TkStopSet& set, uint32_t p0, uint32_t step, uint32_t* best, uint32_t* e0) {
    for (uint32_t p = p0; p < L; p += step) {
        const uint32_t b = B(p);
        if (!((set.mask[b >> 5] >> (b & 31u)) & 1u)) continue;
        const uint32_t avail = L - p;
        for (uint32_t k = 0; k < set.n; ++k) {
            const uint32_t a = set.off[k], len = set.off[k + 1] - a, m = len < avail ? len : avail;
            if (set.blob[a] != b) continue;
            uint32_t i = 1;
            while (i < m && B(p + i) == set.blob[a + i]) ++i;
            if (i < m) continue;
            if (len <= avail) {
                const uint32_t key = p * TK_STOPS_MAX + k;
                if (key < *best) *best = key;
                break;  // (the strings behind k lose to it at this place)
            }
            if (p < *e0) *e0 = p;
        }
    }
}

// The greatest unit start at or before x <= L, where a lead that has accepted every byte up to the end of B is unfinished, not ill-formed:
// x itself unless a sequence is running behind the three bytes before x and takes B[x] -- or B ends at x --, then that sequence's lead.
template <class Buf>
TK_HD uint32_t tk_stream_unit_floor(const Buf& B, uint32_t L, uint32_t x) {
    const uint32_t p1 = x >= 1u ? B(x - 1u) : 0u, p2 = x >= 2u ? B(x - 2u) : 0u, p3 = x >= 3u ? B(x - 3u) : 0u;
    const TkU8rState s = tk_u8r_state_behind(p1, p2, p3);
    if (!s.need) return x;
    if (x < L) {
        const uint32_t b = B(x);
        if (!(tk_u8r_cont(b) && (s.need + 1u != s.len || tk_u8r_first_ok(p1, b)))) return x;
    }
    return x - (s.len - s.need);
}

// What a live row does with B[0, L): it emits B[0, n_emit) repaired as a whole document, takes `state` and `hit`, and keeps B[tail_at, L).
//   best, e0   the wavefront's minima of tk_stream_find_lane (all ones / L: none)
//   found_stop a stop id ended the row's columns; flush: the call is a flush
struct TkStreamCut {
    uint32_t n_emit, state, hit, tail_at;
};
template <class Buf>
TK_HD TkStreamCut tk_stream_decide(const Buf& B, uint32_t L, uint32_t best, uint32_t e0, bool found_stop, bool flush, const TkStopSet& set, uint32_t mode) {
    if (best != TK_STOPS_NO_HIT) {
        const uint32_t k = best % TK_STOPS_MAX, p = best / TK_STOPS_MAX;
        return TkStreamCut{p + ((set.flags & TK_STOPSF_KEEP) ? set.off[k + 1] - set.off[k] : 0u), TK_STREAM_STOP_TEXT, k, L};
    }
    if (found_stop) return TkStreamCut{L, TK_STREAM_STOP_ID, TK_STOPS_NO_HIT, L};
    if (flush) return TkStreamCut{L, TK_STREAM_FLUSHED, TK_STOPS_NO_HIT, L};
    const uint32_t e = mode == TK_STREAM_MODE_BYTES ? e0 : tk_stream_unit_floor(B, L, e0);
    return TkStreamCut{e, TK_STREAM_LIVE, TK_STOPS_NO_HIT, e};
}

// A lane of the repair of B[0, n_emit) as one document: the sixteen bytes from p0 (a multiple of 16) through tk_u8r_lane -- the document
// starts at byte 0 and ends at n_emit; a live row's n_emit is a unit boundary, so its piece is the matching piece of the whole row's
// repair.  Nothing is read at or past n_emit.  mode: TK_U8R_REPLACE or TK_U8R_IGNORE.
template <class Buf, class Out>
TK_HD TkU8rCounts tk_stream_emit_lane(const Buf& B, uint32_t n_emit, uint32_t p0, uint32_t mode, Out& out) {
    if (p0 >= n_emit) return TkU8rCounts{0u, 0u, 0u};
    const uint32_t left = n_emit - p0, nvalid = left < 16u ? left : 16u;
    uint64_t lo = 0, hi = 0;
    for (uint32_t i = 0; i < nvalid; ++i) {
        const uint64_t b = B(p0 + i);
        if (i < 8u) lo |= b << (8u * i);
        else hi |= b << (8u * (i - 8u));
    }
    uint32_t prev = 0;
    for (uint32_t j = 1; j <= 3u && j <= p0; ++j) prev |= B(p0 - j) << (8u * (3u - j));
    const uint32_t bounds = (p0 ? 0u : 1u) | (left <= 16u ? 1u << left : 0u);
    return tk_u8r_lane(lo, hi, nvalid, prev, bounds, 0u, mode, out, TkU8rNoDocs());
}
