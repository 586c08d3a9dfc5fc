// The back end of the encode pipeline (tk_fused.h: tk_k_count_tiles -> scan -> tk_k_place, tk_k_single_front's tail): the layout of a
// tile's run of result words, the words' classes, an entry's count word, how the host sizes what the two passes read, and the rules of
// the two passes that are plain expressions, each stated once.  The kernels keep whatever crosses lanes, the LDS lists, the loads and
// the stores.  Compiles for the host too: tests/test_back_sim.py drives the same rules in the kernels' frame on the CPU.
//   The rules are expression MACROS, as TKD_COUNT is: as functions, forced inline, they changed the code of both kernels -- fewer
// branches and 3 % more time in tk_k_count_tiles, a register tier in tk_k_place (profiles/back_end_rule.txt) -- where a macro is the
// kernel's own text.  They evaluate their arguments more than once: name values, not expressions with effects.
#pragma once
#include <stdint.h>

#include "tk_common.h"  // TK_HD, TK_TILE

// A tile's run of result words, res[tile * TKF_CAP ..]: one word per piece that starts in the tile, from the front; from the back the
// number of its pieces that are not tokens (TKF_TAIL_NMISS), the number of its gap chars (TKF_TAIL_NGAP), then the entries of the pieces
// that are not tokens once more, in no particular order -- what the counting pass needs, 0.12 GB per GiB instead of all the result words
// (0.65 GB).  It always fits: a piece that is not a token has at least two bytes, so pieces + missed pieces <= the tile's 3840 bytes.
//
//   0          1          ...  np - 1    |  (unused)  |  CAP - 2 - nm  ...  CAP - 3   CAP - 2   CAP - 1
//   piece 0    piece 1         last      |            |  ref nm - 1    ...  ref 0     ngap      nmiss
#define TKF_CAP 4096  // piece ids per tile: pid = tile * TKF_CAP + k (a 4096-byte tile starts at most 4096 pieces)
#define TKF_TAIL_NMISS (TKF_CAP - 1)
#define TKF_TAIL_NGAP (TKF_CAP - 2)
#define TKF_TAIL_REFS (TKF_CAP - 3)  // the q-th missed piece's entry: res[run + TKF_TAIL_REFS - q]
#define TKF_NONE 0xFFFFFFFFu         // ... of a piece the front kernel had no entry for: counts as the one token its result word holds
// entries of the piece-id space of an n-byte chunk, and the words of its piece-start bitmap (120 per tile: tk_k_place reads all of the last tile's)
TK_HD uint64_t tk_pid_cap(uint64_t n) { return (n / TK_TILE + 1) * TKF_CAP + 64; }
TK_HD uint64_t tk_starts_words(uint64_t nwords, uint64_t ntiles) { return (nwords > ntiles * (TK_TILE / 32) ? nwords : ntiles * (TK_TILE / 32)) + 2; }

// Per-piece result word res[piece id]: a token id (the piece is a vocabulary token, src/lib.rs:367), or a reference to where its
// tokens will be once the merge kernels have run.  A word of the last two classes is LISTED by tk_k_place.
#define TK_RES_FLAG 0x80000000u  // not a single token: TK_RES_FLAG | i = entry i of the chunk's miss data (TkMissData: its result is there)
#define TK_RES_GAP 0x7FFFFFFFu   // no token at all: a char at which a pat_str of the generic engine matches nothing (find_iter skips it, src/lib.rs:365)
#define TK_RES_FLAGGED(w) (((w) & TK_RES_FLAG) != 0u)
#define TK_RES_LISTED(w) (((w) & TK_RES_FLAG) || (w) == TK_RES_GAP)
#define TK_RES_ENTRY(w) ((w) & ~TK_RES_FLAG)

// An entry's count word (TkMissTab / TkMissOvf::res_cnt): the token count; with TKD_INLINE_BIT the tokens are tok[0 .. count); without it
// tok[0] (res_tok) is the token (count 1) or the staging position of the tokens.
#define TKD_INLINE 13
#define TKD_INLINE_BIT 0x40000000u
#define TKD_COUNT(w) ((w) & 0x3FFFFFFFu)
#define TK_BIGCOPY 4096  // token runs from this length on are copied by tk_k_bigcopy
#ifndef TKP_STAGE
#define TKP_STAGE 1024  // a tile of at most this many tokens is put together in LDS (tk_k_place)
#endif

// ---- the count pass
// An entry's token count from a ref of the tail (TKF_NONE: one token; refs below ovf_base are table slots, the others overflow entries):
// a table slot's count byte cnt8[ref] says it, unless it says 255 -- then, and for an overflow entry, the entry's count word does (the
// ESCAPE).  In steps, because the pass asks for all its count bytes before it looks at any: which byte (a ref without one reads byte
// 0), whether the ref escapes -- one that does not counts its byte if it is in the table, else one --, which entry's head the escape
// reads (a ref that does not escape: the first overflow entry).
#define TK_REF_IN_TAB(ref, ovf_base) ((ref) < (ovf_base))
#define TK_REF_CNT8_AT(ref, in_tab) ((in_tab) ? (ref) : 0u)
#define TK_REF_ESCAPES(ref, in_tab, cb) ((ref) != TKF_NONE && (!(in_tab) || (cb) == 255u))
#define TK_REF_HEAD_AT(ref, esc, ovf_base) ((esc) ? (ref) : (ovf_base))
// tokens of a tile = its pieces - its gap chars + what its pieces that are not tokens have beyond one token each
#define TK_TILE_TOKENS(np, ng, extra) ((np) - (ng) + (extra))

// ---- the place pass
// The index among a tile's pieces of the piece that starts at position `it` of the tile = the set bits of the tile's start bitmap before
// it: a0, a1 = the two bitmap words of the sixty-four positions `it` lies in (their group: TK_START_GROUP), px = the set bits before them.
#define TK_START_GROUP(it) (((it) >> 5) >> 1)
#define TK_PIECE_INDEX(it, a0, a1, px)                                                                                                          \
    ((px) + ((((it) >> 5) & 1u) ? (uint32_t)__builtin_popcount(a0) + (uint32_t)__builtin_popcount((a1) & ((1u << ((it) & 31u)) - 1u)) \
                                : (uint32_t)__builtin_popcount((a0) & ((1u << ((it) & 31u)) - 1u))))
// A listed piece's place among the tile's tokens: the tokens of the steps so far + its index in the step + the sum of `count - 1` over
// the listed pieces before it (cum includes its own `extra`; a gap char's is minus one: the sums are modulo 2^32).
#define TK_PIECE_PLACE(run, pidx, cum, extra) ((run) + (pidx) + ((cum) - (extra)))
// A document's token offset: the tokens of the chunks before, and within the chunk the tile's place + the tokens of the steps so far +
// its first piece's index in the step + the sum over the listed pieces before that.  The sum in 32 bits FIRST: `ex` is negative behind
// gap chars, as an unsigned number that only works modulo 2^32 (token offsets within a chunk fit 32 bits).
#define TK_DOC_TOK_OFF(tok_base, run0, run, j, ex) ((tok_base) + (uint64_t)(uint32_t)((run0) + (run) + (j) + (ex)))
// Where a flagged piece's `cnt` tokens come from, asked in this order: the entry's first token word alone (a long piece that is a token
// after all, tk_k_bincount; entries written that way), the entry itself (its count word says so), else the staging area -- from which
// a piece is copied in place unless it has TK_BIGCOPY tokens and more (a tile that goes through LDS holds no piece that long).
#define TK_FROM_HEAD(cnt) ((cnt) == 1u)
#define TK_FROM_ENTRY(res_cnt) ((res_cnt) & TKD_INLINE_BIT)
#define TK_FROM_STAGING(cnt) ((cnt) > 1u)
#define TK_COPIED_IN_PLACE(tile_staged, cnt) ((tile_staged) || (cnt) < TK_BIGCOPY)
