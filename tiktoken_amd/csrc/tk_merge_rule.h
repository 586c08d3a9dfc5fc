// Long pieces (more than TK_GLANE_MAX bytes): the rules of tk_k_merge_rounds, tk_k_merge_rounds_wide and tk_k_merge_long (tk_fused.h)
// that are plain C++ -- which parts survive a round, how the summaries of the wavefronts' ranges compose, when a round is not valid, a
// piece's first parts and ranks, and the index arithmetic of the level tree of the one-merge-at-a-time form.  No kernels, nothing that
// crosses lanes, no barriers: the kernels keep the scans, shuffles, barriers, loads and stores and call these for the rest.  Compiles for
// the host too: tests/test_merge_sim.py drives them wavefront by wavefront on the CPU against the oracle's byte_pair_merge.
//
// A round (byte_pair_merge, src/lib.rs:140-196, always merges the leftmost pair of the lowest rank m): as long as no pair that a merge
// creates ranks below m, the reference's next picks are the other rank-m pairs, left to right, skipping the ones a pick has consumed --
// within a run of overlapping rank-m pairs the even ones.  So a part survives unless the run of rank-m pairs that ends right before it
// has odd length, and the state that crosses lanes, rows, wavefronts and workgroups is the parity of that run.
#pragma once
#include <stdint.h>

#include "tk_common.h"  // TK_HD, TK_RANK_MAX

#define TK_MERGE_MARK 0x80000000u  // on a part of P1: made by this round's merge (token ids stay below 2^31: checked at tk_create)
#define TK_MERGE_EPL 8             // parts per lane and row

struct TkRunState {  // segment summary for the run-parity scan: is the segment all rank-m pairs, parity of its trailing run of them
    uint32_t all, par;
};
TK_HD TkRunState tk_run_combine(TkRunState a, TkRunState b) { return TkRunState{a.all & b.all, b.all ? (a.par ^ b.par) : b.par}; }

// Lane rule: c = parity of the run of rank-m pairs that ends right before the lane's first part, fm = rank-m flags of its parts, n_in =
// how many of them lie inside the range.  A part right after an odd count of rank-m pairs is absorbed.
struct TkLaneKeep {
    uint32_t mask, count, par;  // the parts kept, how many, the parity that leaves the lane
};
TK_HD TkLaneKeep tk_merge_lane_rule(uint32_t c, uint32_t fm, uint32_t n_in) {
    TkLaneKeep k{0u, 0u, c};
    for (uint32_t q = 0; q < TK_MERGE_EPL; ++q) {
        const uint32_t keep = (uint32_t)(q < n_in) & (k.par ^ 1u);
        k.mask |= keep << q;
        k.count += keep;
        k.par = ((fm >> q) & 1u) ? (k.par ^ 1u) : 0u;
    }
    return k;
}

// Lane state: rank-m flags (parts beyond the range: none) and run state of a lane's parts from their ranks
TK_HD TkRunState tk_merge_lane_state(const uint32_t rk[TK_MERGE_EPL], uint32_t m, uint32_t n_in, uint32_t& fm) {
    TkRunState v{1u, 0u};
    fm = 0;
    for (uint32_t q = 0; q < TK_MERGE_EPL; ++q) {
        const bool in = q < n_in;
        const uint32_t f = in ? (uint32_t)(rk[q] == m) : 0u;
        fm |= f << q;
        if (in) v = tk_run_combine(v, TkRunState{f, f});
    }
    return v;
}

// What a wavefront publishes about its range of `len` parts: the run state, keep0 = the parts that survive if no run enters the range,
// and -- a run of odd length that enters flips the fate of exactly the `lead` parts of the run of rank-m pairs the range starts with and
// of the one after them -- whether that stretch is odd: then one part fewer survives
struct TkRangeSum {
    uint32_t all, par, keep0, odd;
};
TK_HD TkRangeSum tk_range_summary(TkRunState acc, uint32_t keep0, uint32_t lead, uint32_t len) {
    const uint32_t aff = lead + 1u < len ? lead + 1u : len;
    return TkRangeSum{acc.all, acc.par, keep0, aff & 1u};
}
// survivors of a range given the state that enters it; st <- the state that leaves it
TK_HD uint32_t tk_range_enter(TkRunState& st, TkRangeSum s) {
    const uint32_t k = s.keep0 - (st.par & s.odd);
    st = tk_run_combine(st, TkRunState{s.all, s.par});
    return k;
}

// Validity of a round.  Part i is kept and picked (its own pair has rank m, f): if the next pick of this round is the pair right after
// (part i + 2 of cnt, its pair of rank m), the pair (merged part, its still unmerged right neighbour) exists between the two picks and
// must not rank below m.  rank(k), id(k): the round's input.
template <class Rank, class Id, class Probe>
TK_HD bool tk_round_between_bad(uint32_t m, uint32_t f, uint32_t i, uint32_t cnt, Rank rank, Id id, Probe probe) {
    return f && i + 2u < cnt && rank(i + 2u) == m && probe(m, id(i + 2u)) < m;
}
// d. the rank of pair j of the round's output of `total` parts (the last part: none).  A pair is new when a merge made one of its parts:
// probed and stored -- put(j, rank) --, and if it ranks below m the reference would have picked it before the rest of this round (bad).
// Every other pair keeps the rank that pass c copied: old(j).  part(k): the output, marks and all.
template <class Part, class Old, class Put, class Probe>
TK_HD uint32_t tk_round_rank(uint32_t m, uint32_t j, uint32_t total, Part part, Old old, Put put, Probe probe, bool& bad) {
    const uint32_t a = part(j), b = j + 1u < total ? part(j + 1u) : 0u;
    uint32_t r = TK_RANK_MAX;
    if (j + 1u < total && !((a | b) & TK_MERGE_MARK)) r = old(j);
    else {
        if (j + 1u < total) r = probe(a & ~TK_MERGE_MARK, b & ~TK_MERGE_MARK);
        put(j, r);
        bad |= r < m;
    }
    return r;
}
// c. a lane's kept parts (keepm, of its parts i0 ..) go to o, o + 1, ...: a picked part as m, marked, every other as it is; the ranks
// are copied (still right when neither the part nor the next one changes).  out(o, part, rank) stores.  True: the round is not valid.
template <class Rank, class Id, class Out, class Probe>
TK_HD bool tk_round_move_lane(uint32_t m, uint32_t i0, uint32_t keepm, uint32_t fm, const uint32_t rk[TK_MERGE_EPL], uint32_t o, uint32_t cnt, Rank rank,
                              Id id, Out out, Probe probe) {
    bool bad = false;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t q = 0; q < TK_MERGE_EPL; ++q) {
        if ((keepm >> q) & 1u) {
            const uint32_t i = i0 + q, f = (fm >> q) & 1u;
            out(o, f ? (m | TK_MERGE_MARK) : id(i), rk[q]);
            ++o;
            bad |= tk_round_between_bad(m, f, i, cnt, rank, id, probe);
        }
    }
    return bad;
}

// Part k of a piece of n bytes at text + s, and the rank of its pair with part k + 1 (the last part: none)
template <class Tables>
TK_HD void tk_piece_part(const Tables& T, const uint8_t* __restrict__ text, uint64_t s, uint32_t k, uint32_t n, uint32_t& id, uint32_t& rank) {
    const uint32_t b0 = text[s + k];
    id = T.byte_rank[b0];
    rank = k + 1u < n ? T.pair2[(b0 << 8) | text[s + k + 1u]] : TK_RANK_MAX;
}

// tk_k_merge_long: a 64-ary tree of minima over the keys rank << 32 | position.  Level 0 is the n parts themselves; level l >= 1 has
// cnt[l] = ceil(cnt[l - 1] / 64) entries at lv[off[l] ..]; the top level nl is the first of at most 64 entries.
#define TK_LONG_NONE 0xFFFFFFFFu
#define TK_MAX_LEVELS 6  // (64^6 parts and more: no piece is that long)
TK_HD int tk_long_levels(uint32_t n, uint32_t cnt[TK_MAX_LEVELS + 1], uint32_t off[TK_MAX_LEVELS + 1]) {
    int nl = 0;
    cnt[0] = n;
    off[0] = 0;
    uint32_t c = n, o = 0;
    do {
        c = (c + 63u) >> 6;
        ++nl;
        cnt[nl] = c;
        off[nl] = o;
        o += c;
    } while (c > 64u);
    return nl;
}
// entry k of level l - 1 as level l sees it (beyond the level: nothing)
template <class Rk, class Lv>
TK_HD uint64_t tk_long_key(const uint32_t* cnt, const uint32_t* off, int l, uint32_t k, Rk rk, Lv lv) {
    return k < cnt[l - 1] ? (l == 1 ? (((uint64_t)rk[k] << 32) | k) : lv[off[l - 1] + k]) : ~0ull;
}
// One merge of part i (the new token m) with its right neighbour j = nx[i]: nn = nx[j] (n: none), pp = pv[i] (TK_LONG_NONE: none).
// The links and ranks around i; r_i = rank of (m, part nn).  The rank of (part pp, m) is rk[pp]'s, stored by whoever probed it.
template <class A>
TK_HD void tk_long_link(A id, A rk, A nx, A pv, uint32_t n, uint32_t m, uint32_t i, uint32_t j, uint32_t nn, uint32_t r_i) {
    id[i] = m;
    nx[i] = nn;
    if (nn < n) pv[nn] = i;
    rk[j] = TK_RANK_MAX;
    id[j] = TK_RANK_MAX;  // absorbed (no token has this id): the emit compacts on it
    rk[i] = r_i;
}
// the blocks of level l whose minimum a merge at i, j, pp has changed: those of pp (none: i's), i and j, each once
struct TkLongBlocks {
    uint32_t b[3];
    bool on[3];
};
TK_HD TkLongBlocks tk_long_blocks(int l, uint32_t i, uint32_t j, uint32_t pp) {
    const uint32_t bp = (pp != TK_LONG_NONE ? pp : i) >> (6 * l), bi = i >> (6 * l), bj = j >> (6 * l);
    return TkLongBlocks{{bp, bi, bj}, {true, bi != bp, bj != bi && bj != bp}};
}
