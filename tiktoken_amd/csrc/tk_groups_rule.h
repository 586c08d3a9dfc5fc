// Near-duplicate groups from fingerprints, and the selection of kept documents: the parts of the device passes of tk_groups.h that are
// plain C++ -- the shape of a groups call, the size of the claim table and how the bands are cut into rounds over it, where a key starts
// its probe, the probe of the claim and of the join, how many lanes share a pair and what one of them counts, find and union of the
// lock-free forest, and what a document contributes to a selection.  The rule is stated in include/tiktoken_amd.h.  Compiles for the host
// too; the memory accesses that have to be atomic on the device go through a `Mem` the caller hands in (tk_groups.h: TkGrpDeviceMem).
//
// The claim table: one region of S slots per band of a round, S the power of two >= 2 n, so a region is at most half full and a linear
// probe always ends at an empty slot.  A slot holds a DOCUMENT INDEX (TK_GRP_EMPTY: none), never a key: the key of a slot is
// band[slot's document][j], every value of a key is an ordinary one, and the four bytes of a slot change only among documents of one key
// (EMPTY -> the first claimant, then downwards by minimum).  Which key class owns a slot is decided once, by the first claim; every
// document of a key walks the same slots and sees the same classes, so all of them end in the same slot, whose final value is the
// lowest of them: rep_j(d).  The edges follow from the inputs alone, and the components of a graph do not depend on the order in which
// its edges are joined: group, keep and n_kept are functions of (sig, band, n_shingles, min_match), whatever the schedule.
#pragma once
#include <stdint.h>

#include "tk_fingerprint_rule.h"  // tk_fp_mix, tk_fp_shape

#define TK_GRP_EMPTY 0xFFFFFFFFu
#define TK_GRP_TABLE_BYTES (256ull << 20)  // the table of a round: as many bands as fit in this, at least one
#define TK_SEL_TILE 1024u                  // output positions per workgroup step of the copy
#define TK_SEL_THREADS 256u

struct TkGrp {
    uint64_t n;  // documents (below 2^32 - 1)
    uint32_t P, B, min_match;
    uint32_t lanes;      // lanes that share one pair in the join: tk_grp_pair_lanes(P)
    uint64_t S;          // slots of a region
    uint32_t per_round;  // bands of a round
};

// Slots of a region: the power of two >= 2 n (at least 2)
TK_HD uint64_t tk_grp_slots(uint64_t n) {
    uint64_t s = 2;
    while (s < 2 * n) s <<= 1;
    return s;
}
// Lanes of a wavefront that share one pair: each takes 4 signature positions (16 bytes of either row); a power of two, so that whole
// pairs fill the wavefront -- 64 / lanes of them at a time
TK_HD uint32_t tk_grp_pair_lanes(uint32_t P) {
    uint32_t g = 1;
    while (g * 4 < P) g <<= 1;
    return g;
}
// The shape of a call.  0, or why it is refused: 2 n_perm, 3 bands, 4 too many documents.
TK_HD int tk_grp_shape(uint64_t n, uint32_t P, uint32_t B, uint32_t min_match, TkGrp* g) {
    TkFp fp;
    const int why = tk_fp_shape(1, P, B, 0, 0, n, &fp);
    if (why) return why;
    if (n >= 0xFFFFFFFFull) return 4;
    g->n = n, g->P = P, g->B = B, g->min_match = min_match;
    g->lanes = tk_grp_pair_lanes(P);
    g->S = tk_grp_slots(n);
    const uint64_t fit = TK_GRP_TABLE_BYTES / (g->S * 4);
    g->per_round = fit < 1 ? 1u : fit > B ? B : (uint32_t)fit;
    return 0;
}
TK_HD uint64_t tk_grp_start(uint64_t key, uint64_t S) { return tk_fp_mix(key) & (S - 1); }

// The claim of (document d, band j) on the region `slot` (S slots): the walk from the key's start; an empty slot is claimed, a slot of
// another key stepped over, a slot of this key lowered to d -- read first: a slot that holds d or less already needs no atomic.
// Mem: load(p), cas(p, expected, desired) -> the old value, min(p, v).
template <class Mem>
TK_HD void tk_grp_claim(Mem& m, uint32_t* slot, uint64_t S, const uint64_t* band, uint32_t B, uint32_t j, uint32_t d) {
    const uint64_t key = band[(uint64_t)d * B + j];
    for (uint64_t at = tk_grp_start(key, S);; at = (at + 1) & (S - 1)) {
        uint32_t e = m.load(slot + at);
        if (e == TK_GRP_EMPTY) {
            e = m.cas(slot + at, TK_GRP_EMPTY, d);
            if (e == TK_GRP_EMPTY) return;
        }
        if (band[(uint64_t)e * B + j] != key) continue;
        if (e > d) m.min(slot + at, d);
        return;
    }
}
// rep_j(d) once every claim is done: the value of the slot of d's key (a live d has claimed, so the walk ends before an empty slot;
// one that meets an empty slot all the same -- a table nobody filled -- answers d: no edge)
TK_HD uint32_t tk_grp_rep(const uint32_t* slot, uint64_t S, const uint64_t* band, uint32_t B, uint32_t j, uint32_t d) {
    const uint64_t key = band[(uint64_t)d * B + j];
    for (uint64_t at = tk_grp_start(key, S);; at = (at + 1) & (S - 1)) {
        const uint32_t e = slot[at];
        if (e == TK_GRP_EMPTY) return d;
        if (band[(uint64_t)e * B + j] == key) return e;
    }
}

// Lane q of the lanes that share the pair (a, b): how many of the signature positions 4 q .. 4 q + 3 below P agree.  vec: P is a
// multiple of 4 and sig is 16-byte aligned -- one 16-byte load per row; otherwise word by word, and nothing is read past a row's end.
struct TkGrpQuad {
    uint32_t x, y, z, w;
};
TK_HD uint32_t tk_grp_match4(const uint32_t* sig, uint32_t P, bool vec, uint32_t a, uint32_t b, uint32_t q) {
    const uint32_t p0 = 4 * q;
    if (p0 >= P) return 0;
    const uint32_t *ra = sig + (uint64_t)a * P + p0, *rb = sig + (uint64_t)b * P + p0;
    if (vec) {
        const TkGrpQuad u = *(const TkGrpQuad*)ra, v = *(const TkGrpQuad*)rb;
        return (u.x == v.x) + (u.y == v.y) + (u.z == v.z) + (u.w == v.w);
    }
    uint32_t c = 0;
    for (uint32_t i = 0; i < 4 && p0 + i < P; ++i) c += ra[i] == rb[i];
    return c;
}

// The forest: parent[x] <= x, a root is its own parent, and a parent only ever moves to a smaller member of the same component -- so
// a walk upwards ends, whatever it reads meanwhile, at a document that was a root when it was read.  Path halving by plain stores is
// safe: it writes an ancestor of x over parent[x], to a document that is no root and never becomes one again (tk_grp_union changes roots only).
template <class Mem>
TK_HD uint32_t tk_grp_find(Mem& m, uint32_t* parent, uint32_t x) {
    for (;;) {
        const uint32_t p = m.load(parent + x);
        if (p == x) return x;
        const uint32_t gp = m.load(parent + p);
        if (gp != p) m.store(parent + x, gp);
        x = gp;
    }
}
// Join the components of a and b: the larger root goes under the smaller, so a root is the lowest index of its component.  A compare-
// and-swap that fails has met somebody else's progress: the roots are looked up again.
template <class Mem>
TK_HD void tk_grp_union(Mem& m, uint32_t* parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = tk_grp_find(m, parent, a), b = tk_grp_find(m, parent, b);
        if (a == b) return;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        if (m.cas(parent + hi, hi, lo) == hi) return;
    }
}

// Selection.  What document d adds to the two sums: 1 and its length when it is kept.  A tok_off that does not ascend gives lengths of
// 0, never a negative one.
TK_HD uint64_t tk_sel_len(const uint8_t* keep, const uint64_t* tok_off, uint64_t d) {
    if (!keep[d]) return 0;
    const uint64_t a = tok_off[d], b = tok_off[d + 1];
    return b > a ? b - a : 0;
}
// Output position g of the kept documents [i0, i1] (tok_off_out[i0] <= g): the kept document that owns it, and the source position.
// Nothing outside tok_off_out[0 .. n_kept], doc[0 .. n_kept) and tok_off[0 .. n) is read.
TK_HD uint64_t tk_sel_source(const uint64_t* tok_off, const uint64_t* tok_off_out, const uint32_t* doc, uint64_t i0, uint64_t i1, uint64_t g) {
    const uint64_t i = tk_last_le(tok_off_out, i0, i1 + 1, g);
    return tok_off[doc[i]] + (g - tok_off_out[i]);
}
