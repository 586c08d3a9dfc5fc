// Packed sample rows: the parts of the device passes of tk_sample_rows.h that are plain C++ -- what a call may say, a sample's placed length
// and its trained elements, the successor of a sample as a row start, a round of pointer doubling, a sample's row and column, a row's
// segments, and a whole lane of the write pass (tk_srow_lane).  Compiles for the host too: tests/test_sample_rows_sim.py drives them entry
// by entry and lane by lane on the CPU.  The rule itself is stated in include/tiktoken_amd.h (tk_pack_samples_device).
//
// Samples, parts, streams, truncation and training are tk_samples_rule.h's; nothing of them is restated here.  On top of them:
//   c[s]      the placed lengths of the samples before s (c[n]: all of them), f[s] the placed samples before s: exclusive sums, 64-bit
//   succ[s]   for a placed s, the sample that starts the next row if s starts one: the first j > s with c[j + 1] - c[s] > L (n: none)
//   mark[s]   1 where s starts a row: the orbit of the first placed sample under succ, found by pointer doubling (tk_srow_double_entry)
//   ex[s]     the row starts before s (ex[n] = R): sample_row[s] = ex[s + 1] - 1 for a placed s
// so next-fit, a loop in which every step depends on the one before, becomes sums, searches and ceil(log2 n) rounds of independent entries.
#pragma once
#include <stdint.h>

#include "tk_samples_rule.h"

#define TK_SMPF_SKIP_LONG 4u     // (= TK_SMP_SKIP_LONG, TK_SMP_IGNORE_FIRST of the C ABI; tk_api.hip asserts it)
#define TK_SMPF_IGNORE_FIRST 8u

// the report words: tk_samples_rule.h's (the count, scan and per-sample passes are its kernels), then the rows and the segments
enum { TK_SROW_R = TK_SMP_WORDS, TK_SROW_NSEGS, TK_SROW_WORDS };

// What the spec, the role table and the figures of a call alone decide: tk_smp_shape's refusals 1 .. 8, then 11 width_multiple != 0,
// 12 TK_SMP_LEFT.  The TkSmp it fills is the one the samples passes and the lanes take: W = L = max_len, R is settled on the device.
inline int tk_srow_shape(uint64_t n_tokens, uint64_t n_parts, uint64_t n_samples, uint64_t n_roles, const uint32_t* role_off, uint32_t max_len, uint32_t width_multiple,
                         uint32_t bos, uint32_t eos, uint32_t pad, int32_t ignore, uint32_t flags, TkSmp* p) {
    const int why = tk_smp_shape(n_tokens, n_parts, n_samples, n_roles, role_off, max_len, 0u, bos, eos, pad, ignore, flags, p);
    p->R = 0;
    p->W = max_len;
    if (why) return why;
    if (width_multiple) return 11;
    if (flags & TK_SMPF_LEFT) return 12;
    return 0;
}
// R once the placement has run.  0, or why it is refused: 9 the parts have 2^32 elements or more, 10 R * L >= 2^32.
TK_HD int tk_srow_size(TkSmp* p, uint64_t total, uint64_t R) {
    p->R = R;
    if (total >> 32) return 9;
    if ((R * p->W) >> 32) return 10;
    return 0;
}
// the rounds of pointer doubling n samples need: the least k with 2^k >= n (a chain has at most n members, so distances stay below 2^k)
TK_HD uint32_t tk_srow_rounds(uint64_t n) {
    uint32_t k = 0;
    while ((1ull << k) < n) ++k;
    return k;
}

// whether the first kept element of a sample with len > 0 is trained
template <class In, class Roles>
TK_HD bool tk_srow_first_trained(const TkSmp& p, const TkSmpRow& w, const In& in, const Roles& t) {
    uint64_t g = 0, k = 0;
    int src = tk_smp_source(p, w, w.lo, &g);
    if (src == TK_SMP_SRC_BOS) return false;
    if (src == TK_SMP_SRC_EOS) return tk_smp_trained(src, tk_smp_eos_trained(w, in.part_role, t));
    TkSmpPart c;
    tk_smp_part_load(in, t, tk_last_le(in.pstart, w.a, w.b, g), &c);
    src = tk_smp_in_part(g - c.ps, c.n_before, c.n_body, &k);
    return tk_smp_trained(src, c.trains);
}
// Sample s of the placed-length pass, behind the per-sample pass of tk_samples_rule.h (full, len, n_trained are its figures): plen -> c[s],
// the placed flag -> f[s] (both become exclusive sums in the scan behind this), and n_trained[s] becomes the packed rows' figure: 0 for a
// sample that is not placed, one less where TK_SMP_IGNORE_FIRST masks a trained first element.
template <class In, class Roles>
TK_HD void tk_srow_plen_entry(const TkSmp& p, const In& in, const Roles& t, uint64_t s, const uint64_t* full, const uint32_t* len, uint32_t* n_trained, uint64_t* c,
                              uint64_t* f) {
    uint32_t plen = len[s];
    if ((p.flags & TK_SMPF_SKIP_LONG) && full[s] > p.max_len) plen = 0;
    uint32_t nt = plen ? n_trained[s] : 0u;
    if (plen && (p.flags & TK_SMPF_IGNORE_FIRST)) {
        TkSmpRow w;
        tk_smp_row_load(p, in.sample_off, in.pstart, s, &w);
        if (tk_srow_first_trained(p, w, in, t)) --nt;
    }
    n_trained[s] = nt;
    c[s] = plen;
    f[s] = plen ? 1u : 0u;
}

// Entry s <= n of the successor pass: succ[s] and the first mark.  A placed s followed as a row start by j means the samples [s, j) fit a
// row and j does not: c[j] - c[s] <= L < c[j + 1] - c[s], so j is the last index in (s, n] with c[j] <= c[s] + L -- one exists, plen <= L --
// and j == n says that everything behind s fits.  j is placed (c[j + 1] > c[j]) and j > s: chains ascend.  An unplaced s and entry n point
// at n, where every chain ends.  The mark: the first placed sample starts row 0.
template <class C, class F>
TK_HD void tk_srow_succ_entry(C c, F f, uint64_t n, uint32_t L, uint64_t s, uint32_t* succ, uint32_t* mark) {
    uint32_t j = (uint32_t)n, m = 0u;
    if (s < n) {
        const uint64_t cs = c[s];
        if (c[s + 1] > cs) {
            j = (uint32_t)tk_last_le(c, s + 1, n + 1, cs + L);
            m = f[s] == 0 ? 1u : 0u;
        }
    }
    succ[s] = j;
    mark[s] = m;
}
// Entry s <= n of a round of pointer doubling: jin[s] is the 2^k-th successor of s (n: the chain ends before); a marked s marks it, and
// jout[s] becomes the 2^(k+1)-th.  Marks only ever land on members of the chain and are stores of 1, so a round's result does not depend on
// the order of its entries: an entry that sees a mark made in the same round marks a member the next round would have marked.  After
// round k every member less than 2^(k+1) steps from the first is marked.
template <class J>
TK_HD void tk_srow_double_entry(J jin, uint64_t n, uint64_t s, uint32_t* jout, uint32_t* mark) {
    const uint32_t j = jin[s];
    if (mark[s] && j < n) mark[j] = 1u;
    jout[s] = jin[j];
}
// Sample s of the place pass, behind the exclusive sum of the marks (ex[s]: the row starts before s, ex[n] = R): its row and column, and
// where it starts a row that row's first sample and whether the row has a padding tail (fill < L: the fill is c[succ] - c[s]).  The first
// sample of the row of a later sample is the last t with ex[t] <= row.
template <class E, class C, class S>
TK_HD void tk_srow_place_entry(E ex, C c, S succ, uint32_t L, uint64_t s, uint32_t* sample_row, uint32_t* sample_col, uint32_t* row_sample, uint32_t* row_pad) {
    const uint64_t cs = c[s];
    if (c[s + 1] == cs) {
        sample_row[s] = TK_ROWS_NONE;
        sample_col[s] = 0u;
        return;
    }
    const uint32_t before = ex[s], row = ex[s + 1] - 1u;
    sample_row[s] = row;
    if (before == row) {
        sample_col[s] = 0u;
        row_sample[row] = (uint32_t)s;
        row_pad[row] = c[succ[s]] - cs < L ? 1u : 0u;
    } else {
        sample_col[s] = (uint32_t)(cs - c[tk_last_le(ex, 0, s + 1, row)]);
    }
}
// Row r of the segment pass, behind the exclusive sum of row_pad (pads: the rows with a tail before r): the segment starts below r * L
template <class F, class RS>
TK_HD uint32_t tk_srow_row_seg(F f, RS row_sample, uint64_t r, uint32_t pads) { return (uint32_t)f[row_sample[r]] + pads; }

// The passes' own arrays as a lane reads them (the device passes pointers, the CPU simulation readers that check every index)
template <class C, class F, class RS, class RG>
struct TkSrowIn {
    C c;
    F f;
    RS row_sample;
    RG row_seg;
};
// A row as a lane carries it: its samples [a, b), the placed elements before it, its fill, where its segments start in cu_seqlens
struct TkSrowRow {
    uint64_t a, b, cbase, fa;
    uint32_t fill, seg0, seg_pad;  // seg_pad: the index of the padding tail's segment (read only where fill < L)
};
template <class Rows>
TK_HD void tk_srow_row_load(const Rows& rw, uint32_t r, TkSrowRow* o) {
    o->a = rw.row_sample[r];
    o->b = rw.row_sample[r + 1];
    o->cbase = rw.c[o->a];
    o->fa = rw.f[o->a];
    o->fill = (uint32_t)(rw.c[o->b] - o->cbase);
    o->seg0 = rw.row_seg[r];
    o->seg_pad = rw.row_seg[r + 1] - 1u;
}

// A lane of the write pass: ids, labels, seg and pos of the eight positions from i0 < N = R * L on, positions at and past N left as
// padding; a position with pos == 0 puts itself into cu_seqlens through cu.put(index, position) -- a sample's first element at the row's
// first segment plus the placed samples between, a padding tail's first position at the row's last.  The lane steps from row to row (with
// L < 8 through up to eight of them), inside a row from sample to sample (behind a run of unplaced samples it searches once more instead of
// stepping through the run) and inside a sample from part to part as tk_smp_lane does.  Eight positions of one padding tail are settled
// from the row's figures alone.  `tok` as in tk_smp_lane.
template <class Tok, class In, class Rows, class Roles, class Cu>
TK_HD void tk_srow_lane(const TkSmp& p, const Tok& tok, const In& in, const Rows& rw, const Roles& t, uint32_t i0, uint32_t N, uint32_t id[8], int32_t lab[8],
                        uint32_t sg[8], uint32_t ps[8], Cu& cu) {
    const uint32_t L = p.W;
    uint32_t r = i0 / L, col = i0 - r * L;
    TkSrowRow row;
    tk_srow_row_load(rw, r, &row);
    const bool one_row = (uint64_t)col + 8 <= L;
    if (one_row && col >= row.fill) {  // eight columns of one padding tail
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (uint32_t j = 0; j < 8; ++j) {
            id[j] = p.pad;
            lab[j] = p.ignore;
            sg[j] = TK_ROWS_NONE;
            ps[j] = col + j - row.fill;
        }
        if (col == row.fill) cu.put(row.seg_pad, i0);
        return;
    }
    uint64_t s = 0, cs = 0, ce = 0;  // the sample, its elements [cs, ce) among the placed ones
    TkSmpRow w = {};  // (loaded before it is read: have_s)
    bool have_s = false, have = false, wide = false;
    TkSmpPart c;
    uint32_t tw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (one_row && col + 8 <= row.fill) {  // eight elements of one row: body tokens of one part of one sample?
        const uint64_t g = row.cbase + col;
        s = tk_last_le(rw.c, row.a, row.b, g);
        cs = rw.c[s];
        tk_smp_row_load(p, in.sample_off, in.pstart, s, &w);
        ce = cs + w.len;
        have_s = true;
        const uint64_t q0 = (uint64_t)w.lo + (g - cs);
        if (g + 8 <= ce && q0 >= p.has_bos && q0 + 8 + p.has_eos <= w.full) {
            const uint64_t e = w.base + (q0 - p.has_bos);
            tk_smp_part_load(in, t, tk_last_le(in.pstart, w.a, w.b, e), &c);
            have = true;
            const uint64_t i = e - c.ps;
            wide = i >= c.n_before && i + 8 <= c.n_before + c.n_body && tok.eight(c.toff + (i - c.n_before), tw);
        }
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < 8; ++j) {
        id[j] = p.pad;
        lab[j] = p.ignore;
        sg[j] = TK_ROWS_NONE;
        ps[j] = 0u;
        if (N - i0 > (uint32_t)j) {
            if (col < row.fill) {
                const uint64_t g = row.cbase + col;
                if (!have_s || g >= ce) {
                    if (!have_s) {
                        s = tk_last_le(rw.c, row.a, row.b, g);
                    } else {  // the next sample that owns a position: the one after, unless that one is not placed
                        ++s;
                        if (rw.c[s + 1] <= g) s = tk_last_le(rw.c, s + 1, row.b, g);
                    }
                    cs = rw.c[s];
                    tk_smp_row_load(p, in.sample_off, in.pstart, s, &w);
                    ce = cs + w.len;
                    have_s = true;
                    have = false;
                }
                const uint32_t at = (uint32_t)(g - cs);
                uint64_t e = 0, k = 0;
                int src = tk_smp_source(p, w, (uint64_t)w.lo + at, &e);
                bool trains;
                uint32_t v;
                if (src == TK_SMP_SRC_BOS) {
                    v = p.bos;
                    trains = false;
                } else if (src == TK_SMP_SRC_EOS) {
                    v = p.eos;
                    trains = tk_smp_eos_trained(w, in.part_role, t);
                } else {
                    if (!have) {
                        tk_smp_part_load(in, t, tk_last_le(in.pstart, w.a, w.b, e), &c);
                        have = true;
                    } else if (e >= c.pe) {
                        uint64_t q = c.p + 1;
                        if (in.pstart[q + 1] <= e) q = tk_last_le(in.pstart, q + 1, w.b, e);
                        tk_smp_part_load(in, t, q, &c);
                    }
                    src = tk_smp_in_part(e - c.ps, c.n_before, c.n_body, &k);
                    trains = c.trains;
                    v = src == TK_SMP_SRC_BODY ? (wide ? tw[j] : tok.one(c.toff + k)) : src == TK_SMP_SRC_BEFORE ? t.ids[c.id0 + (uint32_t)k] : t.ids[c.id0 + c.n_before + (uint32_t)k];
                }
                id[j] = v;
                if (tk_smp_trained(src, trains) && !(at == 0u && (p.flags & TK_SMPF_IGNORE_FIRST))) lab[j] = (int32_t)v;
                sg[j] = (uint32_t)s;
                ps[j] = at;
                if (at == 0u) cu.put(row.seg0 + (uint32_t)(rw.f[s] - row.fa), i0 + (uint32_t)j);
            } else {
                ps[j] = col - row.fill;
                if (col == row.fill) cu.put(row.seg_pad, i0 + (uint32_t)j);
            }
            if (++col == L) {
                col = 0u;
                if (++r < p.R) {
                    tk_srow_row_load(rw, r, &row);
                    have_s = false;
                }
            }
        }
    }
}
