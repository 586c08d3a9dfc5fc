// Supervised samples from a packed batch: the parts of the device passes of tk_samples.h that are plain C++ -- what a call's figures and its
// role table may say, how many elements a part contributes, which part of a sample holds a stream position, where the element at a position
// comes from (bos, a role's before ids, the body, its after ids, eos or padding), whether it is trained, a sample's lengths and its trained
// elements, and a whole lane of the write pass (tk_smp_lane).  Compiles for the host too: tests/test_samples_sim.py drives them lane by lane
// on the CPU.  The rule itself is stated in include/tiktoken_amd.h (tk_assemble_samples_device).
//
// A part p of role r contributes cnt(p) = |before(r)| + n_p + |after(r)| elements; pstart[p] is the number of elements of the parts before
// it (pstart[n_parts]: all of them), so sample s, the parts [a, b) = [sample_off[s], sample_off[s + 1]), has E = pstart[b] - pstart[a] body
// elements and the stream [bos] E elements [eos].
#pragma once
#include <stdint.h>

#include "tk_rows_rule.h"  // TK_ROWS_NONE, tk_rows_off_check, tk_report_min, tk_last_le, tk_row_width

#define TK_SMPF_KEEP_TAIL 1u  // (= TK_SMP_KEEP_TAIL, TK_SMP_LEFT of the C ABI; tk_api.hip asserts it)
#define TK_SMPF_LEFT 2u
#define TK_SMP_MAX_ROLES 256u
#define TK_SMP_MAX_ROLE_IDS 4096u

struct TkSmp {
    uint64_t n_tokens, n_parts, n_samples;  // T, the parts, the samples (= R)
    uint32_t n_roles, max_len, width_multiple, bos, eos, pad, flags;
    int32_t ignore;
    uint32_t has_bos, has_eos;
    uint64_t R;  // = n_samples
    uint32_t W;  // width (tk_smp_size: known after the per-sample pass)
};

// What the spec, the role table and the figures of a call alone decide.  0, or why it is refused: 1 max_len == 0, 2 no roles but parts,
// 3 more than 256 roles, 4 role_off does not ascend from 0, 5 more than 4096 role ids, 6 T >= 2^32, 7 too many parts, 8 too many samples.
// role_off: host memory, 2 * n_roles + 1 entries (not read when n_roles == 0).
inline int tk_smp_shape(uint64_t n_tokens, uint64_t n_parts, uint64_t n_samples, uint64_t n_roles, const uint32_t* role_off, uint32_t max_len, uint32_t width_multiple,
                        uint32_t bos, uint32_t eos, uint32_t pad, int32_t ignore, uint32_t flags, TkSmp* p) {
    p->n_tokens = n_tokens;
    p->n_parts = n_parts;
    p->n_samples = n_samples;
    p->n_roles = (uint32_t)n_roles;
    p->max_len = max_len;
    p->width_multiple = width_multiple;
    p->bos = bos;
    p->eos = eos;
    p->pad = pad;
    p->ignore = ignore;
    p->flags = flags;
    p->has_bos = bos != TK_ROWS_NONE ? 1u : 0u;
    p->has_eos = eos != TK_ROWS_NONE ? 1u : 0u;
    p->R = n_samples;
    p->W = 0;
    if (!max_len) return 1;
    if (!n_roles && n_parts) return 2;
    if (n_roles > TK_SMP_MAX_ROLES) return 3;
    if (n_roles) {
        if (role_off[0] != 0) return 4;
        for (uint64_t i = 0; i < 2 * n_roles; ++i)
            if (role_off[i] > role_off[i + 1]) return 4;
        if (role_off[2 * n_roles] > TK_SMP_MAX_ROLE_IDS) return 5;
    }
    if (n_tokens >> 32) return 6;
    if (n_parts >= 0xFFFFFFFFull) return 7;
    if (n_samples >= 0xFFFFFFFFull) return 8;
    return 0;
}
// W once the per-sample pass has run.  0, or why it is refused: 9 the parts have 2^32 elements or more, 10 R * W >= 2^32.
TK_HD int tk_smp_size(TkSmp* p, uint64_t total, uint32_t longest) {
    p->W = tk_row_width(p->max_len, p->width_multiple, longest);
    if (total >> 32) return 9;
    if ((p->R * p->W) >> 32) return 10;
    return 0;
}

// The role table as a lane reads it: off[2 r] .. off[2 r + 1] are the before ids of role r in `ids`, off[2 r + 1] .. off[2 r + 2] its after
// ids.  The device hands its copy in the LDS in, the CPU simulation index-checked readers.
template <class Off, class Ids, class Train>
struct TkSmpRoles {
    Off off;
    Ids ids;
    Train train;
};
template <class Roles>
TK_HD uint32_t tk_smp_n_before(const Roles& t, uint32_t role) { return t.off[2 * role + 1] - t.off[2 * role]; }
template <class Roles>
TK_HD uint32_t tk_smp_n_after(const Roles& t, uint32_t role) { return t.off[2 * role + 2] - t.off[2 * role + 1]; }
// the elements of a part: before ids, body tokens, after ids
TK_HD uint64_t tk_smp_part_count(uint32_t n_before, uint64_t n_body, uint32_t n_after) { return (uint64_t)n_before + n_body + n_after; }

// the words the passes report in (unsigned long long each): the lowest tk_rows_bad_key of tok_off (TK_BAD_OFF; all ones = none) and of
// sample_off, the first part whose role is no role (all ones = none), the elements of all parts, the longest len
enum { TK_SMP_BAD_SOFF = TK_BAD_OFF + 1, TK_SMP_BAD_ROLE, TK_SMP_TOTAL, TK_SMP_LONGEST, TK_SMP_WORDS };

// Entry i of the count pass, i <= max(n_parts, n_samples): entry i of tok_off and of sample_off is checked where it exists (an offending
// one goes into its report word; nothing is indexed with either), the role of part i is checked, and pstart[i] = the elements of part i
// (0 where its entry or its role offends).  `off` of the role table: global memory here, 2 * n_roles + 1 entries.
template <class Off, class SOff, class Role, class ROff>
TK_HD void tk_smp_count_entry(const TkSmp& p, Off tok_off, SOff sample_off, Role part_role, ROff role_off, uint64_t i, uint64_t* pstart, unsigned long long* words) {
    if (i <= p.n_parts) {
        uint64_t a, b;
        const uint32_t why = tk_rows_off_check(tok_off, i, p.n_parts, p.n_tokens, &a, &b, words + TK_BAD_OFF);
        if (i < p.n_parts) {
            const uint32_t role = part_role[i];
            uint64_t cnt = 0;
            if (role >= p.n_roles) tk_report_min(words + TK_SMP_BAD_ROLE, i);
            else cnt = tk_smp_part_count(role_off[2 * role + 1] - role_off[2 * role], why ? 0 : b - a, role_off[2 * role + 2] - role_off[2 * role + 1]);
            pstart[i] = cnt;
        }
    }
    if (i <= p.n_samples) {
        uint64_t a, b;
        tk_rows_off_check(sample_off, i, p.n_samples, p.n_parts, &a, &b, words + TK_SMP_BAD_SOFF);
    }
}
// whether the count pass has reported anything that forbids indexing with the caller's arrays
TK_HD bool tk_smp_reported(const unsigned long long* words) {
    return words[TK_BAD_OFF] != ~0ull || words[TK_SMP_BAD_SOFF] != ~0ull || words[TK_SMP_BAD_ROLE] != ~0ull;
}

// A sample as the passes carry it: its parts [a, b), the element its first part starts at, its stream length, what the row keeps.  The part
// that holds element g (counted over all parts) is tk_last_le(pstart, lo, hi, g), searched in [lo, hi) of [a, b) (pstart[lo] <= g).
struct TkSmpRow {
    uint64_t a, b, base, full;
    uint32_t len, lo;  // elements kept; the stream position of the first one (below 2^32: full - len with len = max_len)
};
template <class SOff, class PS>
TK_HD void tk_smp_row_load(const TkSmp& p, SOff sample_off, PS pstart, uint64_t s, TkSmpRow* w) {
    w->a = sample_off[s];
    w->b = sample_off[s + 1];
    w->base = pstart[w->a];
    w->full = p.has_bos + (pstart[w->b] - w->base) + p.has_eos;
    w->len = (uint32_t)(w->full < p.max_len ? w->full : p.max_len);
    w->lo = (p.flags & TK_SMPF_KEEP_TAIL) ? (uint32_t)(w->full - w->len) : 0u;  // (full - len < 2^32 + 2: the parts' elements are below 2^32 when a row is written)
}

// Where the element at stream position q < full of a sample comes from.  For TK_SMP_SRC_BODY / _BEFORE / _AFTER *g is the element's index
// over all parts: the caller finds its part and calls tk_smp_in_part.
enum { TK_SMP_SRC_PAD = 0, TK_SMP_SRC_BOS, TK_SMP_SRC_EOS, TK_SMP_SRC_PART, TK_SMP_SRC_BEFORE, TK_SMP_SRC_BODY, TK_SMP_SRC_AFTER };
TK_HD int tk_smp_source(const TkSmp& p, const TkSmpRow& w, uint64_t q, uint64_t* g) {
    if (p.has_bos && q == 0) return TK_SMP_SRC_BOS;
    if (p.has_eos && q + 1 == w.full) return TK_SMP_SRC_EOS;
    *g = w.base + (q - p.has_bos);
    return TK_SMP_SRC_PART;
}
// ... inside its part: element i = g - pstart[part] of before (n_before ids) body (n_body tokens) after; *k = the index inside that run
TK_HD int tk_smp_in_part(uint64_t i, uint32_t n_before, uint64_t n_body, uint64_t* k) {
    if (i < n_before) {
        *k = i;
        return TK_SMP_SRC_BEFORE;
    }
    if (i < n_before + n_body) {
        *k = i - n_before;
        return TK_SMP_SRC_BODY;
    }
    *k = i - n_before - n_body;
    return TK_SMP_SRC_AFTER;
}
// whether it is trained: the body and the after ids of a part whose role trains; eos with the sample's last part; bos and before ids never
TK_HD bool tk_smp_trained(int src, bool role_trains) { return role_trains && (src == TK_SMP_SRC_BODY || src == TK_SMP_SRC_AFTER || src == TK_SMP_SRC_EOS); }
template <class Role, class Roles>
TK_HD bool tk_smp_eos_trained(const TkSmpRow& w, Role part_role, const Roles& t) { return w.b > w.a && t.train[part_role[w.b - 1]] != 0; }

// n_trained of a row: the trained elements among the stream positions [lo, lo + len), from the parts' clipped overlaps -- a part that
// trains contributes the overlap of [pstart[p] + n_before, pstart[p + 1]) with the window -- plus the eos where it is kept and trained.
template <class PS, class Role, class Roles>
TK_HD uint32_t tk_smp_n_trained(const TkSmp& p, const TkSmpRow& w, PS pstart, Role part_role, const Roles& t) {
    const uint64_t E = w.full - p.has_bos - p.has_eos, end = (uint64_t)w.lo + w.len;  // the window in stream positions: [lo, end)
    const uint64_t e0 = w.lo > p.has_bos ? w.lo - p.has_bos : 0, e1 = end > p.has_bos ? (end - p.has_bos < E ? end - p.has_bos : E) : 0;  // ... in body elements
    uint64_t n = 0;
    if (e0 < e1) {
        const uint64_t g0 = w.base + e0, g1 = w.base + e1;
        for (uint64_t q = tk_last_le(pstart, w.a, w.b, g0); q < w.b; ++q) {
            const uint64_t ps = pstart[q], pe = pstart[q + 1];
            if (ps >= g1) break;
            const uint32_t role = part_role[q];
            if (!t.train[role]) continue;
            const uint64_t lo = ps + tk_smp_n_before(t, role) > g0 ? ps + tk_smp_n_before(t, role) : g0, hi = pe < g1 ? pe : g1;
            if (lo < hi) n += hi - lo;
        }
    }
    if (p.has_eos && w.len && end == w.full && tk_smp_eos_trained(w, part_role, t)) ++n;
    return (uint32_t)n;
}

// Sample s of the per-sample pass (tk_k_smp_samples): its full_len, len and n_trained; returns len
template <class SOff, class PS, class Role, class Roles>
TK_HD uint32_t tk_smp_sample_entry(const TkSmp& p, SOff sample_off, PS pstart, Role part_role, const Roles& t, uint64_t s, uint64_t* full, uint32_t* len, uint32_t* n_trained) {
    TkSmpRow w;
    tk_smp_row_load(p, sample_off, pstart, s, &w);
    full[s] = w.full;
    len[s] = w.len;
    n_trained[s] = tk_smp_n_trained(p, w, pstart, part_role, t);
    return w.len;
}

// The caller's arrays and the passes' own as a lane reads them; every member is indexed with [] (the device passes pointers, the CPU
// simulation readers that check every index)
template <class Off, class SOff, class Role, class PS>
struct TkSmpIn {
    Off tok_off;
    SOff sample_off;
    Role part_role;
    PS pstart;
};

// The part a lane is in, carried from element to element
struct TkSmpPart {
    uint64_t p, ps, pe, toff, n_body;  // the part, its elements [ps, pe), tok_off[p], its body tokens
    uint32_t role, n_before, id0;      // its role; the before ids; where they start in the role table's ids (the after ids follow them)
    bool trains;
};
template <class In, class Roles>
TK_HD void tk_smp_part_load(const In& in, const Roles& t, uint64_t q, TkSmpPart* c) {
    c->p = q;
    c->ps = in.pstart[q];
    c->pe = in.pstart[q + 1];
    c->toff = in.tok_off[q];
    c->n_body = in.tok_off[q + 1] - c->toff;
    c->role = in.part_role[q];
    c->n_before = tk_smp_n_before(t, c->role);
    c->id0 = t.off[2 * c->role];
    c->trains = t.train[c->role] != 0;
}

// A lane of the write pass: ids, labels and mask bytes (byte j = 1 on an element) of the eight positions from i0 < N = R * W on, positions
// at and past N left as padding.  The lane steps from row to row (with W < 8 through up to eight of them) and inside a row from part to
// part: a position at or beyond the current part's end moves on to the next part that owns an element (behind a run of empty parts it
// searches once more instead of stepping through the run).  Eight positions of one row that are all padding are settled from len alone:
// no part is looked for.  `tok` fetches body tokens: tok.one(i) is tokens[i], and tok.eight(i, out) fetches tokens[i .. i + 8) as two
// 16-byte words where their address allows it and says whether it did -- asked where the eight positions are body tokens of one part.
// N is below 2^32, so positions, rows and columns are 32-bit.
template <class Tok, class In, class Roles>
TK_HD void tk_smp_lane(const TkSmp& p, const Tok& tok, const In& in, const Roles& t, uint32_t i0, uint32_t N, uint32_t id[8], int32_t lab[8], uint64_t* mask_out) {
    uint32_t r = i0 / p.W, col = i0 - r * p.W;
    TkSmpRow w;
    tk_smp_row_load(p, in.sample_off, in.pstart, r, &w);
    uint32_t lead = (p.flags & TK_SMPF_LEFT) ? p.W - w.len : 0u;  // columns in front of the elements
    const bool one_row = (uint64_t)col + 8 <= p.W;
    if (one_row && (col >= lead + w.len || col + 8 <= lead)) {  // eight columns of padding
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int j = 0; j < 8; ++j) {
            id[j] = p.pad;
            lab[j] = p.ignore;
        }
        *mask_out = 0;
        return;
    }
    TkSmpPart c;
    bool have = false;
    uint32_t tw[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool wide = false;
    if (one_row && col >= lead && col - lead + 8 <= w.len) {  // eight elements of one row: body tokens of one part?
        const uint64_t q0 = (uint64_t)w.lo + (col - lead);
        if (q0 >= p.has_bos && q0 + 8 + p.has_eos <= w.full) {
            const uint64_t g = w.base + (q0 - p.has_bos);
            tk_smp_part_load(in, t, tk_last_le(in.pstart, w.a, w.b, g), &c);
            have = true;
            const uint64_t i = g - c.ps;
            wide = i >= c.n_before && i + 8 <= c.n_before + c.n_body && tok.eight(c.toff + (i - c.n_before), tw);
        }
    }
    uint64_t mask = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < 8; ++j) {
        id[j] = p.pad;
        lab[j] = p.ignore;
        if (N - i0 > (uint32_t)j) {
            if (col >= lead && col - lead < w.len) {
                uint64_t g = 0, k = 0;
                int src = tk_smp_source(p, w, (uint64_t)w.lo + (col - lead), &g);
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
                        tk_smp_part_load(in, t, tk_last_le(in.pstart, w.a, w.b, g), &c);
                        have = true;
                    } else if (g >= c.pe) {  // the next part that owns an element: the one after, unless that one is empty
                        uint64_t q = c.p + 1;
                        if (in.pstart[q + 1] <= g) q = tk_last_le(in.pstart, q + 1, w.b, g);
                        tk_smp_part_load(in, t, q, &c);
                    }
                    src = tk_smp_in_part(g - c.ps, c.n_before, c.n_body, &k);
                    trains = c.trains;
                    v = src == TK_SMP_SRC_BODY ? (wide ? tw[j] : tok.one(c.toff + k)) : src == TK_SMP_SRC_BEFORE ? t.ids[c.id0 + (uint32_t)k] : t.ids[c.id0 + c.n_before + (uint32_t)k];
                }
                id[j] = v;
                if (tk_smp_trained(src, trains)) lab[j] = (int32_t)v;
                mask |= 1ull << (8 * j);
            }
            if (++col == p.W) {
                col = 0u;
                if (++r < p.R) {
                    tk_smp_row_load(p, in.sample_off, in.pstart, r, &w);
                    lead = (p.flags & TK_SMPF_LEFT) ? p.W - w.len : 0u;
                    have = false;
                }
            }
        }
    }
    *mask_out = mask;
}
