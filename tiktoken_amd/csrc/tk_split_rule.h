// Text chunks from a packed batch and its text: the parts of the device passes of tk_split.h that are plain C++ -- what a tk_split_spec may
// say, the class of one token boundary (separator match, then legal), one step of a document's chain from the class planes, the walk from a
// start to a limit, a whole block of the walk pass, a document of the stitch pass, the fold of a plane word, the rank of a position among
// the starts, and the chunk record of one start.  Compiles for the host too: tests/test_split_sim.py drives them the way the kernels do,
// "wavefronts" of 64 lanes included.  The rule itself is stated in include/tiktoken_amd.h (tk_split_device).
//
// Positions.  g is a global token index (tokens[g]); a document's tokens are [g0, g0 + n), s / e are indices inside it.  The planes are bit
// arrays over g, W = T / 64 + 1 words of 64 bits each: planes 0 .. L - 1 hold the boundaries whose level is l, plane L the legal ones; bit g
// speaks of the boundary before token g and is 0 where a document starts.  `cut` holds the chunk starts of the true chains, `spec` those of
// the speculative walks.  A block is K consecutive positions (K a multiple of 64: whole plane words); a document's part inside one block
// is a segment.
#pragma once
#include <stdint.h>

#include "tk_rows_rule.h"  // tk_rows_off_check, tk_report_min, tk_last_le

#define TK_SPLIT_MAX_LEVELS 4u
#define TK_SPLIT_MAX_SEPS 4u
#define TK_SPLIT_MAX_PART 16u
#define TK_SPLITC_HARD 0xFDu  // (= TK_SPLIT_HARD .. TK_SPLIT_END of the C ABI; tk_api.hip asserts it)
#define TK_SPLITC_FORCED 0xFEu
#define TK_SPLITC_END 0xFFu
#define TK_SPLIT_NOWHERE 0xFFFFFFFFu  // no join in a block, no exit from it
#define TK_SPLIT_K_DEFAULT 4096u

struct TkSplitSep {  // (the layout of tk_split_sep)
    uint8_t tail_len, head_len;
    uint8_t tail[16], head[16];
};
struct TkSplit {
    uint64_t n_tokens, n_docs;  // T, the documents
    uint64_t W;                 // words of a plane
    uint32_t N, M, O, L, K;     // max_tokens, min_tokens, overlap, levels, tokens of a block
    uint32_t n_seps[4];
    TkSplitSep sep[4][4];
};

// What the spec and the figures of a call alone decide.  0, or why it is refused: 1 M == 0, 2 M + 3 > N, 3 O >= M, 4 more than 4 levels, 5
// more than 4 separators in a level, 6 a separator part longer than 16 bytes, 7 a separator with both parts empty, 8 K neither 0 nor a
// multiple of 64, 9 T >= 2^32, 10 n_docs >= 2^32 - 1, 11 an unknown flag.  `seps`: n_levels rows of four, as in tk_split_spec.
template <class Sep>
TK_HD int tk_split_shape(uint64_t n_tokens, uint64_t n_docs, uint32_t max_tokens, uint32_t min_tokens, uint32_t overlap, uint32_t n_levels, const uint32_t* n_seps,
                         const Sep (*seps)[4], uint32_t seg_tokens, uint32_t flags, TkSplit* p) {
    if (flags) return 11;
    if (!min_tokens) return 1;
    if ((uint64_t)min_tokens + 3 > max_tokens) return 2;
    if (overlap >= min_tokens) return 3;
    if (n_levels > TK_SPLIT_MAX_LEVELS) return 4;
    for (uint32_t l = 0; l < n_levels; ++l) {
        if (n_seps[l] > TK_SPLIT_MAX_SEPS) return 5;
        for (uint32_t k = 0; k < n_seps[l]; ++k) {
            if (seps[l][k].tail_len > TK_SPLIT_MAX_PART || seps[l][k].head_len > TK_SPLIT_MAX_PART) return 6;
            if (!seps[l][k].tail_len && !seps[l][k].head_len) return 7;
        }
    }
    if (seg_tokens & 63u) return 8;
    if (n_tokens >> 32) return 9;
    if (n_docs >= 0xFFFFFFFFull) return 10;
    p->n_tokens = n_tokens;
    p->n_docs = n_docs;
    p->W = n_tokens / 64 + 1;
    p->N = max_tokens;
    p->M = min_tokens;
    p->O = overlap;
    p->L = n_levels;
    // the library's choice: blocks of at least eight chunks, so that a speculative walk has steps in which to meet the true chain
    uint64_t k = seg_tokens;
    if (!k) {
        k = ((uint64_t)max_tokens * 8 + 63) & ~63ull;
        k = k < TK_SPLIT_K_DEFAULT ? TK_SPLIT_K_DEFAULT : k > (1u << 30) ? (1u << 30) : k;
    }
    p->K = (uint32_t)k;
    for (uint32_t l = 0; l < 4; ++l) {
        p->n_seps[l] = l < n_levels ? n_seps[l] : 0u;
        for (uint32_t j = 0; j < 4; ++j) {
            TkSplitSep& o = p->sep[l][j];
            const bool live = l < n_levels && j < p->n_seps[l];
            o.tail_len = live ? seps[l][j].tail_len : 0;
            o.head_len = live ? seps[l][j].head_len : 0;
            for (uint32_t i = 0; i < 16; ++i) {
                o.tail[i] = live ? seps[l][j].tail[i] : 0;
                o.head[i] = live ? seps[l][j].head[i] : 0;
            }
        }
    }
    return 0;
}

// ---- the class of one boundary ----
enum { TK_SPLIT_CLS_LEGAL = 4, TK_SPLIT_CLS_NONE = 5 };  // legal without a level; not legal (0 .. 3: legal, and that level)
// The boundary at byte `at` of the text, inside the document [doc_b, doc_e) (doc_b < at < doc_e).  text[i] is byte i of the batch.
template <class Text>
TK_HD uint32_t tk_split_class(const TkSplit& p, Text text, uint64_t doc_b, uint64_t doc_e, uint64_t at) {
    if ((text[at] & 0xC0u) == 0x80u) return TK_SPLIT_CLS_NONE;
    for (uint32_t l = 0; l < p.L; ++l)
        for (uint32_t k = 0; k < p.n_seps[l]; ++k) {
            const TkSplitSep& q = p.sep[l][k];
            if (q.tail_len > at - doc_b || q.head_len > doc_e - at) continue;  // (checked inside the document)
            bool same = true;
            for (uint32_t i = 0; same && i < q.tail_len; ++i) same = text[at - q.tail_len + i] == q.tail[i];
            for (uint32_t i = 0; same && i < q.head_len; ++i) same = text[at + i] == q.head[i];
            if (same) return l;
        }
    return TK_SPLIT_CLS_LEGAL;
}
// the planes a class sets: bit l for its level, bit L for legal
TK_HD uint32_t tk_split_class_bits(const TkSplit& p, uint32_t cls) {
    if (cls == TK_SPLIT_CLS_NONE) return 0u;
    return (1u << p.L) | (cls < p.L ? 1u << cls : 0u);
}
// Position g < T of the class pass: the planes its boundary sets (none where a document starts).  The document is searched in [d_lo, d_hi).
template <class Text, class Off, class Start>
TK_HD uint32_t tk_split_class_at(const TkSplit& p, Text text, Off doc_off, Off tok_off, Start byte_start, uint64_t d_lo, uint64_t d_hi, uint64_t g) {
    const uint64_t d = tk_last_le(tok_off, d_lo, d_hi, g);
    if (g == tok_off[d]) return 0u;
    const uint64_t doc_b = doc_off[d], doc_e = doc_off[d + 1], at = doc_b + byte_start[g];
    if (at <= doc_b || at >= doc_e) return 0u;  // (never for spans that add up to the text; nothing outside the document is read)
    return tk_split_class_bits(p, tk_split_class(p, text, doc_b, doc_e, at));
}
// the documents a workgroup's threads search between: those of its first position b0 < T and of its last
template <class Off>
TK_HD void tk_split_block_docs(const TkSplit& p, Off tok_off, uint64_t b0, uint64_t block, uint64_t* d_lo, uint64_t* d_hi) {
    const uint64_t last = p.n_tokens - b0 > block ? b0 + block - 1 : p.n_tokens - 1;
    *d_lo = tk_last_le(tok_off, 0, p.n_docs, b0);
    *d_hi = tk_last_le(tok_off, *d_lo, p.n_docs, last) + 1;
}

// ---- bits of a plane ----
TK_HD uint64_t tk_split_from(uint32_t bit) { return ~0ull << bit; }                          // bits >= bit (bit < 64)
TK_HD uint64_t tk_split_upto(uint32_t bit) { return bit == 63u ? ~0ull : (1ull << (bit + 1)) - 1; }  // bits <= bit
// word w of the window [a, b] (a >> 6 <= w <= b >> 6): the bits of it that lie inside
TK_HD uint64_t tk_split_window_mask(uint64_t w, uint64_t a, uint64_t b) {
    uint64_t m = ~0ull;
    if (w == (a >> 6)) m &= tk_split_from((uint32_t)a & 63u);
    if (w == (b >> 6)) m &= tk_split_upto((uint32_t)b & 63u);
    return m;
}
// the last / first set bit of plane pl in [a, b] (a <= b < 64 W), all ones if there is none: one thread, word by word
template <class Planes>
TK_HD uint64_t tk_split_last_in(const Planes& P, uint32_t pl, uint64_t a, uint64_t b) {
    for (uint64_t w = b >> 6;; --w) {
        const uint64_t v = P.word(pl, w) & tk_split_window_mask(w, a, b);
        if (v) return w * 64 + 63 - (uint64_t)__builtin_clzll(v);
        if (w == (a >> 6)) return ~0ull;
    }
}
template <class Planes>
TK_HD uint64_t tk_split_first_in(const Planes& P, uint32_t pl, uint64_t a, uint64_t b) {
    for (uint64_t w = a >> 6; w <= (b >> 6); ++w) {
        const uint64_t v = P.word(pl, w) & tk_split_window_mask(w, a, b);
        if (v) return w * 64 + (uint64_t)__builtin_ctzll(v);
    }
    return ~0ull;
}

// ---- the choice inside a window ----
// The boundary a window [a, b] of global positions gives: the lowest level that occurs, of it the last; no level: the last legal one
// (*cut = TK_SPLITC_HARD); none legal: all ones.  One thread:
template <class Planes>
TK_HD uint64_t tk_split_pick(const TkSplit& p, const Planes& P, uint64_t a, uint64_t b, uint32_t* cut) {
    for (uint32_t pl = 0; pl <= p.L; ++pl) {
        const uint64_t e = tk_split_last_in(P, pl, a, b);
        if (e != ~0ull) {
            *cut = pl < p.L ? pl : TK_SPLITC_HARD;
            return e;
        }
    }
    return ~0ull;
}
// ... and a wavefront, when the window's words of all L + 1 planes are at most 64: lane `lane` fetches word lane % nw of plane lane / nw,
// masked to the window (tk_split_probe); the ballot of the lanes whose word is not 0 then holds, plane after plane, which words have a
// boundary, and the answer is in the highest such word of the first such plane (tk_split_choose; wave.word(lane) is that lane's word).
TK_HD uint32_t tk_split_window_words(uint64_t a, uint64_t b) { return (uint32_t)((b >> 6) - (a >> 6)) + 1u; }
TK_HD bool tk_split_fits(const TkSplit& p, uint64_t a, uint64_t b) { return (b >> 6) - (a >> 6) < 64u && tk_split_window_words(a, b) * (p.L + 1u) <= 64u; }
template <class Planes>
TK_HD uint64_t tk_split_probe(const TkSplit& p, const Planes& P, uint32_t lane, uint64_t a, uint64_t b) {
    const uint32_t nw = tk_split_window_words(a, b), pl = lane / nw;
    if (pl > p.L) return 0ull;
    const uint64_t w = (a >> 6) + lane % nw;
    return P.word(pl, w) & tk_split_window_mask(w, a, b);
}
template <class Wave>
TK_HD uint64_t tk_split_choose(const TkSplit& p, uint64_t ballot, uint64_t a, uint64_t b, const Wave& wave, uint32_t* cut) {
    const uint32_t nw = tk_split_window_words(a, b);
    const uint64_t all = nw == 64u ? ~0ull : (1ull << nw) - 1;
    for (uint32_t pl = 0; pl <= p.L; ++pl) {
        const uint64_t part = (ballot >> (pl * nw)) & all;
        if (part) {
            const uint32_t j = 63u - (uint32_t)__builtin_clzll(part);
            const uint64_t v = wave.word(pl * nw + j);
            *cut = pl < p.L ? pl : TK_SPLITC_HARD;
            return ((a >> 6) + j) * 64 + 63 - (uint64_t)__builtin_clzll(v);
        }
    }
    return ~0ull;
}
// What a wavefront is to the rule: gather(f) runs f(lane) in every lane and returns the ballot of the lanes whose result is not 0,
// word(lane) is that lane's result afterwards; every lane of the wavefront is in the call with the same arguments.  The device's is
// TkWave64 (tk_split.h); the CPU simulation's computes the 64 lanes one after the other; TkSplitSolo is a thread on its own.
struct TkSplitSolo {};
template <class Planes, class Wave>
TK_HD uint64_t tk_split_pick(const TkSplit& p, const Planes& P, Wave& wave, uint64_t a, uint64_t b, uint32_t* cut) {
    if (!tk_split_fits(p, a, b)) return tk_split_pick(p, P, a, b, cut);
    const uint64_t ballot = wave.gather([&](uint32_t lane) { return tk_split_probe(p, P, lane, a, b); });
    return tk_split_choose(p, ballot, a, b, wave, cut);
}
template <class Planes>
TK_HD uint64_t tk_split_pick(const TkSplit& p, const Planes& P, TkSplitSolo&, uint64_t a, uint64_t b, uint32_t* cut) {
    return tk_split_pick(p, P, a, b, cut);
}

// ---- one step of the chain ----
// where the chunk behind a cut at e begins (e: an interior boundary of the document at g0): the smallest legal boundary in [e - O, e], else e
template <class Planes>
TK_HD uint64_t tk_split_restart(const TkSplit& p, const Planes& P, uint64_t g0, uint64_t e) {
    if (!p.O) return e;
    const uint64_t f = tk_split_first_in(P, p.L, g0 + e - p.O, g0 + e);  // (e - O > 0: e >= M > O)
    return f != ~0ull ? f - g0 : e;
}
struct TkSplitStep {
    uint64_t e, next;  // the chunk is [s, e); the next one starts at `next` (n when the chain ends)
    uint32_t cut;
};
// The chunk that starts at token s < n of the document [g0, g0 + n)
template <class Planes, class Wave>
TK_HD void tk_split_next(const TkSplit& p, const Planes& P, Wave& wave, uint64_t g0, uint64_t n, uint64_t s, TkSplitStep* st) {
    if (n - s <= p.N) {
        st->e = st->next = n;
        st->cut = TK_SPLITC_END;
        return;
    }
    uint32_t cut = TK_SPLITC_FORCED;
    const uint64_t e = tk_split_pick(p, P, wave, g0 + s + p.M, g0 + s + p.N, &cut);  // (s + N < n: all interior)
    st->e = e != ~0ull ? e - g0 : s + p.N;
    st->cut = cut;
    st->next = tk_split_restart(p, P, g0, st->e);
}

// ---- walks ----
// From the start s along the chain while the starts lie below lim <= n: mark(g) for every start, *steps counts them.  Returns the first
// start at or beyond lim (n when the chain has ended).
template <class Planes, class Wave, class Mark>
TK_HD uint64_t tk_split_walk(const TkSplit& p, const Planes& P, Wave& wave, uint64_t g0, uint64_t n, uint64_t s, uint64_t lim, Mark& mark, uint64_t* steps) {
    while (s < lim) {
        mark(g0 + s);
        TkSplitStep st;
        tk_split_next(p, P, wave, g0, n, s, &st);
        s = st.next;
        ++*steps;
    }
    return s;
}
// The guessed start of a speculative walk in the block that begins at lo, inside the document [g0, g0 + n) (g0 < lo): where the chunk
// behind the cut of the window [lo + O, lo + O + N - M] begins -- the cut a chain standing at lo + O - M would make, so a place where
// chains that come from further left are likely to pass.  The window ends before `end` (the block's end or the document's).  All ones:
// no legal boundary there, no walk.  (It affects only the speed: the stitch pass trusts a speculative start only when the true chain
// stands on it.)
template <class Planes, class Wave>
TK_HD uint64_t tk_split_guess(const TkSplit& p, const Planes& P, Wave& wave, uint64_t g0, uint64_t lo, uint64_t end) {
    const uint64_t a = lo + p.O;
    uint64_t b = a + (p.N - p.M);
    if (b >= end) b = end - 1;
    if (a > b) return ~0ull;
    uint32_t cut;
    const uint64_t e = tk_split_pick(p, P, wave, a, b, &cut);
    return e != ~0ull ? tk_split_restart(p, P, g0, e - g0) : ~0ull;  // (>= lo - g0: e >= lo + O)
}

enum { TK_SPLIT_ST_SEGS = 0, TK_SPLIT_ST_JOINED, TK_SPLIT_ST_STITCH, TK_SPLIT_ST_SPEC, TK_SPLIT_STATS };
// Block b of the walk pass (one wavefront): the document that runs into the block from the left is walked from a guessed start, marking
// `spec`; every document that starts in the block is walked from its start, marking `cut`.  Both stop at the block's end; where the
// document goes on behind it, exit_at[b] = the first start of that walk at or beyond the end (a global position; T at most).
// stats[]: TK_SPLIT_ST_SEGS and TK_SPLIT_ST_SPEC are counted here (added with add(word, v)).
template <class Planes, class Wave, class Off, class MarkCut, class MarkSpec, class Add>
TK_HD void tk_split_block(const TkSplit& p, const Planes& P, Wave& wave, Off tok_off, uint64_t b, MarkCut& mark_cut, MarkSpec& mark_spec, uint32_t* exit_at, Add& add) {
    const uint64_t lo = b * p.K, hi = p.n_tokens - lo > p.K ? lo + p.K : p.n_tokens;  // (lo < T)
    uint64_t d = tk_last_le(tok_off, 0, p.n_docs, lo), segs = 0, spec_steps = 0, true_steps = 0;
    uint64_t g0 = tok_off[d], g1 = tok_off[d + 1];  // (the document that holds lo: not empty)
    if (g0 < lo) {
        const uint64_t end = g1 < hi ? g1 : hi;
        const uint64_t s = tk_split_guess(p, P, wave, g0, lo, end);
        ++segs;
        if (s != ~0ull) {
            const uint64_t out = tk_split_walk(p, P, wave, g0, g1 - g0, s, end - g0, mark_spec, &spec_steps);
            if (g1 > hi) exit_at[b] = (uint32_t)(g0 + out);
        }
        if (g1 >= hi) d = p.n_docs;  // (nothing starts in this block)
        else d = d + 1 < p.n_docs ? tk_last_le(tok_off, d + 1, p.n_docs, g1) : p.n_docs;  // the document that holds g1: empty ones are stepped over
    }
    while (d < p.n_docs) {
        g0 = tok_off[d];
        g1 = tok_off[d + 1];
        if (g0 >= hi || g1 == g0) break;  // (g1 == g0: only empty documents are left)
        const uint64_t end = g1 < hi ? g1 : hi;
        ++segs;
        const uint64_t out = tk_split_walk(p, P, wave, g0, g1 - g0, 0, end - g0, mark_cut, &true_steps);
        if (g1 > hi) exit_at[b] = (uint32_t)(g0 + out);
        if (g1 >= hi || d + 1 >= p.n_docs) break;
        d = tk_last_le(tok_off, d + 1, p.n_docs, g1);
    }
    add(TK_SPLIT_ST_SEGS, segs);
    add(TK_SPLIT_ST_SPEC, spec_steps);
}
// Document d of the stitch pass (one wavefront; only a document of more than one block has work): the true chain leaves the document's
// first block at exit_at[], and in every later block it enters it walks, marking `cut`, until it stands on a position whose spec bit is
// set -- the join: from there the speculative walk of that block is the true chain, join_at[block] = the position, and the chain goes on
// where that walk left the block -- or until it leaves the block.  A block the chain jumps over, or does not join in, keeps
// join_at = TK_SPLIT_NOWHERE.  spec.bit(g): bit g of the spec plane.
template <class Planes, class Wave, class Off, class Spec, class MarkCut, class Add>
TK_HD void tk_split_stitch(const TkSplit& p, const Planes& P, Wave& wave, Off tok_off, const Spec& spec, uint64_t d, MarkCut& mark_cut, const uint32_t* exit_at,
                           uint32_t* join_at, Add& add) {
    const uint64_t g0 = tok_off[d], g1 = tok_off[d + 1];
    if (g1 == g0 || (g1 - 1) / p.K == g0 / p.K) return;
    uint64_t pos = exit_at[g0 / p.K], steps = 0, joined = 0;
    while (pos < g1) {
        const uint64_t b = pos / p.K, hi = (b + 1) * p.K, end = g1 < hi ? g1 : hi;
        bool join = false;
        while (pos < end && !(join = spec.bit(pos))) {
            mark_cut(pos);
            TkSplitStep st;
            tk_split_next(p, P, wave, g0, g1 - g0, pos - g0, &st);
            pos = g0 + st.next;
            ++steps;
        }
        if (join) {
            join_at[b] = (uint32_t)pos;
            ++joined;
            pos = g1 > hi ? exit_at[b] : g1;  // (a walk that ends with its document has no exit: the chain ends there too)
        }
    }
    add(TK_SPLIT_ST_STITCH, steps);
    add(TK_SPLIT_ST_JOINED, joined);
}

// ---- fold, count, rank ----
// word w of `cut` once the speculative starts from its block's join on are the truth
TK_HD uint64_t tk_split_fold(const TkSplit& p, uint64_t cut_w, uint64_t spec_w, uint64_t w, const uint32_t* join_at) {
    const uint64_t j = join_at[w * 64 / p.K];
    if (j == TK_SPLIT_NOWHERE || j >= (w + 1) * 64) return cut_w;
    return cut_w | (j <= w * 64 ? spec_w : spec_w & tk_split_from((uint32_t)j & 63u));
}
// The starts below position g <= T: cnt[] holds the starts before every count block of cb_words words (the scan's result)
template <class Words, class Cnt>
TK_HD uint64_t tk_split_rank(Words cut, Cnt cnt, uint32_t cb_words, uint64_t g) {
    const uint64_t w = g >> 6, blk = w / cb_words;
    uint64_t r = cnt[blk];
    for (uint64_t i = blk * cb_words; i < w; ++i) r += (uint64_t)__builtin_popcountll(cut[i]);
    return r + (uint64_t)__builtin_popcountll(cut[w] & ~tk_split_from((uint32_t)g & 63u));
}

// ---- the record of one start ----
struct TkSplitOut {
    uint32_t *doc, *tok_begin, *tok_end, *byte_begin, *byte_end, *char_begin, *char_end;
    uint8_t* cut;
};
// Chunk i starts at the global position g: its document, its end (the step from g once more) and its places in the text, from the spans
// (byte_start / char_start per token, byte_off / char_off per document)
template <class Planes, class Off, class Start, class DocOff>
TK_HD void tk_split_record(const TkSplit& p, const Planes& P, Off tok_off, Start byte_start, Start char_start, DocOff byte_off, DocOff char_off, uint64_t g, uint64_t i,
                           const TkSplitOut& o) {
    const uint64_t d = tk_last_le(tok_off, 0, p.n_docs, g), g0 = tok_off[d], n = tok_off[d + 1] - g0;
    TkSplitStep st;
    TkSplitSolo solo;
    tk_split_next(p, P, solo, g0, n, g - g0, &st);
    const bool last = st.e == n;
    o.doc[i] = (uint32_t)d;
    o.tok_begin[i] = (uint32_t)(g - g0);
    o.tok_end[i] = (uint32_t)st.e;
    o.byte_begin[i] = byte_start[g];
    o.char_begin[i] = char_start[g];
    o.byte_end[i] = last ? (uint32_t)(byte_off[d + 1] - byte_off[d]) : byte_start[g0 + st.e];
    o.char_end[i] = last ? (uint32_t)(char_off[d + 1] - char_off[d]) : char_start[g0 + st.e];
    o.cut[i] = (uint8_t)st.cut;
}
