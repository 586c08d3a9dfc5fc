// Repetition statistics per document: the parts of the device passes of tk_repeat.h that are plain C++ -- which sizes a call takes, which
// documents a workgroup owns, the slot word of the table in LDS and the slot of the table in HBM, an n-gram's hash in either, the walk
// that inserts an occurrence and the walk that finds it again, the region of a long document, and the popcount over a range of bits.  The
// rule is stated in include/tiktoken_amd.h.  Compiles for the host too.
//
// The two classes.  A document of L <= C = TK_RP_LDS_TOKENS tokens is short: the workgroup of the tile of T = TK_RP_TILE positions in
// which it starts owns it, counts its n-grams in a table in LDS and writes its rows with plain stores.  A longer one is counted in a
// table in HBM (tiles of TK_RP_LTILE positions, atomics into its rows).
//
// Why T = 1024, C = 2048, 4096 slots of 4 bytes, 512 lanes.  A workgroup stages at most T + C - 1 = 3071 ids (12 KiB), the document of
// every staged position as the 16-bit offset of its first token in the tile (6 KiB), the length of the document that starts at a tile
// position (2 KiB), a most-frequent count per such document (4 KiB), the table (16 KiB) and four rows of bit words (1.3 KiB): 42 KiB, so
// three workgroups share the 160 KiB of a CU's LDS and 24 of its 32 wavefront slots are taken.  The documents a tile owns hold T tokens
// on average, a load of 0.25; at most 3071, a load of 0.75, where a walk is long but ends (there is always an empty slot).  A slot is
// one 32-bit word -- 12 bits of position, 8 of the hash as a tag, 12 of count, which holds C -- so that a claim is one 32-bit
// compare-and-swap and a further occurrence one atomic add; two words per slot, or 8192 slots, would leave two workgroups per CU.
// C = 4096 needs 13-bit fields and 64 KiB for one workgroup; C = 1024 sends every document of 1025 .. 2048 tokens, common in the
// corpora this is for, to HBM.  Each lane keeps the slots of its six positions in registers between the insert and the count.
#pragma once
#include <stdint.h>

#include "tk_ngram_rule.h"  // tk_ng_starts_end, tk_ng_key, tk_ng_smear, tk_ng_bits, tk_ng_popc; tk_fp_hash, tk_fp_walk; tk_last_le

#define TK_RP_TILE 1024u                               // positions in which a workgroup's documents start
#define TK_RP_LDS_TOKENS 2048u                         // the longest short document
#define TK_RP_THREADS 512u                             // lanes of the LDS class
#define TK_RP_SPAN (TK_RP_TILE + TK_RP_LDS_TOKENS)     // positions a workgroup may stage
#define TK_RP_PER_LANE (TK_RP_SPAN / TK_RP_THREADS)    // positions of a lane
#define TK_RP_SLOTS 4096u                              // slots of the table in LDS
#define TK_RP_MAX_SIZES 8u
#define TK_RP_MAX_DOC (1ull << 31)                     // a document of that many tokens is refused
#define TK_RP_SEED 0x5245504541540001ull
#define TK_RP_NONE 0xFFFFu                             // a staged position no owned document holds
#define TK_RP_LTILE TK_NG_TILE                         // positions of a tile of the long class (its staging is tk_ng_stage)
#define TK_RP_LTHREADS TK_NG_THREADS

struct TkRp {
    uint32_t n_sizes, k[TK_RP_MAX_SIZES];
    uint64_t n_tokens, n_docs;
    uint64_t base, end;  // the long class's table covers the positions [base, end): a region starts at slot 4 (tok_off[d] - base)
};

// The sizes of a call.  0, or why they are refused: 1 their number, 2 a size.
TK_HD int tk_rp_shape(const uint32_t* sizes, uint64_t n_sizes, uint64_t n_tokens, uint64_t n_docs, TkRp* p) {
    if (n_sizes < 1 || n_sizes > TK_RP_MAX_SIZES || !sizes) return 1;
    for (uint32_t i = 0; i < n_sizes; ++i) {
        if (sizes[i] < 1 || sizes[i] > TK_FP_MAX_NGRAM) return 2;
        p->k[i] = sizes[i];
    }
    p->n_sizes = (uint32_t)n_sizes, p->n_tokens = n_tokens, p->n_docs = n_docs, p->base = 0, p->end = n_tokens;
    return 0;
}
TK_HD bool tk_rp_is_long(uint64_t L) { return L > TK_RP_LDS_TOKENS && L < TK_RP_MAX_DOC; }  // (a document past the limit is in no class: its rows are zeros)

// Is the document [s, e) counted in the table in HBM?  (Whatever tok_off holds, a region that passes lies inside the table.)
TK_HD bool tk_rp_in_table(const TkRp& p, uint64_t s, uint64_t e) { return s < e && tk_rp_is_long(e - s) && s >= p.base && e <= p.end; }

// The first document d of [0, n_docs) with tok_off[d] >= g, n_docs when there is none: the tile [g0, g1) owns the documents
// [first_ge(g0), first_ge(g1)), empty ones included, and the last tile every document behind them.
template <class Off>
TK_HD uint64_t tk_rp_first_ge(const Off& tok_off, uint64_t n_docs, uint64_t g) {
    uint64_t a = 0, b = n_docs;
    while (a < b) {
        const uint64_t mid = (a + b) >> 1;
        if (tok_off[mid] < g) a = mid + 1;
        else b = mid;
    }
    return a;
}
TK_HD uint32_t tk_rp_msb(uint64_t x) {  // x != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return 63u - (uint32_t)__clzll((long long)x);
#else
    return 63u - (uint32_t)__builtin_clzll(x);
#endif
}
// The tile offset of the first token of the document that holds the staged position i: the highest bit of `startw` (one bit per tile
// position at which a document that is not empty starts) at or below min(i, tile - 1); TK_RP_NONE when there is none.
template <class Words>
TK_HD uint32_t tk_rp_doc_start(const Words& startw, uint32_t tile, uint32_t i) {
    const uint32_t t = i < tile ? i : tile - 1;
    uint32_t w = t >> 6;
    uint64_t m = startw[w] & tk_ng_bits(0, (t & 63u) + 1);
    while (!m && w) m = startw[--w];
    return m ? w * 64 + tk_rp_msb(m) : TK_RP_NONE;
}
// The set bits of [a, b) of a row of 64-bit words
template <class Words>
TK_HD uint32_t tk_rp_range_popc(const Words& words, uint32_t a, uint32_t b) {
    uint32_t n = 0;
    for (uint32_t w = a >> 6; a < b && w * 64 < b; ++w) {
        const uint32_t lo = a > w * 64 ? a - w * 64 : 0, hi = b < w * 64 + 64 ? b - w * 64 : 64;
        n += tk_ng_popc(words[w] & tk_ng_bits(lo, hi));
    }
    return n;
}

// ---- the table in LDS.  A slot: 0 empty; else bits 0 .. 11 the claimer's staged position + 1, 12 .. 19 a tag, 20 .. 31 the count.
#define TK_RP_ONE (1u << 20)
// ids[at .. at + k) of the document that starts at tile offset ds: the hash chooses the slot and the tag, nothing else
template <class Ids>
TK_HD uint64_t tk_rp_lds_hash(const Ids& ids, uint32_t at, uint32_t k, uint32_t ds) {
    return tk_fp_hash(ids, at, k, TK_RP_SEED) + (uint64_t)(ds + 1) * 0x9E3779B97F4A7C15ull;
}
TK_HD uint32_t tk_rp_lds_ident(uint64_t h, uint32_t pos) { return (pos + 1) | ((uint32_t)(h >> 32) & 0xFFu) << 12; }
// The occurrence at `pos` into the table: the slot that counts its n-gram.  same(q): is the n-gram at staged position q this one -- same
// document, same k ids?  cas(i, v): claims slot i if it is empty, returns what it held; add(i): raises its count.  *claimed: this
// occurrence is the n-gram's first.  S: no slot (a full table; there are more slots than positions).
template <class Table, class Same, class Cas, class Add>
TK_HD uint32_t tk_rp_lds_insert(const Table& table, uint32_t S, uint64_t h, uint32_t pos, Same&& same, Cas&& cas, Add&& add, bool* claimed) {
    const uint32_t id = tk_rp_lds_ident(h, pos);
    uint32_t i = (uint32_t)h & (S - 1);
    *claimed = false;
    for (uint32_t n = 0; n < S; ++n, i = (i + 1) & (S - 1)) {
        uint32_t v = table[i];
        if (v == 0) v = cas(i, id | TK_RP_ONE);
        if (v == 0) return *claimed = true, i;
        if (((v ^ id) & 0xFF000u) == 0 && same((v & 0xFFFu) - 1)) return add(i), i;
    }
    return S;
}
TK_HD uint32_t tk_rp_lds_count(uint32_t slot_word) { return slot_word >> 20; }

// ---- the table in HBM.  A slot: 0 empty; else the low half the claimer's position in its document + 1, the high half the count.
TK_HD uint64_t tk_rp_region_slots(uint64_t L) {  // the power of two >= 2 L: fewer than 4 L
    uint64_t S = 2;
    while (S < 2 * L) S <<= 1;
    return S;
}
#define TK_RP_LONE (1ull << 32)
// As tk_rp_lds_insert, in the region [base, base + S) of `table`; pos and same(q) are positions in the document.
template <class Table, class Same, class Cas, class Add>
TK_HD void tk_rp_long_insert(const Table& table, uint64_t base, uint64_t S, uint64_t key, uint32_t pos, Same&& same, Cas&& cas, Add&& add) {
    uint64_t i = key & (S - 1);
    for (uint64_t n = 0; n < S; ++n, i = (i + 1) & (S - 1)) {
        uint64_t v = table[base + i];
        if (v == 0) v = cas(base + i, (uint64_t)(pos + 1) | TK_RP_LONE);
        if (v == 0) return;
        if (same((uint32_t)v - 1)) return add(base + i);
    }
}
// The slot of an n-gram that was inserted; 0 if it was not
template <class Table, class Same>
TK_HD uint64_t tk_rp_long_find(const Table& table, uint64_t base, uint64_t S, uint64_t key, Same&& same) {
    uint64_t i = key & (S - 1);
    for (uint64_t n = 0; n < S; ++n, i = (i + 1) & (S - 1)) {
        const uint64_t v = table[base + i];
        if (v == 0) return 0;
        if (same((uint32_t)v - 1)) return v;
    }
    return 0;
}
