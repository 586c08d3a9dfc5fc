// BPE training on the device: the parts of tk_train.h that are plain C++ -- the hash of a word, how a slot of the word table names its
// claimant's bytes, the probe loops of the word table and of the pair table, the position key, and what a lane decides about its symbol
// when a pair is merged (run parity included).  Compiles for the host too: tests/test_train_sim.py drives them lane by lane on the CPU.
//
// The rule (include/tiktoken_amd.h, tk_train_bpe): the distinct pieces of the corpus are words with a weight and the corpus offset of their
// first occurrence; symbols 0..255 are the bytes, 256 + k the k-th merge; a symbol keeps the offset of its first byte, so word offset +
// symbol offset orders all symbols as a walk over the corpus meets them.  A step counts the adjacent pairs inside words, weighted; the
// winner is the pair at the smallest position among the pairs with the largest count; every word is rewritten left to right.
#pragma once
#include <stdint.h>

#include "tk_common.h"

// ---- words ----
// Hash of a word's bytes: it selects where the probing starts, nothing more (a slot is taken for the word only after its bytes have been
// compared).  Words of up to TK_TRAIN_HASH_ALL bytes hash every byte, longer ones their length, their first and their last 32 bytes.
// seed 0 is for tests: the length and the first byte alone, so that different words share a hash.
#define TK_TRAIN_HASH_ALL 64u
template <class At>
TK_HD uint64_t tk_train_word8(At&& at, uint32_t o, uint32_t end) {  // up to eight bytes from o on, little-endian
    uint64_t w = 0;
    for (uint32_t j = 0; j < 8u && o + j < end; ++j) w |= (uint64_t)at(o + j) << (8u * j);
    return w;
}
template <class At>
TK_HD uint64_t tk_train_hash(At&& at, uint32_t len, uint64_t seed) {
    uint64_t h = tk_hash_step(seed, len);
    if (!seed) return tk_mix64(tk_hash_step(h, len ? at(0u) : 0u));
    if (len <= TK_TRAIN_HASH_ALL) {
        for (uint32_t o = 0; o < len; o += 8u) h = tk_hash_step(h, tk_train_word8(at, o, len));
    } else {
        for (uint32_t o = 0; o < 32u; o += 8u) h = tk_hash_step(h, tk_train_word8(at, o, len));
        for (uint32_t o = len - 32u; o < len; o += 8u) h = tk_hash_step(h, tk_train_word8(at, o, len));
    }
    return tk_mix64(h);
}

// A slot's key names the bytes of the word that claimed it: 0 = empty; while the claimant's chunk is on the device, its place in the
// chunk's text (pos + 1) below its length; afterwards (TK_TRAIN_IN_BLOB) its place in the call's word blob.  pos, len < 2^31; off < 2^32.
#define TK_TRAIN_IN_BLOB (1ull << 63)
TK_HD uint64_t tk_train_text_ref(uint32_t pos, uint32_t len) { return ((uint64_t)len << 32) | (uint64_t)(pos + 1u); }
TK_HD uint64_t tk_train_blob_ref(uint32_t off, uint32_t len) { return TK_TRAIN_IN_BLOB | ((uint64_t)len << 32) | off; }
TK_HD uint32_t tk_train_ref_len(uint64_t r) { return (uint32_t)(r >> 32) & 0x7FFFFFFFu; }
TK_HD const uint8_t* tk_train_ref_bytes(uint64_t r, const uint8_t* text, const uint8_t* blob) {
    return (r & TK_TRAIN_IN_BLOB) ? blob + (uint32_t)r : text + ((uint32_t)r - 1u);
}

// The slot of a word: open addressing from hash & mask on.  An empty slot is claimed with compare-and-swap (`cas(ptr, expected, desired)`
// returns what was there) by whichever occurrence comes first; a slot that is taken is the word's only if length and bytes are those of its
// claimant, else the probe moves on.  The key is complete the moment it is visible, so nobody waits for anybody.  All ones: no slot in
// mask + 1 probes (the caller sizes the table so that this cannot happen).
template <class Cas>
TK_HD uint64_t tk_train_word_slot(unsigned long long* keys, uint64_t mask, uint64_t hash, uint64_t my_ref, const uint8_t* mine, uint32_t len,
                                  const uint8_t* text, const uint8_t* blob, Cas&& cas) {
    uint64_t s = hash & mask;
    for (uint64_t n = 0; n <= mask; ++n, s = (s + 1u) & mask) {
        unsigned long long cur = keys[s];  // (a stale read can only say "empty": the compare-and-swap decides)
        if (cur == 0ull) cur = cas(&keys[s], 0ull, (unsigned long long)my_ref);
        if (cur == 0ull) return s;
        if (tk_train_ref_len(cur) != len) continue;
        const uint8_t* q = tk_train_ref_bytes(cur, text, blob);
        uint32_t j = 0;
        while (j < len && q[j] == mine[j]) ++j;
        if (j == len) return s;
    }
    return ~0ull;
}
// ... of a word that is known to be in no slot yet (a table that grows takes the old one's words): the first empty slot
template <class Cas>
TK_HD uint64_t tk_train_word_place(unsigned long long* keys, uint64_t mask, uint64_t hash, uint64_t ref, Cas&& cas) {
    uint64_t s = hash & mask;
    for (uint64_t n = 0; n <= mask; ++n, s = (s + 1u) & mask)
        if (keys[s] == 0ull && cas(&keys[s], 0ull, (unsigned long long)ref) == 0ull) return s;
    return ~0ull;
}

// ---- pairs ----
struct TkTrainPair {  // a slot of the pair table, cleared to zero before every step
    unsigned long long key;  // tk_train_pair_key; 0 = empty
    unsigned long long cnt;  // sum of the weights of the words the pair occurs in, once per occurrence
};
TK_HD uint64_t tk_train_pair_key(uint32_t a, uint32_t b) { return (((uint64_t)a << 32) | b) + 1ull; }  // (symbols stay below 2^31)
TK_HD uint64_t tk_train_pair_hash(uint64_t key) { return tk_mix64(key * 0x9E3779B97F4A7C15ull); }
// the pair's slot, claimed if need be (counting) ...
template <class Cas>
TK_HD uint64_t tk_train_pair_slot(TkTrainPair* tab, uint64_t mask, uint64_t key, Cas&& cas) {
    uint64_t s = tk_train_pair_hash(key) & mask;
    for (uint64_t n = 0; n <= mask; ++n, s = (s + 1u) & mask) {
        unsigned long long cur = tab[s].key;
        if (cur == 0ull) cur = cas(&tab[s].key, 0ull, (unsigned long long)key);
        if (cur == 0ull || cur == key) return s;
    }
    return ~0ull;
}
// ... and looked up (after the counting: every pair of the step has its slot)
TK_HD uint64_t tk_train_pair_find(const TkTrainPair* tab, uint64_t mask, uint64_t key) {
    uint64_t s = tk_train_pair_hash(key) & mask;
    for (uint64_t n = 0; n <= mask; ++n, s = (s + 1u) & mask) {
        const unsigned long long cur = tab[s].key;
        if (cur == key) return s;
        if (cur == 0ull) break;
    }
    return ~0ull;
}

// ---- positions ----
// Where a symbol stands in the corpus: the offset of its word's first occurrence plus the offset of its first byte in the word.  Pieces
// do not overlap, so no two symbols of the distinct words share a position, and ascending positions are the order in which a walk over
// all pieces of the corpus meets a symbol (of a word it has not seen before) for the first time.
TK_HD uint64_t tk_train_pos(uint64_t word_first, uint32_t sym_off) { return word_first + sym_off; }

// ---- the rewrite ----
// Symbol i of the arrays, its neighbours inside its word (has_prev / has_next: there is one), the winner (a, b).  For a == b a run of k
// equal symbols merges floor(k / 2) times from its first symbol on: a lane needs d, its distance from the run's start.  Symbol i
// CONTINUES a run when its left neighbour and itself are both a; the run's start is the last symbol at or before i that does not.
// Lanes report tk_train_break_mark (0: continues, else index + 1); the largest mark at or before i, carried across workgroups, is the
// start's index + 1 -- nobody walks back along the run.
enum { TK_TRAIN_KEEP = 0, TK_TRAIN_LEFT = 1, TK_TRAIN_RIGHT = 2 };  // stays; becomes the new symbol; is taken into it (leaves the arrays)
TK_HD bool tk_train_continues(bool has_prev, uint32_t s_prev, uint32_t s, uint32_t a) { return has_prev && s_prev == a && s == a; }
TK_HD uint32_t tk_train_break_mark(uint32_t i, bool continues) { return continues ? 0u : i + 1u; }
TK_HD int tk_train_decide(uint32_t a, uint32_t b, bool has_prev, uint32_t s_prev, uint32_t s, bool has_next, uint32_t s_next, uint32_t d) {
    if (a != b) {  // occurrences cannot overlap: the two neighbours say it all
        if (s == a && has_next && s_next == b) return TK_TRAIN_LEFT;
        if (s == b && has_prev && s_prev == a) return TK_TRAIN_RIGHT;
        return TK_TRAIN_KEEP;
    }
    if (s != a) return TK_TRAIN_KEEP;
    if (d & 1u) return TK_TRAIN_RIGHT;
    return has_next && s_next == a ? TK_TRAIN_LEFT : TK_TRAIN_KEEP;  // (an odd run leaves its last symbol alone)
}
