// BPE training on the device (tk_train_bpe): the merges the reference's educational trainer makes on a corpus (tiktoken/_educational.py:
// bpe_train), pair for pair.  The pre-tokeniser has left the piece starts of a chunk on the device; from there on:
//   tk_k_train_words    one thread per piece: its slot in the word table (open addressing by a 64-bit hash of the bytes; claimed with
//                       compare-and-swap by whichever occurrence comes first, every other one compares its bytes with the claimant's and
//                       moves on if they differ), then atomicAdd on the weight and atomicMin on the corpus offset of the first occurrence
//   tk_k_train_blob     per slot claimed in this chunk: the claimant's bytes go into the call's word blob (they must outlive the chunk's
//                       text) and the key names them there
//   tk_k_train_rehash   a table that grows: every word of the old one into the new one
//   tk_k_train_expand   the blob IS the first symbol array (a byte is its own symbol): per word, the word index and the position key of
//                       every symbol beside it
// and per merge, with no host wait in between (the live symbol count, the winner and the "no pair left" flag are device cells, the
// grids are sized for the first step):
//   (clear of the pair table)
//   tk_k_train_count    every adjacent pair inside a word: its slot in the pair table, atomicAdd of the word's weight; the largest sum any
//                       add has produced is the largest count (atomicMax)
//   tk_k_train_best     every pair whose count is that maximum: atomicMin of its position key
//   tk_k_train_pick     the symbol at that position names the winner; merge and count are appended to the call's result
//   tk_k_train_breaks / tk_k_train_carry   (a == b only) run starts carried across workgroups
//   tk_k_train_decide   per symbol: stays, becomes the new symbol, or leaves (tk_train_decide); survivors per workgroup
//   tk_k_train_offsets  one workgroup: exclusive sums of those counts, the next live count; the step's cells are reset
//   tk_k_train_rewrite  survivors to the other set of arrays
// All atomics are integer adds, minima, maxima and claims of empty slots: the merges do not depend on the order in which they land (the
// layout of the blob and of the table does, and nothing reads it that way).  The rule is tk_train_rule.h's.  Included by tk_api.hip only.
#pragma once
#include "tk_scan.h"
#include "tk_train_rule.h"

#define TKT_BLOCK 256u  // symbols per workgroup of the step's kernels, one per lane

// the cells of a call (unsigned long long each)
enum {
    TKT_LIVE = 0,  // [2] symbols in the arrays of either parity
    TKT_CMAX = 2,  // largest pair count of the step (0 before the counting)
    TKT_BEST,      // smallest position key among the pairs with that count (all ones before)
    TKT_WIN,       // the winner, a << 32 | b
    TKT_DONE,      // 0, or 1 + the step that found no pair: every later kernel does nothing
    TKT_NWORDS,    // distinct words
    TKT_BLOB,      // bytes of the word blob in use
    TKT_FULL,      // a probe found no slot (cannot happen with the sizes the host chooses; checked after every chunk)
    TKT_CELLS
};

struct TkTrainTab {  // the word table
    unsigned long long* key;     // tk_train_text_ref / tk_train_blob_ref of the claimant; 0 = empty
    unsigned long long* weight;  // occurrences
    unsigned long long* first;   // corpus offset of the first one (all ones in an empty slot)
    uint64_t mask;
};

struct TkTrainCas {
    __device__ __forceinline__ unsigned long long operator()(unsigned long long* p, unsigned long long expect, unsigned long long want) const { return atomicCAS(p, expect, want); }
};

__global__ __launch_bounds__(256) void tk_k_train_tab_init(TkTrainTab t) {
    for (uint64_t s = blockIdx.x * 256ull + threadIdx.x; s <= t.mask; s += (uint64_t)gridDim.x * 256) {
        t.key[s] = 0ull;
        t.weight[s] = 0ull;
        t.first[s] = ~0ull;
    }
}

// pstart: P + 1 ascending piece starts of the chunk (bit 31: a char the pattern leaves unmatched -- no word); base: corpus offset of the chunk
__global__ __launch_bounds__(256) void tk_k_train_words(const uint8_t* __restrict__ text, const uint32_t* __restrict__ pstart, uint64_t P, uint64_t base,
                                                        const uint8_t* __restrict__ blob, TkTrainTab t, uint64_t seed, unsigned long long* __restrict__ cells) {
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < P; i += (uint64_t)gridDim.x * 256) {
        const uint32_t s = pstart[i];
        if (s >> 31) continue;
        const uint32_t e = pstart[i + 1] & 0x7FFFFFFFu;
        if (e <= s) continue;
        const uint32_t len = e - s;
        const uint8_t* mine = text + s;
        const uint64_t h = tk_train_hash([&](uint32_t j) { return mine[j]; }, len, seed);
        const uint64_t slot = tk_train_word_slot(t.key, t.mask, h, tk_train_text_ref(s, len), mine, len, text, blob, TkTrainCas());
        if (slot == ~0ull) {
            cells[TKT_FULL] = 1ull;
            continue;
        }
        atomicAdd(&t.weight[slot], 1ull);
        atomicMin(&t.first[slot], (unsigned long long)(base + s));
    }
}

// blob_cap: the host has made room for every byte of the chunk
__global__ __launch_bounds__(256) void tk_k_train_blob(const uint8_t* __restrict__ text, uint8_t* __restrict__ blob, uint64_t blob_cap, TkTrainTab t,
                                                       unsigned long long* __restrict__ cells) {
    for (uint64_t s = blockIdx.x * 256ull + threadIdx.x; s <= t.mask; s += (uint64_t)gridDim.x * 256) {
        const unsigned long long k = t.key[s];
        if (k == 0ull || (k & TK_TRAIN_IN_BLOB)) continue;
        const uint32_t len = tk_train_ref_len(k);
        const unsigned long long off = atomicAdd(&cells[TKT_BLOB], (unsigned long long)len);
        atomicAdd(&cells[TKT_NWORDS], 1ull);
        if (off + len > blob_cap || (off + len) >> 32) {
            cells[TKT_FULL] = 1ull;
            continue;
        }
        const uint8_t* src = tk_train_ref_bytes(k, text, blob);
        for (uint32_t j = 0; j < len; ++j) blob[off + j] = src[j];
        t.key[s] = tk_train_blob_ref((uint32_t)off, len);
    }
}

__global__ __launch_bounds__(256) void tk_k_train_rehash(TkTrainTab from, TkTrainTab to, const uint8_t* __restrict__ blob, uint64_t seed,
                                                         unsigned long long* __restrict__ cells) {
    for (uint64_t s = blockIdx.x * 256ull + threadIdx.x; s <= from.mask; s += (uint64_t)gridDim.x * 256) {
        const unsigned long long k = from.key[s];
        if (k == 0ull) continue;
        const uint8_t* w = tk_train_ref_bytes(k, nullptr, blob);  // (between chunks every key names the blob)
        const uint64_t h = tk_train_hash([&](uint32_t j) { return w[j]; }, tk_train_ref_len(k), seed);
        const uint64_t d = tk_train_word_place(to.key, to.mask, h, k, TkTrainCas());
        if (d == ~0ull) {
            cells[TKT_FULL] = 1ull;
            continue;
        }
        to.weight[d] = from.weight[s];
        to.first[d] = from.first[s];
    }
}

// sym / wid / pos: one entry per byte of the blob
__global__ __launch_bounds__(256) void tk_k_train_expand(TkTrainTab t, const uint8_t* __restrict__ blob, uint64_t n_sym, uint32_t* __restrict__ sym,
                                                         uint32_t* __restrict__ wid, unsigned long long* __restrict__ pos) {
    for (uint64_t s = blockIdx.x * 256ull + threadIdx.x; s <= t.mask; s += (uint64_t)gridDim.x * 256) {
        const unsigned long long k = t.key[s];
        if (!(k & TK_TRAIN_IN_BLOB)) continue;
        const uint32_t len = tk_train_ref_len(k), off = (uint32_t)k;
        if ((uint64_t)off + len > n_sym) continue;
        const unsigned long long first = t.first[s];
        for (uint32_t j = 0; j < len; ++j) {
            sym[off + j] = blob[off + j];
            wid[off + j] = (uint32_t)s;
            pos[off + j] = tk_train_pos(first, j);
        }
    }
}

// What the kernels of a step share.  par: which set of arrays holds the symbols (the other one receives the survivors).
struct TkTrainStep {
    uint32_t* sym[2];
    uint32_t* wid[2];
    unsigned long long* pos[2];
    const unsigned long long* weight;  // per slot of the word table (wid)
    TkTrainPair* pair;
    uint64_t pair_mask;
    uint8_t* dec;                 // per symbol: tk_train_decide's answer
    uint32_t* blk_mark;           // per workgroup: the largest break mark in it, then (in place) the largest one before it
    unsigned long long* blk_cnt;  // per workgroup: survivors, then (in place) the survivors before it
    unsigned long long* cells;
    uint32_t* merges;             // [2 * steps]
    unsigned long long* counts;   // [steps]
    uint32_t step, par;
};

__global__ __launch_bounds__(TKT_BLOCK) void tk_k_train_count(TkTrainStep st) {
    const unsigned long long n = st.cells[TKT_LIVE + st.par];
    const uint64_t i = (uint64_t)blockIdx.x * TKT_BLOCK + threadIdx.x;
    if ((uint64_t)blockIdx.x * TKT_BLOCK >= n || st.cells[TKT_DONE]) return;
    const uint32_t *sym = st.sym[st.par], *wid = st.wid[st.par];
    unsigned long long mx = 0;
    if (i + 1 < n) {
        const uint32_t w = wid[i];
        if (w == wid[i + 1]) {
            const uint64_t s = tk_train_pair_slot(st.pair, st.pair_mask, tk_train_pair_key(sym[i], sym[i + 1]), TkTrainCas());
            if (s != ~0ull) {
                const unsigned long long wt = st.weight[w];
                mx = atomicAdd(&st.pair[s].cnt, wt) + wt;  // (the last add to a slot sees its final count)
            }
        }
    }
    mx = tk_wave_max_u64(mx);
    if ((threadIdx.x & 63u) == 0u && mx) atomicMax(&st.cells[TKT_CMAX], mx);
}

__global__ __launch_bounds__(TKT_BLOCK) void tk_k_train_best(TkTrainStep st) {
    const unsigned long long n = st.cells[TKT_LIVE + st.par], cmax = st.cells[TKT_CMAX];
    const uint64_t i = (uint64_t)blockIdx.x * TKT_BLOCK + threadIdx.x;
    if ((uint64_t)blockIdx.x * TKT_BLOCK >= n || st.cells[TKT_DONE] || !cmax) return;
    const uint32_t *sym = st.sym[st.par], *wid = st.wid[st.par];
    uint64_t best = ~0ull;
    if (i + 1 < n && wid[i] == wid[i + 1]) {
        const uint64_t s = tk_train_pair_find(st.pair, st.pair_mask, tk_train_pair_key(sym[i], sym[i + 1]));
        if (s != ~0ull && st.pair[s].cnt == cmax) best = st.pos[st.par][i];
    }
    best = tk_wave_min_u64(best);
    if ((threadIdx.x & 63u) == 0u && best != ~0ull) atomicMin(&st.cells[TKT_BEST], (unsigned long long)best);
}

__global__ __launch_bounds__(TKT_BLOCK) void tk_k_train_pick(TkTrainStep st) {
    const unsigned long long n = st.cells[TKT_LIVE + st.par], cmax = st.cells[TKT_CMAX], best = st.cells[TKT_BEST];
    const uint64_t i = (uint64_t)blockIdx.x * TKT_BLOCK + threadIdx.x;
    if (st.cells[TKT_DONE]) return;
    if (!cmax) {  // no pair left: this step and every later one do nothing
        if (i == 0) st.cells[TKT_DONE] = 1ull + st.step;
        return;
    }
    if (i + 1 < n && st.pos[st.par][i] == best) {  // (positions are unique)
        const uint32_t a = st.sym[st.par][i], b = st.sym[st.par][i + 1];
        st.cells[TKT_WIN] = ((unsigned long long)a << 32) | b;
        st.merges[2u * st.step] = a;
        st.merges[2u * st.step + 1u] = b;
        st.counts[st.step] = cmax;
    }
}

// a == b: the largest break mark of every workgroup
__global__ __launch_bounds__(TKT_BLOCK) void tk_k_train_breaks(TkTrainStep st) {
    __shared__ uint32_t sh[4];
    const unsigned long long n = st.cells[TKT_LIVE + st.par], win = st.cells[TKT_WIN];
    const uint32_t a = (uint32_t)(win >> 32), b = (uint32_t)win;
    const uint64_t i = (uint64_t)blockIdx.x * TKT_BLOCK + threadIdx.x;
    if ((uint64_t)blockIdx.x * TKT_BLOCK >= n || st.cells[TKT_DONE] || a != b) return;
    const uint32_t *sym = st.sym[st.par], *wid = st.wid[st.par];
    uint32_t mark = 0;
    if (i < n) {
        const bool has_prev = i > 0 && wid[i - 1] == wid[i];
        mark = tk_train_break_mark((uint32_t)i, tk_train_continues(has_prev, has_prev ? sym[i - 1] : 0u, sym[i], a));
    }
    mark = tk_wave_max_u32(mark);
    if ((threadIdx.x & 63u) == 0u) sh[threadIdx.x >> 6] = mark;
    __syncthreads();
    if (threadIdx.x == 0) st.blk_mark[blockIdx.x] = max(max(sh[0], sh[1]), max(sh[2], sh[3]));
}

// ... in place -> the largest mark before every workgroup
__global__ __launch_bounds__(1024) void tk_k_train_carry(TkTrainStep st) {
    __shared__ unsigned long long wsum[16];
    const unsigned long long n = st.cells[TKT_LIVE + st.par], win = st.cells[TKT_WIN];
    if (st.cells[TKT_DONE] || (uint32_t)(win >> 32) != (uint32_t)win) return;
    const uint64_t nb = (n + TKT_BLOCK - 1) / TKT_BLOCK;
    (void)tk_scan_blocks<true>(st.blk_mark, nb, 0ull, wsum);
}

__global__ __launch_bounds__(TKT_BLOCK) void tk_k_train_decide(TkTrainStep st) {
    __shared__ uint32_t sh[4];
    const unsigned long long n = st.cells[TKT_LIVE + st.par], win = st.cells[TKT_WIN];
    const uint32_t a = (uint32_t)(win >> 32), b = (uint32_t)win;
    const uint64_t i = (uint64_t)blockIdx.x * TKT_BLOCK + threadIdx.x;
    if ((uint64_t)blockIdx.x * TKT_BLOCK >= n || st.cells[TKT_DONE]) return;
    const uint32_t *sym = st.sym[st.par], *wid = st.wid[st.par];
    bool has_prev = false, has_next = false;
    uint32_t s = 0, s_prev = 0, s_next = 0;
    if (i < n) {
        s = sym[i];
        const uint32_t w = wid[i];
        has_prev = i > 0 && wid[i - 1] == w;
        has_next = i + 1 < n && wid[i + 1] == w;
        if (has_prev) s_prev = sym[i - 1];
        if (has_next) s_next = sym[i + 1];
    }
    uint32_t d = 0;
    if (a == b) {  // (the same in every lane) the run's start: the largest mark at or before this lane, in the workgroup or before it
        uint32_t mark = i < n ? tk_train_break_mark((uint32_t)i, tk_train_continues(has_prev, s_prev, s, a)) : 0u;
        uint32_t tot;
        const uint32_t before = max(st.blk_mark[blockIdx.x], tk_block_exmax32_256(mark, &tot, sh));
        mark = max(before, mark);
        d = mark ? (uint32_t)i - (mark - 1u) : 0u;  // (symbol 0 never continues: there is a mark)
    }
    int dec = TK_TRAIN_KEEP;
    if (i < n) {
        dec = tk_train_decide(a, b, has_prev, s_prev, s, has_next, s_next, d);
        st.dec[i] = (uint8_t)dec;
    }
    const unsigned long long kept = tk_block_sum_256(i < n && dec != TK_TRAIN_RIGHT ? 1u : 0u, sh);
    if (threadIdx.x == 0) st.blk_cnt[blockIdx.x] = kept;
}

// In place: survivors per workgroup -> survivors before it; the next step's live count; cmax and best are reset for it.
__global__ __launch_bounds__(1024) void tk_k_train_offsets(TkTrainStep st) {
    __shared__ unsigned long long wsum[16];
    const unsigned long long n = st.cells[TKT_LIVE + st.par];
    if (st.cells[TKT_DONE]) return;
    const uint64_t nb = (n + TKT_BLOCK - 1) / TKT_BLOCK;
    const unsigned long long carry = tk_scan_blocks<false>(st.blk_cnt, nb, 0ull, wsum);
    if (threadIdx.x == 0) {
        st.cells[TKT_LIVE + (st.par ^ 1u)] = carry;
        st.cells[TKT_CMAX] = 0ull;
        st.cells[TKT_BEST] = ~0ull;
    }
}

__global__ __launch_bounds__(TKT_BLOCK) void tk_k_train_rewrite(TkTrainStep st) {
    __shared__ uint32_t sh[8];
    const unsigned long long n = st.cells[TKT_LIVE + st.par];
    const uint64_t i = (uint64_t)blockIdx.x * TKT_BLOCK + threadIdx.x;
    if ((uint64_t)blockIdx.x * TKT_BLOCK >= n || st.cells[TKT_DONE]) return;
    const int dec = i < n ? (int)st.dec[i] : TK_TRAIN_RIGHT;
    uint32_t tot;
    const uint64_t at = st.blk_cnt[blockIdx.x] + tk_block_exscan_256(dec != TK_TRAIN_RIGHT ? 1u : 0u, &tot, sh);
    if (dec == TK_TRAIN_RIGHT) return;
    const uint32_t o = st.par ^ 1u;
    st.sym[o][at] = dec == TK_TRAIN_LEFT ? 256u + st.step : st.sym[st.par][i];
    st.wid[o][at] = st.wid[st.par][i];
    st.pos[o][at] = st.pos[st.par][i];  // (a merged symbol keeps the position of its left part)
}
