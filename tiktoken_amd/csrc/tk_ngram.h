// Token n-gram sets on the device: a set of n-gram keys in HBM that some calls fill (tk_k_ng_add) and others ask (tk_k_ng_overlap) --
// per document of a packed batch the n-gram starts whose key is in the set, the tokens inside such an n-gram, the lowest such start, and
// a mask of those tokens.  Nothing in the reference does this: it replaces the host step of the reference's users between "dedup" and
// "pack rows", the check of every document against the n-grams of held-out text.  The rule is stated in include/tiktoken_amd.h; its
// plain C++ is tk_ngram_rule.h's (T and why, the layout of a tile's bits).
//   tk_k_ng_clear    a new or cleared set: table, filter and counter to 0
//   tk_k_ng_add      one workgroup per TK_NG_TILE positions.  The tile's ids and the TK_NG_HALO around them go to LDS, coalesced; a
//                    wavefront per quarter walks the documents that meet it (tk_fp_walk), its lanes hash the n-gram starts side by side
//                    and insert the key: linear probing from the key's low bits, an empty slot claimed by a 64-bit compare-and-swap, the
//                    device counter raised by the lane's claims, the key's bit of the filter set (atomicOr where it is not set yet).
//   tk_k_ng_fill     one thread per document: n_hit = n_covered = 0, first_hit = TK_NG_NONE, n_ngrams from tok_off alone
//   tk_k_ng_overlap  one workgroup per tile.  Key step: the positions [g0 - (k - 1), g1), the left halo recomputed, in four wavefront
//                    shares: keys to LDS, 0 where no n-gram starts.  Probe step: a lane per position, word after word: the key's bit of
//                    the filter first -- S / 2 bytes, a sixteenth of the table, meant to stay in L2 / MALL; a miss costs one 4-byte load --,
//                    the slot walk only where it is set; the wavefront's ballot is the hit word.  Smear step: a lane per word,
//                    tk_ng_smear with the carry from the word before.  Then the mask, a byte per position, and the count step: a
//                    wavefront per quarter walks its documents, a lane per word pops the hit and covered bits of the document's part,
//                    four lanes are summed; a document inside the quarter: plain stores; one that reaches beyond: atomicAdd, atomicMin.
// Everything is queued on the caller's stream; the host waits for nothing.
// What the CPU simulation (tests/test_ngram_sim.py) shares with the kernels: every function of tk_ngram_rule.h; the staging, the
// compare-and-swap, the ballot, the four-lane sum and the flushes are the kernels' own.
// Included by tk_api.hip only.
#pragma once
#include "tk_ngram_rule.h"

#define TK_NG_WORDS (TK_NG_TILE / 64u + 1u)               // a tile's bit words, the left halo's first
#define TK_NG_SEG (TK_NG_TILE / TK_NG_SEGS)               // positions of a segment of the count step
#define TK_NG_SEG_WORDS (TK_NG_SEG / 64u)                 // its words: the lanes that count
static_assert(TK_NG_THREADS == 64u * TK_NG_SEGS && TK_NG_SEG % 64u == 0, "a wavefront per segment, a segment of whole words");
static_assert(TK_NG_SEG_WORDS == 4u, "TkNgSink::counts sums four lanes");
static_assert(TK_NG_HALO >= TK_FP_MAX_NGRAM && TK_NG_LEFT >= TK_FP_MAX_NGRAM && (TK_NG_TILE + TK_NG_LEFT) % 64u == 0, "the halo holds an n-gram; the probe step goes by words");

struct TkNgOut {  // any may be null
    unsigned long long *n_hit, *n_covered, *n_ngrams, *first_hit;
    uint8_t* mask;
    __host__ __device__ bool per_doc() const { return n_hit || n_covered || n_ngrams || first_hit; }
};
struct TkNgSink {
    TkNgOut o;
    // every lane of the wavefront is here; lanes 0 .. 3 hold the segment's words
    __device__ __forceinline__ void counts(uint64_t d, bool whole, uint64_t nh, uint64_t nc, uint64_t first) const {
        unsigned long long v = nh | (nc << 32), f = first;  // (both counts are at most 64)
#pragma unroll
        for (int w = 2; w > 0; w >>= 1) {
            v += __shfl_xor(v, w, 64);
            const unsigned long long g = __shfl_xor(f, w, 64);
            f = g < f ? g : f;
        }
        if ((threadIdx.x & 63u) != 0) return;
        nh = v & 0xFFFFFFFFu, nc = v >> 32;
        if (whole) {
            if (o.n_hit) o.n_hit[d] = nh;
            if (o.n_covered) o.n_covered[d] = nc;
            if (o.first_hit) o.first_hit[d] = f;
        } else {
            if (o.n_hit && nh) atomicAdd(o.n_hit + d, (unsigned long long)nh);
            if (o.n_covered && nc) atomicAdd(o.n_covered + d, (unsigned long long)nc);
            if (o.first_hit && f != TK_NG_NONE) atomicMin(o.first_hit + d, f);
        }
    }
};

// ids[i] = tokens[g0 - TK_NG_HALO + i], 0 outside the batch
__device__ __forceinline__ void tk_ng_stage(uint32_t* ids, const uint32_t* __restrict__ tokens, uint64_t g0, uint64_t n) {
    for (uint32_t i = threadIdx.x; i < TK_NG_TILE + 2 * TK_NG_HALO; i += TK_NG_THREADS) {
        const uint64_t g = g0 + i - TK_NG_HALO;  // (wraps past n before the batch)
        ids[i] = g < n ? tokens[g] : 0u;
    }
}

__global__ __launch_bounds__(256) void tk_k_ng_clear(unsigned long long* table, uint64_t S, uint32_t* filter, uint64_t n_words, unsigned long long* count) {
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < S; i += (uint64_t)gridDim.x * 256) {
        table[i] = 0;
        if (i < n_words) filter[i] = 0;
        if (i == 0) *count = 0;
    }
}

__global__ __launch_bounds__(TK_NG_THREADS) void tk_k_ng_add(TkNg p, const uint32_t* __restrict__ tokens, const uint64_t* __restrict__ tok_off, unsigned long long* table,
                                                             uint32_t* filter, unsigned long long* count) {
    __shared__ uint32_t ids[TK_NG_TILE + 2 * TK_NG_HALO];
    const uint64_t g0 = (uint64_t)blockIdx.x * TK_NG_TILE, g1 = g0 + TK_NG_TILE < p.n_tokens ? g0 + TK_NG_TILE : p.n_tokens;
    tk_ng_stage(ids, tokens, g0, p.n_tokens);
    __syncthreads();
    const uint64_t c0 = g0 + (threadIdx.x >> 6) * TK_NG_SEG, c1 = c0 + TK_NG_SEG < g1 ? c0 + TK_NG_SEG : g1;
    if (c0 >= c1) return;
    uint32_t claimed = 0;
    tk_ng_seg_keys(p, tok_off, ids, g0, c0, c1, threadIdx.x & 63u, 64u, [&](uint64_t, uint64_t key) {
        if (!key) return;
        claimed += tk_ng_insert(table, p.S, key, [&](uint64_t i, uint64_t k) { return (uint64_t)atomicCAS(table + i, 0ull, (unsigned long long)k); });
        const uint64_t b = tk_ng_filter_bit(key, p.S);
        const uint32_t bit = 1u << (b & 31);
        if (!(filter[b >> 5] & bit)) atomicOr(filter + (b >> 5), bit);
    });
    if (claimed) atomicAdd(count, (unsigned long long)claimed);
}

__global__ __launch_bounds__(256) void tk_k_ng_fill(TkNg p, const uint64_t* __restrict__ tok_off, TkNgOut o) {
    for (uint64_t d = blockIdx.x * 256ull + threadIdx.x; d < p.n_docs; d += (uint64_t)gridDim.x * 256) {
        if (o.n_hit) o.n_hit[d] = 0;
        if (o.n_covered) o.n_covered[d] = 0;
        if (o.first_hit) o.first_hit[d] = TK_NG_NONE;
        if (o.n_ngrams) {
            const uint64_t s = tok_off[d], e = tok_off[d + 1];
            o.n_ngrams[d] = tk_ng_starts_end(s, e, p.k) - s;
        }
    }
}

__global__ __launch_bounds__(TK_NG_THREADS) void tk_k_ng_overlap(TkNg p, const uint32_t* __restrict__ tokens, const uint64_t* __restrict__ tok_off,
                                                                 const unsigned long long* __restrict__ table, const uint32_t* __restrict__ filter, TkNgOut o) {
    __shared__ uint32_t ids[TK_NG_TILE + 2 * TK_NG_HALO];
    __shared__ uint64_t keys[TK_NG_TILE + TK_NG_LEFT];  // keys[g - g0 + TK_NG_LEFT]
    __shared__ uint64_t hit[TK_NG_WORDS], cov[TK_NG_WORDS];
    const uint64_t g0 = (uint64_t)blockIdx.x * TK_NG_TILE, g1 = g0 + TK_NG_TILE < p.n_tokens ? g0 + TK_NG_TILE : p.n_tokens;
    const uint64_t h0 = g0 >= p.k - 1 ? g0 - (p.k - 1) : 0;  // the first start that can cover a token of the tile
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    tk_ng_stage(ids, tokens, g0, p.n_tokens);
    __syncthreads();
    {
        const uint64_t seg = (g1 - h0 + TK_NG_SEGS - 1) / TK_NG_SEGS, c0 = h0 + wave * seg, c1 = c0 + seg < g1 ? c0 + seg : g1;
        if (c0 < c1) tk_ng_seg_keys(p, tok_off, ids, g0, c0, c1, lane, 64u, [&](uint64_t g, uint64_t key) { keys[g - g0 + TK_NG_LEFT] = key; });
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < TK_NG_TILE + TK_NG_LEFT; i += TK_NG_THREADS) {  // (whole wavefronts: 64 divides the bound)
        const uint64_t g = g0 + i - TK_NG_LEFT;                                        // (wraps past g1 before the batch)
        const uint64_t key = g - h0 < g1 - h0 ? keys[i] : 0ull;
        const bool in = key && tk_ng_filter_has(filter, p.S, key) && tk_ng_probe(table, p.S, key);
        const unsigned long long b = __ballot(in);
        if (lane == 0) hit[i >> 6] = b;
    }
    __syncthreads();
    if (threadIdx.x >= 1 && threadIdx.x < TK_NG_WORDS) cov[threadIdx.x] = tk_ng_smear(hit[threadIdx.x - 1], hit[threadIdx.x], p.k);
    __syncthreads();
    if (o.mask)
        for (uint32_t i = threadIdx.x; i < (uint32_t)(g1 - g0); i += TK_NG_THREADS) o.mask[g0 + i] = (uint8_t)((cov[(i + TK_NG_LEFT) >> 6] >> (i & 63u)) & 1u);
    if (!o.per_doc()) return;
    const uint64_t c0 = g0 + wave * TK_NG_SEG, c1 = c0 + TK_NG_SEG < g1 ? c0 + TK_NG_SEG : g1;
    const TkNgSink sink{o};
    if (c0 < c1) tk_ng_seg_count(p, tok_off, hit, cov, g0, c0, c1, lane, sink);
}
