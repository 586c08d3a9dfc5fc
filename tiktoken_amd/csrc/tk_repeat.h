// Repetition statistics per document on the device: for every document of a packed batch and every n-gram size of a list, how many
// n-grams it has, how many distinct ones, how many starts repeat an n-gram of the same document, how many tokens lie inside such a
// repeat, and how often the most frequent n-gram occurs -- the figures of the Gopher repetition rules.  Nothing in the reference does
// this: it replaces a Counter of tuples per document and size on the host.  The rule is stated in include/tiktoken_amd.h; its plain C++,
// the two classes of documents and the sizes of everything in LDS are tk_repeat_rule.h's.  Exact: a hash chooses a slot, the ids decide.
//   tk_k_rp_lds         the LDS class.  One workgroup per TK_RP_TILE positions owns the short documents that start there (two searches
//                       in tok_off, no plan).  A lane per document marks its start and length in LDS; the ids up to the end of the last
//                       owned document are staged, coalesced, and every staged position finds its document from the start bits.  Then
//                       per size: the table is cleared; a lane per start hashes its n-gram from LDS and walks from the hash's slot -- an
//                       empty slot is claimed by a 32-bit compare-and-swap, at a taken one the tag, the document and the k ids of the
//                       claimer are compared, a match is an atomic add on the slot's count --; behind a barrier each lane reads the count
//                       of the slot it ended at (kept in a register), the wavefront's ballots are the dup word and the claim word, counts
//                       above 1 go to the document's maximum by an LDS atomic; a lane per word smears dup words into covered words; a
//                       lane per document pops its ranges and stores its row.  No atomic reaches HBM.
//   tk_k_rp_fill        one thread per document: the rows of the long documents -- n_ngrams, top_count 1, zeros -- and the call's
//                       serial number into the flag word if there is one: the long class's launches of a call without one end at once
//   tk_k_rp_long_clear  the regions of the long documents in the table in HBM to 0: a lane per position clears four slots
//   tk_k_rp_long_insert tiles of TK_RP_LTILE positions, ids and halo in LDS (tk_ng_stage); a wavefront per quarter walks its documents,
//                       its lanes insert the starts of the long ones: 64-bit compare-and-swap, the claimer's ids read from `tokens`
//   tk_k_rp_long_count  the tile's starts and the k - 1 before it are looked up again (lookups are idempotent): dup and claim ballots,
//                       the smear with the left halo word as tk_k_ng_overlap's, per-document popcounts of a quarter summed over four
//                       lanes and added to the rows atomically (a long document never lies inside a quarter: C exceeds it), counts above
//                       1 by atomicMax
// No matrix instructions and no floating point: there is no contraction here.  Everything is queued on the caller's stream.
// Included by tk_api.hip only.
#pragma once
#include "tk_ngram.h"  // tk_ng_stage
#include "tk_repeat_rule.h"

#define TK_RP_WORDS (TK_RP_SPAN / 64u)
static_assert(TK_RP_SPAN % TK_RP_THREADS == 0 && TK_RP_THREADS % 64u == 0, "whole wavefronts, every lane the same number of positions");
static_assert(TK_RP_SPAN < 0xFFFu && TK_RP_LDS_TOKENS < 0xFFFu && TK_RP_SLOTS > TK_RP_SPAN, "12-bit fields of a slot; an empty slot is always there");
static_assert(TK_RP_LDS_TOKENS >= TK_RP_LTILE / TK_NG_SEGS, "a long document never lies inside a quarter of a tile");
static_assert(TK_RP_LDS_TOKENS >= TK_FP_MAX_NGRAM, "a long document has an n-gram of every size");

struct TkRpOut {  // uint64[n_docs, n_sizes] each; any may be null
    unsigned long long *n_ngrams, *n_distinct, *n_dup, *n_cov, *top;
    __host__ __device__ bool any() const { return n_ngrams || n_distinct || n_dup || n_cov || top; }
};

__global__ __launch_bounds__(TK_RP_THREADS) void tk_k_rp_lds(TkRp p, const uint32_t* __restrict__ tokens, const uint64_t* __restrict__ tok_off, TkRpOut o) {
    __shared__ uint32_t ids[TK_RP_SPAN];
    __shared__ uint16_t dstart[TK_RP_SPAN];  // the tile offset of the first token of a staged position's document; TK_RP_NONE
    __shared__ uint16_t dlen[TK_RP_TILE];    // the length of the short document that starts at a tile offset; 0
    __shared__ uint32_t top[TK_RP_TILE];     // ... the highest count above 1 of its n-grams
    __shared__ uint32_t table[TK_RP_SLOTS];
    __shared__ unsigned long long startw[TK_RP_TILE / 64u], dupw[TK_RP_WORDS], clmw[TK_RP_WORDS], covw[TK_RP_WORDS];
    __shared__ uint32_t own_end_s;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint64_t g0 = (uint64_t)blockIdx.x * TK_RP_TILE;
    const uint64_t d0 = tk_rp_first_ge(tok_off, p.n_docs, g0);
    const uint64_t d1 = g0 + TK_RP_TILE > p.n_tokens ? p.n_docs : tk_rp_first_ge(tok_off, p.n_docs, g0 + TK_RP_TILE);
    if (d0 >= d1) return;
    for (uint32_t i = tid; i < TK_RP_TILE; i += TK_RP_THREADS) {
        dlen[i] = 0, top[i] = 0;
        if (i < TK_RP_TILE / 64u) startw[i] = 0;
    }
    if (tid == 0) own_end_s = 0;
    __syncthreads();
    for (uint64_t d = d0 + tid; d < d1; d += TK_RP_THREADS) {
        const uint64_t s = tok_off[d], L = tok_off[d + 1] - s;
        if (!L || s - g0 >= TK_RP_TILE) continue;  // (the second: a tok_off that does not ascend)
        const uint32_t a = (uint32_t)(s - g0);
        atomicOr(&startw[a >> 6], 1ull << (a & 63u));
        if (L <= TK_RP_LDS_TOKENS) dlen[a] = (uint16_t)L, atomicMax(&own_end_s, a + (uint32_t)L);
    }
    __syncthreads();
    const uint32_t own_end = own_end_s < TK_RP_SPAN ? own_end_s : TK_RP_SPAN;
    for (uint32_t i = tid; i < own_end; i += TK_RP_THREADS) {
        ids[i] = g0 + i < p.n_tokens ? tokens[g0 + i] : 0u;
        const uint32_t ds = tk_rp_doc_start(startw, TK_RP_TILE, i);
        dstart[i] = ds != TK_RP_NONE && i < ds + dlen[ds] ? (uint16_t)ds : (uint16_t)TK_RP_NONE;
    }
    __syncthreads();
    for (uint32_t si = 0; si < p.n_sizes; ++si) {
        const uint32_t k = p.k[si];
        for (uint32_t i = tid; i < TK_RP_SLOTS; i += TK_RP_THREADS) table[i] = 0;
        __syncthreads();
        uint32_t slot[TK_RP_PER_LANE], claims = 0;
#pragma unroll
        for (uint32_t j = 0; j < TK_RP_PER_LANE; ++j) {
            const uint32_t i = j * TK_RP_THREADS + tid;
            slot[j] = TK_RP_SLOTS;
            if (i >= own_end) continue;
            const uint32_t ds = dstart[i];
            if (ds == TK_RP_NONE || i + k > ds + dlen[ds]) continue;
            bool claimed;
            slot[j] = tk_rp_lds_insert(
                table, TK_RP_SLOTS, tk_rp_lds_hash(ids, i, k, ds), i,
                [&](uint32_t q) {
                    if (q >= own_end || dstart[q] != ds) return false;
                    for (uint32_t t = 0; t < k; ++t)
                        if (ids[q + t] != ids[i + t]) return false;
                    return true;
                },
                [&](uint32_t at, uint32_t v) { return atomicCAS(&table[at], 0u, v); }, [&](uint32_t at) { atomicAdd(&table[at], TK_RP_ONE); }, &claimed);
            claims |= (uint32_t)claimed << j;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t j = 0; j < TK_RP_PER_LANE; ++j) {
            if (j * TK_RP_THREADS >= own_end) break;  // (the same for every lane)
            const uint32_t i = j * TK_RP_THREADS + tid;
            const uint32_t n = slot[j] < TK_RP_SLOTS ? tk_rp_lds_count(table[slot[j]]) : 0u;
            const unsigned long long bd = __ballot(n >= 2), bc = __ballot((claims >> j) & 1u);
            if (lane == 0) dupw[i >> 6] = bd, clmw[i >> 6] = bc;
            if (n >= 2) atomicMax(&top[dstart[i]], n);
        }
        __syncthreads();
        for (uint32_t w = tid; w * 64 < own_end; w += TK_RP_THREADS) covw[w] = tk_ng_smear(w ? dupw[w - 1] : 0ull, dupw[w], k);
        __syncthreads();
        for (uint64_t d = d0 + tid; d < d1; d += TK_RP_THREADS) {
            const uint64_t s = tok_off[d], L = tok_off[d + 1] - s, at = d * p.n_sizes + si;
            if (L > TK_RP_LDS_TOKENS && L < TK_RP_MAX_DOC) continue;  // (the long class's)
            const bool mine = L && L <= TK_RP_LDS_TOKENS && s - g0 < TK_RP_TILE;
            const uint32_t a = mine ? (uint32_t)(s - g0) : 0u, ng = mine && L >= k ? (uint32_t)L - k + 1 : 0u;
            uint32_t most = 0;
            if (mine) most = top[a], top[a] = 0;
            if (o.n_ngrams) o.n_ngrams[at] = ng;
            if (o.n_distinct) o.n_distinct[at] = tk_rp_range_popc(clmw, a, a + ng);
            if (o.n_dup) o.n_dup[at] = tk_rp_range_popc(dupw, a, a + ng);
            if (o.n_cov) o.n_cov[at] = ng ? tk_rp_range_popc(covw, a, a + (uint32_t)L) : 0u;
            if (o.top) o.top[at] = ng ? (most > 1 ? most : 1u) : 0u;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void tk_k_rp_fill(TkRp p, const uint64_t* __restrict__ tok_off, TkRpOut o, unsigned long long* flag, unsigned long long serial) {
    bool any = false;
    for (uint64_t d = blockIdx.x * 256ull + threadIdx.x; d < p.n_docs; d += (uint64_t)gridDim.x * 256) {
        const uint64_t L = tok_off[d + 1] - tok_off[d];
        if (!tk_rp_is_long(L)) continue;
        any = true;
        for (uint32_t si = 0; si < p.n_sizes; ++si) {
            const uint64_t at = d * p.n_sizes + si;
            if (o.n_ngrams) o.n_ngrams[at] = L - p.k[si] + 1;
            if (o.n_distinct) o.n_distinct[at] = 0;
            if (o.n_dup) o.n_dup[at] = 0;
            if (o.n_cov) o.n_cov[at] = 0;
            if (o.top) o.top[at] = 1;
        }
    }
    if (any) atomicMax(flag, serial);
}

__global__ __launch_bounds__(TK_RP_LTHREADS) void tk_k_rp_long_clear(TkRp p, const uint64_t* __restrict__ tok_off, unsigned long long* table, const unsigned long long* flag,
                                                                     unsigned long long serial) {
    if (*flag != serial) return;
    const uint64_t g0 = (uint64_t)blockIdx.x * TK_RP_LTILE, g1 = g0 + TK_RP_LTILE < p.n_tokens ? g0 + TK_RP_LTILE : p.n_tokens;
    const uint64_t c0 = g0 + (threadIdx.x >> 6) * (TK_RP_LTILE / TK_NG_SEGS), c1 = c0 + TK_RP_LTILE / TK_NG_SEGS < g1 ? c0 + TK_RP_LTILE / TK_NG_SEGS : g1;
    if (c0 >= c1) return;
    tk_fp_walk(tok_off, p.n_docs, c0, c1, [&](uint64_t, uint64_t s, uint64_t e, uint64_t a, uint64_t b) {
        if (!tk_rp_in_table(p, s, e)) return;
        const uint64_t S = tk_rp_region_slots(e - s);
        for (uint64_t g = a + (threadIdx.x & 63u); g < b; g += 64)
            for (uint64_t r = 4 * (g - s); r < 4 * (g - s) + 4 && r < S; ++r) table[4 * (s - p.base) + r] = 0;
    });
}

// Is the n-gram of k ids at ids[at] the one at position q of the document that starts at s?
__device__ __forceinline__ bool tk_rp_long_same(const uint32_t* ids, uint32_t at, const uint32_t* __restrict__ tokens, uint64_t s, uint32_t q, uint32_t k) {
    for (uint32_t t = 0; t < k; ++t)
        if (tokens[s + q + t] != ids[at + t]) return false;
    return true;
}

__global__ __launch_bounds__(TK_RP_LTHREADS) void tk_k_rp_long_insert(TkRp p, uint32_t k, const uint32_t* __restrict__ tokens, const uint64_t* __restrict__ tok_off,
                                                                      unsigned long long* table, const unsigned long long* flag, unsigned long long serial) {
    __shared__ uint32_t ids[TK_NG_TILE + 2 * TK_NG_HALO];
    if (*flag != serial) return;
    const uint64_t g0 = (uint64_t)blockIdx.x * TK_RP_LTILE, g1 = g0 + TK_RP_LTILE < p.n_tokens ? g0 + TK_RP_LTILE : p.n_tokens;
    tk_ng_stage(ids, tokens, g0, p.n_tokens);
    __syncthreads();
    const uint64_t c0 = g0 + (threadIdx.x >> 6) * (TK_RP_LTILE / TK_NG_SEGS), c1 = c0 + TK_RP_LTILE / TK_NG_SEGS < g1 ? c0 + TK_RP_LTILE / TK_NG_SEGS : g1;
    if (c0 >= c1) return;
    tk_fp_walk(tok_off, p.n_docs, c0, c1, [&](uint64_t, uint64_t s, uint64_t e, uint64_t a, uint64_t b) {
        if (!tk_rp_in_table(p, s, e)) return;
        const uint64_t S = tk_rp_region_slots(e - s), v1 = tk_ng_starts_end(s, e, k), vb = v1 < b ? v1 : b;
        for (uint64_t g = a + (threadIdx.x & 63u); g < vb; g += 64) {
            const uint32_t at = (uint32_t)(g - g0) + TK_NG_HALO;
            tk_rp_long_insert(
                table, 4 * (s - p.base), S, tk_ng_key(ids, at, k, TK_RP_SEED), (uint32_t)(g - s), [&](uint32_t q) { return q + k <= e - s && tk_rp_long_same(ids, at, tokens, s, q, k); },
                [&](uint64_t i, uint64_t v) { return (uint64_t)atomicCAS(table + i, 0ull, (unsigned long long)v); }, [&](uint64_t i) { atomicAdd(table + i, (unsigned long long)TK_RP_LONE); });
        }
    });
}

__global__ __launch_bounds__(TK_RP_LTHREADS) void tk_k_rp_long_count(TkRp p, uint32_t si, const uint32_t* __restrict__ tokens, const uint64_t* __restrict__ tok_off,
                                                                     const unsigned long long* __restrict__ table, TkRpOut o, const unsigned long long* flag,
                                                                     unsigned long long serial) {
    __shared__ uint32_t ids[TK_NG_TILE + 2 * TK_NG_HALO];
    __shared__ uint64_t keys[TK_NG_TILE + TK_NG_LEFT], pdoc[TK_NG_TILE + TK_NG_LEFT];  // of the position g: [g - g0 + TK_NG_LEFT]; key 0: no start of a long document
    __shared__ uint64_t hit[TK_NG_WORDS], clm[TK_NG_WORDS], cov[TK_NG_WORDS];
    if (*flag != serial) return;
    const uint32_t k = p.k[si], wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t g0 = (uint64_t)blockIdx.x * TK_RP_LTILE, g1 = g0 + TK_RP_LTILE < p.n_tokens ? g0 + TK_RP_LTILE : p.n_tokens;
    const uint64_t h0 = g0 >= k - 1 ? g0 - (k - 1) : 0;
    tk_ng_stage(ids, tokens, g0, p.n_tokens);
    __syncthreads();
    {
        const uint64_t seg = (g1 - h0 + TK_NG_SEGS - 1) / TK_NG_SEGS, c0 = h0 + wave * seg, c1 = c0 + seg < g1 ? c0 + seg : g1;
        if (c0 < c1)
            tk_fp_walk(tok_off, p.n_docs, c0, c1, [&](uint64_t d, uint64_t s, uint64_t e, uint64_t a, uint64_t b) {
                const uint64_t v1 = tk_rp_in_table(p, s, e) ? tk_ng_starts_end(s, e, k) : s;
                for (uint64_t g = a + lane; g < b; g += 64) {
                    const uint64_t i = g - g0 + TK_NG_LEFT;  // (g >= g0 - 31)
                    keys[i] = g < v1 ? tk_ng_key(ids, (uint32_t)(g + TK_NG_HALO - g0), k, TK_RP_SEED) : 0ull;
                    pdoc[i] = d;
                }
            });
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < TK_NG_TILE + TK_NG_LEFT; i += TK_RP_LTHREADS) {  // (whole wavefronts: 64 divides the bound)
        const uint64_t g = g0 + i - TK_NG_LEFT;                                         // (wraps past g1 before the batch)
        const uint64_t key = g - h0 < g1 - h0 ? keys[i] : 0ull;
        uint32_t n = 0;
        bool first = false;
        if (key) {
            const uint64_t d = pdoc[i], s = tok_off[d], e = tok_off[d + 1];
            const uint32_t at = i - TK_NG_LEFT + TK_NG_HALO;
            const uint64_t v = tk_rp_long_find(table, 4 * (s - p.base), tk_rp_region_slots(e - s), key,
                                               [&](uint32_t q) { return q + k <= e - s && tk_rp_long_same(ids, at, tokens, s, q, k); });
            n = (uint32_t)(v >> 32);
            first = g >= g0 && (uint32_t)v - 1 == (uint32_t)(g - s);
            if (g >= g0 && n >= 2 && o.top) atomicMax(o.top + d * p.n_sizes + si, (unsigned long long)n);
        }
        const unsigned long long bd = __ballot(n >= 2), bc = __ballot(first);
        if (lane == 0) hit[i >> 6] = bd, clm[i >> 6] = bc;
    }
    __syncthreads();
    if (threadIdx.x >= 1 && threadIdx.x < TK_NG_WORDS) cov[threadIdx.x] = tk_ng_smear(hit[threadIdx.x - 1], hit[threadIdx.x], k);
    __syncthreads();
    const uint64_t c0 = g0 + wave * (TK_RP_LTILE / TK_NG_SEGS), c1 = c0 + TK_RP_LTILE / TK_NG_SEGS < g1 ? c0 + TK_RP_LTILE / TK_NG_SEGS : g1;
    if (c0 >= c1) return;
    const uint64_t w0 = c0 + 64ull * lane, w1 = w0 + 64, word = (w0 - g0 + TK_NG_LEFT) / 64;  // this lane's word, as positions (lanes 0 .. 3 have one)
    tk_fp_walk(tok_off, p.n_docs, c0, c1, [&](uint64_t d, uint64_t s, uint64_t e, uint64_t a, uint64_t b) {
        if (!tk_rp_in_table(p, s, e)) return;  // (the same for every lane of the wavefront)
        const uint64_t lo = a > w0 ? a : w0, hi = b < w1 ? b : w1;
        unsigned long long v = 0, nd = 0;
        if (lo < hi) {
            const uint64_t m = tk_ng_bits((uint32_t)(lo - w0), (uint32_t)(hi - w0));
            v = tk_ng_popc(hit[word] & m) | ((unsigned long long)tk_ng_popc(cov[word] & m) << 32), nd = tk_ng_popc(clm[word] & m);
        }
#pragma unroll
        for (int w = 2; w > 0; w >>= 1) v += __shfl_xor(v, w, 64), nd += __shfl_xor(nd, w, 64);
        if (lane != 0) return;
        const uint64_t at = d * p.n_sizes + si;
        if (o.n_dup && (v & 0xFFFFFFFFu)) atomicAdd(o.n_dup + at, v & 0xFFFFFFFFull);
        if (o.n_cov && (v >> 32)) atomicAdd(o.n_cov + at, v >> 32);
        if (o.n_distinct && nd) atomicAdd(o.n_distinct + at, nd);
    });
}
