// Near-duplicate fingerprints on the device: a packed batch (ids, tok_off) -> per document a MinHash signature over its token shingles,
// the LSH band keys of that signature, an exact hash and the shingle count.  Nothing in the reference does this: it replaces the host
// step of the reference's users between "tokenise" and "pack rows" (MinHash over n-grams, banded, plus an exact hash).  The rule is
// stated in include/tiktoken_amd.h; its plain C++ is tk_fingerprint_rule.h's.
//   tk_k_fp_fill    one thread per signature value: sig = TK_FP_NONE; per document: the exact sum and n_shingles = 0
//   tk_k_fp_tile    one workgroup per TK_FP_TILE positions.  The tile's ids and the TK_FP_MAX_NGRAM - 1 behind them go to LDS.  Hash step:
//                   a wavefront per quarter of the tile walks the documents that meet it (tk_last_le, then one by one: the branch at a
//                   document's end is the wavefront's), its lanes hash the shingle starts side by side into LDS and add up the exact
//                   hash's terms; a wavefront sum per document part.  Signature step: the tile in slices of tk_fp_slice_lanes(P) lanes,
//                   a lane per permutation: the lane walks its slice's hashes in document order, the running minimum in a register,
//                   and flushes at a document's end or the slice's.  A document inside the segment or slice: plain stores; one that
//                   reaches beyond: atomicMin, atomicAdd.
//   tk_k_fp_finish  one thread per (document, band): the band key from the finished signature; band 0 closes the exact hash
// Everything is queued on the caller's stream; the host waits for nothing.
// What the CPU simulation (tests/test_fingerprint_sim.py) shares with the kernels: every function of tk_fingerprint_rule.h; the staging,
// the wavefront sum, the atomics and the stores are the kernels' own.
// Included by tk_api.hip only.
#pragma once
#include "tk_fingerprint_rule.h"

#define TK_FP_WAVES (TK_FP_THREADS / 64u)
static_assert(TK_FP_TILE % TK_FP_THREADS == 0 && TK_FP_TILE % TK_FP_WAVES == 0, "a tile is whole segments and whole slices");

struct TkFpOut {  // any may be null
    uint32_t* sig;
    unsigned long long *exact, *n_shingles;
};
struct TkFpSink {
    TkFpOut o;
    uint32_t P;
    // every lane of the wavefront is here
    __device__ __forceinline__ void sums(uint64_t d, bool whole, uint64_t sum, uint64_t n) const {
        unsigned long long v = sum;
#pragma unroll
        for (int w = 32; w > 0; w >>= 1) v += __shfl_xor(v, w, 64);
        if ((threadIdx.x & 63u) != 0) return;
        if (whole) {
            if (o.exact) o.exact[d] = v;
            if (o.n_shingles) o.n_shingles[d] = n;
        } else {
            if (o.exact) atomicAdd(o.exact + d, v);
            if (o.n_shingles && n) atomicAdd(o.n_shingles + d, (unsigned long long)n);
        }
    }
    __device__ __forceinline__ void sig(uint64_t d, bool whole, uint32_t perm, uint32_t v) const {
        if (whole) o.sig[d * P + perm] = v;
        else if (v != TK_FP_NONE) atomicMin(o.sig + d * P + perm, v);
    }
};

__global__ __launch_bounds__(256) void tk_k_fp_fill(TkFp p, TkFpOut o) {
    const uint64_t n_sig = o.sig ? p.n_docs * p.P : 0, n = n_sig > p.n_docs ? n_sig : p.n_docs;
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        if (i < n_sig) o.sig[i] = TK_FP_NONE;
        if (i < p.n_docs) {
            if (o.exact) o.exact[i] = 0;
            if (o.n_shingles) o.n_shingles[i] = 0;
        }
    }
}

__global__ __launch_bounds__(TK_FP_THREADS) void tk_k_fp_tile(TkFp p, const uint32_t* __restrict__ tokens, const uint64_t* __restrict__ tok_off, TkFpOut o) {
    __shared__ uint32_t ids[TK_FP_TILE + TK_FP_MAX_NGRAM];
    __shared__ uint64_t hash[TK_FP_TILE];
    const uint64_t g0 = (uint64_t)blockIdx.x * TK_FP_TILE, g1 = g0 + TK_FP_TILE < p.n_tokens ? g0 + TK_FP_TILE : p.n_tokens;
    for (uint32_t i = threadIdx.x; i < TK_FP_TILE + TK_FP_MAX_NGRAM; i += TK_FP_THREADS) ids[i] = g0 + i < p.n_tokens ? tokens[g0 + i] : 0u;
    __syncthreads();
    const TkFpSink sink{o, p.P};
    {
        const uint32_t seg = TK_FP_TILE / TK_FP_WAVES;
        const uint64_t c0 = g0 + (threadIdx.x >> 6) * seg, c1 = c0 + seg < g1 ? c0 + seg : g1;
        if (c0 < c1) tk_fp_seg_hash(p, tok_off, ids, g0, c0, c1, threadIdx.x & 63u, 64u, hash, sink);  // (a whole wavefront)
    }
    __syncthreads();
    if (!o.sig) return;
    const uint32_t lanes = tk_fp_slice_lanes(p.P), len = TK_FP_TILE / (TK_FP_THREADS / lanes), perm = threadIdx.x % lanes;
    const uint64_t c0 = g0 + (uint64_t)(threadIdx.x / lanes) * len, c1 = c0 + len < g1 ? c0 + len : g1;
    if (perm < p.P && c0 < c1) tk_fp_slice_sig(p, tok_off, hash, g0, c0, c1, perm, sink);
}

__global__ __launch_bounds__(256) void tk_k_fp_finish(TkFp p, const uint64_t* __restrict__ tok_off, const uint32_t* __restrict__ sig, uint64_t* __restrict__ band,
                                                      uint64_t* __restrict__ exact) {
    const uint64_t n = p.n_docs * p.B;
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) tk_fp_finish(p, tok_off, i / p.B, (uint32_t)(i % p.B), sig, band, exact);
}
