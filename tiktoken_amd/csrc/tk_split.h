// Text chunks on the device: a packed batch (ids, tok_off), its text (utf8, doc_off) and the token spans -> every document cut into chunks
// of at most max_tokens tokens, at the best separator the window [min_tokens, max_tokens] offers, never inside a char.  Nothing in the
// reference does this: it replaces the host loop of the reference's users (a text splitter that counts tokens with the encoder and walks
// every document looking for the last paragraph break, line break or sentence end that fits).  The rule is stated in
// include/tiktoken_amd.h; its plain C++ is tk_split_rule.h's.
//   tk_k_split_check   one thread per tok_off entry: ascending from 0 to n_tokens, or the first offending document into a report word
//                      (nothing is indexed with tok_off before the host has read that word)
//   tk_k_split_class   one thread per token: the class of the boundary before it from up to 16 text bytes on either side; a wavefront's
//                      ballots are one word each of the L + 1 planes (levels, legal): (L + 1) * T / 8 bytes
//   tk_k_split_walk    one wavefront per block of K positions: the documents that start in the block are walked from their start and
//                      mark `cut`; the document that runs into the block is walked from a guessed start and marks `spec`.  A step's
//                      window words of all planes are fetched by the lanes at once: a load, a ballot and a shuffle per step.
//   tk_k_split_stitch  one wavefront per document of more than one block: the true chain walks in a block until it stands on a `spec` bit
//                      (the join) or leaves the block; join_at[block] = the join
//   tk_k_split_count   one thread per plane word: cut |= spec from the block's join on; set bits per TK_DEC_BLOCK positions
//   tk_k_split_scan    one workgroup: exclusive sums of those counts (tk_scan_blocks), C into a report word
//   (the host waits for C and sizes the outputs; it has waited for the check's word before the span passes, which wait themselves)
//   tk_k_split_write   one thread per plane word: the records of its starts (the step from the start once more, tk_last_le for the
//                      document, the spans for bytes and chars)
//   tk_k_split_docs    one thread per document: doc_chunk
// A step's next start is a function of the start alone, so two chains that stand on one position are one chain from there on: that is why
// the marks of a speculative walk may be taken over from the join on, and why the result does not depend on K or on the guess.
// What the CPU simulation (tests/test_split_sim.py) shares with the kernels: every function of tk_split_rule.h named below; the ballots,
// the shuffles, the atomics, the scan and the stores are the kernels' own.
// Included by tk_api.hip only.
#pragma once
#include "tk_decode.h"  // TK_DEC_BLOCK
#include "tk_scan.h"
#include "tk_split_rule.h"

// the words the passes report in (unsigned long long each): the lowest tk_rows_bad_key (TK_BAD_OFF; starts as all ones = none), C, the counters
enum { TK_SPLIT_NCHUNKS = TK_BAD_OFF + 1, TK_SPLIT_STAT0, TK_SPLIT_WORDS = TK_SPLIT_STAT0 + TK_SPLIT_STATS };
#define TK_SPLIT_CB_WORDS (TK_DEC_BLOCK / 64)  // plane words of a count block

struct TkPlanes {  // the class planes, one behind the other
    const unsigned long long* p;
    uint64_t W;
    __device__ __forceinline__ uint64_t word(uint32_t pl, uint64_t w) const { return p[pl * W + w]; }
};
struct TkBits {  // one plane, read
    const unsigned long long* p;
    __device__ __forceinline__ bool bit(uint64_t g) const { return (p[g >> 6] >> (g & 63u)) & 1u; }
};
struct TkMark {  // one plane, written: every lane of the wavefront calls with the same g, lane 0 sets the bit
    unsigned long long* p;
    __device__ __forceinline__ void operator()(uint64_t g) const {
        if ((threadIdx.x & 63u) == 0) atomicOr(p + (g >> 6), 1ull << (g & 63u));
    }
};
struct TkStatAdd {
    unsigned long long* words;
    __device__ __forceinline__ void operator()(int which, uint64_t v) const {
        if ((threadIdx.x & 63u) == 0 && v) atomicAdd(words + TK_SPLIT_STAT0 + which, (unsigned long long)v);
    }
};
// the wavefront as tk_split_rule.h sees it
struct TkWave64 {
    unsigned long long mine = 0;
    template <class F>
    __device__ __forceinline__ uint64_t gather(F&& f) {
        mine = f(threadIdx.x & 63u);
        return __ballot(mine != 0);
    }
    __device__ __forceinline__ uint64_t word(uint32_t lane) const { return __shfl(mine, (int)lane, 64); }
};

__global__ __launch_bounds__(256) void tk_k_split_check(const uint64_t* __restrict__ tok_off, uint64_t n_docs, uint64_t n_tokens, unsigned long long* __restrict__ words) {
    for (uint64_t d = blockIdx.x * 256ull + threadIdx.x; d <= n_docs; d += (uint64_t)gridDim.x * 256) {
        uint64_t a, b;
        tk_rows_off_check(tok_off, d, n_docs, n_tokens, &a, &b, words + TK_BAD_OFF);
    }
}

// planes: (L + 1) * W words; the grid covers the W * 64 positions of a plane, so every word is written
__global__ __launch_bounds__(256) void tk_k_split_class(TkSplit p, const uint8_t* __restrict__ text, const uint64_t* __restrict__ doc_off, const uint64_t* __restrict__ tok_off,
                                                        const uint32_t* __restrict__ byte_start, unsigned long long* __restrict__ planes) {
    __shared__ uint64_t sh_doc[2];
    const uint64_t b0 = blockIdx.x * 256ull, g = b0 + threadIdx.x;
    if (threadIdx.x == 0 && b0 < p.n_tokens) tk_split_block_docs(p, tok_off, b0, 256, &sh_doc[0], &sh_doc[1]);
    __syncthreads();
    uint32_t bits = 0;
    if (g < p.n_tokens) bits = tk_split_class_at(p, text, doc_off, tok_off, byte_start, sh_doc[0], sh_doc[1], g);
    for (uint32_t pl = 0; pl <= p.L; ++pl) {  // (every lane of the wavefront is here)
        const unsigned long long m = __ballot((bits >> pl) & 1u);
        if ((threadIdx.x & 63u) == 0 && (g >> 6) < p.W) planes[pl * p.W + (g >> 6)] = m;
    }
}

__global__ __launch_bounds__(256) void tk_k_split_walk(TkSplit p, const unsigned long long* __restrict__ planes, const uint64_t* __restrict__ tok_off, uint64_t n_blocks,
                                                       unsigned long long* cut, unsigned long long* spec, uint32_t* __restrict__ exit_at, unsigned long long* words) {
    const uint64_t b = blockIdx.x * 4ull + (threadIdx.x >> 6);
    if (b >= n_blocks) return;  // (a whole wavefront)
    const TkPlanes P{planes, p.W};
    TkWave64 wave;
    TkMark mark_cut{cut}, mark_spec{spec};
    TkStatAdd add{words};
    tk_split_block(p, P, wave, tok_off, b, mark_cut, mark_spec, exit_at, add);
}

// exit_at: written by the wavefront's lanes alike (one value); join_at likewise
__global__ __launch_bounds__(256) void tk_k_split_stitch(TkSplit p, const unsigned long long* __restrict__ planes, const uint64_t* __restrict__ tok_off,
                                                         unsigned long long* cut, const unsigned long long* __restrict__ spec, const uint32_t* __restrict__ exit_at,
                                                         uint32_t* __restrict__ join_at, unsigned long long* words) {
    const TkPlanes P{planes, p.W};
    TkWave64 wave;
    TkMark mark_cut{cut};
    TkStatAdd add{words};
    for (uint64_t d = blockIdx.x * 4ull + (threadIdx.x >> 6); d < p.n_docs; d += (uint64_t)gridDim.x * 4)
        tk_split_stitch(p, P, wave, tok_off, TkBits{spec}, d, mark_cut, exit_at, join_at, add);
}

// one thread per plane word; 32 of them are a count block: cnt[count block] = its starts
__global__ __launch_bounds__(256) void tk_k_split_count(TkSplit p, unsigned long long* __restrict__ cut, const unsigned long long* __restrict__ spec,
                                                        const uint32_t* __restrict__ join_at, uint32_t* __restrict__ cnt) {
    const uint64_t w = blockIdx.x * 256ull + threadIdx.x;
    uint32_t c = 0;
    if (w < p.W) {
        const uint64_t v = tk_split_fold(p, cut[w], spec[w], w, join_at);
        cut[w] = v;
        c = (uint32_t)__popcll(v);
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);  // (the sum of each half of the wavefront)
    static_assert(TK_SPLIT_CB_WORDS == 32, "a count block is half a wavefront's words");
    if ((threadIdx.x & 31u) == 0 && w < p.W) cnt[w / TK_SPLIT_CB_WORDS] = c;
}

// In place: cnt -> the starts before every count block; C into the report word
__global__ __launch_bounds__(1024) void tk_k_split_scan(uint32_t* __restrict__ cnt, uint64_t nb, unsigned long long* __restrict__ words) {
    __shared__ unsigned long long wsum[16];
    const unsigned long long carry = tk_scan_blocks<false>(cnt, nb, 0ull, wsum);
    if (threadIdx.x == 0) words[TK_SPLIT_NCHUNKS] = carry;
}

__global__ __launch_bounds__(256) void tk_k_split_write(TkSplit p, const unsigned long long* __restrict__ planes, const unsigned long long* __restrict__ cut,
                                                        const uint32_t* __restrict__ cnt, const uint64_t* __restrict__ tok_off, const uint32_t* __restrict__ byte_start,
                                                        const uint32_t* __restrict__ char_start, const uint64_t* __restrict__ byte_off, const uint64_t* __restrict__ char_off,
                                                        TkSplitOut out) {
    const uint64_t w = blockIdx.x * 256ull + threadIdx.x;
    if (w >= p.W) return;
    uint64_t v = cut[w];
    if (!v) return;
    const TkPlanes P{planes, p.W};
    uint64_t i = tk_split_rank(cut, cnt, TK_SPLIT_CB_WORDS, w * 64);
    for (; v; v &= v - 1, ++i) tk_split_record(p, P, tok_off, byte_start, char_start, byte_off, char_off, w * 64 + (uint64_t)__builtin_ctzll(v), i, out);
}

__global__ __launch_bounds__(256) void tk_k_split_docs(TkSplit p, const unsigned long long* __restrict__ cut, const uint32_t* __restrict__ cnt,
                                                       const uint64_t* __restrict__ tok_off, uint32_t* __restrict__ doc_chunk) {
    for (uint64_t d = blockIdx.x * 256ull + threadIdx.x; d <= p.n_docs; d += (uint64_t)gridDim.x * 256)
        doc_chunk[d] = (uint32_t)tk_split_rank(cut, cnt, TK_SPLIT_CB_WORDS, tok_off[d]);
}
