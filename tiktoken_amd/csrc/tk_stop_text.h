// Stop strings on the device: packed text in HBM -> every document cut at the first place where one of up to sixteen stop strings lies,
// again as packed text, with the string that hit per document (the rule: include/tiktoken_amd.h).  The geometry is the UTF-8 repair's
// (tk_utf8_repair.h): sixteen bytes per lane, 256 lanes, TK_STOPS_BLOCK bytes per workgroup.
//   tk_k_u8r_check    (the repair's) the offsets ascend from 0 to n: the first document that offends
//   tk_k_stops_find   a workgroup stages its bytes, the TK_STOPS_TAIL behind them and the stop set in LDS; a lane tests its sixteen start
//                     positions against the first-byte mask, compares the survivors (tk_stops_lane) and leaves the least key
//                     (position in the document) * 16 + (index in the list) in its document's word: atomicMin, a minimum and not a
//                     first-come claim, for the workgroups of a document run in any order
//   tk_k_stops_rows   a thread per document: kept length and hit from the word; per workgroup the scan of the kept lengths, its sum, the hits
//   tk_k_stops_scan   one workgroup: the sums -> the workgroups' bases (tk_scan_blocks), the total
//   -- the host waits here: a refused call has written into scratch only; no hit anywhere: the input IS the output, no cut pass --
//   tk_k_stops_docs   text_off and hit of every document, into the buffers the caller gets
//   tk_k_stops_cut    a lane per sixteen output bytes (tk_stops_cut_lane): the source misaligned against the destination, one aligned
//                     16-byte store in the interior; every output byte stored exactly once
//   tk_k_stops_ntok   (id matrices) a thread per row: the row's kept tokens whose first byte lies before the end of the kept text
// The find pass runs before the offsets are known to be good: it indexes the offsets with indices only, compares nothing that ends behind
// byte n, and the document it writes to comes from a search, so it lies in [0, n_docs).  Included by tk_api.hip only.
#pragma once
#include "tk_scan.h"
#include "tk_stop_text_rule.h"
#include "tk_utf8_repair.h"  // tk_k_u8r_check

// the words the passes report in (unsigned long long each): the first document whose offset offends (all ones: none; where tk_k_u8r_check
// leaves it), the bytes kept, the documents with a hit
enum { TK_STOPS_BAD_DOC = 0, TK_STOPS_OUT, TK_STOPS_N_HIT, TK_STOPS_WORDS };
static_assert(TK_STOPS_BAD_DOC == TK_U8R_BAD_DOC, "tk_k_u8r_check reports in word 0");
#define TK_STOPS_ROWS_BLOCK 1024  // documents per workgroup of tk_k_stops_rows

struct TkStopsTile {  // a workgroup's staged bytes: position p of the text at tile[p - base]
    const uint8_t* tile;
    uint64_t base;
    __device__ __forceinline__ uint32_t operator()(uint64_t p) const { return tile[p - base]; }
};

// bytes: 16-byte aligned, readable 16 bytes past n.  d_set: the TkStopSet in HBM.  word: n_docs words, all ones.  n_docs >= 1, n >= 1.
__global__ __launch_bounds__(256) void tk_k_stops_find(const uint8_t* __restrict__ bytes, uint64_t n, const uint64_t* __restrict__ off, uint64_t n_docs,
                                                       const uint32_t* __restrict__ d_set, unsigned long long* __restrict__ word) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[TK_STOPS_BLOCK + TK_STOPS_TAIL];
    __shared__ __attribute__((aligned(16))) TkStopSet set;
    const uint64_t base = (uint64_t)blockIdx.x * TK_STOPS_BLOCK;
    // 260 units of 16 bytes; a unit at position a is readable as a whole where a <= n (the text is readable to n + 16)
    for (uint32_t u = threadIdx.x; u < (TK_STOPS_BLOCK + TK_STOPS_TAIL) / 16; u += 256) {
        const uint64_t a = base + 16ull * u;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (a <= n) v = *(const uint4*)(bytes + a);
        *(uint4*)(tile + 16u * u) = v;
    }
    for (uint32_t i = threadIdx.x; i < TK_STOPS_SET_WORDS; i += 256) ((uint32_t*)&set)[i] = d_set[i];
    __syncthreads();
    const TkStopsTile t{tile, base};
    tk_stops_lane(t, set, off, n_docs, n, base + 16ull * threadIdx.x, [&](uint64_t d, unsigned long long key) { atomicMin(word + d, key); });
}

// kept_rel[d]: the kept bytes of the documents before d inside d's workgroup; hit_s[d]; bsum[workgroup]: its kept bytes
__global__ __launch_bounds__(TK_STOPS_ROWS_BLOCK) void tk_k_stops_rows(const uint64_t* __restrict__ off, uint64_t n_docs, const unsigned long long* __restrict__ word,
                                                                       const uint32_t* __restrict__ d_set, unsigned long long* __restrict__ kept_rel,
                                                                       uint32_t* __restrict__ hit_s, unsigned long long* __restrict__ bsum,
                                                                       unsigned long long* __restrict__ words) {
    __shared__ unsigned long long wsum[16];
    __shared__ TkStopSet set;
    for (uint32_t i = threadIdx.x; i < TK_STOPS_SET_WORDS; i += TK_STOPS_ROWS_BLOCK) ((uint32_t*)&set)[i] = d_set[i];
    __syncthreads();
    const uint64_t d = (uint64_t)blockIdx.x * TK_STOPS_ROWS_BLOCK + threadIdx.x;
    unsigned long long kept = 0;
    uint32_t hit = TK_STOPS_NO_HIT;
    if (d < n_docs) kept = tk_stops_kept(word[d], off[d + 1] - off[d], set, &hit);
    unsigned long long tot, hits;
    const unsigned long long ex = tk_scan1024<false>(kept, &tot, wsum);
    (void)tk_scan1024<false>(hit != TK_STOPS_NO_HIT ? 1ull : 0ull, &hits, wsum);
    if (d < n_docs) {
        kept_rel[d] = ex;
        hit_s[d] = hit;
    }
    if (threadIdx.x == 0) {
        bsum[blockIdx.x] = tot;
        if (hits) atomicAdd(words + TK_STOPS_N_HIT, hits);
    }
}

__global__ __launch_bounds__(1024) void tk_k_stops_scan(unsigned long long* __restrict__ bsum, uint64_t nb, unsigned long long* __restrict__ words) {
    __shared__ unsigned long long wsum[16];
    const unsigned long long total = tk_scan_blocks<false>(bsum, nb, 0ull, wsum);
    if (threadIdx.x == 0) words[TK_STOPS_OUT] = total;
}

// text_off: n_docs + 1 (null where no document has a hit: the caller's own offsets are the result); hit: n_docs
__global__ __launch_bounds__(256) void tk_k_stops_docs(uint64_t n_docs, const unsigned long long* __restrict__ base, const unsigned long long* __restrict__ kept_rel,
                                                       const uint32_t* __restrict__ hit_s, const unsigned long long* __restrict__ words, uint64_t* __restrict__ text_off,
                                                       uint32_t* __restrict__ hit) {
    for (uint64_t d = blockIdx.x * 256ull + threadIdx.x; d <= n_docs; d += (uint64_t)gridDim.x * 256) {
        if (d < n_docs) hit[d] = hit_s[d];
        if (text_off) text_off[d] = d < n_docs ? base[d / TK_STOPS_ROWS_BLOCK] + kept_rel[d] : words[TK_STOPS_OUT];
    }
}

struct TkStopsSrc {
    const uint8_t* __restrict__ bytes;
    __device__ __forceinline__ void load16(uint64_t pos, uint64_t* lo, uint64_t* hi) const {
        const uint4 v = *(const uint4*)(bytes + pos);
        *lo = (uint64_t)v.x | ((uint64_t)v.y << 32);
        *hi = (uint64_t)v.z | ((uint64_t)v.w << 32);
    }
    __device__ __forceinline__ uint8_t byte(uint64_t pos) const { return bytes[pos]; }
};
struct TkStopsStores {
    uint8_t* __restrict__ out;
    __device__ __forceinline__ void store16(uint64_t q, uint64_t lo, uint64_t hi) const {
        *(uint4*)(out + q) = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
    }
    __device__ __forceinline__ void byte(uint64_t q, uint8_t v) const { out[q] = v; }
};
// text: 16-byte aligned, n_text + 16 bytes.  off and text_off: checked and made by the passes before.  n_docs >= 1.
__global__ __launch_bounds__(256) void tk_k_stops_cut(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off, const uint64_t* __restrict__ text_off,
                                                      uint64_t n_docs, uint64_t n_text, uint8_t* __restrict__ text) {
    const TkStopsSrc src{bytes};
    TkStopsStores st{text};
    for (uint64_t lane = blockIdx.x * 256ull + threadIdx.x; lane * 16 < n_text; lane += (uint64_t)gridDim.x * 256)
        tk_stops_cut_lane(src, off, text_off, n_docs, n_text, lane * 16, st);
}

// byte_off, text_off: the rows' offsets before and behind the cut; tok_byte: the byte position of every kept token in the decoded bytes
__global__ __launch_bounds__(256) void tk_k_stops_ntok(const uint64_t* __restrict__ tok_off, const uint64_t* __restrict__ byte_off, const uint64_t* __restrict__ text_off,
                                                       const unsigned long long* __restrict__ tok_byte, uint64_t n_rows, uint32_t* __restrict__ n_tok) {
    for (uint64_t r = blockIdx.x * 256ull + threadIdx.x; r < n_rows; r += (uint64_t)gridDim.x * 256)
        n_tok[r] = tk_stops_ntok(tok_byte, tok_off[r], tok_off[r + 1], byte_off[r] + (text_off[r + 1] - text_off[r]));
}
