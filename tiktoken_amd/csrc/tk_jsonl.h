// JSON Lines on the device: a buffer of lines {"text": "...", ...}\n -> the unescaped text of one field per line, packed as the encode
// entries take it (text, doc_off), with the status of every line.  Nothing in the reference does this: it replaces the host loop of the
// reference's users, `for line in f: json.loads(line)["text"]`, in front of every batch encode.  The rule and how it is computed are stated
// in tk_jsonl_rule.h, whose plain C++ the kernels below drive, a wavefront per tile of TK_JSONL_TILE bytes:
//   tk_k_jsonl_sum        the summary of every tile, under both hypotheses of its entry state
//   tk_k_jsonl_carry      one workgroup: exclusive sums and maxima over the summaries (tk_scan_blocks), the entry state of every tile, the
//                         number of lines into a report word (the host waits for it and sizes the per-line arrays)
//   tk_k_jsonl_select     per line: flags, low structural bytes, the last matching key's value, the line's offset; the escaped plane
//   tk_k_jsonl_count      the unescaped length of the selected values per tile; where a value starts and ends in its tiles' counts; bad
//                         escapes and ill-formed UTF-8 into the line's flags
//   tk_k_jsonl_tile_scan  one workgroup: the tiles' counts -> exclusive sums
//   tk_k_jsonl_lines      per line: status and length; per block of 256 lines: bytes and documents; the first line RAISE refuses
//   tk_k_jsonl_line_scan  one workgroup: the blocks' exclusive sums, the totals into report words (the host waits, refuses or sizes the result)
//   tk_k_jsonl_docs       per line: its document, doc_off and line of the document
//   tk_k_jsonl_write      the unescaped bytes, by byte stores of the lanes that own them
// Stores are vector stores of plain C++ throughout.  Included by tk_api.hip only.
#pragma once
#include "tk_jsonl_rule.h"
#include "tk_scan.h"

struct TkJsonlWave {  // the wavefront as tk_jsonl_rule.h sees it
    uint32_t lane, r = 0, p = 0;
    __device__ __forceinline__ explicit TkJsonlWave() : lane(threadIdx.x & 63u) {}
    template <class F>
    __device__ __forceinline__ uint64_t ballot(F&& f) { return __ballot(f(lane)); }
    template <class F>
    __device__ __forceinline__ void each(F&& f) { f(lane); }
    template <class F>
    __device__ __forceinline__ void once(F&& f) { if (lane == 0) f(); }
    template <class F>
    __device__ __forceinline__ uint32_t scan(F&& f) {
        const uint32_t v = f(lane), inc = tk_wave_scan_u32(v, (int)lane);
        p = inc - v;
        return __shfl(inc, 63, 64);
    }
    __device__ __forceinline__ uint32_t& reg(uint32_t) { return r; }
    __device__ __forceinline__ uint32_t pre(uint32_t) const { return p; }
};

__global__ __launch_bounds__(256) void tk_k_jsonl_sum(TkJsonl j, TkJsonlTiles T) {
    const uint32_t t = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (t >= j.n_tiles) return;  // (a whole wavefront)
    TkJsonlWave w;
    tk_jsonl_tile_sum(j, w, t, T);
}

// exclusive scan in place, sums or maxima; the total in every thread
template <bool MAX, class V>
__device__ __forceinline__ unsigned long long tk_jsonl_scan(V* a, uint32_t n, unsigned long long* wsum) {
    const unsigned long long tot = tk_scan_blocks<MAX>(a, (uint64_t)n, 0ull, wsum);
    __syncthreads();
    return tot;
}
__global__ __launch_bounds__(1024) void tk_k_jsonl_carry(TkJsonl j, TkJsonlTiles T, TkJsonlCarry* __restrict__ entry, unsigned long long* __restrict__ words) {
    __shared__ unsigned long long wsum[16];
    const uint32_t nt = j.n_tiles;
    tk_jsonl_scan<true>(T.nonbs, nt, wsum);
    tk_jsonl_scan<true>(T.nl, nt, wsum);
    tk_jsonl_scan<true>(T.nonws, nt, wsum);
    const unsigned long long lines = tk_jsonl_scan<false>(T.nnl, nt, wsum);
    for (uint32_t t = threadIdx.x; t < nt; t += 1024u) tk_jsonl_carry_q(j, T, t);
    __syncthreads();
    tk_jsonl_scan<false>(T.nq, nt, wsum);
    tk_jsonl_scan<true>(T.lastq, nt, wsum);
    for (uint32_t t = threadIdx.x; t < nt; t += 1024u) tk_jsonl_carry_d(j, T, t);
    __syncthreads();
    tk_jsonl_scan<false>((uint32_t*)T.d, nt, wsum);
    for (uint32_t t = threadIdx.x; t < nt; t += 1024u) entry[t] = tk_jsonl_carry_entry(j, T, t);
    if (threadIdx.x == 0) words[TK_JSONL_W_LINES] = lines;
}

struct TkJsonlSelectOut {
    TkJsonlLines L;
    uint64_t* line_off_;
    unsigned long long* ep;
    __device__ __forceinline__ void flag(uint32_t line, uint32_t bits) const { atomicOr(L.flags + line, bits); }
    __device__ __forceinline__ void low(uint32_t line) const { atomicAdd(L.low + line, 1u); }
    __device__ __forceinline__ void vmax(uint32_t line, uint64_t v) const { atomicMax((unsigned long long*)L.vmax + line, (unsigned long long)v); }
    __device__ __forceinline__ void line_off(uint32_t line, uint32_t pos) const { line_off_[line] = pos; }
    __device__ __forceinline__ void eplane(uint32_t word, uint64_t m) const { ep[word] = m; }
};
__global__ __launch_bounds__(256) void tk_k_jsonl_select(TkJsonl j, const TkJsonlCarry* __restrict__ entry, TkJsonlLines L, uint64_t* __restrict__ line_off,
                                                         unsigned long long* __restrict__ ep) {
    const uint32_t t = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (t >= j.n_tiles) return;
    TkJsonlWave w;
    TkJsonlSelectOut out{L, line_off, ep};
    tk_jsonl_tile_select(j, w, t, entry[t], out);
}

struct TkJsonlCountSink {
    TkJsonlLines L;
    uint32_t* cnt;
    __device__ __forceinline__ void bad(uint32_t line, uint32_t bits) const { atomicOr(L.flags + line, bits); }
    __device__ __forceinline__ void vstart(uint32_t line, uint32_t rel) const { L.vs_rel[line] = rel; }
    __device__ __forceinline__ void vend(uint32_t line, uint32_t pos, uint32_t rel) const { L.ve_pos[line] = pos, L.ve_rel[line] = rel; }
    __device__ __forceinline__ void bytes(uint32_t, uint32_t, uint32_t, uint32_t) const {}
    __device__ __forceinline__ void done(uint32_t t, uint32_t total) const { cnt[t] = total; }
};
__global__ __launch_bounds__(256) void tk_k_jsonl_count(TkJsonl j, const TkJsonlCarry* __restrict__ entry, const unsigned long long* __restrict__ ep, TkJsonlLines L,
                                                        uint32_t* __restrict__ cnt) {
    const uint32_t t = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (t >= j.n_tiles) return;
    TkJsonlWave w;
    TkJsonlCountSink sink{L, cnt};
    tk_jsonl_tile_text(j, w, t, entry[t], (const uint64_t*)ep, L.vmax, sink);
}
__global__ __launch_bounds__(1024) void tk_k_jsonl_tile_scan(uint32_t* __restrict__ cnt, uint32_t n_tiles) {
    __shared__ unsigned long long wsum[16];
    tk_scan_blocks<false>(cnt, (uint64_t)n_tiles, 0ull, wsum);
}

// blk_len / blk_docs: per block of TK_JSONL_LB lines
__global__ __launch_bounds__(256) void tk_k_jsonl_lines(TkJsonl j, TkJsonlLines L, const uint32_t* __restrict__ G, uint32_t n_lines, uint32_t* __restrict__ blk_len,
                                                        uint32_t* __restrict__ blk_docs, unsigned long long* __restrict__ words) {
    __shared__ uint32_t sh[8];
    const uint32_t line = blockIdx.x * TK_JSONL_LB + threadIdx.x;
    uint32_t len = 0, keep = 0;
    if (line < n_lines) {
        tk_jsonl_line(j, L, G, line);
        const uint32_t st = L.status[line];
        keep = tk_jsonl_keeps(j.mode, st) ? 1u : 0u;
        len = L.len[line];
        if (j.mode == TK_JSONL_M_RAISE && st != TK_JSONL_ST_OK && st != TK_JSONL_ST_BLANK) atomicMin(words + TK_JSONL_W_BADLINE, (unsigned long long)line);
    }
    const unsigned long long a = tk_block_sum_256(len, sh);
    __syncthreads();
    const unsigned long long b = tk_block_sum_256(keep, sh);
    if (threadIdx.x == 0) blk_len[blockIdx.x] = (uint32_t)a, blk_docs[blockIdx.x] = (uint32_t)b;
}
__global__ __launch_bounds__(1024) void tk_k_jsonl_line_scan(uint32_t* __restrict__ blk_len, uint32_t* __restrict__ blk_docs, uint32_t nb, unsigned long long* __restrict__ words) {
    __shared__ unsigned long long wsum[16];
    const unsigned long long text = tk_scan_blocks<false>(blk_len, (uint64_t)nb, 0ull, wsum);
    __syncthreads();
    const unsigned long long docs = tk_scan_blocks<false>(blk_docs, (uint64_t)nb, 0ull, wsum);
    if (threadIdx.x == 0) words[TK_JSONL_W_TEXT] = text, words[TK_JSONL_W_DOCS] = docs;
}
__global__ __launch_bounds__(256) void tk_k_jsonl_docs(TkJsonl j, TkJsonlLines L, uint32_t n_lines, const uint32_t* __restrict__ blk_len, const uint32_t* __restrict__ blk_docs,
                                                       uint64_t n_docs, uint64_t n_text, uint64_t* __restrict__ doc_off, uint64_t* __restrict__ doc_line) {
    __shared__ uint32_t sh[8];
    const uint32_t line = blockIdx.x * TK_JSONL_LB + threadIdx.x;
    uint32_t len = 0, keep = 0;
    if (line < n_lines) {
        keep = tk_jsonl_keeps(j.mode, L.status[line]) ? 1u : 0u;
        len = L.len[line];
    }
    uint32_t tot;
    const uint32_t at = blk_len[blockIdx.x] + tk_block_exscan_256(len, &tot, sh);
    const uint32_t d = blk_docs[blockIdx.x] + tk_block_exscan_256(keep, &tot, sh);
    if (line < n_lines) {
        L.doc[line] = keep ? d : 0xFFFFFFFFu;
        if (keep) doc_off[d] = at, doc_line[d] = line;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) doc_off[n_docs] = n_text;
}

struct TkJsonlWriteSink {
    TkJsonlLines L;
    const uint32_t* G;
    const uint64_t* doc_off;
    uint8_t* text;
    uint32_t tile, gt;
    __device__ __forceinline__ void bad(uint32_t, uint32_t) const {}
    __device__ __forceinline__ void vstart(uint32_t, uint32_t) const {}
    __device__ __forceinline__ void vend(uint32_t, uint32_t, uint32_t) const {}
    __device__ __forceinline__ void bytes(uint32_t line, uint32_t rel, uint32_t v, uint32_t n) const {
        if (L.status[line] != TK_JSONL_ST_OK || L.doc[line] == 0xFFFFFFFFu) return;
        const uint32_t vpos = (uint32_t)(L.vmax[line] >> 1) - 1u;
        uint8_t* o = text + doc_off[L.doc[line]] + ((gt + rel) - (G[vpos / tile] + L.vs_rel[line]));
        for (uint32_t i = 0; i < n; ++i) o[i] = (uint8_t)(v >> (8u * i));
    }
    __device__ __forceinline__ void done(uint32_t, uint32_t) const {}
};
__global__ __launch_bounds__(256) void tk_k_jsonl_write(TkJsonl j, const TkJsonlCarry* __restrict__ entry, const unsigned long long* __restrict__ ep, TkJsonlLines L,
                                                        const uint32_t* __restrict__ G, const uint64_t* __restrict__ doc_off, uint8_t* __restrict__ text) {
    const uint32_t t = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (t >= j.n_tiles) return;
    TkJsonlWave w;
    TkJsonlWriteSink sink{L, G, doc_off, text, j.tile, G[t]};
    tk_jsonl_tile_text(j, w, t, entry[t], (const uint64_t*)ep, L.vmax, sink);
}
