// Decoding id matrices on the device: what a generation, evaluation or reranking loop hands back -- ids [R, W] in HBM, uint32, int32 or
// int64, a strided slice of a wider matrix as often as not, rows that end at the first stop id with padding or garbage behind it, special
// tokens mixed in -- -> the compact (tokens, tok_off) the decode passes of tk_decode.h take, with n_kept and stop_col per row.  Nothing in
// the reference does this: it replaces the host loop of the reference's users (the matrix copied to the host, trimmed row by row in Python,
// the lists handed to decode_batch; elsewhere `batch_decode(ids, skip_special_tokens=True)`).  The rule is stated in
// include/tiktoken_amd.h; its plain C++ is tk_decode_rows_rule.h's.  A post-pass in front of the decode kernels, which run as they are:
//   tk_k_drows_stop    a workgroup per (row, tile of TK_DEC_BLOCK columns), eight columns per lane: thread 0 of a row's tile 0 checks the
//                      row's begin and end (the first offending row goes into a report word), every lane looks for the first stop id
//                      among its columns in [begin, end), and the tile's first goes into the row's word by atomicMin: a minimum, not a
//                      first-come claim, so the order of the tiles does not matter
//   tk_k_drows_count   behind it: the kept ids of every tile, and the first kept id without a decode entry as the minimum over the 64-bit
//                      row-major position
//   tk_k_drows_scan    one workgroup: exclusive sums of those counts in place (tk_scan_blocks), K into a report word
//   (the host reads the report words, refuses or sizes the outputs; the passes above work in scratch arrays only, so a refused call leaves
//   the previous result whole)
//   tk_k_drows_rows    one thread per row: tok_off, n_kept, stop_col
//   tk_k_drows_write   the kept ids of a lane's eight columns, compacted: the lane's count, a wavefront prefix and a workgroup prefix in
//                      LDS (tk_block_exscan_256) on top of the tile's scanned offset give the place of the lane's first kept id.  No global
//                      counter hands out places: the order of the ids is the rule's, not the scheduler's.
// Tiles over (row, columns), not a wavefront per row: 4096 rows of 64 columns and 4 rows of 131072 columns both fill the device.
// The matrix is the caller's and not padded: a lane reads its eight columns as 16-byte loads only where all eight are columns of the row
// and their address allows it, one by one otherwise, and only columns of the row's [begin, end) at that -- begin and end are compared with W
// before anything is indexed with them, so no kernel reads out of bounds whatever they hold.
// What the CPU simulation (tests/test_decode_rows_sim.py) shares with the kernels: tk_drows_tile, tk_drows_range, tk_drows_stop_lane,
// tk_drows_stop_min, tk_drows_stop_col, tk_drows_count_lane, tk_drows_keep_lane, tk_drows_store_lane, tk_drows_row_entry; the wave
// reduction, the scans and the stores are the kernels' own.
// Included by tk_api.hip only.
#pragma once
#include "tk_decode.h"
#include "tk_decode_rows_rule.h"
#include "tk_scan.h"

// The caller's matrix as a lane reads it.  MODE: 0 uint32, 1 int32, 2 int64; an element widens to 64 bits (tk_decode_rows_rule.h).
template <int MODE>
struct TkIdMatrix {
    const void* __restrict__ p;
    __device__ __forceinline__ uint64_t one(uint64_t i) const {
        if (MODE == 2) return (uint64_t)((const int64_t*)p)[i];
        if (MODE == 1) return (uint64_t)(int64_t)((const int32_t*)p)[i];
        return ((const uint32_t*)p)[i];
    }
    static __device__ __forceinline__ uint64_t wide(uint32_t x) { return MODE == 1 ? (uint64_t)(int64_t)(int32_t)x : (uint64_t)x; }
    // elements [i, i + 8) as 16-byte loads -- two of them, four for int64 -- where their address is a multiple of 16
    __device__ __forceinline__ bool eight(uint64_t i, uint64_t out[8]) const {
        if (MODE == 2) {
            const uint64_t* q = (const uint64_t*)p + i;
            if ((uintptr_t)q & 15u) return false;
            const ulonglong2 a = *(const ulonglong2*)q, b = *(const ulonglong2*)(q + 2), c = *(const ulonglong2*)(q + 4), d = *(const ulonglong2*)(q + 6);
            out[0] = a.x, out[1] = a.y, out[2] = b.x, out[3] = b.y, out[4] = c.x, out[5] = c.y, out[6] = d.x, out[7] = d.y;
            return true;
        }
        const uint32_t* q = (const uint32_t*)p + i;
        if ((uintptr_t)q & 15u) return false;
        const uint4 a = *(const uint4*)q, b = *(const uint4*)(q + 4);
        out[0] = wide(a.x), out[1] = wide(a.y), out[2] = wide(a.z), out[3] = wide(a.w), out[4] = wide(b.x), out[5] = wide(b.y), out[6] = wide(b.z), out[7] = wide(b.w);
        return true;
    }
};
// The stores of the write pass: straight to the token array
struct TkDrowsOut {
    uint32_t* __restrict__ tokens;
    __device__ __forceinline__ void put(uint64_t i, uint32_t id) const { tokens[i] = id; }
};

// found: a word per row, all ones before the pass.  The grid may be smaller than the tiles: a workgroup then goes on with tile t + gridDim.x.
template <int MODE>
__global__ __launch_bounds__(256) void tk_k_drows_stop(const void* __restrict__ ids, const uint32_t* __restrict__ begin, const uint32_t* __restrict__ end, TkDrows p,
                                                       uint64_t n_tiles, uint32_t* __restrict__ found, unsigned long long* __restrict__ words) {
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        uint64_t r, col0;
        uint32_t b, e;
        tk_drows_tile(p, t, TK_DEC_BLOCK, &r, &col0);
        const bool ok = tk_drows_range(p, begin, begin != nullptr, end, end != nullptr, r, &b, &e);
        if (!ok && col0 == 0 && threadIdx.x == 0) tk_report_min(words + TK_DROWS_BAD_ROW, r);
        const uint64_t c0 = col0 + threadIdx.x * 8u;
        uint32_t first = 0xFFFFFFFFu;
        if (p.n_stop && c0 < p.W) first = tk_drows_stop_lane(p, TkIdMatrix<MODE>{ids}, r, c0, b, e);
        first = tk_wave_min_u32(first);  // (every lane is here: the loop's count is the workgroup's)
        if ((threadIdx.x & 63) == 0 && first != 0xFFFFFFFFu) tk_drows_stop_min(found + r, first);
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void tk_k_drows_count(const void* __restrict__ ids, const uint32_t* __restrict__ begin, const uint32_t* __restrict__ end, TkDrows p,
                                                        uint64_t n_tiles, const uint32_t* __restrict__ found, const uint2* __restrict__ dec, uint32_t n_ids,
                                                        unsigned long long* __restrict__ cnt, unsigned long long* __restrict__ words) {
    __shared__ uint32_t sh[4];
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        uint64_t r, col0;
        uint32_t b, e, live_end;
        tk_drows_tile(p, t, TK_DEC_BLOCK, &r, &col0);
        tk_drows_range(p, begin, begin != nullptr, end, end != nullptr, r, &b, &e);
        tk_drows_stop_col(p, found[r], e, &live_end);
        if (!tk_drows_tile_live(col0, TK_DEC_BLOCK, b, live_end)) {  // (the same in every thread)
            if (threadIdx.x == 0) cnt[t] = 0ull;
            continue;
        }
        const uint64_t c0 = col0 + threadIdx.x * 8u;
        uint32_t n = 0;
        if (c0 < p.W) n = tk_drows_count_lane(p, TkIdMatrix<MODE>{ids}, dec, n_ids, r, c0, b, live_end, words);
        const unsigned long long tot = tk_block_sum_256(n, sh);
        if (threadIdx.x == 0) cnt[t] = tot;
        __syncthreads();  // (sh is the next tile's)
    }
}

// In place: cnt -> the kept ids before every tile; K into its report word
__global__ __launch_bounds__(1024) void tk_k_drows_scan(unsigned long long* __restrict__ cnt, uint64_t n_tiles, unsigned long long* __restrict__ words) {
    __shared__ unsigned long long wsum[16];
    const unsigned long long carry = tk_scan_blocks<false>(cnt, n_tiles, 0ull, wsum);
    if (threadIdx.x == 0) words[TK_DROWS_K] = carry;
}

__global__ __launch_bounds__(256) void tk_k_drows_rows(const uint32_t* __restrict__ begin, const uint32_t* __restrict__ end, TkDrows p,
                                                       const unsigned long long* __restrict__ tile_off, const uint32_t* __restrict__ found, uint64_t K,
                                                       uint64_t* __restrict__ tok_off, uint32_t* __restrict__ n_kept, uint32_t* __restrict__ stop_col) {
    for (uint64_t r = blockIdx.x * 256ull + threadIdx.x; r <= p.R; r += (uint64_t)gridDim.x * 256)
        tk_drows_row_entry(p, tile_off, found, begin, begin != nullptr, end, end != nullptr, K, r, tok_off, n_kept, stop_col);
}

// tile_off: the scanned counts.  tokens: the library's own buffer, K ids.
template <int MODE>
__global__ __launch_bounds__(256) void tk_k_drows_write(const void* __restrict__ ids, const uint32_t* __restrict__ begin, const uint32_t* __restrict__ end, TkDrows p,
                                                        uint64_t n_tiles, const uint32_t* __restrict__ found, const uint2* __restrict__ dec, uint32_t n_ids,
                                                        const unsigned long long* __restrict__ tile_off, uint32_t* __restrict__ tokens) {
    __shared__ uint32_t sh[8];
    const TkDrowsOut out{tokens};
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        uint64_t r, col0, v[8];
        uint32_t b, e, live_end, bad, keep = 0, tot;
        tk_drows_tile(p, t, TK_DEC_BLOCK, &r, &col0);
        tk_drows_range(p, begin, begin != nullptr, end, end != nullptr, r, &b, &e);
        tk_drows_stop_col(p, found[r], e, &live_end);
        if (!tk_drows_tile_live(col0, TK_DEC_BLOCK, b, live_end)) continue;  // (the same in every thread)
        const uint64_t c0 = col0 + threadIdx.x * 8u;
        if (c0 < p.W) keep = tk_drows_keep_lane(p, TkIdMatrix<MODE>{ids}, dec, n_ids, r, c0, b, live_end, v, &bad);
        const uint32_t before = tk_block_exscan_256(tk_drows_popc8(keep), &tot, sh);  // (ends behind a barrier: sh is the next tile's)
        if (keep) tk_drows_store_lane(keep, v, tile_off[t] + before, out);
    }
}
