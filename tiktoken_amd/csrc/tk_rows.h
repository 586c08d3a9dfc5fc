// Training rows on the device: a packed batch (ids, tok_off) -> the stream [bos] document [eos] ... cut into rows of seq_len, and for every
// position the document it belongs to, its position inside the segment, and the segment boundaries (cu_seqlens, and row_seg: where the
// segments of every row begin in cu_seqlens).  Nothing in the reference does this: it replaces the host loop of the reference's users, the
// data-preparation script that appends a separator to every encoded document, concatenates and reshapes.  The rule is tk_rows_rule.h's.
// Built like the span passes of tk_offsets.h (TK_DEC_BLOCK positions per workgroup, eight consecutive positions per lane):
//   tk_k_rows_mark    one thread per tok_off entry: the entry is checked (ascending from 0 to n_tokens; the first offending document goes
//                     into a report word) and the start of every document that owns a position -> a bitmap over the stream positions
//   tk_k_rows_count   per workgroup: segment starts = marked bits | row starts, a coincidence counted once
//   tk_k_rows_scan    one workgroup: exclusive sums of those counts (tk_scan_blocks), the number of segments, the closing cu_seqlens entry
//   tk_k_rows_write   ids (uint32 or uint16), doc, pos, the cu_seqlens entries at their scanned indices, row_seg at row starts
// How a lane learns its document: it SEARCHES tok_off once, for its first position, and walks along the documents from there (a position
// at or beyond the current document's end moves on to the next one; behind a run of empty documents with k == 0 the walk searches once
// more instead of stepping through the run).  The other way -- the last document start before every lane travelling through max-scans, as
// in tk_k_span_write -- gives the START of the lane's document but not its INDEX, which `doc` needs and which with k == 0 is not the number
// of marks before the lane either (empty documents own no position): the search would still be there, so the carried maximum is not.  The
// search is short: thread 0 of a workgroup searches all of tok_off for the workgroup's first and last position, the lanes search between
// the two results (a workgroup of 2048 positions rarely holds more than a few documents).
// tok_off is the caller's: tk_k_rows_mark never indexes with an entry it has not compared with n_tokens, and tk_k_rows_write does nothing
// when the report word names a document, so no kernel reads or writes out of bounds whatever tok_off holds.
// Included by tk_api.hip only.
#pragma once
#include "tk_decode.h"
#include "tk_rows_rule.h"
#include "tk_scan.h"

// the words the passes report in (unsigned long long each): the lowest tk_rows_bad_key (TK_BAD_OFF; starts as all ones = none), the segments
enum { TK_ROWS_NSEGS = TK_BAD_OFF + 1, TK_ROWS_WORDS };

__global__ __launch_bounds__(256) void tk_k_rows_mark(const uint64_t* __restrict__ tok_off, TkRows r, uint32_t* __restrict__ bm, unsigned long long* __restrict__ words) {
    for (uint64_t d = blockIdx.x * 256ull + threadIdx.x; d <= r.n_docs; d += (uint64_t)gridDim.x * 256) {
        uint64_t a, b;
        tk_rows_off_check(tok_off, d, r.n_docs, r.n_tokens, &a, &b, words + TK_BAD_OFF);
        const uint64_t p = tk_rows_mark_at(a, b, d, r);
        if (p != ~0ull) atomicOr(&bm[p >> 5], 1u << (p & 31u));
    }
}

// marks: the bitmap as bytes -- a lane's eight positions are one of them
__global__ __launch_bounds__(256) void tk_k_rows_count(const uint8_t* __restrict__ marks, TkRows r, unsigned long long* __restrict__ cnt) {
    __shared__ uint32_t sh[4];
    const uint64_t i0 = (uint64_t)blockIdx.x * TK_DEC_BLOCK + (uint64_t)threadIdx.x * 8;
    uint32_t bits = 0;
    if (i0 < r.M) bits = tk_rows_seg_bits(marks[i0 >> 3], tk_rows_row_bits((uint32_t)i0 % r.seq_len, r.seq_len), tk_rows_valid_bits(i0, r.M));
    const unsigned long long tot = tk_block_sum_256((uint32_t)__popc(bits), sh);
    if (threadIdx.x == 0) cnt[blockIdx.x] = tot;
}

// In place: cnt -> the segment starts before every workgroup.  cu_seqlens closes with M; row_seg[R] is written here when no position R * L
// exists to write it (M == R * L: always without drop_last, and with it when there is no tail).
__global__ __launch_bounds__(1024) void tk_k_rows_scan(unsigned long long* __restrict__ cnt, uint64_t nb, TkRows r, uint32_t* __restrict__ cu,
                                                       uint32_t* __restrict__ row_seg, unsigned long long* __restrict__ words) {
    __shared__ unsigned long long wsum[16];
    const unsigned long long carry = tk_scan_blocks<false>(cnt, nb, 0ull, wsum);
    if (threadIdx.x == 0) {
        words[TK_ROWS_NSEGS] = carry;
        cu[carry] = (uint32_t)r.M;
        if (r.R * r.seq_len == r.M) row_seg[r.R] = (uint32_t)carry;
    }
}

// The caller's token array as a lane of a write pass reads it (tk_rows_lane, tk_pad_lane): eight ids as two 16-byte loads where their
// address is a multiple of 16
struct TkTokens {
    const uint32_t* __restrict__ p;
    __device__ __forceinline__ uint32_t one(uint64_t i) const { return p[i]; }
    __device__ __forceinline__ bool eight(uint64_t i, uint32_t out[8]) const {
        if ((uintptr_t)(p + i) & 15u) return false;
        const uint4 a = *(const uint4*)(p + i), b = *(const uint4*)(p + i + 4);
        out[0] = a.x, out[1] = a.y, out[2] = a.z, out[3] = a.w, out[4] = b.x, out[5] = b.y, out[6] = b.z, out[7] = b.w;
        return true;
    }
};
// ... and how its eight ids leave, as uint32 or uint16 (the host has checked that every id of the vocabulary fits; ids of no vocabulary are
// cut, as a uint16 store cuts them): a whole lane as 16-byte stores (ids_out 16-byte aligned, i0 a multiple of 8), the last lane's one by
// one, each behind the caller's test that the position exists
template <bool IDS16>
__device__ __forceinline__ void tk_ids_store8(void* __restrict__ ids_out, uint64_t i0, const uint32_t id[8]) {
    if (IDS16) {
        *(uint4*)((uint16_t*)ids_out + i0) = make_uint4((id[0] & 0xFFFFu) | (id[1] << 16), (id[2] & 0xFFFFu) | (id[3] << 16), (id[4] & 0xFFFFu) | (id[5] << 16),
                                                        (id[6] & 0xFFFFu) | (id[7] << 16));
    } else {
        *(uint4*)((uint32_t*)ids_out + i0) = make_uint4(id[0], id[1], id[2], id[3]);
        *(uint4*)((uint32_t*)ids_out + i0 + 4) = make_uint4(id[4], id[5], id[6], id[7]);
    }
}
template <bool IDS16>
__device__ __forceinline__ void tk_ids_store1(void* __restrict__ ids_out, uint64_t i, uint32_t id) {
    if (IDS16) ((uint16_t*)ids_out)[i] = (uint16_t)id;
    else ((uint32_t*)ids_out)[i] = id;
}

// ids_out, doc_out, pos_out: 16-byte aligned (the library's own buffers): a lane's eight positions leave as 16-byte stores.  tokens is the
// caller's: its eight ids arrive as two 16-byte loads where the stream is the token array (k == 0) and the pointer allows it.  Otherwise
// (bos / eos shift the ids by a different amount in every document, so no aligned word holds a lane's ids) they arrive as eight 4-byte
// loads per lane, as in the span passes: for one j the lanes of a wavefront are 32 bytes apart, so an instruction uses 4 bytes of every
// 32 and the eight of them together read every cache line of the wavefront's 2 KiB once from HBM and seven times from the L1.  What a lane
// computes is tk_rows_lane (tk_rows_rule.h), the same statements the CPU simulation runs.
template <bool IDS16>
__global__ __launch_bounds__(256) void tk_k_rows_write(const uint32_t* __restrict__ tokens, const uint64_t* __restrict__ tok_off, TkRows r,
                                                       const unsigned long long* __restrict__ seg_base, const unsigned long long* __restrict__ words,
                                                       void* __restrict__ ids_out, uint32_t* __restrict__ doc_out, uint32_t* __restrict__ pos_out,
                                                       uint32_t* __restrict__ cu, uint32_t* __restrict__ row_seg) {
    __shared__ uint32_t sh[8];
    __shared__ uint64_t sh_doc[2];
    if (words[TK_BAD_OFF] != ~0ull) return;  // (the same in every thread) tok_off does not describe the batch: nothing is indexed with it
    const uint64_t b0 = (uint64_t)blockIdx.x * TK_DEC_BLOCK, i0 = b0 + (uint64_t)threadIdx.x * 8;
    if (threadIdx.x == 0) tk_rows_block_docs(r, tok_off, b0, TK_DEC_BLOCK, &sh_doc[0], &sh_doc[1]);
    __syncthreads();
    uint32_t seg = 0, rows = 0;
    if (i0 < r.M) {
        uint32_t id[8], dc[8], ps[8];
        tk_rows_lane(r, TkTokens{tokens}, tok_off, sh_doc[0], sh_doc[1], i0, id, dc, ps, &seg, &rows);
        if (i0 + 8 <= r.M) {
            tk_ids_store8<IDS16>(ids_out, i0, id);
            *(uint4*)(doc_out + i0) = make_uint4(dc[0], dc[1], dc[2], dc[3]);
            *(uint4*)(doc_out + i0 + 4) = make_uint4(dc[4], dc[5], dc[6], dc[7]);
            *(uint4*)(pos_out + i0) = make_uint4(ps[0], ps[1], ps[2], ps[3]);
            *(uint4*)(pos_out + i0 + 4) = make_uint4(ps[4], ps[5], ps[6], ps[7]);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (i0 + j < r.M) {
                    tk_ids_store1<IDS16>(ids_out, i0 + j, id[j]);
                    doc_out[i0 + j] = dc[j];
                    pos_out[i0 + j] = ps[j];
                }
        }
    }
    uint32_t tot;
    uint64_t at = seg_base[blockIdx.x] + tk_block_exscan_256((uint32_t)__popc(seg), &tot, sh);
    while (seg) {
        const uint32_t j = (uint32_t)__ffs((int)seg) - 1u;
        seg &= seg - 1u;
        cu[at] = (uint32_t)(i0 + j);
        if ((rows >> j) & 1u) row_seg[(uint32_t)(i0 + j) / r.seq_len] = (uint32_t)at;
        ++at;
    }
}
