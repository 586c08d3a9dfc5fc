// Padded model inputs on the device: a packed batch (ids, tok_off) -> one row per document, truncated to max_len and padded left or right,
// or -- TK_PAD_WINDOWS -- as many overlapping rows as a long document needs; ids and an attention mask as [R, W], and per row its length,
// its document and its first body token.  Nothing in the reference does this: it replaces the host loop of the reference's users
// (`enc.encode(t)[:n]` plus list padding, a token-window text splitter).  The rule is stated in include/tiktoken_amd.h; its plain C++ is
// tk_padded_rule.h's.  Built like the row passes of tk_rows.h:
//   tk_k_pad_count   one thread per tok_off entry: the entry is checked (ascending from 0 to n_tokens; the first offending document goes
//                    into a report word), the rows the document owns -> doc_row[d], the longest row of all -> a report word
//   tk_k_pad_scan    one workgroup: exclusive sums of those counts in place (tk_scan_blocks), R into doc_row[n_docs] and a report word
//   (the host reads the report words, settles W, refuses or sizes the outputs; the two passes above work in a scratch array, and doc_row
//   is copied into the result's buffer only once the call is accepted, so a refused call leaves the previous result whole)
//   tk_k_pad_rows    one thread per row: len, row_doc, row_tok (also when W == 0)
//   tk_k_pad_write   ids (uint32 or uint16) and mask over the R * W positions, TK_DEC_BLOCK per workgroup, eight consecutive ones per lane
// How a lane learns its row's document: every document owns a row, so doc_row ascends strictly and one binary search finds the document of
// the lane's first row; from there the lane steps from row to row (with W < 8 through up to eight of them), and a row beyond the document's
// last is the next document's first.  Thread 0 of a workgroup searches all of doc_row for the workgroup's first and last row, the lanes
// search between the two results.
// tok_off is the caller's: tk_k_pad_count indexes nothing with it, and the host launches the other passes only when no entry was reported,
// so no kernel reads or writes out of bounds whatever tok_off holds.
// What the CPU simulation (tests/test_padded_sim.py) shares with the kernels: tk_pad_count_entry (the body of tk_k_pad_count's loop),
// tk_pad_row_entry (tk_k_pad_rows'), tk_pad_block_docs and tk_pad_lane (tk_k_pad_write); the wave reduction, the atomicMax, the scan and
// the stores are the kernels' own.
// Included by tk_api.hip only.
#pragma once
#include "tk_decode.h"
#include "tk_padded_rule.h"
#include "tk_rows.h"  // TkTokens, tk_ids_store8, tk_ids_store1
#include "tk_scan.h"

// the words the passes report in (unsigned long long each): the lowest tk_rows_bad_key (TK_BAD_OFF; starts as all ones = none), R, the longest len
enum { TK_PAD_NROWS = TK_BAD_OFF + 1, TK_PAD_LONGEST, TK_PAD_WORDS };

__global__ __launch_bounds__(256) void tk_k_pad_count(const uint64_t* __restrict__ tok_off, TkPad p, uint32_t* __restrict__ doc_row, unsigned long long* __restrict__ words) {
    uint32_t longest = 0;
    for (uint64_t d = blockIdx.x * 256ull + threadIdx.x; d <= p.n_docs; d += (uint64_t)gridDim.x * 256) {
        const uint32_t l = tk_pad_count_entry(p, tok_off, d, doc_row, words);
        longest = l > longest ? l : longest;
    }
    longest = tk_wave_max_u32(longest);  // (behind the loop: every lane is here)
    if ((threadIdx.x & 63) == 0 && longest) atomicMax(words + TK_PAD_LONGEST, (unsigned long long)longest);
}

// In place: doc_row -> the rows before every document, R behind them (64-bit in the report word: the host refuses 2^32 rows and more)
__global__ __launch_bounds__(1024) void tk_k_pad_scan(uint32_t* __restrict__ doc_row, uint64_t n_docs, unsigned long long* __restrict__ words) {
    __shared__ unsigned long long wsum[16];
    const unsigned long long carry = tk_scan_blocks<false>(doc_row, n_docs, 0ull, wsum);
    if (threadIdx.x == 0) {
        words[TK_PAD_NROWS] = carry;
        doc_row[n_docs] = (uint32_t)carry;
    }
}

__global__ __launch_bounds__(256) void tk_k_pad_rows(const uint64_t* __restrict__ tok_off, const uint32_t* __restrict__ doc_row, TkPad p, uint32_t* __restrict__ len,
                                                     uint32_t* __restrict__ row_doc, uint32_t* __restrict__ row_tok) {
    for (uint64_t r = blockIdx.x * 256ull + threadIdx.x; r < p.R; r += (uint64_t)gridDim.x * 256) tk_pad_row_entry(p, tok_off, doc_row, r, len, row_doc, row_tok);
}

// ids_out, mask_out: 16-byte aligned (the library's own buffers): a lane's eight ids leave as 16-byte stores, its eight mask bytes as one
// 8-byte store.  tokens is the caller's: the eight ids arrive as two 16-byte loads where the lane's positions are eight body tokens of one
// row and their address allows it (a row's body starts wherever its document and its window do, so that is one lane in four), otherwise
// as 4-byte loads, as in tk_k_rows_write.  What a lane computes is tk_pad_lane (tk_padded_rule.h), the same statements the CPU simulation runs.
template <bool IDS16>
__global__ __launch_bounds__(256) void tk_k_pad_write(const uint32_t* __restrict__ tokens, const uint64_t* __restrict__ tok_off, const uint32_t* __restrict__ doc_row, TkPad p,
                                                      void* __restrict__ ids_out, uint8_t* __restrict__ mask_out) {
    __shared__ uint64_t sh_doc[2];
    const uint32_t N = (uint32_t)(p.R * p.W);  // (below 2^32, above 0: the host launches nothing otherwise)
    const uint32_t b0 = blockIdx.x * (uint32_t)TK_DEC_BLOCK, i0 = b0 + threadIdx.x * 8u;  // (b0 < N; an i0 that wraps lies beyond N: the test below asks b0)
    if (threadIdx.x == 0) tk_pad_block_docs(p, doc_row, b0, TK_DEC_BLOCK, N, &sh_doc[0], &sh_doc[1]);
    __syncthreads();
    if (N - b0 <= threadIdx.x * 8u) return;
    uint32_t id[8];
    uint64_t mask;
    tk_pad_lane(p, TkTokens{tokens}, tok_off, doc_row, sh_doc[0], sh_doc[1], i0, N, id, &mask);
    if (N - i0 >= 8u) {
        tk_ids_store8<IDS16>(ids_out, i0, id);
        *(unsigned long long*)(mask_out + i0) = mask;
    } else {
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j)
            if (N - i0 > j) {
                tk_ids_store1<IDS16>(ids_out, i0 + j, id[j]);
                mask_out[i0 + j] = (uint8_t)(mask >> (8 * j));
            }
    }
}
