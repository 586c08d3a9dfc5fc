// Decode on the device: token ids -> bytes (reference CoreBPE::decode_bytes, src/lib.rs:345-358: concatenate decoder[token] for every
// token; Encoding.decode_batch / decode_bytes_batch, tiktoken/core.py:331-350, map it over documents).  A gather plus a prefix sum:
//   tk_k_dec_len     length of every token from the id -> {offset, length} table (an id without entry raises the reference's KeyError)
//                    and the byte count of every workgroup of 2048 tokens
//   tk_k_dec_scan64  exclusive prefix sum of those counts (64-bit: outputs may exceed 4 GiB)
//   tk_k_dec_copy    workgroup base + local scan = byte offset of every token; one lane per token copies its bytes to their place
//   tk_k_dec_docoff  byte offset of every document of a packed batch
// Included by tk_api.hip only (itself, and through tk_offsets.h and tk_rows.h).
#pragma once
#include "tk_kernels.h"
#include "tk_device.h"
#include "tk_decode_rule.h"  // TK_DEC_SPEC, TK_DEC_BLOCK, tk_dec_len_of, tk_dec_lane, tk_dec_doc_off

__global__ __launch_bounds__(256) void tk_k_dec_len(const uint32_t* __restrict__ tokens, uint64_t n, const uint2* __restrict__ dec,
                                                    uint32_t n_ids, uint32_t* __restrict__ lens, unsigned long long* __restrict__ bsum,
                                                    unsigned long long* __restrict__ bad /* position of the first token without entry; ~0 = none */,
                                                    uint64_t pos_base /* position of tokens[0] in the caller's batch (a batch is decoded in ranges) */) {
    __shared__ uint32_t sh[4];
    const uint64_t i0 = (uint64_t)blockIdx.x * TK_DEC_BLOCK + (uint64_t)threadIdx.x * 8;
    uint32_t sum = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint64_t i = i0 + j;
        uint32_t len = 0;
        if (i < n) {
            const uint32_t t = tokens[i];
            len = tk_dec_len_of(dec, n_ids, t);
            if (len == 0u) atomicMin(bad, (unsigned long long)(pos_base + i));  // (every real token has at least one byte)
            lens[i] = len;
        }
        sum += len;
    }
    const unsigned long long tot = tk_block_sum_256(sum, sh);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

// single-workgroup exclusive scan of the per-workgroup sums (64-bit); total -> total_out[0]
__global__ __launch_bounds__(1024) void tk_k_dec_scan64(unsigned long long* __restrict__ a, uint64_t nb, unsigned long long* __restrict__ total_out) {
    __shared__ unsigned long long wsum[16];
    const unsigned long long total = tk_scan_blocks<false>(a, nb, 0ull, wsum);
    if (threadIdx.x == 0) total_out[0] = total;
}

// byte offset of every token: workgroup base + local exclusive scan; then the copy.  A lane owns eight consecutive tokens, so its bytes
// are one contiguous stretch of the output: they stream through a 64-bit register aligned with the destination -- one aligned 8-byte
// store per eight bytes (the first and the last word of the stretch, shared with the neighbours, go out byte by byte), sources read as
// aligned words and shifted (tk_load8: the blobs are readable 16 bytes past their ends).
__global__ __launch_bounds__(256) void tk_k_dec_copy(const uint32_t* __restrict__ tokens, uint64_t n, const uint2* __restrict__ dec,
                                                     const uint32_t* __restrict__ lens, const unsigned long long* __restrict__ bbase,
                                                     const uint8_t* __restrict__ tok_bytes, const uint8_t* __restrict__ spec_bytes,
                                                     uint8_t* __restrict__ out, unsigned long long* __restrict__ tok_byte_off /* may be null */,
                                                     unsigned long long off_base /* bytes of the batch before this range (added to tok_byte_off only) */) {
    __shared__ uint32_t sh[8];
    const uint64_t i0 = (uint64_t)blockIdx.x * TK_DEC_BLOCK + (uint64_t)threadIdx.x * 8;
    uint32_t len[8], mine = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        len[j] = i0 + j < n ? lens[i0 + j] : 0u;
        mine += len[j];
    }
    uint32_t tot;
    const uint32_t ex = tk_block_exscan_256(mine, &tot, sh);
    const unsigned long long at = bbase[blockIdx.x] + ex;
    TkDecStores stores{out};
    tk_dec_lane(tokens, i0, n, len, at, dec, tok_bytes, spec_bytes, stores, tok_byte_off, off_base);
}

// byte_off[d] = byte offset of the first token of document d (tok_off: n_docs + 1 token offsets, non-decreasing)
__global__ __launch_bounds__(256) void tk_k_dec_docoff(const uint64_t* __restrict__ tok_off, uint64_t n_docs, uint64_t n,
                                                       const unsigned long long* __restrict__ tok_byte_off,
                                                       const unsigned long long* __restrict__ total, uint64_t* __restrict__ byte_off) {
    for (uint64_t d = blockIdx.x * 256ull + threadIdx.x; d <= n_docs; d += (uint64_t)gridDim.x * 256) {
        byte_off[d] = tk_dec_doc_off(tok_off, d, n, tok_byte_off, total);
    }
}
