// Token spans on the device (reference Encoding.decode_with_offsets, tiktoken/core.py:312-335, over whole batches): for every token of a
// packed batch the byte and the char at which it starts in its own document, the byte and char offsets of the documents, and a strict
// UTF-8 check of the decoded documents.  Built like the decode passes of tk_decode.h (TK_DEC_BLOCK tokens per workgroup, eight per lane):
//   tk_k_span_mark    document starts -> a bitmap (over the tokens for the span passes, over the decoded bytes for the UTF-8 check)
//   tk_k_span_len     tk_k_dec_len plus the char count of every token (the second per-id table, tk_char_word), and per workgroup the
//                     bytes, the chars and where the last document start of the workgroup lies
//   tk_k_span_scan    one workgroup: exclusive 64-bit sums of both counts, and for every workgroup where the last document start BEFORE
//                     it lies (a max-scan: offsets only grow along the batch)
//   tk_k_span_write   offsets of every token, rebased to its document's start; a token that starts documents writes the first one's offsets
//   tk_k_span_docs    per document: the offsets of documents behind empty ones; 4 GiB and more is refused; token bytes against the
//                     text's length (encode side)
//   tk_k_utf8_docs    sixteen bytes per lane, the first ill-formed document
// How a token learns its document's start: the marked scan above.  The other way -- every lane searches tok_off for its first token -- needs
// the documents' offsets BEFORE the spans, i.e. the write pass twice; it was built, measured and dropped (profiles/offsets_path.txt).
// A batch may be run in ranges of tokens (tk_decode_batch_spans: ids arrive and spans leave while the next range is scanned): the scan
// kernel takes the sums and the last document start of the ranges before from four words and leaves its own there; offsets stay the batch's.
// tk_k_span_len leaves the lengths and tk_k_span_scan the workgroups' byte bases where tk_k_dec_copy reads them: the bytes follow with that
// kernel unchanged.  Included by tk_api.hip only.
#pragma once
#include "tk_decode.h"
#include "tk_span_rule.h"

// the words the passes report in (unsigned long long each; the first four start as all ones = none)
// TK_SPAN_BYTES .. TK_SPAN_MARK_C: the scan's carry -- bytes and chars so far, offset + 1 of the last document start so far (0: none)
enum { TK_SPAN_BAD_TOKEN = 0, TK_SPAN_BIG_DOC, TK_SPAN_GAP_DOC, TK_SPAN_BAD_UTF8, TK_SPAN_BYTES, TK_SPAN_CHARS, TK_SPAN_MARK_B, TK_SPAN_MARK_C, TK_SPAN_WORDS };

__global__ __launch_bounds__(256) void tk_k_span_mark(const uint64_t* __restrict__ off, uint64_t count, uint64_t limit, uint32_t* __restrict__ bm) {
    for (uint64_t d = blockIdx.x * 256ull + threadIdx.x; d < count; d += (uint64_t)gridDim.x * 256) {
        const uint64_t p = off[d];
        if (p <= limit) atomicOr(&bm[p >> 5], 1u << (p & 31u));
    }
}

// first index d of off[0 .. count) with off[d] >= v (count if none)
__device__ __forceinline__ uint64_t tk_lower_bound64(const uint64_t* __restrict__ off, uint64_t count, uint64_t v) {
    uint64_t lo = 0, hi = count;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (off[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// the last index d of off[0 .. count) with off[d] <= v (off[0] <= v)
__device__ __forceinline__ uint64_t tk_last_le64(const uint64_t* __restrict__ off, uint64_t count, uint64_t v) {
    uint64_t lo = 0, hi = count;  // first index with off > v
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (off[mid] <= v) lo = mid + 1;
        else hi = mid;
    }
    return lo ? lo - 1 : 0;
}

// One range of a batch: n tokens from position pos_base on (tokens, marks, lens and the per-workgroup arrays point at the range; pos_base
// is a multiple of TK_DEC_BLOCK).  end = 1 in the batch's last range: its workgroups cover the position n as well, behind the last
// token, where the documents that end the batch "start".
__global__ __launch_bounds__(256) void tk_k_span_len(const uint32_t* __restrict__ tokens, uint64_t n, uint32_t end, uint64_t pos_base,
                                                     const uint2* __restrict__ dec, const uint32_t* __restrict__ cw, uint32_t n_ids,
                                                     const uint8_t* __restrict__ marks, uint32_t* __restrict__ lens, unsigned long long* __restrict__ bsum,
                                                     unsigned long long* __restrict__ csum, unsigned long long* __restrict__ mkey,
                                                     unsigned long long* __restrict__ words) {
    __shared__ uint32_t sh[8];
    __shared__ unsigned long long sh64[4];
    const uint64_t i0 = (uint64_t)blockIdx.x * TK_DEC_BLOCK + (uint64_t)threadIdx.x * 8;
    const uint32_t mk = i0 < n + end ? marks[i0 >> 3] : 0u;
    uint32_t sum = 0, chars = 0, mark_b = 0, mark_c = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint64_t i = i0 + j;
        if ((mk >> j) & 1u) mark_b = sum, mark_c = chars;
        if (i < n) {
            const uint32_t t = tokens[i];
            const uint32_t len = t < n_ids ? dec[t].y : 0u;
            if (len == 0u) atomicMin(words + TK_SPAN_BAD_TOKEN, (unsigned long long)(pos_base + i));  // (every real token has at least one byte)
            else chars += cw[t] & ~TK_SPAN_CONT;
            lens[i] = len;
            sum += len;
        }
    }
    uint32_t tot_b, tot_c;
    const uint32_t ex_b = tk_block_exscan_256(sum, &tot_b, sh);
    const uint32_t ex_c = tk_block_exscan_256(chars, &tot_c, sh);
    unsigned long long last;
    (void)tk_block_exmax64_256(mk ? tk_span_key(ex_b + mark_b, ex_c + mark_c) : 0ull, &last, sh64);
    if (threadIdx.x == 0) {
        bsum[blockIdx.x] = tot_b;
        csum[blockIdx.x] = tot_c;
        mkey[blockIdx.x] = last;
    }
}

// In place: bsum / csum -> the bytes / chars of the batch before every workgroup of the range.  doc_b / doc_c [w]: byte / char offset in the batch of the last document
// start before workgroup w (0 where there is none: only the batch's first workgroup, whose first token starts document 0).
__global__ __launch_bounds__(1024) void tk_k_span_scan(unsigned long long* __restrict__ bsum, unsigned long long* __restrict__ csum,
                                                       const unsigned long long* __restrict__ mkey, uint64_t nb, unsigned long long* __restrict__ doc_b,
                                                       unsigned long long* __restrict__ doc_c, unsigned long long* __restrict__ words) {
    __shared__ unsigned long long wsum[16];
    // (the same in every thread; marks: offset + 1, 0 = none.  Every thread has read the words before thread 0 writes them: the loop's barriers)
    unsigned long long carry_b = words[TK_SPAN_BYTES], carry_c = words[TK_SPAN_CHARS], carry_mb = words[TK_SPAN_MARK_B], carry_mc = words[TK_SPAN_MARK_C];
    __syncthreads();
    for (uint64_t base = 0; base < nb; base += 1024) {
        const uint64_t i = base + threadIdx.x;
        unsigned long long tb, tc, tmb, tmc;
        const unsigned long long at_b = carry_b + tk_scan1024<false>(i < nb ? bsum[i] : 0ull, &tb, wsum);
        const unsigned long long at_c = carry_c + tk_scan1024<false>(i < nb ? csum[i] : 0ull, &tc, wsum);
        const unsigned long long key = i < nb ? mkey[i] : 0ull;
        const unsigned long long mb = tk_scan1024<true>(tk_span_mark_at(at_b, key, true), &tmb, wsum);
        const unsigned long long mc = tk_scan1024<true>(tk_span_mark_at(at_c, key, false), &tmc, wsum);
        if (i < nb) {
            bsum[i] = at_b;
            csum[i] = at_c;
            const unsigned long long b = tk_max64(carry_mb, mb), ch = tk_max64(carry_mc, mc);
            doc_b[i] = b ? b - 1ull : 0ull;
            doc_c[i] = ch ? ch - 1ull : 0ull;
        }
        carry_b += tb;
        carry_c += tc;
        carry_mb = tk_max64(carry_mb, tmb);
        carry_mc = tk_max64(carry_mc, tmc);
    }
    if (threadIdx.x == 0) {
        words[TK_SPAN_BYTES] = carry_b;
        words[TK_SPAN_CHARS] = carry_c;
        words[TK_SPAN_MARK_B] = carry_mb;
        words[TK_SPAN_MARK_C] = carry_mc;
    }
}

// A range, as tk_k_span_len.  A token that starts documents writes the offsets of the FIRST of them (several start at one position when
// documents are empty); tk_k_span_docs gives the others theirs.
__global__ __launch_bounds__(256) void tk_k_span_write(const uint32_t* __restrict__ tokens, uint64_t n, uint32_t end, uint64_t pos_base,
                                                       const uint32_t* __restrict__ cw, uint32_t n_ids, const uint32_t* __restrict__ lens,
                                                       const uint8_t* __restrict__ marks, const uint64_t* __restrict__ tok_off, uint64_t n_docs,
                                                       const unsigned long long* __restrict__ bbase, const unsigned long long* __restrict__ cbase,
                                                       const unsigned long long* __restrict__ doc_b, const unsigned long long* __restrict__ doc_c,
                                                       uint32_t* __restrict__ byte_start, uint32_t* __restrict__ char_start, uint64_t* __restrict__ byte_off,
                                                       uint64_t* __restrict__ char_off) {
    __shared__ uint32_t sh[8];
    __shared__ unsigned long long sh64[4];
    const uint64_t i0 = (uint64_t)blockIdx.x * TK_DEC_BLOCK + (uint64_t)threadIdx.x * 8;
    const uint32_t mk = i0 < n + end ? marks[i0 >> 3] : 0u;
    uint32_t len[8], word[8], sum = 0, chars = 0, mark_b = 0, mark_c = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint64_t i = i0 + j;
        len[j] = word[j] = 0u;
        if ((mk >> j) & 1u) mark_b = sum, mark_c = chars;
        if (i < n) {
            const uint32_t t = tokens[i];
            len[j] = lens[i];
            word[j] = t < n_ids ? cw[t] : 0u;
        }
        sum += len[j];
        chars += word[j] & ~TK_SPAN_CONT;
    }
    uint32_t tot;
    const uint32_t ex_b = tk_block_exscan_256(sum, &tot, sh), ex_c = tk_block_exscan_256(chars, &tot, sh);
    const unsigned long long wg_b = bbase[blockIdx.x], wg_c = cbase[blockIdx.x];
    unsigned long long any;
    const unsigned long long before = tk_block_exmax64_256(mk ? tk_span_key(ex_b + mark_b, ex_c + mark_c) : 0ull, &any, sh64);
    // where the current document starts
    unsigned long long base_b = before ? wg_b + tk_span_key_bytes(before) : doc_b[blockIdx.x];
    unsigned long long base_c = before ? wg_c + tk_span_key_chars(before) : doc_c[blockIdx.x];
    unsigned long long at_b = wg_b + ex_b, at_c = wg_c + ex_c;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint64_t i = i0 + j;
        if (i >= n + end) break;
        if (((mk >> j) & 1u) || i == n) {  // documents start here: theirs are the offsets of this position
            base_b = at_b;
            base_c = at_c;
            const uint64_t k = tk_lower_bound64(tok_off, n_docs + 1, pos_base + i);
            if (k <= n_docs && tok_off[k] == pos_base + i) {
                byte_off[k] = at_b;
                char_off[k] = at_c;
            }
        }
        if (i < n) {
            byte_start[i] = (uint32_t)(at_b - base_b);  // (a document of 4 GiB and more: tk_k_span_docs)
            char_start[i] = tk_span_char_start(at_c - base_c, word[j]);
        }
        at_b += len[j];
        at_c += word[j] & ~TK_SPAN_CONT;
    }
}

// Per document, after the last range: a document that starts where the one before it starts (that one is empty) takes the offsets of the
// first document at that position; 4 GiB and more is refused; doc_off (may be null): the offsets of the documents' TEXT when the tokens
// come from an encode call -- the tokens' bytes must add up to it.  (Reads only entries tk_k_span_write wrote, writes only the others.)
__device__ __forceinline__ uint64_t tk_span_first_at(const uint64_t* __restrict__ tok_off, uint64_t n_docs, uint64_t d) {
    return d && tok_off[d] == tok_off[d - 1] ? tk_lower_bound64(tok_off, n_docs + 1, tok_off[d]) : d;
}
__global__ __launch_bounds__(256) void tk_k_span_docs(const uint64_t* __restrict__ tok_off, uint64_t* __restrict__ byte_off, uint64_t* __restrict__ char_off,
                                                      const uint64_t* __restrict__ doc_off, uint64_t n_docs, unsigned long long* __restrict__ words) {
    for (uint64_t d = blockIdx.x * 256ull + threadIdx.x; d <= n_docs; d += (uint64_t)gridDim.x * 256) {
        const uint64_t f = tk_span_first_at(tok_off, n_docs, d);
        const uint64_t at = byte_off[f];
        if (f != d) {
            byte_off[d] = at;
            char_off[d] = char_off[f];
        }
        if (d == n_docs) continue;
        const uint64_t len = byte_off[tk_span_first_at(tok_off, n_docs, d + 1)] - at;
        if (len >> 32) atomicMin(words + TK_SPAN_BIG_DOC, (unsigned long long)d);
        if (doc_off && len != doc_off[d + 1] - doc_off[d]) atomicMin(words + TK_SPAN_GAP_DOC, (unsigned long long)d);
    }
}

// bytes: 16-byte aligned, readable 16 bytes past n.  docb: bit p = a document starts at byte p (bit n: the text's end), readable one word past bit n + 16.
__global__ __launch_bounds__(256) void tk_k_utf8_docs(const uint8_t* __restrict__ bytes, uint64_t n, const uint32_t* __restrict__ docb,
                                                      const uint64_t* __restrict__ byte_off, uint64_t n_docs, unsigned long long* __restrict__ words) {
    const uint64_t p0 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    const uint32_t nvalid = p0 < n ? (n - p0 < 16 ? (uint32_t)(n - p0) : 16u) : 0u;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (nvalid) v = *(const uint4*)(bytes + p0);
    uint32_t prev = __shfl_up(v.w, 1, 64);  // the neighbour lane's last four bytes
    if ((threadIdx.x & 63) == 0) prev = (nvalid && p0) ? *(const uint32_t*)(bytes + p0 - 4) : 0u;
    if (!nvalid) return;
    uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {  // (what lies behind the text is not text)
        if (nvalid <= 4u * k) w[k] = 0u;
        else if (nvalid < 4u * k + 4u) w[k] &= (1u << (8u * (nvalid - 4u * k))) - 1u;
    }
    const uint32_t bw = docb[p0 >> 5], sh = (uint32_t)(p0 & 31u);
    const uint32_t bounds = ((bw >> sh) & 0xFFFFu) | ((sh ? (docb[(p0 >> 5) + 1] & 1u) : ((bw >> 16) & 1u)) << 16);
    const uint32_t err = tk_utf8_lane_errors(w, prev >> 8, bounds, nvalid);
    if (err) atomicMin(words + TK_SPAN_BAD_UTF8, (unsigned long long)tk_last_le64(byte_off, n_docs + 1, p0 + (uint32_t)(__ffs((int)err) - 1)));
}
