// UTF-8 repair on the device: any packed text in HBM -> what bytes.decode("utf-8", "replace" / "ignore") makes of every document, again
// as packed UTF-8, with the byte, char and replaced-unit offsets of the documents (the rule: include/tiktoken_amd.h).  Built like
// tk_k_utf8_docs (tk_offsets.h): sixteen bytes per lane from one 16-byte load, the three bytes before from the neighbour lane, the
// document boundaries from the bitmap over the bytes (tk_k_span_mark).  A workgroup is 256 lanes, TK_U8R_BLOCK bytes.
//   tk_k_u8r_check   the offsets ascend from 0 to n: the first document that offends
//   tk_k_u8r_count   a lane's three counts (tk_u8r_lane without a stream), their prefixes inside the workgroup and the workgroup's sums;
//                    the lane's place in its workgroup's output; for the first document that starts at a byte, the three prefixes there
//   tk_k_u8r_scan    a workgroup per count: the sums -> the workgroups' bases, 64-bit, and the three totals
//   -- the host waits here: a refused call has written into scratch only; no unit replaced: the input IS the output, no write pass --
//   tk_k_u8r_docs    per document: base of the workgroup of its first byte + the prefix there; documents behind empty ones take the
//                    offsets of the first document at their byte (one search each, as tk_k_span_docs)
//   tk_k_u8r_write   a lane's step again, with a stream from base + place on: no barrier, no atomics, the order is the input's
// The count pass runs before the offsets are known to be good: it indexes nothing with an offset's VALUE (it searches the offsets for a
// byte position and writes at the index found), and the bitmap holds no bit beyond n.  Included by tk_api.hip only.
#pragma once
#include "tk_offsets.h"  // tk_lower_bound64, tk_span_first_at, tk_k_span_mark
#include "tk_utf8_repair_rule.h"

// the words the passes report in (unsigned long long each): the first document whose offset offends (all ones: none), then the totals
enum { TK_U8R_BAD_DOC = 0, TK_U8R_OUT, TK_U8R_CHARS, TK_U8R_REPL, TK_U8R_WORDS };

__global__ __launch_bounds__(256) void tk_k_u8r_check(const uint64_t* __restrict__ off, uint64_t n_docs, uint64_t n, unsigned long long* __restrict__ words) {
    for (uint64_t d = blockIdx.x * 256ull + threadIdx.x; d <= n_docs; d += (uint64_t)gridDim.x * 256) {
        const uint64_t a = off[d];
        const bool bad = (d == 0 && a != 0) || (d < n_docs ? a > off[d + 1] : a != n);
        if (bad) atomicMin(words + TK_U8R_BAD_DOC, (unsigned long long)d);
    }
}

// A lane's sixteen bytes, the three before them and its bounds.  bytes: 16-byte aligned, readable 16 bytes past n; docb: readable one
// word past bit n + 16.  The lane at p0 <= n exists (the position n has documents that start there), with nvalid == 0 where p0 == n.
struct TkU8rLaneIn {
    uint64_t lo, hi;
    uint32_t nvalid, prev, bounds, before;
};
__device__ __forceinline__ TkU8rLaneIn tk_u8r_load(const uint8_t* __restrict__ bytes, uint64_t n, const uint32_t* __restrict__ docb, uint64_t p0) {
    TkU8rLaneIn in{0ull, 0ull, 0u, 0u, 0u, 0u};
    in.nvalid = p0 < n ? (n - p0 < 16 ? (uint32_t)(n - p0) : 16u) : 0u;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (in.nvalid) v = *(const uint4*)(bytes + p0);
    uint32_t prev = __shfl_up(v.w, 1, 64);  // the neighbour lane's last four bytes
    if ((threadIdx.x & 63) == 0) prev = (in.nvalid && p0) ? *(const uint32_t*)(bytes + p0 - 4) : 0u;
    in.prev = prev >> 8;
    in.lo = (uint64_t)v.x | ((uint64_t)v.y << 32);
    in.hi = (uint64_t)v.z | ((uint64_t)v.w << 32);
    if (p0 <= n) in.bounds = tk_u8r_bounds(docb, p0, &in.before);
    return in;
}
__device__ __forceinline__ bool tk_u8r_plain(const TkU8rLaneIn& in) {  // ASCII behind a finished sequence: every byte is a unit of its own
    return !((in.lo | in.hi | (uint64_t)in.prev) & 0x8080808080808080ull);
}

// rel: 3 x (n_docs + 1) words -- out, chars, repl before the byte at which document k starts, inside that byte's workgroup (written for the
// first document at a byte only); place[lane]: the lane's output inside its workgroup's; sums: 3 x nb.
__global__ __launch_bounds__(256) void tk_k_u8r_count(const uint8_t* __restrict__ bytes, uint64_t n, const uint32_t* __restrict__ docb,
                                                      const uint64_t* __restrict__ off, uint64_t n_docs, uint32_t mode, uint64_t nb,
                                                      unsigned long long* __restrict__ sums, uint16_t* __restrict__ place, uint32_t* __restrict__ rel) {
    __shared__ uint32_t sh[8];
    const uint64_t lane = (uint64_t)blockIdx.x * 256 + threadIdx.x, p0 = lane * 16;
    const TkU8rLaneIn in = tk_u8r_load(bytes, n, docb, p0);
    TkU8rNoStream none;
    TkU8rCounts c{in.nvalid, in.nvalid, 0u};
    const bool plain = tk_u8r_plain(in);
    const uint32_t starts = in.bounds & 0xFFFFu & ((2u << in.nvalid) - 1u);  // documents that start at the lane's bytes 0 .. nvalid
    // the one step takes along what the lane's bytes before its FIRST document start were charged: few lanes hold a second start
    const uint32_t first_i = starts ? (uint32_t)__ffs((int)starts) - 1u : 0u;
    TkU8rCounts first_at{first_i, first_i, 0u};
    if (!plain)
        c = tk_u8r_lane(in.lo, in.hi, in.nvalid, in.prev, in.bounds, in.before, mode, none, [&](uint32_t i, const TkU8rCounts& at) {
            if (i == first_i) first_at = at;
        });
    // bytes and chars in one scan, 16 bits each: a workgroup leaves at most 3 x TK_U8R_BLOCK + 3 bytes, and no more chars than bytes
    uint32_t tot_oc, tot_r;
    const uint32_t ex_oc = tk_block_exscan_256(c.out | (c.chars << 16), &tot_oc, sh), ex_r = tk_block_exscan_256(c.repl, &tot_r, sh);
    const uint32_t ex_o = ex_oc & 0xFFFFu, ex_c = ex_oc >> 16;
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = tot_oc & 0xFFFFu;
        sums[nb + blockIdx.x] = tot_oc >> 16;
        sums[2 * nb + blockIdx.x] = tot_r;
    }
    if (p0 <= n) place[lane] = (uint16_t)ex_o;  // (at most 3 x TK_U8R_BLOCK)
    if (!starts) return;
    auto doc = [&](uint32_t i, const TkU8rCounts& at) {
        const uint64_t p = p0 + i, k = tk_lower_bound64(off, n_docs + 1, p);
        if (k <= n_docs && off[k] == p) {
            rel[k] = ex_o + at.out;
            rel[n_docs + 1 + k] = ex_c + at.chars;
            rel[2 * (n_docs + 1) + k] = ex_r + at.repl;
        }
    };
    doc(first_i, first_at);
    const uint32_t more = starts & (starts - 1u);  // documents of a few bytes: further starts in the lane
    if (!more) return;
    if (plain) {
        for (uint32_t m = more; m; m &= m - 1u) {
            const uint32_t i = (uint32_t)__ffs((int)m) - 1u;
            doc(i, TkU8rCounts{i, i, 0u});
        }
    } else {
        (void)tk_u8r_lane(in.lo, in.hi, in.nvalid, in.prev, in.bounds, in.before, mode, none, [&](uint32_t i, const TkU8rCounts& at) {
            if (i != first_i) doc(i, at);
        });
    }
}

// three workgroups, one per count: the sums of nb workgroups -> their bases, in place; the total
__global__ __launch_bounds__(1024) void tk_k_u8r_scan(unsigned long long* __restrict__ sums, uint64_t nb, unsigned long long* __restrict__ words) {
    __shared__ unsigned long long wsum[16];
    const unsigned long long total = tk_scan_blocks<false>(sums + blockIdx.x * nb, nb, 0ull, wsum);
    if (threadIdx.x == 0) words[TK_U8R_OUT + blockIdx.x] = total;
}

// off: checked by now (tk_k_u8r_check), so off[d] >> 12 names a workgroup.  out: 3 x (n_docs + 1): text_off, char_off, repl_off.
__global__ __launch_bounds__(256) void tk_k_u8r_docs(const uint64_t* __restrict__ off, uint64_t n_docs, uint64_t nb, const unsigned long long* __restrict__ base,
                                                     const uint32_t* __restrict__ rel, uint64_t* __restrict__ out) {
    for (uint64_t d = blockIdx.x * 256ull + threadIdx.x; d <= n_docs; d += (uint64_t)gridDim.x * 256) {
        const uint64_t f = tk_span_first_at(off, n_docs, d), w = off[f] / TK_U8R_BLOCK;
#pragma unroll
        for (uint32_t k = 0; k < 3u; ++k) out[k * (n_docs + 1) + d] = base[k * nb + w] + rel[k * (n_docs + 1) + f];
    }
}

// text: the output, 8-byte aligned, n_text + 16 bytes
__global__ __launch_bounds__(256) void tk_k_u8r_write(const uint8_t* __restrict__ bytes, uint64_t n, const uint32_t* __restrict__ docb, uint32_t mode,
                                                      const unsigned long long* __restrict__ base, const uint16_t* __restrict__ place, uint8_t* __restrict__ text) {
    const uint64_t lane = (uint64_t)blockIdx.x * 256 + threadIdx.x, p0 = lane * 16;
    const TkU8rLaneIn in = tk_u8r_load(bytes, n, docb, p0);
    if (!in.nvalid) return;
    TkDecStores stores{text};
    TkU8rStream<TkDecStores> stream(stores, base[blockIdx.x] + place[lane]);
    if (tk_u8r_plain(in)) {
        uint64_t lo = in.lo, hi = in.hi;
        for (uint32_t left = in.nvalid; left; left -= left < 4u ? left : 4u) {
            const uint32_t nbytes = left < 4u ? left : 4u;
            stream.put((uint32_t)lo & (nbytes < 4u ? (1u << (8u * nbytes)) - 1u : 0xFFFFFFFFu), nbytes);
            lo = (lo >> 32) | (hi << 32);
            hi >>= 32;
        }
    } else {
        (void)tk_u8r_lane(in.lo, in.hi, in.nvalid, in.prev, in.bounds, in.before, mode, stream, TkU8rNoDocs());
    }
    stream.finish();
}
