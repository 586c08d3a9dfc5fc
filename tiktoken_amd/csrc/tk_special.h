// Special tokens in raw text: what the marking kernels (tk_k_spec_cand / tk_k_spec_resolve, the allowed set) and the scan for a
// disallowed one (tk_k_spec_find) share.  Host-compilable like tk_device.h, so that a CPU test can drive the same code.
//
//   tk_special_at      longest special token of a masked set that matches at a position        (src/lib.rs:386-402)
//   tk_spec_hits16     positions among sixteen text bytes at which some special token may start
//   tk_spec_find16     leftmost position among them at which a token of the set does match      (tiktoken/core.py:116-124: the search
//                      for a disallowed special token over the whole string, before anything is encoded)
#pragma once
#include <string.h>

#include <vector>

#include "tk_device.h"
#include "tk_tables.h"

// Longest allowed special token that matches at text[pos..] without crossing a document start.
// Returns its length (0 = none) and index.  The next 32 text bytes and the document starts among the next 64 positions are read once; a
// special token of at most 32 bytes is compared with them word by word (four independent loads of its bytes instead of a load per byte
// that waits for the byte before it: the resolving pass calls this two or three times per candidate, one lane of a wavefront at a time).
TK_HD uint64_t tk_bits64(const uint32_t* __restrict__ bm, uint64_t pos) {  // bits [pos, pos + 64) of a bitmap (readable two words past them)
    const uint64_t wi = pos >> 5;
    const uint32_t sh = (uint32_t)(pos & 31);
    const uint32_t w0 = bm[wi], w1 = bm[wi + 1], w2 = bm[wi + 2];
    const uint64_t lo = ((uint64_t)w1 << 32) | w0;
    return sh ? ((lo >> sh) | ((uint64_t)w2 << (64u - sh))) : lo;
}
TK_HD uint32_t tk_special_at(const TkTables& T, const uint8_t* __restrict__ text, uint64_t pos, uint64_t n, const uint8_t* __restrict__ allowed,
                             const uint32_t* __restrict__ docb, uint32_t* idx_out) {
    uint32_t b0 = text[pos];
    if (!((T.spec_first[b0 >> 5] >> (b0 & 31)) & 1u)) return 0;
    uint64_t tw[4];  // (the text is readable 64 bytes past n)
#pragma unroll
    for (int i = 0; i < 4; ++i) tw[i] = tk_load8(text, pos + 8u * i);
    const uint64_t db = docb ? tk_bits64(docb, pos + 1) : 0ull;  // document starts at pos + 1 .. pos + 64
    uint32_t best = 0, bi = 0;
    for (uint32_t k = 0; k < T.n_spec; ++k) {
        // (round 6: a token's first eight bytes, length and offset in one load that depends on nothing -- the loads of all tokens are in flight
        // together; a candidate that is no special token, "<|x", leaves after it.  Offsets, first byte and bytes were four dependent loads per token.)
#if defined(__HIP_DEVICE_COMPILE__)
        const uint4 hd = ((const uint4*)T.spec_head)[k];
#else
        const struct { uint32_t x, y, z, w; } hd = {T.spec_head[4 * k], T.spec_head[4 * k + 1], T.spec_head[4 * k + 2], T.spec_head[4 * k + 3]};
#endif
        const uint32_t o = hd.w, len = hd.z;
        if (len <= best || pos + len > n) continue;
        if (tk_mask_low_bytes(tw[0] ^ (((uint64_t)hd.y << 32) | hd.x), len < 8u ? len : 8u) != 0ull) continue;
        if (allowed && !allowed[k]) continue;
        bool ok = true;
        if (len <= 32u) {
#pragma unroll
            for (int i = 1; i < 4; ++i)
                if (8u * i < len) ok = ok && tk_mask_low_bytes(tw[i] ^ tk_load8(T.spec_bytes, (uint64_t)o + 8u * i), len - 8u * i) == 0ull;
            ok = ok && (db & ((1ull << (len - 1u)) - 1ull)) == 0ull;
        } else {
            for (uint32_t i = 1; i < len && ok; ++i) ok = (text[pos + i] == T.spec_bytes[o + i]) && !(docb && tk_bit(docb, pos + i));
        }
        if (ok) {
            best = len;
            bi = k;
        }
    }
    *idx_out = bi;
    return best;
}


#if defined(__HIP_DEVICE_COMPILE__)
TK_HD uint32_t tk_ctz32(uint32_t v) { return (uint32_t)(__ffs((int)v) - 1); }  // (v != 0)
#else
TK_HD uint32_t tk_ctz32(uint32_t v) { return (uint32_t)__builtin_ctz(v); }
#endif

// Sixteen text bytes (w: little-endian words; nxt: the byte behind them): bit k is set where byte k may start a special token.  Almost
// every byte fails the first-byte test.  With at most four distinct first bytes (every stock encoding: '<') the test is four byte-equality
// tests per 32-bit word (x ^ c has a zero byte; the borrow may mark a byte above a true hit as well: a false candidate, which
// tk_special_at rejects); otherwise the 256-bit set decides byte by byte.  Then the byte behind a hit must be some special token's
// second byte ("<" is common in web text, "<|" is not).
TK_HD uint32_t tk_spec_hits16(const TkTables& T, const uint32_t w[4], uint32_t nxt) {
    uint32_t hits = 0;
    if (T.n_spec_fb <= 4u) {
        for (uint32_t f = 0; f < T.n_spec_fb; ++f) {
            const uint32_t c4 = ((T.spec_fb >> (8u * f)) & 0xFFu) * 0x01010101u;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const uint32_t x = w[d] ^ c4;
                const uint32_t z = (x - 0x01010101u) & ~x & 0x80808080u;  // bit 7 of every zero byte (and, rarely, of a 0x01 above one)
                // bits 7, 15, 23, 31 -> bits 0..3
                hits |= (((z >> 7) | (z >> 14) | (z >> 21) | (z >> 28)) & 0xFu) << (4 * d);
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint32_t b = (w[k >> 2] >> ((k & 3) * 8)) & 0xFFu;
            hits |= ((T.spec_first[b >> 5] >> (b & 31)) & 1u) << k;
        }
    }
    if (hits) {
        uint32_t keep = 0;
        for (uint32_t m = hits; m; m &= m - 1) {
            const uint32_t k = tk_ctz32(m);
            const uint32_t b1 = k < 15u ? (w[(k + 1) >> 2] >> (((k + 1) & 3u) * 8u)) & 0xFFu : nxt;
            keep |= ((T.spec_second[b1 >> 5] >> (b1 & 31u)) & 1u) << k;
        }
        hits = keep;
    }
    return hits;
}

// The disallowed scan's share of one lane: the leftmost position among text[p0, p0 + 16) that lies below `limit` (and below n) and at
// which a special token of the set `disallowed` (a byte per special token, as `allowed` above) matches wholly inside one document;
// ~0 if there is none.  `hits`: tk_spec_hits16 of those bytes.  Matches are looked for in the raw text, whatever the allowed set makes
// of it: the reference searches the whole string before it encodes anything (tiktoken/core.py:116-124).
TK_HD uint64_t tk_spec_find16(const TkTables& T, const uint8_t* __restrict__ text, uint64_t p0, uint64_t n, uint32_t hits,
                              const uint8_t* __restrict__ disallowed, const uint32_t* __restrict__ docb, uint64_t limit) {
    for (; hits; hits &= hits - 1) {
        const uint64_t pos = p0 + tk_ctz32(hits);
        if (pos >= n || pos >= limit) break;
        uint32_t idx;
        if (tk_special_at(T, text, pos, n, disallowed, docb, &idx)) return pos;
    }
    return ~0ull;
}

// The resolving pass's share of one candidate (tk_k_spec_resolve): overlapping candidates are resolved exactly as a left-to-right search
// would (src/lib.rs:389-401,432) -- the candidate at `pos` is taken iff the greedy non-overlapping walk from the head of its overlap
// cluster lands on it.  A taken candidate is marked: its first byte in spec_start and brk, its other bytes in spec_in, the byte behind
// it (inside the text) in brk.  `cand`: the candidates of tk_k_spec_cand, readable two words past a position's; max_len: the longest
// registered special token.  Marks go through or_bit(bitmap, word, mask): an atomic OR on the device, |= on the host.
// (Earlier candidates are looked for in the 64 bits of the bitmap before the position -- two loads, not one per bit; with special tokens
// of 66 bytes and more the walk goes bit by bit.)  The head walk asks about every earlier candidate of the cluster: a cluster of L
// overlapping candidates costs about L * L / 2 calls of tk_special_at.
template <class OrBit>
TK_HD void tk_spec_resolve_one(const TkTables& T, const uint8_t* __restrict__ text, uint64_t n, const uint8_t* __restrict__ allowed,
                               const uint32_t* __restrict__ docb, const uint32_t* __restrict__ cand, uint32_t max_len, uint64_t pos,
                               uint32_t* __restrict__ spec_start, uint32_t* __restrict__ spec_in, uint32_t* __restrict__ brk, OrBit or_bit) {
    uint32_t idx;
    // head of the overlap cluster: walk left while some earlier candidate's span covers `h`
    uint64_t h = pos;
    for (;;) {
        bool moved = false;
        uint64_t lo = h >= (uint64_t)(max_len - 1) ? h - (max_len - 1) : 0;
        if (max_len <= 65u && h >= 64u) {
            uint64_t before = tk_bits64(cand, h - 64u);          // candidates at h - 64 .. h - 1 (bit 63 = h - 1)
            before = h > lo ? (before & (~0ull << (64u - (uint32_t)(h - lo)))) : 0ull;  // only those at lo .. h - 1
            while (before) {  // nearest first
                const uint32_t b = 63u - tk_clz64(before);
                before &= ~(1ull << b);
                const uint64_t j = h - 64u + b;
                if (j + tk_special_at(T, text, j, n, allowed, docb, &idx) > h) {
                    h = j;
                    moved = true;
                    break;
                }
            }
        } else {
            for (uint64_t j = h; j-- > lo;) {
                if (tk_bit(cand, j) && j + tk_special_at(T, text, j, n, allowed, docb, &idx) > h) {
                    h = j;
                    moved = true;
                    break;
                }
            }
        }
        if (!moved) break;
    }
    // greedy walk from the head
    uint64_t cur = h;
    bool taken = false;
    while (cur <= pos) {
        if (cur == pos) {
            taken = true;
            break;
        }
        uint64_t nx = cur + tk_special_at(T, text, cur, n, allowed, docb, &idx);
        while (nx <= pos && !tk_bit(cand, nx)) ++nx;
        cur = nx;
    }
    if (!taken) return;
    uint32_t len = tk_special_at(T, text, pos, n, allowed, docb, &idx);
    or_bit(spec_start, pos >> 5, 1u << (pos & 31));
    or_bit(brk, pos >> 5, 1u << (pos & 31));
    for (uint64_t a = pos + 1, b = pos + len; a < b;) {  // the token's interior, a word of the bitmap at a time
        const uint64_t we = (a | 31u) + 1u, hi = we < b ? we : b;
        const uint32_t cnt = (uint32_t)(hi - a);
        or_bit(spec_in, a >> 5, (cnt >= 32u ? 0xFFFFFFFFu : ((1u << cnt) - 1u)) << (a & 31u));
        a = hi;
    }
    if (pos + len < n) or_bit(brk, (pos + len) >> 5, 1u << ((pos + len) & 31));
}

// (host) What the functions above ask of TkTables beyond the host tables' arrays: every special token's head (T.spec_head points at a copy of
// `head` wherever the caller keeps it), the set of first bytes in both forms, the set of second bytes.
static inline void tk_spec_tables(const TkHostTables& H, std::vector<uint32_t>& head, TkTables& D) {
    head.assign(4 * (H.spec_id.size() + 1), 0u);
    for (size_t k = 0; k < H.spec_id.size(); ++k) {
        const uint32_t o = H.spec_off[k], len = H.spec_off[k + 1] - o;
        uint64_t h8 = 0;
        for (uint32_t i = 0; i < len && i < 8u; ++i) h8 |= (uint64_t)H.spec_bytes[o + i] << (8u * i);
        head[4 * k] = (uint32_t)h8;
        head[4 * k + 1] = (uint32_t)(h8 >> 32);
        head[4 * k + 2] = len;
        head[4 * k + 3] = o;
    }
    D.n_spec = (uint32_t)H.spec_id.size();
    memcpy(D.spec_first, H.spec_first, sizeof D.spec_first);
    D.spec_fb = 0;
    D.n_spec_fb = 0;
    for (uint32_t b = 0; b < 256; ++b)
        if ((H.spec_first[b >> 5] >> (b & 31)) & 1u) {
            if (D.n_spec_fb < 4) D.spec_fb |= b << (8 * D.n_spec_fb);
            D.n_spec_fb += 1;
        }
    if (D.n_spec_fb > 4) D.n_spec_fb = 0xFF;
    memset(D.spec_second, 0, sizeof D.spec_second);
    for (size_t k = 0; k + 1 < H.spec_off.size(); ++k) {
        const uint32_t o = H.spec_off[k], len = H.spec_off[k + 1] - o;
        if (len < 2) memset(D.spec_second, 0xFF, sizeof D.spec_second);
        else D.spec_second[H.spec_bytes[o + 1] >> 5] |= 1u << (H.spec_bytes[o + 1] & 31);
    }
}
