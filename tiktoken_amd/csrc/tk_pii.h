// Masking personal data in packed text on the device: packed text (text, doc_off) in, packed text out with every e-mail address and
// every (public) IPv4 address replaced by a fixed placeholder; per document how many of each.  The last text stage of C4-, CCNet-,
// Gopher- and FineWeb-style builds (DataTrove's PIIFormatter) before the text is encoded.  Nothing in the reference does this: it
// replaces re.sub per document on the host.  The rule is stated in include/tiktoken_amd.h; its plain C++ -- an e-mail from its '@', an
// address from its first digit, the SWAR trigger masks -- is tk_pii_rule.h's.
//
// The first text pass here that writes bytes its input did not hold, and the first without a carry between tiles: a decision reads at
// most TK_PII_BACK bytes before its trigger and TK_PII_AHEAD behind it, so a tile that stages that much around itself decides alone.
// A workgroup of TK_PII_THREADS lanes takes a tile of TK_PII_TILE bytes with TK_PII_HALO bytes before and behind it -- the WINDOW, 298
// lanes' worth of 16-byte loads (byte loads where the pointer is not aligned or the text ends, zeros outside the text), lanes 0 .. 41
// taking a halo chunk besides their own.  Document starts inside the window are bits in LDS, found by two tk_last_le on doc_off; a
// decision's bounds are the bits around its trigger, so a candidate searches nothing.
//   triggers  a lane's '@' bytes and its digits behind a byte outside [A-Za-z0-9_.] (or at a document's start), by SWAR over its 16
//             bytes.  Lanes without one do nothing more: nearly all on ordinary text.
//   e-mails   every '@' of the window whose match can reach the tile or an address that reaches the tile is decided -- those of the
//             halo AGAIN, by this tile as by its neighbour: the result follows from the text alone, so nothing is handed over.  A match
//             sets its bytes in the `gone` bitmap, and its start bit where it starts in the tile.
//   addresses after a barrier: a candidate whose first byte is `gone` lies in an e-mail and is none.  (No address starts inside another
//             one, so the bits addresses set meanwhile never decide a candidate.)
//   tk_k_pii_find   per tile the bytes it writes: kept ones plus the placeholders of the matches that START in it; per document n_email
//                   and n_ip by 64-bit atomics from the deciding lanes (the document by tk_last_le among the window's entries).
//   tk_k_pii_scan   one workgroup of 1024 over the tiles' bytes, in place (tk_scan_blocks: right past 1024 tiles); counts.
//   tk_k_pii_write  reads the total: where it exceeds the capacity no byte of text is stored, and without doc_off_out the kernel returns
//                   at once.  The decisions again; a lane's output offset is an exclusive scan over the workgroup (the lanes with a
//                   match counted in its high bits).  A tile without a match is a shifted vector copy out of the window.  Otherwise kept bytes
//                   and placeholder bytes go to LDS at their offsets, TK_PII_ROUND bytes of output at a time, shifted by the low four
//                   bits of the destination, and from there to HBM in 16-byte rows.  doc_off_out[i] for every doc_off[i] in the tile.
// Sums commute: every value is a function of (text, doc_off, spec) alone.  No table in HBM, no host wait, no floating point; all stores
// are vector stores of plain C++.  No matrix instructions: there is no contraction here.  A doc_off that does not ascend cannot make an
// access leave the arrays: an entry of doc_off is only ever an index i <= n_docs found by tk_last_le, or a window position checked
// against the window; text is read at window positions below N; what is written to text_out lies below the scanned total, which the
// write pass has compared with the capacity.
// Included by tk_api.hip only.
#pragma once
#include "tk_pii_rule.h"
#include "tk_scan.h"

#define TK_PII_WIN (TK_PII_TILE + 2u * TK_PII_HALO)            // bytes of the window
#define TK_PII_CHUNKS (TK_PII_WIN / TK_PII_LANE)               // 16-byte chunks of it
#define TK_PII_HALO_CHUNKS (TK_PII_HALO / TK_PII_LANE)         // ... of a halo
#define TK_PII_WORDS (TK_PII_WIN / 32u)                        // words of a bit per window position
#define TK_PII_ROUND 8192u                                     // bytes of output the write pass holds in LDS at a time
#define TK_PII_AT_FIRST (TK_PII_HALO - 14u - TK_PII_AHEAD)     // the window positions of the '@' bytes that are decided: the first can end
#define TK_PII_AT_LAST (TK_PII_HALO + TK_PII_TILE + TK_PII_MAX_LOCAL)  // behind an address that reaches the tile, the last starts in the tile
static_assert(TK_PII_TILE == TK_PII_THREADS * TK_PII_LANE && TK_PII_WIN % 32u == 0 && 2u * TK_PII_HALO_CHUNKS <= TK_PII_THREADS, "a lane a chunk of the tile, some a halo chunk too");
static_assert(TK_PII_AT_FIRST >= TK_PII_BACK && TK_PII_AT_LAST + TK_PII_AHEAD + 1u <= TK_PII_WIN, "every decision reads inside the window");
static_assert(TK_PII_MAX_BYTES + TK_PII_WIN <= 0xFFFFFFFFull && TK_PII_ROUND % 16u == 0, "window positions fit 32 bits; whole rows");

struct TkPiiShared {
    alignas(16) uint8_t txt[TK_PII_WIN];  // txt[r]: the byte at window position r, text position g0 - TK_PII_HALO + r; 0 outside the text
    uint32_t brk[TK_PII_WORDS];           // bit r: a document starts at window position r
    uint32_t gone[TK_PII_WORDS];          // bit r: the byte lies in a match
    uint32_t st[2][TK_PII_TILE / 32u];    // bit i: an e-mail / an address starts at the tile's byte i
    uint32_t ph[2][TK_PII_MAX_PLACEHOLDER / 4];
    uint32_t i0, i1;                      // the entries of doc_off that can lie in the window: [i0, i1]
};
// The lane's view of its chunk of the tile once the decisions are made
struct TkPiiLane {
    uint32_t keep, st_email, st_ip, bytes;  // bit j: byte j is kept / starts a match; the bytes the lane writes
};

// the last bit at or before r, the first behind r; `floor` / `ceil` where none lies between
__device__ __forceinline__ int32_t tk_pii_brk_back(const uint32_t* w, int32_t r, int32_t floor) {
    for (int32_t k = r >> 5; 32 * k + 31 >= floor && k >= 0; --k) {
        const uint32_t m = k == (r >> 5) ? w[k] & (0xFFFFFFFFu >> (31 - (r & 31))) : w[k];
        if (m) return max(floor, 32 * k + 31 - (int32_t)__clz((int)m));
    }
    return floor;
}
__device__ __forceinline__ int32_t tk_pii_brk_ahead(const uint32_t* w, int32_t r, int32_t ceil) {
    for (int32_t k = (r + 1) >> 5; 32 * k < ceil; ++k) {
        const uint32_t m = k == ((r + 1) >> 5) ? w[k] & (0xFFFFFFFFu << ((r + 1) & 31)) : w[k];
        if (m) return min(ceil, 32 * k + (int32_t)__ffs((int)m) - 1);
    }
    return ceil;
}
// bits [a, b) of a bitmap in LDS, 0 <= a < b <= 32 * its words
__device__ __forceinline__ void tk_pii_set_bits(uint32_t* w, int32_t a, int32_t b) {
    for (int32_t k = a >> 5; 32 * k < b; ++k) {
        const uint32_t from = max(a, 32 * k) & 31, to = min(b, 32 * k + 32) - 32 * k;  // 1 <= to <= 32
        atomicOr(w + k, (0xFFFFFFFFu >> (32u - to)) & (0xFFFFFFFFu << from));
    }
}

// The decisions of the tile of block blockIdx.x: sh.gone and sh.st, and the lane's view of its own chunk.  COUNT: the documents' n_email
// and n_ip (null ones skipped) are added to.  Every lane of the workgroup is here.
template <bool COUNT>
__device__ __forceinline__ TkPiiLane tk_pii_decide(const TkPii& q, const uint8_t* __restrict__ text, const uint64_t* __restrict__ doc_off, bool aligned, TkPiiShared& sh,
                                                    unsigned long long* n_email, unsigned long long* n_ip) {
    const uint32_t tid = threadIdx.x;
    const int64_t N = (int64_t)q.n_bytes, g0 = (int64_t)blockIdx.x * TK_PII_TILE, w0 = g0 - TK_PII_HALO;
    const int32_t vlo = w0 < 0 ? (int32_t)-w0 : 0, vhi = N - w0 < (int64_t)TK_PII_WIN ? (int32_t)(N - w0) : (int32_t)TK_PII_WIN;  // the text's window positions: [vlo, vhi)
    // the lane's chunks: its own of the tile, and for lanes 0 .. 41 one of the halo before (0 .. 20) or behind the tile
    const uint32_t mine = TK_PII_HALO_CHUNKS + tid, other = tid < TK_PII_HALO_CHUNKS ? tid : TK_PII_HALO_CHUNKS + TK_PII_THREADS + (tid - TK_PII_HALO_CHUNKS);
    const uint32_t n_chunks = tid < 2u * TK_PII_HALO_CHUNKS ? 2u : 1u;
    for (uint32_t i = 0; i < n_chunks; ++i) {
        const uint32_t c = i ? other : mine;
        const int64_t at = w0 + (int64_t)c * TK_PII_LANE;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (aligned && at >= 0 && at + TK_PII_LANE <= N) {
            v = *(const uint4*)(text + at);
        } else {
            uint32_t b[4] = {0, 0, 0, 0};
            for (uint32_t j = 0; j < TK_PII_LANE; ++j)
                if (at + j >= 0 && at + j < N) b[j >> 2] |= (uint32_t)text[at + j] << (8u * (j & 3u));
            v = make_uint4(b[0], b[1], b[2], b[3]);
        }
        *(uint4*)(sh.txt + c * TK_PII_LANE) = v;
    }
    for (uint32_t k = tid; k < TK_PII_WORDS; k += TK_PII_THREADS) sh.brk[k] = 0, sh.gone[k] = 0;
    if (tid < TK_PII_TILE / 32u) sh.st[0][tid] = 0, sh.st[1][tid] = 0;
    if (tid < 2u * (TK_PII_MAX_PLACEHOLDER / 4)) (&sh.ph[0][0])[tid] = (&q.ph[0][0])[tid];
    if (tid == 0) sh.i0 = (uint32_t)tk_last_le(doc_off, 0, q.n_docs + 1, (uint64_t)(w0 < 0 ? 0 : w0)), sh.i1 = (uint32_t)tk_last_le(doc_off, 0, q.n_docs + 1, (uint64_t)(w0 + TK_PII_WIN - 1));
    __syncthreads();
    for (uint64_t i = (uint64_t)sh.i0 + tid; i <= sh.i1; i += TK_PII_THREADS) {
        const uint64_t r = doc_off[i] - (uint64_t)w0;  // (wraps below the window)
        if (r < TK_PII_WIN) atomicOr(&sh.brk[r >> 5], 1u << (r & 31u));
    }
    __syncthreads();
    auto rd = [&](int64_t r) -> uint32_t { return sh.txt[r]; };  // (a decision reads inside its bounds, the bounds lie inside the window)
    // what a match that starts at window position s gives its document and the tile
    auto starts = [&](int32_t s, uint32_t kind, unsigned long long* per_doc) {
        const uint32_t i = (uint32_t)s - TK_PII_HALO;
        if (i >= TK_PII_TILE) return;
        atomicOr(&sh.st[kind][i >> 5], 1u << (i & 31u));
        if (COUNT && per_doc) {
            const uint64_t d = tk_last_le(doc_off, sh.i0, (uint64_t)sh.i1 + 1, (uint64_t)(w0 + s));
            if (d < q.n_docs) atomicAdd(per_doc + d, 1ull);
        }
    };
    for (uint32_t i = 0; i < n_chunks; ++i) {
        const uint32_t c = i ? other : mine;
        const uint4 v = *(const uint4*)(sh.txt + c * TK_PII_LANE);
        uint32_t at, dig, wdot;
        tk_pii_lane_masks(v.x | ((uint64_t)v.y << 32), v.z | ((uint64_t)v.w << 32), &at, &dig, &wdot);
#pragma unroll 1
        for (; at; at &= at - 1u) {
            const int32_t p = (int32_t)(c * TK_PII_LANE) + __ffs((int)at) - 1;
            if (p < (int32_t)TK_PII_AT_FIRST || p > (int32_t)TK_PII_AT_LAST || p < vlo || p >= vhi) continue;
            const int32_t lo = tk_pii_brk_back(sh.brk, p, max(vlo, p - TK_PII_BACK)), hi = tk_pii_brk_ahead(sh.brk, p, min(vhi, p + 1 + TK_PII_AHEAD));
            int64_t s, e;
            if (!tk_pii_email(rd, lo, hi, p, &s, &e)) continue;
            tk_pii_set_bits(sh.gone, (int32_t)s, (int32_t)e);
            starts((int32_t)s, 0u, n_email);
        }
    }
    __syncthreads();
    for (uint32_t i = 0; i < n_chunks; ++i) {
        const uint32_t c = i ? other : mine;
        if (c + 1u < TK_PII_HALO_CHUNKS || c >= TK_PII_HALO_CHUNKS + TK_PII_THREADS) continue;  // (an address that reaches the tile starts in the chunk before it or in it)
        const uint32_t r0 = c * TK_PII_LANE;  // (a multiple of 16: the chunk's 16 bits lie in one word)
        const uint4 v = *(const uint4*)(sh.txt + r0);
        uint32_t at, dig, wdot;
        tk_pii_lane_masks(v.x | ((uint64_t)v.y << 32), v.z | ((uint64_t)v.w << 32), &at, &dig, &wdot);
        if (!dig) continue;
        const uint32_t brk = (sh.brk[r0 >> 5] >> (r0 & 31u)) & 0xFFFFu, before = tk_pii_word(sh.txt[r0 - 1u]) || sh.txt[r0 - 1u] == '.';
        uint32_t cand = dig & (~((wdot << 1) | before) | brk) & 0xFFFFu;
#pragma unroll 1
        for (; cand; cand &= cand - 1u) {
            const int32_t p = (int32_t)r0 + __ffs((int)cand) - 1;
            if (p + 14 < (int32_t)TK_PII_HALO || p < vlo || p >= vhi || ((sh.gone[p >> 5] >> (p & 31)) & 1u)) continue;
            const int32_t lo = tk_pii_brk_back(sh.brk, p, max(vlo, p - 1)), hi = tk_pii_brk_ahead(sh.brk, p, min(vhi, p + TK_PII_IP_AHEAD));
            uint32_t a = 0, b = 0;
            const uint32_t len = tk_pii_ip(rd, lo, hi, p, &a, &b);
            if (!len || (q.public_only && tk_pii_ip_private(a, b))) continue;
            tk_pii_set_bits(sh.gone, p, p + (int32_t)len);
            starts(p, 1u, n_ip);
        }
    }
    __syncthreads();
    const uint32_t r0 = mine * TK_PII_LANE, t0 = tid * TK_PII_LANE;
    const int64_t left = N - (g0 + t0);
    const uint32_t valid = left <= 0 ? 0u : left >= (int64_t)TK_PII_LANE ? 0xFFFFu : (1u << left) - 1u;
    TkPiiLane L;
    L.keep = ~(sh.gone[r0 >> 5] >> (r0 & 31u)) & valid;
    L.st_email = (sh.st[0][t0 >> 5] >> (t0 & 31u)) & 0xFFFFu, L.st_ip = (sh.st[1][t0 >> 5] >> (t0 & 31u)) & 0xFFFFu;
    L.bytes = (uint32_t)__popc(L.keep) + (uint32_t)__popc(L.st_email) * q.len_email + (uint32_t)__popc(L.st_ip) * q.len_ip;
    return L;
}

// words: the call's total, e-mails and addresses; the documents' counts
__global__ __launch_bounds__(256) void tk_k_pii_clear(unsigned long long* words, unsigned long long* n_email, unsigned long long* n_ip, uint64_t n_docs) {
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n_docs; i += (uint64_t)gridDim.x * 256) {
        if (n_email) n_email[i] = 0;
        if (n_ip) n_ip[i] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x < 4u) words[threadIdx.x] = 0;
}

__global__ __launch_bounds__(TK_PII_THREADS) void tk_k_pii_find(TkPii q, const uint8_t* __restrict__ text, const uint64_t* __restrict__ doc_off, bool aligned,
                                                               unsigned long long* __restrict__ tiles, unsigned long long* words, unsigned long long* n_email,
                                                               unsigned long long* n_ip) {
    __shared__ TkPiiShared sh;
    __shared__ uint32_t wsum[3][4];
    const TkPiiLane L = tk_pii_decide<true>(q, text, doc_off, aligned, sh, n_email, n_ip);
    const unsigned long long bytes = tk_block_sum_256(L.bytes, wsum[0]), ne = tk_block_sum_256((uint32_t)__popc(L.st_email), wsum[1]), ni = tk_block_sum_256((uint32_t)__popc(L.st_ip), wsum[2]);
    if (threadIdx.x) return;
    tiles[blockIdx.x] = bytes;
    if (ne) atomicAdd(words + 1, ne);
    if (ni) atomicAdd(words + 2, ni);
}

// tiles: bytes -> the bytes of the tiles before; words[0]: the total.  cap: of text_out, ~0 for a call that only counts.
__global__ __launch_bounds__(1024) void tk_k_pii_scan(unsigned long long* tiles, uint64_t n_tiles, unsigned long long* words, unsigned long long cap, unsigned long long* __restrict__ counts) {
    __shared__ unsigned long long wsum[16];
    const unsigned long long total = tk_scan_blocks<false>(tiles, n_tiles, 0ull, wsum);
    if (threadIdx.x) return;
    words[0] = total;
    if (counts) counts[0] = total, counts[1] = words[1], counts[2] = words[2], counts[3] = total > cap ? 1ull : 0ull;
}

__global__ __launch_bounds__(TK_PII_THREADS) void tk_k_pii_write(TkPii q, const uint8_t* __restrict__ text, const uint64_t* __restrict__ doc_off, bool aligned,
                                                                const unsigned long long* __restrict__ tiles, const unsigned long long* __restrict__ words, unsigned long long cap,
                                                                uint8_t* __restrict__ text_out, unsigned long long* __restrict__ doc_off_out) {
    __shared__ TkPiiShared sh;
    __shared__ alignas(16) uint8_t out[TK_PII_ROUND];  // the round's bytes: out[x - x0] for the output position x = shift + the byte's offset in the tile's output
    __shared__ uint32_t before_of[TK_PII_THREADS];     // the bytes of the lanes before a lane
    __shared__ uint32_t wsum[8];
    if (words[0] > cap) text_out = nullptr;  // (every lane alike) too small: no byte of text is stored
    if (!text_out && !doc_off_out) return;
    const uint32_t tid = threadIdx.x;
    const uint64_t g0 = (uint64_t)blockIdx.x * TK_PII_TILE;
    const TkPiiLane L = tk_pii_decide<false>(q, text, doc_off, aligned, sh, nullptr, nullptr);
    // (a tile writes fewer than 2^20 bytes: the lanes with a match are counted above them)
    uint32_t sum;
    const uint32_t ex = tk_block_exscan_256(L.bytes + ((L.st_email | L.st_ip) ? 1u << 20 : 0u), &sum, wsum) & 0xFFFFFu, total = sum & 0xFFFFFu;
    const uint64_t dst = tiles[blockIdx.x], in_tile = q.n_bytes > g0 ? q.n_bytes - g0 : 0ull;
    const bool plain = !(sum >> 20) && total == (in_tile < TK_PII_TILE ? in_tile : TK_PII_TILE);  // no match starts here and every byte is kept
    before_of[tid] = ex;
    __syncthreads();
    if (text_out) {
        uint8_t* const g = text_out + dst;
        const uint32_t shift = (uint32_t)((uintptr_t)g & 15u), end = shift + total;
        if (plain) {
            // nothing goes and nothing comes: the row of output positions [x, x + 16) holds the tile's bytes [x - shift, x - shift + 16)
            for (uint32_t x = tid * 16u; x < end; x += TK_PII_THREADS * 16u) {
                const uint8_t* const src = sh.txt + TK_PII_HALO + x;  // (row x of the tile; the row before it exists: the halo)
                if (x >= shift && x + 16u <= end) {
                    const uint4 a = *(const uint4*)(src - 16), b = *(const uint4*)src;
                    const uint64_t w[4] = {a.x | ((uint64_t)a.y << 32), a.z | ((uint64_t)a.w << 32), b.x | ((uint64_t)b.y << 32), b.z | ((uint64_t)b.w << 32)};
                    const uint32_t k = 16u - shift, s = 8u * (k & 7u);  // the row starts at byte k of (a, b), 1 <= k <= 16
                    const uint64_t u0 = k >= 16u ? w[2] : k >= 8u ? w[1] : w[0], u1 = k >= 16u ? w[3] : k >= 8u ? w[2] : w[1], u2 = k >= 16u ? 0ull : k >= 8u ? w[3] : w[2];
                    const uint64_t lo = s ? (u0 >> s) | (u1 << (64u - s)) : u0, hi = s ? (u1 >> s) | (u2 << (64u - s)) : u1;
                    *(uint4*)(g + (x - shift)) = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
                } else {
                    for (uint32_t i = x < shift ? shift : x; i < x + 16u && i < end; ++i) g[i - shift] = sh.txt[TK_PII_HALO + i - shift];
                }
            }
        } else {
            const uint8_t* const own = sh.txt + TK_PII_HALO + tid * TK_PII_LANE;
            const uint8_t* const ph_email = (const uint8_t*)sh.ph[0];
            const uint8_t* const ph_ip = (const uint8_t*)sh.ph[1];
#pragma unroll 1
            for (uint32_t x0 = 0; x0 < end; x0 += TK_PII_ROUND) {
                uint32_t x = shift + ex;
                if (L.bytes && x + L.bytes > x0 && x < x0 + TK_PII_ROUND) {
                    auto put = [&](uint32_t b) {
                        if (x - x0 < TK_PII_ROUND) out[x - x0] = (uint8_t)b;  // (wraps below the round)
                        ++x;
                    };
#pragma unroll 1
                    for (uint32_t j = 0; j < TK_PII_LANE; ++j) {
                        if ((L.st_email >> j) & 1u)
                            for (uint32_t k = 0; k < q.len_email; ++k) put(ph_email[k]);
                        if ((L.st_ip >> j) & 1u)
                            for (uint32_t k = 0; k < q.len_ip; ++k) put(ph_ip[k]);
                        if ((L.keep >> j) & 1u) put(own[j]);
                    }
                }
                __syncthreads();
                const uint32_t x1 = min(end, x0 + TK_PII_ROUND);
                for (uint32_t lo = x0 + tid * 16u; lo < x1; lo += TK_PII_THREADS * 16u) {  // out[lo - x0 ..) is g[lo - shift ..): the same 16-byte word
                    if (lo >= shift && lo + 16u <= x1) {
                        *(uint4*)(g + (lo - shift)) = *(const uint4*)(out + (lo - x0));
                    } else {
                        for (uint32_t i = lo < shift ? shift : lo; i < lo + 16u && i < x1; ++i) g[i - shift] = out[i - x0];
                    }
                }
                __syncthreads();
            }
        }
    }
    // The entries of doc_off at the tile's positions, and at position T for the tile behind: the same value, that tile's `dst`.  The first
    // tile starts at entry 0: the empty documents at position 0 lie before the last entry that is <= 0.  A placeholder lies behind the
    // start of its document: only the matches that start before the position count.
    if (doc_off_out)
        for (uint64_t i = (blockIdx.x ? (uint64_t)sh.i0 : 0ull) + tid; i <= sh.i1; i += TK_PII_THREADS) {
            const uint64_t r = doc_off[i] - g0;  // (wraps below g0)
            if (r < TK_PII_TILE) {
                const uint32_t r0 = TK_PII_HALO + ((uint32_t)r & ~15u), t0 = (uint32_t)r & ~15u, below = (1u << (r & 15u)) - 1u;
                const int64_t left = (int64_t)q.n_bytes - (int64_t)(g0 + t0);
                const uint32_t valid = left <= 0 ? 0u : left >= (int64_t)TK_PII_LANE ? 0xFFFFu : (1u << left) - 1u;
                const uint32_t keep = ~(sh.gone[r0 >> 5] >> (r0 & 31u)) & valid & below;
                const uint32_t ne = (sh.st[0][t0 >> 5] >> (t0 & 31u)) & below, ni = (sh.st[1][t0 >> 5] >> (t0 & 31u)) & below;
                doc_off_out[i] = dst + before_of[r >> 4] + (uint32_t)__popc(keep) + (uint32_t)__popc(ne) * q.len_email + (uint32_t)__popc(ni) * q.len_ip;
            } else if (r == TK_PII_TILE) {
                doc_off_out[i] = dst + total;
            }
        }
}
