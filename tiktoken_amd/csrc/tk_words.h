// Word statistics per document on the device: for every document of packed text (text, doc_off) its words, the chars in them, the words
// with a letter, which of up to 32 stop words occur, its '#' and ellipses, its lines and the lines that end in terminal punctuation -- the
// word-level rules of the Gopher quality filter and the line-punctuation rule of C4 and FineWeb, on the text before it is encoded.  Nothing
// in the reference does this: it replaces text.split() per document on the host.  The rule is stated in include/tiktoken_amd.h; its plain
// C++ -- the white-space patterns, the masks, the element of the scans -- is tk_words_rule.h's.
//
// A workgroup of TK_WD_THREADS lanes takes a tile of TK_WD_TILE bytes, a lane 16 of them by one 16-byte load (byte loads where the
// pointer is not aligned or the text ends); the tile, two bytes before it (is this byte the tail of a white-space char?) and three behind
// it (the letter decode, the white-space tail) go to LDS, the document starts from two positions before the tile to three behind it --
// found by two tk_last_le on doc_off -- into a bit per position.  A lane's masks (white space, content, cuts, leads, letters, dots, '#',
// line ends) are SWAR words of 16 bits; a lane whose bytes are all ASCII never reads LDS or the class table for them, any other decodes at
// its lead bytes >= 0x80 alone: the class through uc_bmp below U+10000, through the two stages above.
//   tk_k_wd_clear  the documents' sums to 0
//   tk_k_wd_sum    per tile: the word and the dots that are open at its end (TkWdRun: 20 bytes), by a segmented scan under tk_wd_join over
//                  the wavefront by __shfl_up and over the four wavefronts through LDS.  No multiplication: a word's bytes, chars,
//                  has-letter and first 8 bytes compose exactly.
//   tk_k_wd_carry  one workgroup of 1024: the same scan over the tiles' summaries, a thread a stretch of tiles, in place: every tile gets
//                  the run that enters it.  A word or a dot run of many MiB costs this scan and no lane ever walks it.
//   tk_k_wd_count  the tile again.  A lane visits its EVENTS in order -- the cuts that end a word, '#', U+2026, the starts of dot runs,
//                  line ends -- and nothing else: a word is bytes [start, cut) of the lane by shifts and popcounts, joined to the scanned
//                  run that enters the lane where no cut lies before it, and is tested against the stop words' 64 bits and length; a line
//                  end needs the byte before the cut alone.  A lane gathers in registers while the document stays the same; a wavefront
//                  that lies inside one document adds once per sum (a butterfly), other lanes add for themselves: to the document's sums
//                  in LDS (the first TK_WD_DOCS documents of a tile) or to HBM directly; at the end a lane per document flushes to HBM.
//   tk_k_wd_final  a thread per document: the sums -> the eight outputs, null ones skipped
// Sums and the OR of the stop bits commute: the result is a function of (text, doc_off, stop words, terminal) alone.  There is no table,
// no host wait and no floating point; all stores are vector stores of plain C++.  No matrix instructions: there is no contraction here.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): see DESIGN.md.  Included by tk_api.hip only.
#pragma once
#include "tk_scan.h"
#include "tk_words_rule.h"

#define TK_WD_NONE 0xFFFFFFFFu
#define TK_WD_BRK_WORDS (TK_WD_TILE / 64u + 2u)  // bit 64 + r: a document starts at the tile's position r, -64 <= r < T + 64
static_assert(TK_WD_TILE == TK_WD_THREADS * TK_WD_LANE && TK_WD_WAVE == 64u * TK_WD_LANE && TK_WD_TILE == 64u * 64u, "a lane 16 bytes, whole wavefronts, 64 words of bits");
static_assert(TK_WD_DOCS <= TK_WD_THREADS, "a lane per gathered document at the flush");
static_assert(TK_WD_MAX_BYTES + TK_WD_TILE <= 0xFFFFFFFFull, "positions of the last tile are 32-bit");

struct TkWdTab {  // the class of a code point: the library's own table, whatever the core's split pattern
    const uint8_t *bmp, *stage1, *stage2;
};
struct TkWdOut {  // uint64[n_docs] each; any may be null
    unsigned long long *n_words, *word_chars, *n_alpha_words, *stop_mask, *n_hash, *n_ellipsis, *n_lines, *n_punct_lines;
};

__device__ __forceinline__ TkWdRun tk_wd_shfl_up(const TkWdRun& v, int o) {
    return TkWdRun{__shfl_up((unsigned long long)v.packed, o, 64), __shfl_up(v.bytes, o, 64), __shfl_up(v.chars, o, 64), __shfl_up(v.flags, o, 64)};
}
// The exclusive scan under tk_wd_join over a workgroup of whole wavefronts (at most 16), `init` before the first lane; *total: `init`
// and every lane's value.  wsum: a slot per wavefront in LDS, free again when the call returns.
__device__ __forceinline__ TkWdRun tk_wd_block_exscan(TkWdRun v, const TkWdRun& init, TkWdRun* wsum, TkWdRun* total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const TkWdRun u = tk_wd_shfl_up(v, o);
        if ((int)lane >= o) v = tk_wd_join(u, v);
    }
    if (lane == 63u) wsum[wave] = v;
    TkWdRun ex = tk_wd_shfl_up(v, 1);
    if (lane == 0) ex = tk_wd_empty();
    __syncthreads();
    TkWdRun pre = init;
#pragma unroll 1
    for (uint32_t w = 0; w < n_waves; ++w) {
        if (w == wave) ex = tk_wd_join(pre, ex);
        if (w < wave || total) pre = tk_wd_join(pre, wsum[w]);
    }
    if (total) *total = pre;
    __syncthreads();
    return ex;
}

struct TkWdShared {
    alignas(16) uint8_t txt[TK_WD_TILE + 32];     // txt[16 + i]: byte i of the tile; txt[14], txt[15] and txt[16 + T .. 18 + T]: the bytes beside it, 0 outside the text
    unsigned long long brkw[TK_WD_BRK_WORDS];
    uint32_t brkpre[TK_WD_TILE / 64];             // the starts at the tile's positions before a word of 64 positions
    TkWdRun wsum[4];
    uint32_t i0, i1;  // the entries of doc_off that can lie in [g0 - 2, g0 + T + 3]: [i0, i1]
};

// The tile of block t into LDS and the lane's view of it.  Every lane of the workgroup is here.
__device__ __forceinline__ TkWdLane tk_wd_stage(const TkWd& p, const TkWdTab& tab, const uint8_t* __restrict__ text, const uint64_t* __restrict__ doc_off, bool aligned,
                                                TkWdShared& sh) {
    const uint32_t tid = threadIdx.x;
    const uint64_t g0 = (uint64_t)blockIdx.x * TK_WD_TILE, N = p.n_bytes;
    TkWdLane L;
    L.pos = tid * TK_WD_LANE;
    const uint64_t at = g0 + L.pos;
    uint64_t lo = 0, hi = 0;
    if (aligned && at + TK_WD_LANE <= N) {
        const uint4 v = *(const uint4*)(text + at);
        lo = v.x | ((uint64_t)v.y << 32), hi = v.z | ((uint64_t)v.w << 32);
    } else {
        for (uint32_t j = 0; j < TK_WD_LANE && at + j < N; ++j) {
            const uint64_t b = text[at + j];
            if (j < 8) lo |= b << (8 * j);
            else hi |= b << (8 * (j - 8));
        }
    }
    *(uint4*)(sh.txt + 16 + L.pos) = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
    if (tid < 2) sh.txt[14 + tid] = g0 + tid >= 2 ? text[g0 + tid - 2] : 0;  // (g0 is 0 or at least T)
    if (tid >= TK_WD_THREADS - 3) {
        const uint64_t q = g0 + TK_WD_TILE + (tid - (TK_WD_THREADS - 3));
        sh.txt[16 + q - g0] = q < N ? text[q] : 0;
    }
    if (tid < TK_WD_BRK_WORDS) sh.brkw[tid] = 0;
    if (tid == 0) sh.i0 = (uint32_t)tk_last_le(doc_off, 0, p.n_docs + 1, g0 ? g0 - 2 : 0), sh.i1 = (uint32_t)tk_last_le(doc_off, 0, p.n_docs + 1, g0 + TK_WD_TILE + 3);
    __syncthreads();
    for (uint64_t i = (uint64_t)sh.i0 + tid; i <= sh.i1; i += TK_WD_THREADS) {
        const uint64_t r = doc_off[i] - g0 + 64;  // (wraps more than 64 below g0)
        if (r < 64ull * TK_WD_BRK_WORDS) atomicOr(&sh.brkw[r >> 6], 1ull << (r & 63u));
    }
    __syncthreads();
    if (tid < 64u) {
        const uint32_t c = (uint32_t)__popcll(sh.brkw[1 + tid]);
        sh.brkpre[tid] = tk_wave_scan_u32(c, (int)tid) - c;
    }
    __syncthreads();
    const uint32_t w = L.pos + 62u, s = w & 63u;  // bit 64 + pos - 2 and the 31 behind it; s is 62, 14, 30 or 46
    const uint32_t B = (uint32_t)((sh.brkw[w >> 6] >> s) | (sh.brkw[(w >> 6) + 1] << (64u - s)));
    const uint32_t n_left = at >= N ? 0u : N - at < 17u ? (uint32_t)(N - at) : 17u;
    const uint8_t* mine = sh.txt + 16 + L.pos;
    tk_wd_lane_masks(
        lo, hi, n_left, B, mine[16], [&](int k) -> uint32_t { return mine[k]; },
        [&](uint32_t cp) -> bool {
            uint32_t cl = tab.bmp[cp < 0x10000u ? cp : 0xFFFFu];
            if (cp >= 0x10000u) cl = cp <= 0x10FFFFu ? tab.stage2[(uint32_t)tab.stage1[cp >> 8] * 256u + (cp & 255u)] : (uint32_t)TK_C_OT;
            return (TK_M_L >> cl) & 1u;
        },
        &L);
    L.rank = sh.brkpre[L.pos >> 6] + (uint32_t)__popcll(sh.brkw[1 + (L.pos >> 6)] & ((1ull << (L.pos & 63u)) - 1ull));
    return L;
}

__global__ __launch_bounds__(256) void tk_k_wd_clear(unsigned long long* a, uint64_t n) {
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) a[i] = 0;
}

__global__ __launch_bounds__(TK_WD_THREADS) void tk_k_wd_sum(TkWd p, TkWdTab tab, const uint8_t* __restrict__ text, const uint64_t* __restrict__ doc_off, bool aligned,
                                                             TkWdRun* __restrict__ tiles) {
    __shared__ TkWdShared sh;
    const TkWdLane L = tk_wd_stage(p, tab, text, doc_off, aligned, sh);
    TkWdRun total;
    tk_wd_block_exscan(tk_wd_lane_tail(L), tk_wd_empty(), sh.wsum, &total);
    if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}

__global__ __launch_bounds__(1024) void tk_k_wd_carry(uint32_t n_tiles, TkWdRun* __restrict__ tiles) {
    __shared__ TkWdRun wsum[16];
    const uint32_t per = (n_tiles + 1023u) / 1024u;
    const uint64_t a = (uint64_t)threadIdx.x * per < n_tiles ? (uint64_t)threadIdx.x * per : n_tiles, b = a + per < n_tiles ? a + per : n_tiles;
    TkWdRun mine = tk_wd_empty();
    for (uint64_t t = a; t < b; ++t) mine = tk_wd_join(mine, tiles[t]);
    TkWdRun run = tk_wd_block_exscan(mine, tk_wd_empty(), wsum, nullptr);
    for (uint64_t t = a; t < b; ++t) {
        const TkWdRun s = tiles[t];
        tiles[t] = run;
        run = tk_wd_join(run, s);
    }
}

struct TkWdAcc {  // what a lane has gathered for one document
    uint32_t words, chars, alpha, stop, hash, ellipsis, lines, punct;
};
__device__ __forceinline__ uint32_t tk_wd_wave_or(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(TK_WD_THREADS) void tk_k_wd_count(TkWd p, TkWdTab tab, const uint8_t* __restrict__ text, const uint64_t* __restrict__ doc_off, bool aligned,
                                                               const TkWdRun* __restrict__ tiles, unsigned long long* sums) {
    __shared__ TkWdShared sh;
    __shared__ uint32_t docid[TK_WD_DOCS];            // the document of a local index; TK_WD_NONE
    __shared__ uint32_t acc[TK_WD_SUMS][TK_WD_DOCS];  // its sums of this tile
    const uint32_t tid = threadIdx.x;
    const uint64_t g0 = (uint64_t)blockIdx.x * TK_WD_TILE;
    const TkWdLane L = tk_wd_stage(p, tab, text, doc_off, aligned, sh);
    // Local documents: index 0 owns the byte before the tile; index r > 0 is the non-empty document at the r-th start bit at or behind g0.
    if (tid < TK_WD_DOCS) docid[tid] = tid == 0 && g0 && p.n_docs ? (uint32_t)tk_last_le(doc_off, 0, p.n_docs, g0 - 1) : TK_WD_NONE;
    for (uint32_t f = 0; f < TK_WD_SUMS; ++f)
        if (tid < TK_WD_DOCS) acc[f][tid] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)sh.i0 + tid; i <= sh.i1 && i < p.n_docs; i += TK_WD_THREADS) {
        const uint64_t s = doc_off[i], r = s - g0;
        if (r >= TK_WD_TILE || doc_off[i + 1] <= s) continue;
        const uint32_t li = sh.brkpre[r >> 6] + (uint32_t)__popcll(sh.brkw[1 + (r >> 6)] & ((2ull << (r & 63u)) - 1ull));
        if (li < TK_WD_DOCS) docid[li] = (uint32_t)i;
    }
    __syncthreads();
    const TkWdRun before = tk_wd_block_exscan(tk_wd_lane_tail(L), tiles[blockIdx.x], sh.wsum, nullptr);
    // a document's sums: li its local index, pos a position it owns
    auto put = [&](uint32_t li, uint64_t pos, const TkWdAcc& a) {
        const uint32_t v[TK_WD_SUMS] = {a.words, a.chars, a.alpha, a.stop, a.hash, a.ellipsis, a.lines, a.punct};
        if (!(a.words | a.hash | a.ellipsis | a.lines)) return;  // (chars, alpha and stop come with words, punct with lines)
        if (li < TK_WD_DOCS) {
#pragma unroll
            for (uint32_t f = 0; f < TK_WD_SUMS; ++f)
                if (v[f]) f == TK_WD_S_STOP ? atomicOr(&acc[f][li], v[f]) : atomicAdd(&acc[f][li], v[f]);
        } else {
            const uint64_t d = tk_last_le(doc_off, 0, p.n_docs, pos);
            if (d >= p.n_docs) return;
#pragma unroll
            for (uint32_t f = 0; f < TK_WD_SUMS; ++f)
                if (v[f]) f == TK_WD_S_STOP ? atomicOr(sums + (uint64_t)f * p.n_docs + d, (unsigned long long)v[f]) : atomicAdd(sums + (uint64_t)f * p.n_docs + d, (unsigned long long)v[f]);
        }
    };
    TkWdAcc a{0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t cur = L.doc(0), moved = 0;
    uint64_t cur_pos = g0 + L.pos;
    auto enter = [&](uint32_t li, uint64_t pos) {
        if (li == cur) return;
        put(cur, cur_pos, a);
        a = TkWdAcc{0, 0, 0, 0, 0, 0, 0, 0};
        cur = li, cur_pos = pos, moved = 1;
    };
    const uint32_t ends = tk_wd_ends(L, before), dstart = tk_wd_dot_starts(L), sym = L.hash | L.ell | L.lend | dstart;
#pragma unroll 1
    for (uint32_t ev = ends | sym; ev; ev &= ev - 1u) {
        const uint32_t j = (uint32_t)__ffs((int)ev) - 1u;
        const uint64_t here = g0 + L.pos + j;
        if ((ends >> j) & 1u) {  // a finished word: it belongs to the document of the byte before the cut
            enter(L.doc_before(j), here - 1);
            const TkWdRun w = tk_wd_word(L, before, j);
            a.words += 1u, a.chars += w.chars, a.alpha += w.flags & TK_WD_F_ALPHA, a.stop |= tk_wd_stop_bits(p, w);
        }
        if ((sym >> j) & 1u) {
            enter(L.doc(j), here);
            a.hash += (L.hash >> j) & 1u, a.ellipsis += (L.ell >> j) & 1u;
            if ((dstart >> j) & 1u) a.ellipsis += tk_wd_dot_triples(L, before, j);
            if ((L.lend >> j) & 1u) a.lines += 1u, a.punct += tk_wd_is_terminal(p, L.byte(j)) ? 1u : 0u;
        }
    }
    if (__all(!moved && cur == __shfl(cur, 0, 64))) {  // the wavefront lies in one document
        const TkWdAcc t{tk_wave_sum_u32(a.words), tk_wave_sum_u32(a.chars), tk_wave_sum_u32(a.alpha), tk_wd_wave_or(a.stop),
                        tk_wave_sum_u32(a.hash),  tk_wave_sum_u32(a.ellipsis), tk_wave_sum_u32(a.lines), tk_wave_sum_u32(a.punct)};
        if ((tid & 63u) == 0) put(cur, cur_pos, t);
    } else {
        put(cur, cur_pos, a);
    }
    __syncthreads();
    if (tid < TK_WD_DOCS && docid[tid] != TK_WD_NONE) {
        const uint64_t d = docid[tid];
        for (uint32_t f = 0; f < TK_WD_SUMS; ++f) {
            const uint32_t v = acc[f][tid];
            if (v) f == TK_WD_S_STOP ? atomicOr(sums + (uint64_t)f * p.n_docs + d, (unsigned long long)v) : atomicAdd(sums + (uint64_t)f * p.n_docs + d, (unsigned long long)v);
        }
    }
}

__global__ __launch_bounds__(256) void tk_k_wd_final(uint64_t n_docs, const unsigned long long* __restrict__ sums, TkWdOut o) {
    for (uint64_t d = blockIdx.x * 256ull + threadIdx.x; d < n_docs; d += (uint64_t)gridDim.x * 256) {
        auto s = [&](uint32_t f) { return sums[(uint64_t)f * n_docs + d]; };
        if (o.n_words) o.n_words[d] = s(TK_WD_S_WORDS);
        if (o.word_chars) o.word_chars[d] = s(TK_WD_S_CHARS);
        if (o.n_alpha_words) o.n_alpha_words[d] = s(TK_WD_S_ALPHA);
        if (o.stop_mask) o.stop_mask[d] = s(TK_WD_S_STOP);
        if (o.n_hash) o.n_hash[d] = s(TK_WD_S_HASH);
        if (o.n_ellipsis) o.n_ellipsis[d] = s(TK_WD_S_ELLIPSIS);
        if (o.n_lines) o.n_lines[d] = s(TK_WD_S_LINES);
        if (o.n_punct_lines) o.n_punct_lines[d] = s(TK_WD_S_PUNCT);
    }
}
