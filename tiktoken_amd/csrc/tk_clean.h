// Cleaning packed text line by line on the device: packed text (text, doc_off) in, packed text out without the lines that fail C4's line
// rules -- too few words, a word too long, no terminal punctuation at the end, an ellipsis at the end, a blocked phrase -- and without
// the documents that hold a blocked phrase; per document the lines each rule holds for.  C4's clean_page and DataTrove's C4QualityFilter
// on the text before it is encoded.  Nothing in the reference does this: it replaces a loop over text.split("\n") per document on the
// host.  The rule is stated in include/tiktoken_amd.h; its plain C++ -- the fold, the phrase table, the element of the scans, a line's
// verdict -- is tk_clean_rule.h's; the white-space masks are the word statistics' (tk_wd_lane_masks), the keep mask is the line sets'
// (tk_ls_keep_mask).
//
// A workgroup of TK_CL_THREADS lanes takes a tile of TK_CL_TILE bytes, a lane 16 of them by one 16-byte load (byte loads where the
// pointer is not aligned or the text ends).  The tile goes to LDS FOLDED (A-Z + 0x20: no white-space pattern and no '\n' holds a
// capital, so the word rule's look-around reads the same there; a lane's own 16 bytes stay raw in registers), with two bytes before
// it and TK_CL_HALO behind it, zeros past N; the document starts from 64 positions before the tile to 64 behind it -- found by two
// tk_last_le on doc_off -- into a bit per position.
// Phrases: the 32 slots (16 line, 16 document phrases) are kernel arguments, copied to LDS with two tables of 256 words made from them,
// m1[b]: the slots whose first byte is b, m2[b]: those whose second byte is b or that have one byte.  A lane tests its 16 start
// positions: the 256-bit set of first bytes rejects almost all, m1 & m2 nearly all of the rest, and only a slot that passes both is
// compared byte by byte in LDS, up to the document's end, which a 64-bit window of the start bits gives.
//   tk_k_cl_sum     per tile the element (TkClSt, 28 bytes) of the line open at its end: a segmented scan under tk_cl_join over the
//                   wavefront by __shfl_up and over the four wavefronts through LDS.  Line phrases are searched here too: the flag
//                   of a line that leaves the tile is part of the element.
//   tk_k_cl_carry   one workgroup of 1024: the same scan over the tiles' elements, a thread a stretch of tiles, in place: every tile
//                   gets the element that enters it.  A line or a word of many MiB costs this scan and no lane ever walks it.
//   tk_k_cl_decide  the tile again, with the document phrases.  A lane closes the lines that end in its bytes: bytes [start, cut) of
//                   the lane by shifts and popcounts, joined to the scanned element where no cut lies before; the verdict reads at
//                   most three bytes of the text.  A dropped line sets the bit of its START in a bitmap of a bit per position.  Sums
//                   and document-phrase bits go to the document's words in LDS (the first TK_CL_DOCS documents of a tile) or to HBM
//                   directly; at the end a lane per document flushes to HBM.
//   tk_k_cl_final   a thread per document: the sums -> the eight outputs, null ones skipped, n_kept closed against doc_hit; the lines
//                   that are not written are summed into a report word.
//   tk_k_cl_keep    (text out only, as the next two) the tile again: the start of the line that enters a lane is an exclusive
//                   max-scan begun with the start the carry pass left, so the drop bit of a long line is ONE read; the lane's keep
//                   mask is the line sets', less the bytes of documents whose doc_hit word is set; the popcounts give the tile's bytes.
//   tk_k_cl_scan    one workgroup of 1024 over the tiles' kept bytes, in place (tk_scan_blocks)
//   tk_k_cl_write   the masks again; kept bytes are compacted in LDS, shifted by the low four bits of the destination, so 16-byte words
//                   of LDS are 16-byte stores; doc_off_out[i] for every doc_off[i] in the tile; the last tile writes counts.
//   tk_k_cl_report  (counting only) counts = (0, lines not written)
// Sums, maxima and ORs commute: every value is a function of (text, doc_off, spec) alone.  No table in HBM, no host wait, no floating
// point; all stores are vector stores of plain C++.  No matrix instructions: there is no contraction here.  A doc_off that does not
// ascend cannot make an access leave the arrays: an entry of doc_off is only ever an index i <= n_docs found by tk_last_le, a bit
// position checked against the bitmap's size, or a tile position checked against the tile; what is written to text_out is a prefix sum
// of popcounts of bytes below N.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): see DESIGN.md.  Included by tk_api.hip only.
#pragma once
#include "tk_clean_rule.h"
#include "tk_scan.h"

#define TK_CL_NONE 0xFFFFFFFFu
#define TK_CL_HALO 32u                           // bytes behind the tile in LDS: a phrase that starts at the tile's last byte
#define TK_CL_BRK_WORDS (TK_CL_TILE / 64u + 2u)  // bit 64 + r: a document starts at the tile's position r, -64 <= r < T + 64
static_assert(TK_CL_TILE == TK_CL_THREADS * TK_CL_LANE && TK_CL_WAVE == 64u * TK_CL_LANE && TK_CL_TILE == 64u * 64u, "a lane 16 bytes, whole wavefronts, 64 words of bits");
static_assert(TK_CL_DOCS <= TK_CL_THREADS && TK_CL_SLOTS * (TK_CL_MAX_PHRASE_BYTES / 4) == TK_CL_THREADS, "a lane per gathered document and per word of the phrase table");
static_assert(TK_CL_MAX_BYTES + TK_CL_TILE <= 0xFFFFFFFFull && TK_CL_MAX_PHRASE_BYTES <= TK_CL_HALO + 1u, "positions of the last tile are 32-bit; a phrase ends in the halo");
static_assert(TK_CL_LANE == TK_WD_LANE && TK_CL_LANE == TK_LN_LANE, "the word rule's and the line sets' lane");

struct TkClOut {  // uint64[n_docs] each; any may be null
    unsigned long long *n_lines, *n_kept, *n_short, *n_long, *n_no_end, *n_ellipsis, *n_phrase, *doc_hit;
};

__device__ __forceinline__ TkClSt tk_cl_shfl_up(const TkClSt& v, int o) {
    return TkClSt{__shfl_up(v.start, o, 64), __shfl_up(v.words, o, 64), __shfl_up(v.longest, o, 64), __shfl_up(v.head, o, 64),
                  __shfl_up(v.open, o, 64),  __shfl_up(v.end, o, 64),   __shfl_up(v.flags, o, 64)};
}
// The exclusive scan under tk_cl_join over a workgroup of whole wavefronts (at most 16), `init` before the first lane; *total: `init`
// and every lane's value.  wsum: a slot per wavefront in LDS, free again when the call returns.
__device__ __forceinline__ TkClSt tk_cl_block_exscan(TkClSt v, const TkClSt& init, TkClSt* wsum, TkClSt* total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const TkClSt u = tk_cl_shfl_up(v, o);
        if ((int)lane >= o) v = tk_cl_join(u, v);
    }
    if (lane == 63u) wsum[wave] = v;
    TkClSt ex = tk_cl_shfl_up(v, 1);
    if (lane == 0) ex = tk_cl_empty();
    __syncthreads();
    TkClSt pre = init;
#pragma unroll 1
    for (uint32_t w = 0; w < n_waves; ++w) {
        if (w == wave) ex = tk_cl_join(pre, ex);
        if (w < wave || total) pre = tk_cl_join(pre, wsum[w]);
    }
    if (total) *total = pre;
    __syncthreads();
    return ex;
}

struct TkClShared {
    alignas(16) uint8_t txt[TK_CL_TILE + 64];  // txt[16 + i]: byte i of the tile, folded, -2 <= i < T + TK_CL_HALO; 0 outside the text
    unsigned long long brkw[TK_CL_BRK_WORDS];
    uint32_t brkpre[TK_CL_TILE / 64];  // the starts at the tile's positions before a word of 64 positions
    uint32_t m1[256], m2[256];         // bit s: slot s has the byte first / second (or no second byte)
    uint32_t ph[TK_CL_SLOTS][TK_CL_MAX_PHRASE_BYTES / 4];
    uint32_t first[8];
    uint8_t len[TK_CL_SLOTS];
    TkClSt wsum[4];
    uint32_t i0, i1;  // the entries of doc_off that can lie in [g0 - 2, g0 + T + 63]: [i0, i1]
};

// The tile of block t into LDS and the lane's view of it, lhit apart.  tables: the phrase tables too.  Every lane of the workgroup is here.
__device__ __forceinline__ TkClLane tk_cl_stage(const TkCl& q, const uint8_t* __restrict__ text, const uint64_t* __restrict__ doc_off, bool aligned, bool tables, TkClShared& sh) {
    const uint32_t tid = threadIdx.x, pos = tid * TK_CL_LANE;
    const uint64_t g0 = (uint64_t)blockIdx.x * TK_CL_TILE, N = q.n_bytes, at = g0 + pos;
    uint64_t lo = 0, hi = 0;
    if (aligned && at + TK_CL_LANE <= N) {
        const uint4 v = *(const uint4*)(text + at);
        lo = v.x | ((uint64_t)v.y << 32), hi = v.z | ((uint64_t)v.w << 32);
    } else {
        for (uint32_t j = 0; j < TK_CL_LANE && at + j < N; ++j) {
            const uint64_t b = text[at + j];
            if (j < 8) lo |= b << (8 * j);
            else hi |= b << (8 * (j - 8));
        }
    }
    const uint64_t flo = tk_cl_fold8(lo), fhi = tk_cl_fold8(hi);
    *(uint4*)(sh.txt + 16 + pos) = make_uint4((uint32_t)flo, (uint32_t)(flo >> 32), (uint32_t)fhi, (uint32_t)(fhi >> 32));
    if (tid < 2) sh.txt[14 + tid] = g0 + tid >= 2 ? (uint8_t)tk_cl_fold(text[g0 + tid - 2]) : 0;  // (g0 is 0 or at least T)
    if (tid >= TK_CL_THREADS - TK_CL_HALO) {
        const uint64_t p = g0 + TK_CL_TILE + (tid - (TK_CL_THREADS - TK_CL_HALO));
        sh.txt[16 + p - g0] = p < N ? (uint8_t)tk_cl_fold(text[p]) : 0;
    }
    if (tid < TK_CL_BRK_WORDS) sh.brkw[tid] = 0;
    if (tables) {
        (&sh.ph[0][0])[tid] = (&q.ph[0][0])[tid];
        if (tid < TK_CL_SLOTS) sh.len[tid] = q.len[tid];
        if (tid < 8) sh.first[tid] = q.first[tid];
        uint32_t a = 0, b = 0;
        for (uint32_t s = 0; s < TK_CL_SLOTS; ++s) {
            const uint32_t n = q.len[s];
            if (n && tk_cl_ph_byte(q.ph[s], 0) == tid) a |= 1u << s;
            if (n == 1u || (n && tk_cl_ph_byte(q.ph[s], 1) == tid)) b |= 1u << s;
        }
        sh.m1[tid] = a, sh.m2[tid] = b;
    }
    if (tid == 0) sh.i0 = (uint32_t)tk_last_le(doc_off, 0, q.n_docs + 1, g0 ? g0 - 2 : 0), sh.i1 = (uint32_t)tk_last_le(doc_off, 0, q.n_docs + 1, g0 + TK_CL_TILE + 63);
    __syncthreads();
    for (uint64_t i = (uint64_t)sh.i0 + tid; i <= sh.i1; i += TK_CL_THREADS) {
        const uint64_t r = doc_off[i] - g0 + 64;  // (wraps more than 64 below g0)
        if (r < 64ull * TK_CL_BRK_WORDS) atomicOr(&sh.brkw[r >> 6], 1ull << (r & 63u));
    }
    __syncthreads();
    if (tid < 64u) {
        const uint32_t c = (uint32_t)__popcll(sh.brkw[1 + tid]);
        sh.brkpre[tid] = tk_wave_scan_u32(c, (int)tid) - c;
    }
    __syncthreads();
    const uint32_t w = pos + 62u, s = w & 63u;  // bit 64 + pos - 2 and the 31 behind it; s is 62, 14, 30 or 46
    const uint32_t B = (uint32_t)((sh.brkw[w >> 6] >> s) | (sh.brkw[(w >> 6) + 1] << (64u - s)));
    const uint32_t n_left = at >= N ? 0u : N - at < 17u ? (uint32_t)(N - at) : 17u;
    const uint8_t* mine = sh.txt + 16 + pos;
    TkClLane L;
    tk_wd_lane_masks(
        lo, hi, n_left, B, mine[16], [&](int k) -> uint32_t { return mine[k]; }, [](uint32_t) -> bool { return false; }, &L.w);
    L.w.pos = pos;
    L.w.rank = sh.brkpre[pos >> 6] + (uint32_t)__popcll(sh.brkw[1 + (pos >> 6)] & ((1ull << (pos & 63u)) - 1ull));
    tk_cl_lane_masks((uint32_t)at, n_left, &L);
    return L;
}
// bit j: a line phrase occurs at byte j of the lane; on_doc(j, bits): the document phrases that occur there (slots & want, want 0xFFFF
// for the line phrases alone).  After tk_cl_stage with tables.
template <class OnDoc>
__device__ __forceinline__ uint32_t tk_cl_phrases(const TkCl& q, const TkClLane& L, const TkClShared& sh, uint32_t want, OnDoc&& on_doc) {
    if (!(want & ((q.n_line ? 0xFFFFu : 0u) | (q.n_doc ? 0xFFFF0000u : 0u))) || !L.valid) return 0;
    const uint32_t pos = L.w.pos, wi = (64u + pos) >> 6, ws = pos & 63u;  // bit k of W: a document starts at the lane's byte k
    const unsigned long long W = (sh.brkw[wi] >> ws) | (ws ? sh.brkw[wi + 1] << (64u - ws) : 0ull);
    const uint8_t* mine = sh.txt + 16 + pos;
    const uint64_t left = q.n_bytes - L.at;  // (valid: at < N)
    uint32_t lhit = 0;
#pragma unroll 1
    for (uint32_t m = L.valid; m; m &= m - 1u) {
        const uint32_t j = (uint32_t)__ffs((int)m) - 1u, b0 = mine[j];
        if (!((sh.first[b0 >> 5] >> (b0 & 31u)) & 1u)) continue;
        uint32_t cand = sh.m1[b0] & sh.m2[mine[j + 1]] & want, hit = 0;
        if (!cand) continue;
        const unsigned long long next = W >> (j + 1u);
        uint32_t room = next ? (uint32_t)__ffsll((long long)next) : 64u;  // bytes from here to the document's end
        if (left - j < room) room = (uint32_t)(left - j);
        for (; cand; cand &= cand - 1u) {
            const uint32_t i = (uint32_t)__ffs((int)cand) - 1u;
            if (tk_cl_occurs(sh.ph[i], sh.len[i], room, [&](uint32_t k) -> uint32_t { return mine[j + k]; })) hit |= 1u << i;
        }
        if (hit & 0xFFFFu) lhit |= 1u << j;
        if (hit >> 16) on_doc(j, hit >> 16);
    }
    return lhit;
}
// The documents of a tile by local index, after tk_cl_stage: index 0 owns the byte before the tile; index r > 0 is the non-empty document
// at the r-th start bit at or behind g0.  docid: TK_CL_DOCS words of LDS; a barrier before they are read.
__device__ __forceinline__ void tk_cl_local_docs(const TkCl& q, const uint64_t* __restrict__ doc_off, const TkClShared& sh, uint32_t* docid) {
    const uint32_t tid = threadIdx.x;
    const uint64_t g0 = (uint64_t)blockIdx.x * TK_CL_TILE;
    if (tid < TK_CL_DOCS) docid[tid] = tid == 0 && g0 && q.n_docs ? (uint32_t)tk_last_le(doc_off, 0, q.n_docs, g0 - 1) : TK_CL_NONE;
    __syncthreads();
    for (uint64_t i = (uint64_t)sh.i0 + tid; i <= sh.i1 && i < q.n_docs; i += TK_CL_THREADS) {
        const uint64_t s = doc_off[i], r = s - g0;
        if (r >= TK_CL_TILE || doc_off[i + 1] <= s) continue;
        const uint32_t li = sh.brkpre[r >> 6] + (uint32_t)__popcll(sh.brkw[1 + (r >> 6)] & ((2ull << (r & 63u)) - 1ull));
        if (li < TK_CL_DOCS) docid[li] = (uint32_t)i;
    }
}

__global__ __launch_bounds__(256) void tk_k_cl_clear(unsigned long long* a, uint64_t n) {
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) a[i] = 0;
}

__global__ __launch_bounds__(TK_CL_THREADS) void tk_k_cl_sum(TkCl q, const uint8_t* __restrict__ text, const uint64_t* __restrict__ doc_off, bool aligned,
                                                             TkClSt* __restrict__ tiles) {
    __shared__ TkClShared sh;
    TkClLane L = tk_cl_stage(q, text, doc_off, aligned, true, sh);
    L.lhit = tk_cl_phrases(q, L, sh, 0xFFFFu, [](uint32_t, uint32_t) {});
    TkClSt total;
    tk_cl_block_exscan(tk_cl_lane_tail(L), tk_cl_empty(), sh.wsum, &total);
    if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}

__global__ __launch_bounds__(1024) void tk_k_cl_carry(uint32_t n_tiles, TkClSt* __restrict__ tiles) {
    __shared__ TkClSt wsum[16];
    const uint32_t per = (n_tiles + 1023u) / 1024u;
    const uint64_t a = (uint64_t)threadIdx.x * per < n_tiles ? (uint64_t)threadIdx.x * per : n_tiles, b = a + per < n_tiles ? a + per : n_tiles;
    TkClSt mine = tk_cl_empty();
    for (uint64_t t = a; t < b; ++t) mine = tk_cl_join(mine, tiles[t]);
    TkClSt run = tk_cl_block_exscan(mine, tk_cl_empty(), wsum, nullptr);
    for (uint64_t t = a; t < b; ++t) {
        const TkClSt s = tiles[t];
        tiles[t] = run;
        run = tk_cl_join(run, s);
    }
}

__global__ __launch_bounds__(TK_CL_THREADS) void tk_k_cl_decide(TkCl q, const uint8_t* __restrict__ text, const uint64_t* __restrict__ doc_off, bool aligned,
                                                                const TkClSt* __restrict__ tiles, uint32_t* bitmap, unsigned long long* sums) {
    __shared__ TkClShared sh;
    __shared__ uint32_t docid[TK_CL_DOCS];            // the document of a local index; TK_CL_NONE
    __shared__ uint32_t acc[TK_CL_SUMS][TK_CL_DOCS];  // its sums of this tile
    const uint32_t tid = threadIdx.x;
    const uint64_t g0 = (uint64_t)blockIdx.x * TK_CL_TILE;
    TkClLane L = tk_cl_stage(q, text, doc_off, aligned, true, sh);
    for (uint32_t f = 0; f < TK_CL_SUMS; ++f)
        if (tid < TK_CL_DOCS) acc[f][tid] = 0;
    tk_cl_local_docs(q, doc_off, sh, docid);
    __syncthreads();
    // a document's sums: li its local index, pos a position it owns
    auto put = [&](uint32_t li, uint64_t pos, uint32_t f, uint32_t v) {
        if (li < TK_CL_DOCS) {
            f == TK_CL_S_HIT ? atomicOr(&acc[f][li], v) : atomicAdd(&acc[f][li], v);
        } else {
            const uint64_t d = tk_last_le(doc_off, 0, q.n_docs, pos);
            if (d >= q.n_docs) return;
            unsigned long long* const a = sums + (uint64_t)f * q.n_docs + d;
            f == TK_CL_S_HIT ? atomicOr(a, (unsigned long long)v) : atomicAdd(a, (unsigned long long)v);
        }
    };
    L.lhit = tk_cl_phrases(q, L, sh, 0xFFFFFFFFu, [&](uint32_t j, uint32_t bits) { put(L.w.doc(j), g0 + L.w.pos + j, TK_CL_S_HIT, bits); });
    const TkClSt before = tk_cl_block_exscan(tk_cl_lane_tail(L), tiles[blockIdx.x], sh.wsum, nullptr);
#pragma unroll 1
    for (uint32_t ev = tk_cl_closes(L, before); ev; ev &= ev - 1u) {
        const uint32_t j = (uint32_t)__ffs((int)ev) - 1u;
        const TkClSt line = tk_cl_line(L, before, j);
        const uint32_t r = tk_cl_judge(q, line, [&](uint32_t p) -> uint32_t { return text[p]; });  // (p < N: a byte of the line)
        const uint32_t li = L.w.doc_before(j);
        const uint64_t pos = g0 + L.w.pos + j - 1;  // the line's last byte
        put(li, pos, TK_CL_S_LINES, 1u);
        if (!r) continue;
        put(li, pos, TK_CL_S_DROPPED, 1u);
        if (r & TK_CL_R_SHORT) put(li, pos, TK_CL_S_SHORT, 1u);
        if (r & TK_CL_R_LONG) put(li, pos, TK_CL_S_LONG, 1u);
        if (r & TK_CL_R_NO_END) put(li, pos, TK_CL_S_NO_END, 1u);
        if (r & TK_CL_R_ELLIPSIS) put(li, pos, TK_CL_S_ELLIPSIS, 1u);
        if (r & TK_CL_R_PHRASE) put(li, pos, TK_CL_S_PHRASE, 1u);
        if (bitmap) atomicOr(bitmap + (line.start >> 5), 1u << (line.start & 31u));  // (start <= pos < N: inside the bitmap)
    }
    __syncthreads();
    if (tid < TK_CL_DOCS && docid[tid] != TK_CL_NONE) {
        const uint64_t d = docid[tid];
        for (uint32_t f = 0; f < TK_CL_SUMS; ++f) {
            const uint32_t v = acc[f][tid];
            unsigned long long* const a = sums + (uint64_t)f * q.n_docs + d;
            if (v) f == TK_CL_S_HIT ? atomicOr(a, (unsigned long long)v) : atomicAdd(a, (unsigned long long)v);
        }
    }
}

__global__ __launch_bounds__(256) void tk_k_cl_final(uint64_t n_docs, const unsigned long long* __restrict__ sums, TkClOut o, unsigned long long* words) {
    unsigned long long gone = 0;
    for (uint64_t d = blockIdx.x * 256ull + threadIdx.x; d < n_docs; d += (uint64_t)gridDim.x * 256) {
        auto s = [&](uint32_t f) { return sums[(uint64_t)f * n_docs + d]; };
        const unsigned long long kept = s(TK_CL_S_HIT) ? 0ull : s(TK_CL_S_LINES) - s(TK_CL_S_DROPPED);
        gone += s(TK_CL_S_LINES) - kept;
        if (o.n_lines) o.n_lines[d] = s(TK_CL_S_LINES);
        if (o.n_kept) o.n_kept[d] = kept;
        if (o.n_short) o.n_short[d] = s(TK_CL_S_SHORT);
        if (o.n_long) o.n_long[d] = s(TK_CL_S_LONG);
        if (o.n_no_end) o.n_no_end[d] = s(TK_CL_S_NO_END);
        if (o.n_ellipsis) o.n_ellipsis[d] = s(TK_CL_S_ELLIPSIS);
        if (o.n_phrase) o.n_phrase[d] = s(TK_CL_S_PHRASE);
        if (o.doc_hit) o.doc_hit[d] = s(TK_CL_S_HIT);
    }
    if (gone) atomicAdd(words, gone);
}
__global__ void tk_k_cl_report(const unsigned long long* __restrict__ words, unsigned long long* __restrict__ counts) { counts[0] = 0, counts[1] = words[0]; }

struct TkClKeep {  // what the keep and write passes share in LDS
    TkClShared sh;
    uint32_t docid[TK_CL_DOCS];
    uint8_t gone[TK_CL_DOCS];  // the document of a local index is dropped
    uint32_t wmax[4];
};
// The keep mask of the lane's 16 bytes (every lane of the workgroup is here).  hit: the documents' doc_hit words, null without document phrases.
__device__ __forceinline__ uint32_t tk_cl_lane_keep(const TkCl& q, const uint8_t* __restrict__ text, const uint64_t* __restrict__ doc_off, bool aligned,
                                                    const TkClSt* __restrict__ tiles, const uint32_t* __restrict__ bitmap, const unsigned long long* __restrict__ hit, TkClKeep& k,
                                                    TkClLane* lane) {
    const TkClLane L = tk_cl_stage(q, text, doc_off, aligned, false, k.sh);
    *lane = L;
    if (hit) {
        tk_cl_local_docs(q, doc_off, k.sh, k.docid);
        __syncthreads();
        if (threadIdx.x < TK_CL_DOCS) k.gone[threadIdx.x] = k.docid[threadIdx.x] != TK_CL_NONE && hit[k.docid[threadIdx.x]] != 0;
        __syncthreads();
    }
    uint32_t last;
    const uint32_t enters = tiles[blockIdx.x].start, own = tk_block_exmax32_256(tk_ls_open_start(L.lcut, L.lcontent, L.at), &last, k.wmax);
    uint32_t keep = tk_ls_keep_mask(L.valid, L.lcontent, L.lcut, L.w.brk, L.at, own > enters ? own : enters, [&](uint32_t s) { return (bitmap[s >> 5] >> (s & 31u)) & 1u; });
    if (hit)
        keep &= ~tk_cl_doc_mask(L.valid, L.w.brk, L.w.doc(0), [&](uint32_t li, uint32_t j) -> bool {
            if (li < TK_CL_DOCS) return k.gone[li];
            const uint64_t d = tk_last_le(doc_off, 0, q.n_docs, (uint64_t)L.at + j);
            return d < q.n_docs && hit[d] != 0;
        });
    return keep;
}

__global__ __launch_bounds__(TK_CL_THREADS) void tk_k_cl_keep(TkCl q, const uint8_t* __restrict__ text, const uint64_t* __restrict__ doc_off, bool aligned,
                                                              const TkClSt* __restrict__ tiles, const uint32_t* __restrict__ bitmap, const unsigned long long* __restrict__ hit,
                                                              uint32_t* __restrict__ kept) {
    __shared__ TkClKeep k;
    __shared__ uint32_t wsum[4];
    TkClLane L;
    const unsigned long long n = tk_block_sum_256((uint32_t)__popc(tk_cl_lane_keep(q, text, doc_off, aligned, tiles, bitmap, hit, k, &L)), wsum);
    if (threadIdx.x == 0) kept[blockIdx.x] = (uint32_t)n;
}

__global__ __launch_bounds__(1024) void tk_k_cl_scan(uint32_t* kept, uint64_t n_tiles) {
    __shared__ unsigned long long wsum[16];
    tk_scan_blocks<false>(kept, n_tiles, 0ull, wsum);
}

__global__ __launch_bounds__(TK_CL_THREADS) void tk_k_cl_write(TkCl q, const uint8_t* __restrict__ text, const uint64_t* __restrict__ doc_off, bool aligned,
                                                               const TkClSt* __restrict__ tiles, const uint32_t* __restrict__ bitmap, const unsigned long long* __restrict__ hit,
                                                               const uint32_t* __restrict__ base, const unsigned long long* __restrict__ words, uint8_t* __restrict__ text_out,
                                                               unsigned long long* __restrict__ doc_off_out, unsigned long long* __restrict__ counts) {
    __shared__ TkClKeep k;
    __shared__ alignas(16) uint8_t out[TK_CL_TILE + 32];  // the kept bytes, from out[shift]
    __shared__ uint32_t before_of[TK_CL_THREADS];         // the kept bytes of the lanes before a lane
    __shared__ uint16_t keep_of[TK_CL_THREADS];
    __shared__ uint32_t wsum[8];
    const uint32_t tid = threadIdx.x;
    const uint64_t g0 = (uint64_t)blockIdx.x * TK_CL_TILE;
    TkClLane L;
    const uint32_t keep = tk_cl_lane_keep(q, text, doc_off, aligned, tiles, bitmap, hit, k, &L);
    uint32_t total;
    const uint32_t ex = tk_block_exscan_256((uint32_t)__popc(keep), &total, wsum);
    const uint64_t dst = base[blockIdx.x];
    uint8_t* const g = text_out + dst;
    const uint32_t shift = (uint32_t)((uintptr_t)g & 15u), end = shift + total;
    before_of[tid] = ex, keep_of[tid] = (uint16_t)keep;
    {
        uint32_t o = shift + ex;
        for (uint32_t m = keep; m; m &= m - 1u) out[o++] = (uint8_t)L.w.byte((uint32_t)__ffs((int)m) - 1u);
    }
    __syncthreads();
    for (uint32_t lo = tid * 16u; lo < end; lo += TK_CL_THREADS * 16u) {  // out[lo .. lo + 16) is g[lo - shift ..): the same 16-byte word
        if (lo >= shift && lo + 16u <= end) {
            *(uint4*)(g + (lo - shift)) = *(const uint4*)(out + lo);
        } else {
            for (uint32_t i = lo < shift ? shift : lo; i < lo + 16u && i < end; ++i) g[i - shift] = out[i];
        }
    }
    // The entries of doc_off at the tile's positions, and at position T for the tile behind: the same value, that tile's `dst`.  The first
    // tile starts at entry 0: the empty documents at position 0 lie before the last entry that is <= 0.
    if (doc_off_out)
        for (uint64_t i = (blockIdx.x ? (uint64_t)k.sh.i0 : 0ull) + tid; i <= k.sh.i1; i += TK_CL_THREADS) {
            const uint64_t r = doc_off[i] - g0;  // (wraps below g0)
            if (r < TK_CL_TILE) doc_off_out[i] = dst + before_of[r >> 4] + (uint32_t)__popc(keep_of[r >> 4] & ((1u << (r & 15u)) - 1u));
            else if (r == TK_CL_TILE) doc_off_out[i] = dst + total;
        }
    if (blockIdx.x == gridDim.x - 1 && tid == 0 && counts) counts[0] = dst + total, counts[1] = words[0];
}
