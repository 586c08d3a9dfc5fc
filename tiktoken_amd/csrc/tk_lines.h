// Duplicate lines and paragraphs per document on the device: for every document of packed text (text, doc_off) its chars, its lines and
// paragraphs, how many of each repeat an earlier one of the same document and how many chars lie in those, and the lines that start with
// a bullet or end with an ellipsis -- the line-level half of the Gopher repetition rules, on the text before it is encoded.  Nothing in
// the reference does this: it replaces a Counter(text.split("\n")) per document on the host.  The rule is stated in
// include/tiktoken_amd.h; its plain C++ -- the monoid, the masks, the key -- is tk_lines_rule.h's.
//
// A workgroup of TK_LN_THREADS lanes takes a tile of TK_LN_TILE bytes, a lane 16 of them by one 16-byte load (byte loads where the
// pointer is not aligned or the text ends); the tile and one byte on each side go to LDS, the document starts that meet it -- found by
// two tk_last_le on doc_off -- into a bit per position.  A lane's newline, char, content and cut masks are SWAR words of 16 bits.
//   tk_k_ln_clear  words of scratch to 0 (the report words; then the sums and the table, in one launch)
//   tk_k_ln_sum    per tile and segmentation: the run that is open at the tile's end with whether a cut lies before it (a lane hashes
//                  the bytes behind its last cut, a segmented scan under tk_ln_seg_join runs over the wavefront by __shfl_up and over
//                  the four wavefronts through LDS), and the segments that end in the tile.  The open HEAD of a tile is not kept: the
//                  count pass meets it again as the bytes before its first cut.  Also: does doc_off ascend from 0 to N (a report word).
//   tk_k_ln_carry  one workgroup of 1024: the same scan over the tiles' summaries, a thread a stretch of tiles, in place: every tile
//                  gets the run that enters it.  A line of many MiB costs this scan -- one combine per tile it crosses -- and no lane
//                  ever walks it.  The segments of both kinds are summed into a report word: the host waits for it and sizes the table.
//   tk_k_ln_count  the tile again.  A lane whose bytes hold a cut walks up to its last cut: at a cut the run so far -- the scanned
//                  run that enters the lane, then the lane's own bytes -- is a finished segment of end - bytes .. end: its key goes into
//                  the table (64-bit compare-and-swap, linear probing: tk_ng_insert), a line's first and last three bytes are looked at
//                  (LDS inside the tile, HBM outside).  Counts, chars, and the counts and chars of the claims won go to the document's
//                  sums in LDS (the first TK_LN_DOCS documents of a tile; later ones add to HBM directly); at the end a lane per
//                  document flushes: a plain store when the document and its closing cut lie inside the tile, an atomic otherwise.
//   tk_k_ln_final  a thread per document: the sums -> the nine outputs, null ones skipped
// Sums and "did I claim the slot" commute: the members of a class have the same bytes, so whoever claims, the class gives the same
// chars.  All stores are vector stores of plain C++.  No matrix instructions and no floating point: there is no contraction here.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): see DESIGN.md.  Included by tk_api.hip only.
#pragma once
#include "tk_lines_rule.h"
#include "tk_ngram_rule.h"  // tk_ng_insert, tk_ng_popc
#include "tk_scan.h"

#define TK_LN_NONE 0xFFFFFFFFu
static_assert(TK_LN_TILE == TK_LN_THREADS * TK_LN_LANE && TK_LN_WAVE == 64u * TK_LN_LANE && TK_LN_TILE % 64u == 0, "a lane 16 bytes, whole wavefronts, whole words of bits");
static_assert(TK_LN_DOCS <= TK_LN_THREADS, "a lane per gathered document at the flush");
static_assert(TK_LN_MAX_BYTES + TK_LN_TILE <= 0xFFFFFFFFull, "positions of the last tile are 32-bit");

struct TkLnTiles {       // [2][n_tiles], the line kind first
    TkLnSeg* seg;        // tk_k_ln_sum: the tile's summary; tk_k_ln_carry, in place: the run that enters the tile
    uint32_t* nseg;      // 2 (segments whose cut is behind the tile's first position) + (the first position is a cut)
};
struct TkLnOut {  // uint64[n_docs] each; any may be null
    unsigned long long *n_chars, *n_lines, *n_dup_lines, *dup_line_chars, *n_paragraphs, *n_dup_paragraphs, *dup_paragraph_chars, *n_bullet, *n_ellipsis;
};

__device__ __forceinline__ TkLnSeg tk_ln_shfl_up(const TkLnSeg& v, int o) {
    return TkLnSeg{TkLnEl{__shfl_up((unsigned long long)v.e.h1, o, 64), __shfl_up((unsigned long long)v.e.w1, o, 64), __shfl_up((unsigned long long)v.e.h2, o, 64),
                          __shfl_up((unsigned long long)v.e.w2, o, 64), __shfl_up(v.e.bytes, o, 64), __shfl_up(v.e.chars, o, 64)},
                   __shfl_up(v.cut, o, 64)};
}
__device__ __forceinline__ TkLnNSeg tk_ln_shfl_up(const TkLnNSeg& v, int o) {
    return TkLnNSeg{TkLnNEl{__shfl_up((unsigned long long)v.e.h1, o, 64), __shfl_up((unsigned long long)v.e.w1, o, 64), __shfl_up((unsigned long long)v.e.h2, o, 64),
                            __shfl_up((unsigned long long)v.e.w2, o, 64), __shfl_up(v.e.bytes, o, 64), __shfl_up(v.e.len, o, 64)},
                    __shfl_up(v.cut, o, 64)};
}
// The exclusive scan under m.join over a workgroup of whole wavefronts (at most 16), `init` before the first lane; *total: `init` and
// every lane's value.  wsum: a slot per wavefront in LDS, free again when the call returns.  m: TkLnRaw or TkLnNorm, below.
template <class M>
__device__ __forceinline__ typename M::Seg tk_ln_block_exscan(const M& m, typename M::Seg v, const typename M::Seg& init, typename M::Seg* wsum, typename M::Seg* total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
#pragma unroll 1
    for (int o = 1; o < 64; o <<= 1) {
        const typename M::Seg u = tk_ln_shfl_up(v, o);
        if ((int)lane >= o) v = m.join(u, v);
    }
    if (lane == 63u) wsum[wave] = v;
    typename M::Seg ex = tk_ln_shfl_up(v, 1);
    if (lane == 0) ex = M::empty();
    __syncthreads();
    typename M::Seg pre = init;
#pragma unroll 1
    for (uint32_t w = 0; w < n_waves; ++w) {
        if (w == wave) ex = m.join(pre, ex);
        if (w < wave || total) pre = m.join(pre, wsum[w]);
    }
    if (total) *total = pre;
    __syncthreads();
    return ex;
}

struct TkLnLane {  // what a lane knows of its 16 bytes
    uint64_t lo, hi;
    uint32_t pos;          // of its first byte, from the tile's start
    uint32_t brk;          // bit j: a document starts at byte j; 17 bits
    uint32_t rank;         // document starts at the tile's positions before the lane
    uint32_t chm;          // bit j: byte j is a char of the text
    uint32_t content0, content1, cut0, cut1;  // of the two kinds; read through the selects below: an index would put the lane's view into scratch
    __device__ __forceinline__ uint32_t content(uint32_t kind) const { return kind ? content1 : content0; }
    __device__ __forceinline__ uint32_t cut(uint32_t kind) const { return kind ? cut1 : cut0; }
    __device__ __forceinline__ uint32_t byte(uint32_t j) const { return (uint32_t)((j < 8 ? lo >> (8 * j) : hi >> (8 * (j - 8))) & 0xFFu); }
    __device__ __forceinline__ uint32_t doc(uint32_t j) const { return rank + (uint32_t)__popc(brk & ((2u << j) - 1u)); }  // the local document of byte j
};
struct TkLnShared {
    alignas(16) uint8_t txt[TK_LN_TILE + 32];  // txt[16 + i]: byte i of the tile; txt[15] and txt[16 + T]: the bytes beside it, 0 outside the text
    unsigned long long brkw[TK_LN_TILE / 64 + 1];  // bit i: a document starts at the tile's position i, i <= T
    uint32_t brkpre[TK_LN_TILE / 64];              // the bits of the words before a word
    uint64_t pw[2][TK_LN_LANE + 1];                // B1^i, B2^i
    union {  // a kernel scans one kind of value
        TkLnSeg wsum[4];
        TkLnNSeg nwsum[4];
    };
    uint32_t i0, i1;  // the entries of doc_off that can lie in [g0, g0 + T]: [i0, i1]
};

// The tile of block t into LDS and the lane's view of it.  Every lane of the workgroup is here.
__device__ __forceinline__ TkLnLane tk_ln_stage(const TkLn& p, const uint8_t* __restrict__ text, const uint64_t* __restrict__ doc_off, bool aligned, TkLnShared& sh) {
    const uint32_t tid = threadIdx.x;
    const uint64_t g0 = (uint64_t)blockIdx.x * TK_LN_TILE, N = p.n_bytes;
    TkLnLane L;
    L.pos = tid * TK_LN_LANE;
    const uint64_t at = g0 + L.pos;
    L.lo = L.hi = 0;
    if (aligned && at + TK_LN_LANE <= N) {
        const uint4 v = *(const uint4*)(text + at);
        L.lo = v.x | ((uint64_t)v.y << 32), L.hi = v.z | ((uint64_t)v.w << 32);
    } else {
        for (uint32_t j = 0; j < TK_LN_LANE && at + j < N; ++j) {
            const uint64_t b = text[at + j];
            if (j < 8) L.lo |= b << (8 * j);
            else L.hi |= b << (8 * (j - 8));
        }
    }
    *(uint4*)(sh.txt + 16 + L.pos) = make_uint4((uint32_t)L.lo, (uint32_t)(L.lo >> 32), (uint32_t)L.hi, (uint32_t)(L.hi >> 32));
    if (tid == 0) sh.txt[15] = g0 ? text[g0 - 1] : 0;
    if (tid == TK_LN_THREADS - 1) sh.txt[16 + TK_LN_TILE] = g0 + TK_LN_TILE < N ? text[g0 + TK_LN_TILE] : 0;
    if (tid <= TK_LN_TILE / 64) sh.brkw[tid] = 0;
    if (tid <= TK_LN_LANE) {
        uint64_t a = 1, b = 1;
        for (uint32_t i = 0; i < tid; ++i) a = tk_ln_mulmod(a, p.B1), b = tk_ln_mulmod(b, p.B2);
        sh.pw[0][tid] = a, sh.pw[1][tid] = b;
    }
    if (tid == 0) sh.i0 = (uint32_t)tk_last_le(doc_off, 0, p.n_docs + 1, g0), sh.i1 = (uint32_t)tk_last_le(doc_off, 0, p.n_docs + 1, g0 + TK_LN_TILE);
    __syncthreads();
    for (uint64_t i = (uint64_t)sh.i0 + tid; i <= sh.i1; i += TK_LN_THREADS) {
        const uint64_t r = doc_off[i] - g0;  // (wraps below g0)
        if (r <= TK_LN_TILE) atomicOr(&sh.brkw[r >> 6], 1ull << (r & 63u));
    }
    __syncthreads();
    if (tid < 64u) {
        const uint32_t c = (uint32_t)__popcll(sh.brkw[tid]);
        sh.brkpre[tid] = tk_wave_scan_u32(c, (int)tid) - c;
    }
    __syncthreads();
    const uint32_t w = L.pos >> 6, s = L.pos & 63u, e = L.pos + TK_LN_LANE;
    const unsigned long long word = sh.brkw[w];
    L.brk = (uint32_t)((word >> s) & 0xFFFFu) | ((uint32_t)((sh.brkw[e >> 6] >> (e & 63u)) & 1u) << 16);
    L.rank = sh.brkpre[w] + (uint32_t)__popcll(word & ((1ull << s) - 1ull));
    const uint32_t n_valid = at >= N ? 0u : N - at < TK_LN_LANE ? (uint32_t)(N - at) : TK_LN_LANE, valid = (1u << n_valid) - 1u;
    const uint32_t nl = tk_ln_eq_mask(L.lo, L.hi, '\n') & valid;
    L.chm = ~tk_ln_cont_mask(L.lo, L.hi) & valid;
    uint32_t content[2], cut[2];
    tk_ln_masks(nl, valid, L.brk, sh.txt[15 + L.pos] == '\n', sh.txt[16 + e] == '\n', content, cut);
    L.content0 = content[0], L.content1 = content[1], L.cut0 = cut[0], L.cut1 = cut[1];
    return L;
}
// The run behind the lane's last cut (all of its bytes where it has none), with its powers
__device__ __forceinline__ TkLnSeg tk_ln_lane_tail(const TkLn& p, const TkLnLane& L, uint32_t kind, const TkLnShared& sh) {
    const uint32_t cut = L.cut(kind);
    uint32_t from = 0;
    if (cut) {
        const uint32_t l = 31u - (uint32_t)__clz((int)cut);
        from = l + (((L.content(kind) >> l) & 1u) ^ 1u);  // (a cut by a document start: its byte opens the run)
    }
    TkLnEl e = tk_ln_empty();
#pragma unroll 1
    for (uint32_t j = from; j < TK_LN_LANE; ++j) tk_ln_push(p, e, L.byte(j));
    e.w1 = sh.pw[0][e.bytes], e.w2 = sh.pw[1][e.bytes];
    return TkLnSeg{e, cut ? 1u : 0u};
}

// What the kernels that hash are instantiated over: the value their scans carry, and a lane's bytes as that value sees them.
//   TkLnRaw   the bytes as they are: every kernel of the line statistics, and the line sets with a mask of 0
//   TkLnNorm  the normal form under p.norm (tk_lines_rule.h): the line sets made with a mask.  A lane's classes are SWAR words built once
//             per 16 bytes, case and digits are mapped in the words, and the walk visits only the bytes that are not deleted: a lane of
//             plain lower-case text does the two multiplies per byte of TkLnRaw, a lane of deleted bytes none.
struct TkLnRaw {
    using Seg = TkLnSeg;
    __device__ __forceinline__ TkLnRaw() {}
    __device__ __forceinline__ explicit TkLnRaw(const TkLn&) {}  // (its join needs nothing of the call)
    static __device__ __forceinline__ Seg empty() { return TkLnSeg{tk_ln_empty(), 0u}; }
    static __device__ __forceinline__ Seg enters(const TkLnTiles& T, uint64_t at) { return TkLnSeg{T.seg[at].e, 0u}; }  // the carried run: no cut lies in it
    static __device__ __forceinline__ Seg* tiles(const TkLnTiles& T) { return T.seg; }
    static __device__ __forceinline__ Seg* wsum(TkLnShared& sh) { return sh.wsum; }
    __device__ __forceinline__ Seg join(const Seg& l, const Seg& r) const { return tk_ln_seg_join(l, r); }
    struct View {
        const TkLn& p;
        const TkLnLane& L;
        __device__ __forceinline__ View(const TkLn& p_, const TkLnLane& L_) : p(p_), L(L_) {}
        __device__ __forceinline__ Seg tail(uint32_t kind, const TkLnShared& sh) const { return tk_ln_lane_tail(p, L, kind, sh); }
        __device__ __forceinline__ void push(Seg& run, uint32_t j) const { tk_ln_push(p, run.e, L.byte(j)); }
    };
};
struct TkLnNorm {
    using Seg = TkLnNSeg;
    const TkLn& p;
    __device__ __forceinline__ explicit TkLnNorm(const TkLn& p_) : p(p_) {}
    static __device__ __forceinline__ Seg empty() { return tk_lnn_empty(); }
    static __device__ __forceinline__ Seg* tiles(const TkLnTiles& T) { return reinterpret_cast<TkLnNSeg*>(T.seg); }  // (one size, one place for the raw count)
    static __device__ __forceinline__ Seg enters(const TkLnTiles& T, uint64_t at) {
        Seg s = tiles(T)[at];
        s.cut &= ~TK_LN_NF_CUT;
        return s;
    }
    static __device__ __forceinline__ Seg* wsum(TkLnShared& sh) { return sh.nwsum; }
    __device__ __forceinline__ Seg join(const Seg& l, const Seg& r) const { return tk_lnn_seg_join(p, l, r); }
    struct View {
        const TkLn& p;
        const TkLnLane& L;
        const TkLnNLane c;
        __device__ __forceinline__ View(const TkLn& p_, const TkLnLane& L_) : p(p_), L(L_), c(tk_lnn_lane(L_.lo, L_.hi, p_.norm)) {}
        // the run behind the lane's last cut, with its powers: tk_ln_lane_tail over the normal form
        __device__ __forceinline__ Seg tail(uint32_t kind, const TkLnShared& sh) const {
            const uint32_t cut = L.cut(kind);
            uint32_t from = 0;
            if (cut) {
                const uint32_t l = 31u - (uint32_t)__clz((int)cut);
                from = l + (((L.content(kind) >> l) & 1u) ^ 1u);
            }
            Seg s = tk_lnn_empty();
            tk_lnn_append(p, c, from, TK_LN_LANE, s);
            s.e.w1 = sh.pw[0][s.e.len], s.e.w2 = sh.pw[1][s.e.len];  // (a body is no longer than the bytes it came from)
            s.cut |= cut ? TK_LN_NF_CUT : 0u;
            return s;
        }
        __device__ __forceinline__ void push(Seg& run, uint32_t j) const { tk_lnn_append(p, c, j, j + 1u, run); }
    };
};
__device__ __forceinline__ TkLnSeg tk_ln_block_exscan(TkLnSeg v, const TkLnSeg& init, TkLnSeg* wsum, TkLnSeg* total) {
    return tk_ln_block_exscan(TkLnRaw(), v, init, wsum, total);
}

__global__ __launch_bounds__(256) void tk_k_ln_clear(unsigned long long* a, uint64_t n) {
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) a[i] = 0;
}

// (KINDS: 2, or 1 for the line kind alone -- tk_line_set.h; the same for tk_k_ln_carry, whose report word then counts lines.  M: what is
// hashed, TkLnRaw or TkLnNorm; the lines counted are the raw ones under either)
template <uint32_t KINDS, class M = TkLnRaw>
__global__ __launch_bounds__(TK_LN_THREADS) void tk_k_ln_sum(TkLn p, const uint8_t* __restrict__ text, const uint64_t* __restrict__ doc_off, bool aligned, TkLnTiles T,
                                                             unsigned long long* __restrict__ words) {
    __shared__ TkLnShared sh;
    __shared__ uint8_t last[TK_LN_THREADS];  // bit kind: the lane's last byte is content
    __shared__ uint32_t cnt[2];
    const uint32_t tid = threadIdx.x;
    {  // does doc_off ascend from 0 to N?
        bool bad = false;
        for (uint64_t d = (uint64_t)blockIdx.x * TK_LN_THREADS + tid; d < p.n_docs; d += (uint64_t)gridDim.x * TK_LN_THREADS) bad |= doc_off[d + 1] < doc_off[d];
        if (blockIdx.x == 0 && tid == 0) bad |= doc_off[0] != 0 || doc_off[p.n_docs] != p.n_bytes;
        if (bad) atomicOr(words + TK_LN_W_BAD, 1ull);
    }
    const TkLnLane L = tk_ln_stage(p, text, doc_off, aligned, sh);
    last[tid] = (uint8_t)(((L.content0 >> 15) & 1u) | (((L.content1 >> 15) & 1u) << 1));
    if (tid < 2) cnt[tid] = 0;
    __syncthreads();
    const uint32_t before = tid ? last[tid - 1] : 0u;
    const M m(p);
    const typename M::View view(p, L);
#pragma unroll 1
    for (uint32_t kind = 0; kind < KINDS; ++kind) {
        typename M::Seg total;
        tk_ln_block_exscan(m, view.tail(kind, sh), M::empty(), M::wsum(sh), &total);
        const uint32_t n = tk_wave_sum_u32((uint32_t)__popc(L.cut(kind) & ((L.content(kind) << 1) | ((before >> kind) & 1u))));
        if ((tid & 63u) == 0 && n) atomicAdd(&cnt[kind], n);
        __syncthreads();
        if (tid == 0) {
            const uint64_t at = (uint64_t)kind * p.n_tiles + blockIdx.x;
            M::tiles(T)[at] = total;
            T.nseg[at] = 2u * cnt[kind] + (L.cut(kind) & 1u);
        }
    }
}

template <uint32_t KINDS, class M = TkLnRaw>
__global__ __launch_bounds__(1024) void tk_k_ln_carry(TkLn p, TkLnTiles T, unsigned long long* __restrict__ words) {
    using Seg = typename M::Seg;
    __shared__ Seg wsum[16];
    const M m(p);
    const uint32_t per = (p.n_tiles + 1023u) / 1024u;
    const uint64_t a = (uint64_t)threadIdx.x * per, b = a + per < p.n_tiles ? a + per : p.n_tiles;
    unsigned long long segs = 0;
#pragma unroll 1
    for (uint32_t kind = 0; kind < KINDS; ++kind) {
        Seg* seg = M::tiles(T) + (uint64_t)kind * p.n_tiles;
        const uint32_t* nseg = T.nseg + (uint64_t)kind * p.n_tiles;
        Seg mine = M::empty();
        for (uint64_t t = a; t < b; ++t) mine = m.join(mine, seg[t]);
        Seg run = tk_ln_block_exscan(m, mine, M::empty(), wsum, (Seg*)nullptr);
        for (uint64_t t = a; t < b; ++t) {
            const Seg s = seg[t];
            segs += (nseg[t] >> 1) + ((nseg[t] & 1u) && run.e.bytes ? 1u : 0u);
            seg[t] = run;
            run = m.join(run, s);
        }
    }
    if (segs) atomicAdd(words + TK_LN_W_SEGS, segs);
}

__global__ __launch_bounds__(TK_LN_THREADS) void tk_k_ln_count(TkLn p, const uint8_t* __restrict__ text, const uint64_t* __restrict__ doc_off, bool aligned, TkLnTiles T,
                                                               unsigned long long* table, uint64_t S, unsigned long long* sums) {
    __shared__ TkLnShared sh;
    __shared__ uint32_t docid[TK_LN_DOCS];             // the document of a local index; TK_LN_NONE
    __shared__ uint32_t acc[TK_LN_SUMS][TK_LN_DOCS];  // its sums of this tile
    const uint32_t tid = threadIdx.x;
    const uint64_t g0 = (uint64_t)blockIdx.x * TK_LN_TILE;
    const TkLnLane L = tk_ln_stage(p, text, doc_off, aligned, sh);
    // Local documents: index 0 owns the byte before the tile; index r > 0 is the non-empty document at the r-th start bit.
    if (tid < TK_LN_DOCS) docid[tid] = tid == 0 && g0 && p.n_docs ? (uint32_t)tk_last_le(doc_off, 0, p.n_docs, g0 - 1) : TK_LN_NONE;
    for (uint32_t f = 0; f < TK_LN_SUMS; ++f)
        if (tid < TK_LN_DOCS) acc[f][tid] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)sh.i0 + tid; i <= sh.i1 && i < p.n_docs; i += TK_LN_THREADS) {
        const uint64_t s = doc_off[i], r = s - g0;
        if (r >= TK_LN_TILE || doc_off[i + 1] <= s) continue;
        const uint32_t li = sh.brkpre[r >> 6] + (uint32_t)__popcll(sh.brkw[r >> 6] & ((2ull << (r & 63u)) - 1ull));
        if (li < TK_LN_DOCS) docid[li] = (uint32_t)i;
    }
    __syncthreads();
    auto doc_of = [&](uint32_t li, uint64_t pos) { return li < TK_LN_DOCS ? (uint64_t)docid[li] : tk_last_le(doc_off, 0, p.n_docs, pos); };
    auto add = [&](uint32_t li, uint64_t d, uint32_t f, uint32_t v) {
        if (li < TK_LN_DOCS) atomicAdd(&acc[f][li], v);
        else atomicAdd(sums + (uint64_t)f * p.n_docs + d, (unsigned long long)v);
    };
    {  // chars, per document that owns bytes of the lane; one add per wavefront where it lies inside one document
        const uint32_t li0 = L.doc(0);
        if (__all(!(L.brk & 0xFFFEu) && li0 == __shfl(li0, 0, 64))) {
            const uint32_t n = tk_wave_sum_u32((uint32_t)__popc(L.chm));
            if ((tid & 63u) == 0 && n) add(li0, doc_of(li0, g0 + L.pos), TK_LN_S_CHARS, n);
        } else {
            uint32_t rest = L.brk & 0xFFFEu, from = 0, li = li0;
            while (true) {
                const uint32_t to = rest ? (uint32_t)__ffs((int)rest) - 1u : TK_LN_LANE, n = (uint32_t)__popc(L.chm & ((1u << to) - 1u) & ~((1u << from) - 1u));
                if (n) add(li, doc_of(li, g0 + L.pos + from), TK_LN_S_CHARS, n);
                if (!rest) break;
                rest &= rest - 1u, from = to, ++li;
            }
        }
    }
#pragma unroll 1
    for (uint32_t kind = 0; kind < 2; ++kind) {
        const TkLnSeg enter{T.seg[(uint64_t)kind * p.n_tiles + blockIdx.x].e, 0u};
        const TkLnSeg before = tk_ln_block_exscan(tk_ln_lane_tail(p, L, kind, sh), enter, sh.wsum, nullptr);
        const uint32_t cut = L.cut(kind), cont = L.content(kind);
        if (!cut) continue;
        const uint32_t l = 31u - (uint32_t)__clz((int)cut);
        TkLnEl run = before.e;
#pragma unroll 1
        for (uint32_t j = 0; j <= l; ++j) {
            if (((cut >> j) & 1u) && run.bytes) {  // a finished segment: [end - bytes, end)
                const uint64_t end = g0 + L.pos + j, start = end - run.bytes;
                const uint32_t li = L.rank + (uint32_t)__popc(L.brk & ((1u << j) - 1u)), base = TK_LN_S_SEG + 4u * kind;
                const uint64_t d = doc_of(li, end - 1);
                const bool won = tk_ng_insert(table, S, tk_ln_key(p, kind, d, run), [&](uint64_t i, uint64_t k) { return (uint64_t)atomicCAS(table + i, 0ull, (unsigned long long)k); });
                add(li, d, base, 1u), add(li, d, base + 1u, run.chars);
                if (won) add(li, d, base + 2u, 1u), add(li, d, base + 3u, run.chars);
                if (kind == TK_LN_LINE) {
                    auto at = [&](uint32_t i) -> uint32_t {
                        const uint64_t q = start + i, r = q + 1 - g0;  // (r wraps for a byte two or more before the tile)
                        return r <= TK_LN_TILE + 1u ? sh.txt[15 + r] : text[q];
                    };
                    if (tk_ln_bullet(run.bytes, at)) add(li, d, TK_LN_S_BULLET, 1u);
                    if (tk_ln_ellipsis(run.bytes, at)) add(li, d, TK_LN_S_ELLIPSIS, 1u);
                }
            }
            if ((cut >> j) & 1u) run = tk_ln_empty();
            if (j < l && ((cont >> j) & 1u)) tk_ln_push(p, run, L.byte(j));
        }
    }
    __syncthreads();
    if (tid < TK_LN_DOCS && docid[tid] != TK_LN_NONE) {
        const uint64_t d = docid[tid];
        const bool whole = tid > 0 && doc_off[d + 1] < g0 + TK_LN_TILE;  // (it starts in the tile, and the cut that closes it lies there too)
        for (uint32_t f = 0; f < TK_LN_SUMS; ++f) {
            const uint32_t v = acc[f][tid];
            if (whole) sums[(uint64_t)f * p.n_docs + d] = v;
            else if (v) atomicAdd(sums + (uint64_t)f * p.n_docs + d, (unsigned long long)v);
        }
    }
}

__global__ __launch_bounds__(256) void tk_k_ln_final(uint64_t n_docs, const unsigned long long* __restrict__ sums, TkLnOut o) {
    for (uint64_t d = blockIdx.x * 256ull + threadIdx.x; d < n_docs; d += (uint64_t)gridDim.x * 256) {
        auto s = [&](uint32_t f) { return sums[(uint64_t)f * n_docs + d]; };
        if (o.n_chars) o.n_chars[d] = s(TK_LN_S_CHARS);
        if (o.n_lines) o.n_lines[d] = s(TK_LN_S_SEG);
        if (o.n_dup_lines) o.n_dup_lines[d] = s(TK_LN_S_SEG) - s(TK_LN_S_DIST);
        if (o.dup_line_chars) o.dup_line_chars[d] = s(TK_LN_S_SEGCH) - s(TK_LN_S_DISTCH);
        if (o.n_paragraphs) o.n_paragraphs[d] = s(TK_LN_S_SEG + 4);
        if (o.n_dup_paragraphs) o.n_dup_paragraphs[d] = s(TK_LN_S_SEG + 4) - s(TK_LN_S_DIST + 4);
        if (o.dup_paragraph_chars) o.dup_paragraph_chars[d] = s(TK_LN_S_SEGCH + 4) - s(TK_LN_S_DISTCH + 4);
        if (o.n_bullet) o.n_bullet[d] = s(TK_LN_S_BULLET);
        if (o.n_ellipsis) o.n_ellipsis[d] = s(TK_LN_S_ELLIPSIS);
    }
}
