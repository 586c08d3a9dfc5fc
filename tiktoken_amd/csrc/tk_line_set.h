// Line sets on the device: a set of line keys that lives in device memory across calls, and the pass that rewrites packed text
// (text, doc_off) without the lines the set has seen -- in an earlier call, in an earlier document, or earlier in the same document:
// the line filter of CCNet-, C4- and RefinedWeb-style corpus builds.  Nothing in the reference does this: it replaces a loop over
// text.split("\n") against a Python set on the host.  The rule is stated in include/tiktoken_amd.h; its plain C++ -- the key, the
// first-occurrence word, the keep mask of a lane -- is tk_line_set_rule.h's.
//
// The tile, the lane's view of it, the hash of a run and the scan that hands every lane the run that enters it are the line
// statistics' (tk_lines.h: tk_ln_stage, tk_ln_lane_tail, tk_ln_block_exscan, and its sum and carry kernels over the line kind alone).
// Behind the carry pass and the host's one wait for the report words (doc_off ascends from 0 to N; the lines of the batch, for the
// capacity check):
//   tk_k_ls_clear   a set's table: keys 0, first words all ones, the counter 0 (at creation and tk_line_set_clear, never per call)
//   tk_k_ls_mark    adds only.  The tile again: the lane whose 16 bytes hold a line's closing cut has the finished run, as in
//                   tk_k_ln_count.  Its key goes into the table (64-bit compare-and-swap, linear probing: tk_ng_insert; a claim raises
//                   the set's counter, once per wavefront), then an atomic minimum of (epoch << 32) | start on the slot's first word.
//   tk_k_ls_decide  the tile again, behind the launch boundary.  The same lane finds its key's slot.  Adding: the line is dropped when
//                   the first word is not (epoch, its start) -- the key is older than this call, or a lower start of this call has it.
//                   Not adding: dropped when the key is there.  A dropped line sets the bit of its START in a bitmap of a bit per
//                   position (32-bit atomic or).  Lines and dropped lines per document are gathered in LDS and flushed as
//                   tk_k_ln_count flushes: a plain store when the document lies inside the tile, an atomic otherwise.
//   tk_k_ls_keep    the tile again.  Only lengths matter now: where the run that is open at a lane's end starts is a maximum, so the
//                   start of the run that enters a lane is an exclusive max-scan (tk_block_exmax32_256) begun with the start of the run
//                   that enters the tile, g0 - its bytes, which the carry pass left.  The drop bit of a line that began many tiles
//                   earlier is therefore ONE bitmap read and no walk.  A lane builds its 16-bit keep mask (tk_ls_keep_mask); the
//                   popcounts are summed to the tile's kept bytes.
//   tk_k_ls_scan    one workgroup of 1024 over the tiles' kept bytes, in place: where a tile's bytes go (tk_scan_blocks; no look-back)
//   tk_k_ls_write   the masks again; a lane puts its kept bytes into LDS behind those of the lanes before it, shifted by the low four
//                   bits of the destination, so that 16-byte words of LDS are 16-byte words of the output: vector stores inside, byte
//                   stores at the ragged ends.  A tile from which nothing is dropped is a shifted copy.  For every doc_off[i] in the
//                   tile -- the entries tk_ln_stage has found, empty documents included -- doc_off_out[i] is the kept bytes before
//                   it.  The last tile writes counts.
// Normalising sets (a `normalize` mask, fixed at creation).  tk_k_ln_sum<1>, tk_k_ln_carry<1>, tk_k_ls_mark and tk_k_ls_decide are
// templates over what is hashed: TkLnRaw, the line's bytes, or TkLnNorm, its normal form (tk_lines.h; the value and its join:
// tk_lines_rule.h).  The host chooses from the set's mask, and a set with a mask of 0 launches what it always launched.  Under
// TkLnNorm the key and the eligibility are the normal form's; a line's start, its drop bit, the counts and the capacity stay raw, and
// tk_k_ls_keep, tk_k_ls_scan and tk_k_ls_write, which never hash, are the same kernels: the raw count of the run that enters a tile
// lies at one place in either scan value.
// The text is read five times when adding (four when not) and written once.  All stores are vector stores of plain C++.  No matrix
// instructions and no floating point: there is no contraction here.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): see DESIGN.md.  Included by tk_api.hip only.
#pragma once
#include "tk_line_set_rule.h"
#include "tk_lines.h"

struct TkLsTab {  // a set's table in device memory
    unsigned long long *key, *first;  // [S] each
    unsigned long long* count;        // claims since the last clear
};
struct TkLsKeys {  // the keys as the other workgroups' compare-and-swaps have left them: loads that pass the CU's own cache
    const unsigned long long* key;
    __device__ __forceinline__ uint64_t operator[](uint64_t i) const { return __hip_atomic_load(key + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

__global__ __launch_bounds__(256) void tk_k_ls_clear(TkLsTab tab, uint64_t S) {
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < S; i += (uint64_t)gridDim.x * 256) tab.key[i] = 0, tab.first[i] = TK_LS_FRESH;
    if (blockIdx.x == 0 && threadIdx.x == 0) *tab.count = 0;
}

// The finished lines of a lane: f(j, start, run) at every cut j of the lane that closes a run -- `before`: the scanned run that enters
// the lane --, start its first position.  The walk of tk_k_ln_count over the line kind.
template <class M, class F>
__device__ __forceinline__ void tk_ls_each_line(const typename M::View& view, const typename M::Seg& before, F&& f) {
    const TkLnLane& L = view.L;
    const uint32_t cut = L.cut0, cont = L.content0;
    if (!cut) return;
    const uint32_t l = 31u - (uint32_t)__clz((int)cut), at = blockIdx.x * TK_LN_TILE + L.pos;
    typename M::Seg run = before;
#pragma unroll 1
    for (uint32_t j = 0; j <= l; ++j) {
        if (((cut >> j) & 1u) && run.e.bytes) f(j, at + j - run.e.bytes, run);
        if ((cut >> j) & 1u) run = M::empty();
        if (j < l && ((cont >> j) & 1u)) view.push(run, j);
    }
}
template <class M>
__device__ __forceinline__ typename M::Seg tk_ls_before(const TkLs& q, const typename M::View& view, const TkLnTiles& T, TkLnShared& sh) {
    return tk_ln_block_exscan(M(q.ln), view.tail(TK_LN_LINE, sh), M::enters(T, blockIdx.x), M::wsum(sh), (typename M::Seg*)nullptr);
}

// (M: what is hashed -- TkLnRaw for a set with a mask of 0, TkLnNorm for a normalising one; the same for tk_k_ls_decide)
template <class M>
__global__ __launch_bounds__(TK_LN_THREADS) void tk_k_ls_mark(TkLs q, const uint8_t* __restrict__ text, const uint64_t* __restrict__ doc_off, bool aligned, TkLnTiles T,
                                                              TkLsTab tab) {
    __shared__ TkLnShared sh;
    const TkLnLane L = tk_ln_stage(q.ln, text, doc_off, aligned, sh);
    const typename M::View view(q.ln, L);
    const typename M::Seg before = tk_ls_before<M>(q, view, T, sh);
    uint32_t claims = 0;
    tk_ls_each_line<M>(view, before, [&](uint32_t, uint32_t start, const typename M::Seg& run) {
        if (!tk_ls_eligible(q, run)) return;
        const uint64_t key = tk_ls_key(q.ln.seed, run.e);
        uint64_t slot = q.S;
        const bool won = tk_ng_insert(tab.key, q.S, key, [&](uint64_t i, uint64_t k) {
            const uint64_t v = (uint64_t)atomicCAS(tab.key + i, 0ull, (unsigned long long)k);
            if (v == 0 || v == k) slot = i;
            return v;
        });
        claims += won;
        if (slot == q.S) slot = tk_ls_find(TkLsKeys{tab.key}, q.S, key);  // (the key was met by a load)
        if (slot < q.S) atomicMin(tab.first + slot, (unsigned long long)tk_ls_first(q.epoch, start));
    });
    claims = tk_wave_sum_u32(claims);
    if ((threadIdx.x & 63u) == 0 && claims) atomicAdd(tab.count, (unsigned long long)claims);
}

template <class M>
__global__ __launch_bounds__(TK_LN_THREADS) void tk_k_ls_decide(TkLs q, const uint8_t* __restrict__ text, const uint64_t* __restrict__ doc_off, bool aligned, TkLnTiles T,
                                                                TkLsTab tab, uint32_t* bitmap, unsigned long long* n_lines, unsigned long long* n_dropped,
                                                                unsigned long long* words) {
    __shared__ TkLnShared sh;
    __shared__ uint32_t docid[TK_LN_DOCS];   // the document of a local index; TK_LN_NONE
    __shared__ uint32_t acc[2][TK_LN_DOCS];  // its lines and dropped lines of this tile
    __shared__ uint32_t dropped_here;
    const uint32_t tid = threadIdx.x;
    const uint64_t g0 = (uint64_t)blockIdx.x * TK_LN_TILE;
    const TkLnLane L = tk_ln_stage(q.ln, text, doc_off, aligned, sh);
    // Local documents, as in tk_k_ln_count: index 0 owns the byte before the tile; index r > 0 is the non-empty document at the r-th start bit.
    if (tid < TK_LN_DOCS) docid[tid] = tid == 0 && g0 && q.ln.n_docs ? (uint32_t)tk_last_le(doc_off, 0, q.ln.n_docs, g0 - 1) : TK_LN_NONE;
    if (tid < TK_LN_DOCS) acc[0][tid] = acc[1][tid] = 0;
    if (tid == 0) dropped_here = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)sh.i0 + tid; i <= sh.i1 && i < q.ln.n_docs; i += TK_LN_THREADS) {
        const uint64_t s = doc_off[i], r = s - g0;
        if (r >= TK_LN_TILE || doc_off[i + 1] <= s) continue;
        const uint32_t li = sh.brkpre[r >> 6] + (uint32_t)__popcll(sh.brkw[r >> 6] & ((2ull << (r & 63u)) - 1ull));
        if (li < TK_LN_DOCS) docid[li] = (uint32_t)i;
    }
    __syncthreads();
    const typename M::View view(q.ln, L);
    const typename M::Seg before = tk_ls_before<M>(q, view, T, sh);
    unsigned long long* const outs[2] = {n_lines, n_dropped};
    tk_ls_each_line<M>(view, before, [&](uint32_t j, uint32_t start, const typename M::Seg& run) {
        bool drop = false;
        if (tk_ls_eligible(q, run)) {
            const uint64_t key = tk_ls_key(q.ln.seed, run.e), slot = tk_ls_find(tab.key, q.S, key);
            drop = q.epoch ? slot == q.S || tab.first[slot] != tk_ls_first(q.epoch, start) : slot < q.S;
        }
        if (drop) atomicOr(bitmap + (start >> 5), 1u << (start & 31u)), atomicAdd(&dropped_here, 1u);
        const uint32_t li = L.rank + (uint32_t)__popc(L.brk & ((1u << j) - 1u));
        if (li < TK_LN_DOCS) {
            atomicAdd(&acc[0][li], 1u);
            if (drop) atomicAdd(&acc[1][li], 1u);
        } else if (n_lines || (drop && n_dropped)) {
            const uint64_t d = tk_last_le(doc_off, 0, q.ln.n_docs, g0 + L.pos + j - 1);
            if (n_lines) atomicAdd(n_lines + d, 1ull);
            if (drop && n_dropped) atomicAdd(n_dropped + d, 1ull);
        }
    });
    __syncthreads();
    if (tid < TK_LN_DOCS && docid[tid] != TK_LN_NONE) {
        const uint64_t d = docid[tid];
        const bool whole = tid > 0 && doc_off[d + 1] < g0 + TK_LN_TILE;  // (it starts in the tile, and the cut that closes it lies there too)
        for (uint32_t f = 0; f < 2; ++f) {
            const uint32_t v = acc[f][tid];
            if (!outs[f]) continue;
            if (whole) outs[f][d] = v;
            else if (v) atomicAdd(outs[f] + d, (unsigned long long)v);
        }
    }
    if (tid == 0 && dropped_here) atomicAdd(words + TK_LN_WORDS + TK_LS_W_DROPPED, (unsigned long long)dropped_here);
}

// The keep mask of the lane's 16 bytes (every lane of the workgroup is here).  wmax: four words of LDS.
__device__ __forceinline__ uint32_t tk_ls_lane_keep(const TkLs& q, const TkLnLane& L, const TkLnTiles& T, const uint32_t* __restrict__ bitmap, uint32_t* wmax) {
    const uint32_t g0 = blockIdx.x * TK_LN_TILE, at = g0 + L.pos;
    const uint64_t N = q.ln.n_bytes;
    const uint32_t n_valid = at >= N ? 0u : N - at < TK_LN_LANE ? (uint32_t)(N - at) : TK_LN_LANE, valid = (1u << n_valid) - 1u;
    uint32_t last;
    const uint32_t enters = g0 - T.seg[blockIdx.x].e.bytes, own = tk_block_exmax32_256(tk_ls_open_start(L.cut0, L.content0, at), &last, wmax);
    return tk_ls_keep_mask(valid, L.content0, L.cut0, L.brk, at, own > enters ? own : enters, [&](uint32_t s) { return (bitmap[s >> 5] >> (s & 31u)) & 1u; });
}

__global__ __launch_bounds__(TK_LN_THREADS) void tk_k_ls_keep(TkLs q, const uint8_t* __restrict__ text, const uint64_t* __restrict__ doc_off, bool aligned, TkLnTiles T,
                                                              const uint32_t* __restrict__ bitmap, uint32_t* __restrict__ kept) {
    __shared__ TkLnShared sh;
    __shared__ uint32_t wmax[4], wsum[4];
    const TkLnLane L = tk_ln_stage(q.ln, text, doc_off, aligned, sh);
    const unsigned long long n = tk_block_sum_256((uint32_t)__popc(tk_ls_lane_keep(q, L, T, bitmap, wmax)), wsum);
    if (threadIdx.x == 0) kept[blockIdx.x] = (uint32_t)n;
}

__global__ __launch_bounds__(1024) void tk_k_ls_scan(uint32_t* kept, uint64_t n_tiles) {
    __shared__ unsigned long long wsum[16];
    tk_scan_blocks<false>(kept, n_tiles, 0ull, wsum);
}

__global__ __launch_bounds__(TK_LN_THREADS) void tk_k_ls_write(TkLs q, const uint8_t* __restrict__ text, const uint64_t* __restrict__ doc_off, bool aligned, TkLnTiles T,
                                                               const uint32_t* __restrict__ bitmap, const uint32_t* __restrict__ base, const unsigned long long* __restrict__ words,
                                                               uint8_t* __restrict__ text_out, unsigned long long* __restrict__ doc_off_out, unsigned long long* __restrict__ counts) {
    __shared__ TkLnShared sh;
    __shared__ alignas(16) uint8_t out[TK_LN_TILE + 32];  // the kept bytes, from out[shift]
    __shared__ uint32_t before_of[TK_LN_THREADS];         // the kept bytes of the lanes before a lane
    __shared__ uint16_t keep_of[TK_LN_THREADS];
    __shared__ uint32_t wmax[4], wsum[8];
    const uint32_t tid = threadIdx.x;
    const uint64_t g0 = (uint64_t)blockIdx.x * TK_LN_TILE;
    const TkLnLane L = tk_ln_stage(q.ln, text, doc_off, aligned, sh);
    const uint32_t keep = tk_ls_lane_keep(q, L, T, bitmap, wmax);
    uint32_t total;
    const uint32_t ex = tk_block_exscan_256((uint32_t)__popc(keep), &total, wsum);
    const uint64_t dst = base[blockIdx.x];
    uint8_t* const g = text_out + dst;
    const uint32_t shift = (uint32_t)((uintptr_t)g & 15u), end = shift + total;
    before_of[tid] = ex, keep_of[tid] = (uint16_t)keep;
    {
        uint32_t o = shift + ex;
        for (uint32_t m = keep; m; m &= m - 1u) out[o++] = (uint8_t)L.byte((uint32_t)__ffs((int)m) - 1u);
    }
    __syncthreads();
    for (uint32_t lo = tid * 16u; lo < end; lo += TK_LN_THREADS * 16u) {  // out[lo .. lo + 16) is g[lo - shift ..): the same 16-byte word
        if (lo >= shift && lo + 16u <= end) {
            *(uint4*)(g + (lo - shift)) = *(const uint4*)(out + lo);
        } else {
            for (uint32_t i = lo < shift ? shift : lo; i < lo + 16u && i < end; ++i) g[i - shift] = out[i];
        }
    }
    // i0 is the LAST entry at or below g0: empty documents that share g0 with it lie before i0.  The tile before this one writes them, at
    // its position T -- the same value, this tile's `dst` --, and the first tile starts at entry 0.
    if (doc_off_out)
        for (uint64_t i = (blockIdx.x ? (uint64_t)sh.i0 : 0ull) + tid; i <= sh.i1; i += TK_LN_THREADS) {
            const uint64_t r = doc_off[i] - g0;  // (wraps below g0)
            if (r < TK_LN_TILE) doc_off_out[i] = dst + before_of[r >> 4] + (uint32_t)__popc(keep_of[r >> 4] & ((1u << (r & 15u)) - 1u));
            else if (r == TK_LN_TILE) doc_off_out[i] = dst + total;
        }
    if (blockIdx.x == gridDim.x - 1 && tid == 0 && counts) counts[0] = dst + total, counts[1] = words[TK_LN_WORDS + TK_LS_W_DROPPED];
}
