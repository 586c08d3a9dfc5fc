// Near-duplicate groups on the device: fingerprints (sig, band, n_shingles: tk_fingerprint.h's results) -> for every document the lowest
// index of its group, a keep mask, the number kept; and the selection of kept documents out of a packed batch.  Nothing in the reference
// does this: it is the host step behind the fingerprints (Fingerprints.duplicate_groups: B sorts and a Python loop over the close pairs,
// then numpy indexing of ids copied out).  The rule is stated in include/tiktoken_amd.h; its plain C++ is tk_groups_rule.h's.
// Groups, per round of bands (the table holds per_round regions):
//   tk_k_grp_clear   slots = TK_GRP_EMPTY (a kernel, not a memset: the pass may be recorded into a graph); first round: parent[d] = d
//   tk_k_grp_claim   one thread per (live document, band): tk_grp_claim -- a compare-and-swap on an empty slot, an atomicMin on a slot
//                    of the same key, and that only where the slot read first holds a larger index
//   tk_k_grp_join    behind the kernel boundary the slots are final.  A wavefront takes 64 (document, band) items and looks up every
//                    item's rep.  An item needs a comparison when rep != d, no lower lane of the wavefront holds the same pair (the
//                    bands of a document are neighbouring lanes: identical documents would compare B times otherwise) and
//                    find(d) != find(rep) (a union of one component changes nothing).  The pairs that remain are listed in LDS
//                    (a ballot, the rank among its bits) and worked off 64 / lanes at a time: tk_grp_pair_lanes(P) lanes per pair,
//                    16 bytes of either row per lane, the count summed over the lanes (tk_lanes_sum_u32); lane 0 of a pair with
//                    count >= min_match joins: tk_grp_union, a compare-and-swap of the larger root under the smaller.
//   tk_k_grp_flat    group[d] = find(d), keep[d], one atomicAdd of a workgroup's count into n_kept
// Selection:
//   tk_k_sel_count   per workgroup of 256 documents: kept documents, kept tokens
//   tk_k_sel_scan    the one workgroup of 1024 threads: both arrays scanned in place; counts_out; the closing offset
//   tk_k_sel_place   the same workgroups again: a kept document's new index and new start -> tok_off_out, doc_out
//   tk_k_sel_copy    by OUTPUT tiles of TK_SEL_TILE positions: the kept documents that meet the tile (tk_last_le on tok_off_out), then
//                    every lane its positions, coalesced stores; a document of many MiB costs what many small ones cost, an empty
//                    kept document nothing but its offset
// Everything is queued on the caller's stream; the host waits for nothing.  Included by tk_api.hip only.
#pragma once
#include "tk_groups_rule.h"
#include "tk_scan.h"

struct TkGrpDeviceMem {  // device-wide, relaxed: the forest and the table need single-copy atomicity and progress, no ordering
    __device__ __forceinline__ uint32_t load(const uint32_t* p) const { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ void store(uint32_t* p, uint32_t v) const { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ uint32_t cas(uint32_t* p, uint32_t expected, uint32_t desired) const { return atomicCAS(p, expected, desired); }
    __device__ __forceinline__ void min(uint32_t* p, uint32_t v) const { atomicMin(p, v); }
};

__global__ __launch_bounds__(256) void tk_k_grp_clear(uint32_t* __restrict__ slot, uint64_t n_slots, uint32_t* __restrict__ parent, uint64_t n, unsigned long long* n_kept) {
    const uint64_t m = n_slots > n ? n_slots : n;
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < m; i += (uint64_t)gridDim.x * 256) {
        if (i < n_slots) slot[i] = TK_GRP_EMPTY;
        if (parent && i < n) parent[i] = (uint32_t)i;
    }
    if (n_kept && !blockIdx.x && !threadIdx.x) *n_kept = 0;
}

__global__ __launch_bounds__(256) void tk_k_grp_claim(TkGrp g, const uint64_t* __restrict__ band, const uint64_t* __restrict__ n_shingles, uint32_t* slot, uint32_t j0, uint32_t nb) {
    TkGrpDeviceMem m;
    const uint64_t items = g.n * nb;
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < items; i += (uint64_t)gridDim.x * 256) {
        const uint32_t d = (uint32_t)(i / nb), r = (uint32_t)(i % nb);
        if (n_shingles[d]) tk_grp_claim(m, slot + r * g.S, g.S, band, g.B, j0 + r, d);
    }
}

__global__ __launch_bounds__(256) void tk_k_grp_join(TkGrp g, const uint32_t* __restrict__ sig, const uint64_t* __restrict__ band, const uint64_t* __restrict__ n_shingles,
                                                     const uint32_t* __restrict__ slot, uint32_t* parent, uint32_t j0, uint32_t nb, bool vec) {
    __shared__ uint32_t pair_a[256], pair_b[256];  // per wavefront: the 64 entries from its first lane on
    TkGrpDeviceMem m;
    const uint32_t lane = threadIdx.x & 63u, w0 = threadIdx.x & ~63u;
    const uint32_t per_step = 64u / g.lanes, sub = lane / g.lanes, q = lane % g.lanes, back = nb < 64u ? nb : 64u;
    const uint64_t items = g.n * nb;
    for (uint64_t base = blockIdx.x * 256ull; base < items; base += (uint64_t)gridDim.x * 256) {  // (the same trips for the whole workgroup)
        const uint64_t i = base + threadIdx.x;
        uint32_t d = TK_GRP_EMPTY, rep = TK_GRP_EMPTY;
        if (i < items) {
            d = (uint32_t)(i / nb);
            const uint32_t r = (uint32_t)(i % nb);
            rep = n_shingles[d] ? tk_grp_rep(slot + r * g.S, g.S, band, g.B, j0 + r, d) : d;
        }
        bool need = rep != d;
        for (uint32_t o = 1; o < back; ++o) {  // the bands of a document are at most `back` lanes apart
            const uint32_t od = __shfl_up(d, o, 64), orep = __shfl_up(rep, o, 64);
            if (lane >= o && od == d && orep == rep) need = false;
        }
        if (need && tk_grp_find(m, parent, d) == tk_grp_find(m, parent, rep)) need = false;
        const unsigned long long listed = __ballot(need);
        const uint32_t cnt = (uint32_t)__popcll(listed);
        if (need) {
            const uint32_t at = w0 + (uint32_t)__popcll(listed & ((1ull << lane) - 1));
            pair_a[at] = d, pair_b[at] = rep;
        }
        __syncthreads();
        for (uint32_t t = 0; t < cnt; t += per_step) {  // (the same trips for the whole wavefront)
            const uint32_t k = t + sub;
            uint32_t a = 0, b = 0, c = 0;
            if (k < cnt) {
                a = pair_a[w0 + k], b = pair_b[w0 + k];
                c = tk_grp_match4(sig, g.P, vec, a, b, q);
            }
            c = tk_lanes_sum_u32(c, g.lanes);
            if (k < cnt && q == 0 && c >= g.min_match) tk_grp_union(m, parent, a, b);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void tk_k_grp_flat(uint64_t n, uint32_t* parent, uint32_t* __restrict__ group, uint8_t* __restrict__ keep, unsigned long long* n_kept) {
    __shared__ uint32_t sh[4];
    TkGrpDeviceMem m;
    const uint64_t d = blockIdx.x * 256ull + threadIdx.x;
    uint32_t kept = 0;
    if (d < n) {
        const uint32_t root = tk_grp_find(m, parent, (uint32_t)d);
        kept = root == (uint32_t)d;
        if (group) group[d] = root;
        if (keep) keep[d] = (uint8_t)kept;
    }
    const unsigned long long sum = tk_block_sum_256(kept, sh);
    if (n_kept && !threadIdx.x && sum) atomicAdd(n_kept, sum);
}

// ---- selection ----
// What a workgroup of 256 documents knows of itself: in every thread, whether its document is kept, how many kept documents and kept
// tokens of the workgroup stand before it, and the workgroup's two totals.
struct TkSelBlock {
    uint32_t kept, docs_before, docs;
    unsigned long long toks_before, toks;
};
__device__ __forceinline__ TkSelBlock tk_sel_block(const uint8_t* __restrict__ keep, const uint64_t* __restrict__ tok_off, uint64_t n, uint64_t d, uint32_t* sh32 /*[8]*/,
                                                   unsigned long long* sh64 /*[4]*/) {
    TkSelBlock b;
    b.kept = d < n && keep[d];
    const unsigned long long len = d < n ? tk_sel_len(keep, tok_off, d) : 0;
    b.docs_before = tk_block_exscan_256(b.kept, &b.docs, sh32);
    b.toks_before = tk_block_exscan64_256(len, &b.toks, sh64);
    return b;
}
__global__ __launch_bounds__(256) void tk_k_sel_count(const uint8_t* __restrict__ keep, const uint64_t* __restrict__ tok_off, uint64_t n, unsigned long long* __restrict__ blk_docs,
                                                      unsigned long long* __restrict__ blk_toks) {
    __shared__ uint32_t sh32[8];
    __shared__ unsigned long long sh64[4];
    const TkSelBlock b = tk_sel_block(keep, tok_off, n, blockIdx.x * 256ull + threadIdx.x, sh32, sh64);
    if (!threadIdx.x) blk_docs[blockIdx.x] = b.docs, blk_toks[blockIdx.x] = b.toks;
}
__global__ __launch_bounds__(1024) void tk_k_sel_scan(unsigned long long* blk_docs, unsigned long long* blk_toks, uint64_t n_blocks, uint64_t* __restrict__ tok_off_out,
                                                      uint64_t* __restrict__ counts_out) {
    __shared__ unsigned long long wsum[16];
    const unsigned long long n_kept = tk_scan_blocks<false>(blk_docs, n_blocks, 0ull, wsum);
    const unsigned long long toks = tk_scan_blocks<false>(blk_toks, n_blocks, 0ull, wsum);
    if (!threadIdx.x) counts_out[0] = n_kept, counts_out[1] = toks, tok_off_out[n_kept] = toks;
}
__global__ __launch_bounds__(256) void tk_k_sel_place(const uint8_t* __restrict__ keep, const uint64_t* __restrict__ tok_off, uint64_t n, const unsigned long long* __restrict__ blk_docs,
                                                      const unsigned long long* __restrict__ blk_toks, uint64_t* __restrict__ tok_off_out, uint32_t* __restrict__ doc_out) {
    __shared__ uint32_t sh32[8];
    __shared__ unsigned long long sh64[4];
    const uint64_t d = blockIdx.x * 256ull + threadIdx.x;
    const TkSelBlock b = tk_sel_block(keep, tok_off, n, d, sh32, sh64);
    if (!b.kept) return;
    const uint64_t i = blk_docs[blockIdx.x] + b.docs_before;  // (below n: one per kept document)
    tok_off_out[i] = blk_toks[blockIdx.x] + b.toks_before;
    doc_out[i] = (uint32_t)d;
}
__global__ __launch_bounds__(TK_SEL_THREADS) void tk_k_sel_copy(const uint32_t* __restrict__ tokens, uint64_t n_tokens, const uint64_t* __restrict__ tok_off,
                                                                const uint64_t* __restrict__ tok_off_out, const uint32_t* __restrict__ doc_out,
                                                                const uint64_t* __restrict__ counts, uint32_t* __restrict__ tokens_out) {
    const uint64_t n_kept = counts[0], total = counts[1] < n_tokens ? counts[1] : n_tokens;  // (more than n_tokens: a tok_off that does not ascend)
    for (uint64_t g0 = (uint64_t)blockIdx.x * TK_SEL_TILE; g0 < total; g0 += (uint64_t)gridDim.x * TK_SEL_TILE) {
        const uint64_t g1 = g0 + TK_SEL_TILE < total ? g0 + TK_SEL_TILE : total;
        const uint64_t i0 = tk_last_le(tok_off_out, 0, n_kept, g0), i1 = tk_last_le(tok_off_out, i0, n_kept, g1 - 1);
        for (uint64_t g = g0 + threadIdx.x; g < g1; g += TK_SEL_THREADS) {
            const uint64_t src = tk_sel_source(tok_off, tok_off_out, doc_out, i0, i1, g);
            tokens_out[g] = src < n_tokens ? tokens[src] : 0u;
        }
    }
}
