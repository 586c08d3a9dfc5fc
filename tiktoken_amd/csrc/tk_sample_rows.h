// Packed sample rows on the device: the samples of tk_samples.h, several to a row of max_len -- placed next-fit in input order, whole or
// not at all -- with ids, labels, the sample and the position inside it per element, and the segment boundaries (cu_seqlens, row_seg) that
// block-diagonal / variable-length attention takes.  Nothing in the reference does this: it replaces the packing loop of an SFT trainer's
// data collator.  The rule is stated in include/tiktoken_amd.h; its plain C++ is tk_sample_rows_rule.h's.
// Next-fit is a loop whose every step waits for the one before.  Here it is sums, searches and pointer doubling:
//   tk_k_smp_count / _scan / _samples   tk_samples.h's, unchanged: the three caller arrays are checked, pstart, full_len, len, n_trained
//   tk_k_srow_plen    one thread per sample: the placed length and the placed flag, n_trained as the packed rows count it
//   tk_k_srow_sums    one workgroup: exclusive sums of both (tk_scan_blocks), c[] and f[]
//   tk_k_srow_succ    one thread per sample: its successor as a row start, by binary search in c[]; the first placed sample is marked
//   tk_k_srow_double  ceil(log2 n_samples) launches, the number known on the host, nothing waited for in between: a marked sample marks its
//                     2^k-th successor, every sample's jump becomes its 2^(k+1)-th (two jump arrays, in turns).  No thread walks a chain.
//   tk_k_srow_rows    one workgroup: the exclusive sum of the marks: sample_row; R
//   tk_k_srow_place   one thread per sample: sample_row, sample_col, and per row its first sample and whether it has a padding tail
//   tk_k_srow_segs    one workgroup: the exclusive sum of the tails: row_seg; n_segs
//   (the host reads the report words once, refuses or sizes the outputs; everything above works in scratch arrays)
//   tk_k_srow_write   ids, labels, seg and pos over the R * L positions, TK_DEC_BLOCK per workgroup, eight consecutive ones per lane; the
//                     lane that holds a pos == 0 writes its cu_seqlens entry, whose index follows from row_seg and f[]
// Why one launch per round of doubling and not one workgroup that loops: a round reads and writes n entries with no order among them, so
// it wants the whole device; a dependent launch on one stream costs 1.5 - 2 us, and 15 rounds (n = 20 000 samples) are 30 us beside a write
// pass of hundreds.  One workgroup looping over n entries per round with a barrier between rounds pays a global-memory round trip per 1024
// entries and round instead -- what tk_k_smp_scan's 0.11 ms for 79 000 counts shows, fifteen times over.  Keeping the jump arrays in the LDS
// would cover a few thousand samples only and be a second path to test.
// A round's marks are plain stores of 1 to words other lanes may read in the same launch: whichever lands first, only members of the chain
// are ever marked and all within reach are (tk_srow_double_entry), so the result does not depend on the order.
// Every kernel behind tk_k_smp_count does nothing when a report word names an offender: nothing is indexed with what the caller's arrays
// hold, or with scratch that was computed from them.  tk_k_srow_write is launched only when the call is accepted.
// Included by tk_api.hip only.
#pragma once
#include "tk_sample_rows_rule.h"
#include "tk_samples.h"

using TkSrowInPtr = TkSrowIn<const uint64_t*, const uint64_t*, const uint32_t*, const uint32_t*>;

__global__ __launch_bounds__(256) void tk_k_srow_plen(const uint64_t* __restrict__ tok_off, const uint64_t* __restrict__ sample_off, const uint8_t* __restrict__ part_role,
                                                      const uint64_t* __restrict__ pstart, TkSmpTable tab, TkSmp p, const uint64_t* __restrict__ full,
                                                      const uint32_t* __restrict__ len, uint32_t* __restrict__ n_trained, uint64_t* __restrict__ c, uint64_t* __restrict__ f,
                                                      const unsigned long long* __restrict__ words) {
    if (tk_smp_reported(words)) return;  // (the same in every thread)
    const TkSmpRolesPtr t{tab.off, tab.ids, tab.train};
    const TkSmpInPtr in{tok_off, sample_off, part_role, pstart};
    for (uint64_t s = blockIdx.x * 256ull + threadIdx.x; s < p.n_samples; s += (uint64_t)gridDim.x * 256) tk_srow_plen_entry(p, in, t, s, full, len, n_trained, c, f);
}

// In place: c -> the placed elements before every sample, f -> the placed samples before it, the totals behind them
__global__ __launch_bounds__(1024) void tk_k_srow_sums(uint64_t* __restrict__ c, uint64_t* __restrict__ f, uint64_t n, const unsigned long long* __restrict__ words) {
    __shared__ unsigned long long wsum[16];
    if (tk_smp_reported(words)) return;
    const unsigned long long placed = tk_scan_blocks<false>(c, n, 0ull, wsum);
    const unsigned long long samples = tk_scan_blocks<false>(f, n, 0ull, wsum);
    if (threadIdx.x == 0) {
        c[n] = placed;
        f[n] = samples;
    }
}

__global__ __launch_bounds__(256) void tk_k_srow_succ(const uint64_t* __restrict__ c, const uint64_t* __restrict__ f, uint64_t n, uint32_t L, uint32_t* __restrict__ succ,
                                                      uint32_t* __restrict__ mark, const unsigned long long* __restrict__ words) {
    if (tk_smp_reported(words)) return;
    for (uint64_t s = blockIdx.x * 256ull + threadIdx.x; s <= n; s += (uint64_t)gridDim.x * 256) tk_srow_succ_entry(c, f, n, L, s, succ, mark);
}

// (mark is read and written by different lanes of one launch on purpose: no __restrict__ on it)
__global__ __launch_bounds__(256) void tk_k_srow_double(const uint32_t* __restrict__ jin, uint32_t* __restrict__ jout, uint32_t* mark, uint64_t n,
                                                        const unsigned long long* __restrict__ words) {
    if (tk_smp_reported(words)) return;
    for (uint64_t s = blockIdx.x * 256ull + threadIdx.x; s <= n; s += (uint64_t)gridDim.x * 256) tk_srow_double_entry(jin, n, s, jout, mark);
}

// In place: mark -> the row starts before every sample, R behind them and into its report word
__global__ __launch_bounds__(1024) void tk_k_srow_rows(uint32_t* __restrict__ mark, uint64_t n, unsigned long long* __restrict__ words) {
    __shared__ unsigned long long wsum[16];
    if (tk_smp_reported(words)) return;
    const unsigned long long rows = tk_scan_blocks<false>(mark, n, 0ull, wsum);
    if (threadIdx.x == 0) {
        mark[n] = (uint32_t)rows;
        words[TK_SROW_R] = rows;
    }
}

__global__ __launch_bounds__(256) void tk_k_srow_place(const uint32_t* __restrict__ ex, const uint64_t* __restrict__ c, const uint32_t* __restrict__ succ, uint64_t n, uint32_t L,
                                                       uint32_t* __restrict__ sample_row, uint32_t* __restrict__ sample_col, uint32_t* __restrict__ row_sample,
                                                       uint32_t* __restrict__ row_pad, const unsigned long long* __restrict__ words) {
    if (tk_smp_reported(words)) return;
    for (uint64_t s = blockIdx.x * 256ull + threadIdx.x; s < n; s += (uint64_t)gridDim.x * 256) tk_srow_place_entry(ex, c, succ, L, s, sample_row, sample_col, row_sample, row_pad);
    if (blockIdx.x == 0 && threadIdx.x == 0) row_sample[ex[n]] = (uint32_t)n;  // row_sample[R] (no sample writes it: rows are below R)
}

// In place: row_pad -> row_seg: the padding tails before every row plus the placed samples before its first one; n_segs behind them
__global__ __launch_bounds__(1024) void tk_k_srow_segs(const uint32_t* __restrict__ ex, const uint64_t* __restrict__ f, const uint32_t* __restrict__ row_sample, uint64_t n,
                                                       uint32_t* __restrict__ row_pad, unsigned long long* __restrict__ words) {
    __shared__ unsigned long long wsum[16];
    if (tk_smp_reported(words)) return;
    const uint64_t R = ex[n];
    const unsigned long long pads = tk_scan_blocks<false>(row_pad, R, 0ull, wsum);
    for (uint64_t r = threadIdx.x; r < R; r += 1024) row_pad[r] = tk_srow_row_seg(f, row_sample, r, row_pad[r]);  // (every thread: the entries it scanned itself)
    if (threadIdx.x == 0) {
        row_pad[R] = (uint32_t)(f[n] + pads);
        words[TK_SROW_NSEGS] = f[n] + pads;
    }
}

// cu_seqlens as a lane of the write pass fills it
struct TkSrowCu {
    uint32_t* __restrict__ cu;
    __device__ __forceinline__ void put(uint32_t index, uint32_t position) const { cu[index] = position; }
};

// ids_out, labels_out, seg_out, pos_out: 16-byte aligned (the library's own buffers): a lane's eight values of each leave as two 16-byte
// stores.  tokens is the caller's, fetched as in tk_k_smp_write.  What a lane computes is tk_srow_lane (tk_sample_rows_rule.h), the same
// statements the CPU simulation runs.  cu[n_segs] = N closes cu_seqlens.
__global__ __launch_bounds__(256) void tk_k_srow_write(const uint32_t* __restrict__ tokens, const uint64_t* __restrict__ tok_off, const uint64_t* __restrict__ sample_off,
                                                       const uint8_t* __restrict__ part_role, const uint64_t* __restrict__ pstart, TkSrowInPtr rw, TkSmpTable tab, TkSmp p,
                                                       uint32_t n_segs, uint32_t* __restrict__ ids_out, int32_t* __restrict__ labels_out, uint32_t* __restrict__ seg_out,
                                                       uint32_t* __restrict__ pos_out, uint32_t* __restrict__ cu) {
    __shared__ uint32_t sh_off[2 * TK_SMP_MAX_ROLES + 1];
    __shared__ uint32_t sh_ids[TK_SMP_MAX_ROLE_IDS];
    __shared__ uint8_t sh_train[TK_SMP_MAX_ROLES];
    for (uint32_t i = threadIdx.x; i < 2 * p.n_roles + 1; i += 256) sh_off[i] = tab.off[i];  // (n_roles <= 256, n_ids <= 4096: the host has refused anything else)
    for (uint32_t i = threadIdx.x; i < tab.n_ids; i += 256) sh_ids[i] = tab.ids[i];
    for (uint32_t i = threadIdx.x; i < p.n_roles; i += 256) sh_train[i] = tab.train[i];
    __syncthreads();
    const uint32_t N = (uint32_t)(p.R * p.W);  // (below 2^32, above 0: the host launches nothing otherwise)
    const uint32_t b0 = blockIdx.x * (uint32_t)TK_DEC_BLOCK, i0 = b0 + threadIdx.x * 8u;  // (b0 < N; an i0 that wraps lies beyond N: the test below asks b0)
    if (N - b0 <= threadIdx.x * 8u) return;
    if (i0 == 0u) cu[n_segs] = N;
    uint32_t id[8], sg[8], ps[8];
    int32_t lab[8];
    const TkSrowCu put{cu};
    tk_srow_lane(p, TkTokens{tokens}, TkSmpInPtr{tok_off, sample_off, part_role, pstart}, rw, TkSmpRolesPtr{sh_off, sh_ids, sh_train}, i0, N, id, lab, sg, ps, put);
    if (N - i0 >= 8u) {
        tk_ids_store8<false>(ids_out, i0, id);
        *(int4*)(labels_out + i0) = make_int4(lab[0], lab[1], lab[2], lab[3]);
        *(int4*)(labels_out + i0 + 4) = make_int4(lab[4], lab[5], lab[6], lab[7]);
        tk_ids_store8<false>(seg_out, i0, sg);
        tk_ids_store8<false>(pos_out, i0, ps);
    } else {
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j)
            if (N - i0 > j) {
                ids_out[i0 + j] = id[j];
                labels_out[i0 + j] = lab[j];
                seg_out[i0 + j] = sg[j];
                pos_out[i0 + j] = ps[j];
            }
    }
}
