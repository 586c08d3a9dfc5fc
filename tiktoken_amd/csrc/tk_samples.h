// Supervised samples on the device: a packed batch (ids, tok_off) whose documents are the PARTS of samples -- the messages of a conversation,
// a prompt and its answer -- -> one row per sample: [bos], for every part the before ids of its role, its body, the after ids, [eos];
// truncated to max_len at the head or the tail, padded left or right; ids, an attention mask and labels (the id where the element is
// trained, ignore_index elsewhere) as [R, W], and per sample len, full_len and n_trained.  Nothing in the reference does this: it replaces
// the host loop of the reference's users, the SFT data script that encodes message by message and builds ids and labels as Python lists.
// The rule is stated in include/tiktoken_amd.h; its plain C++ is tk_samples_rule.h's.  Built like the padded passes of tk_padded.h:
//   tk_k_smp_count    one thread per entry of tok_off and of sample_off: both are checked (ascending from 0 to n_tokens / n_parts; the
//                     first offender goes into a report word), every part's role is checked (the first part whose role is none: a report
//                     word), the elements of the part -> pstart[p]
//   tk_k_smp_scan     one workgroup: exclusive sums of those counts in place (tk_scan_blocks), the total behind them and into a report word
//   tk_k_smp_samples  one thread per sample: full_len, len, n_trained (analytically: the parts' clipped overlaps with the kept window),
//                     the longest len -> a report word.  Does nothing when a report word names an offender.
//   (the host reads the report words, settles W, refuses or sizes the outputs; the passes above work in scratch arrays, and the per-sample
//   figures are copied into the result's buffers only once the call is accepted, so a refused call leaves the previous result whole)
//   tk_k_smp_write    ids, labels and mask over the R * W positions, TK_DEC_BLOCK per workgroup, eight consecutive ones per lane
// The role table -- at most 513 offsets, 4096 ids and 256 train flags, 18.3 KiB -- is copied into the LDS by every workgroup of the write
// pass, as much of it as the call has.  A lane reads it at indices that depend on its data (its part's role, the element's place in the
// before or after run): in the LDS that is a ds_read_b32 that shares no path with the lane's token gathers, which go through the vector
// memory pipeline and the L1 like the 16-byte stores behind them; 18.3 KiB of the CU's 160 KiB still leave room for eight workgroups of
// 256, the most the CU's wavefront slots hold.  The copy is 2 * n_roles + 1 + n_ids words per workgroup of 2048 positions -- a chat
// template has a few dozen.  A sample's parts are searched per lane inside [sample_off[s], sample_off[s + 1]) alone (a conversation has
// tens of parts, not thousands), so no workgroup-wide narrowing as in tk_k_pad_write; and a lane whose eight positions are padding of one
// row stops after loading the row's figures: it looks for no part.
// The three caller arrays: tk_k_smp_count indexes nothing with their entries except the role table with a role it has compared with
// n_roles; tk_k_smp_samples runs behind it and does nothing when it reported; the host launches tk_k_smp_write only when nothing was
// reported.  So no kernel reads or writes out of bounds whatever tok_off, sample_off and part_role hold.
// What the CPU simulation (tests/test_samples_sim.py) shares with the kernels: tk_smp_count_entry (the body of tk_k_smp_count's loop),
// tk_smp_reported and tk_smp_sample_entry (tk_k_smp_samples') and tk_smp_lane (tk_k_smp_write); the wave reduction, the atomicMax, the
// scan, the LDS copy of the role table and the stores are the kernels' own.
// Included by tk_api.hip only.
#pragma once
#include "tk_decode.h"
#include "tk_rows.h"  // TkTokens, tk_ids_store8, tk_ids_store1
#include "tk_samples_rule.h"
#include "tk_scan.h"

// the role table in global memory (uploaded per call): off[2 * n_roles + 1], then ids[n_ids], then train[n_roles] as bytes
struct TkSmpTable {
    const uint32_t* __restrict__ off;
    const uint32_t* __restrict__ ids;
    const uint8_t* __restrict__ train;
    uint32_t n_ids;
};
using TkSmpRolesPtr = TkSmpRoles<const uint32_t*, const uint32_t*, const uint8_t*>;
using TkSmpInPtr = TkSmpIn<const uint64_t*, const uint64_t*, const uint8_t*, const uint64_t*>;

__global__ __launch_bounds__(256) void tk_k_smp_count(const uint64_t* __restrict__ tok_off, const uint64_t* __restrict__ sample_off, const uint8_t* __restrict__ part_role,
                                                      TkSmpTable tab, TkSmp p, uint64_t* __restrict__ pstart, unsigned long long* __restrict__ words) {
    const uint64_t n = p.n_parts > p.n_samples ? p.n_parts : p.n_samples;
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * 256) tk_smp_count_entry(p, tok_off, sample_off, part_role, tab.off, i, pstart, words);
}

// In place: pstart -> the elements before every part, the total behind them
__global__ __launch_bounds__(1024) void tk_k_smp_scan(uint64_t* __restrict__ pstart, uint64_t n_parts, unsigned long long* __restrict__ words) {
    __shared__ unsigned long long wsum[16];
    const unsigned long long carry = tk_scan_blocks<false>(pstart, n_parts, 0ull, wsum);
    if (threadIdx.x == 0) {
        words[TK_SMP_TOTAL] = carry;
        pstart[n_parts] = carry;
    }
}

__global__ __launch_bounds__(256) void tk_k_smp_samples(const uint64_t* __restrict__ sample_off, const uint8_t* __restrict__ part_role, const uint64_t* __restrict__ pstart,
                                                        TkSmpTable tab, TkSmp p, uint64_t* __restrict__ full, uint32_t* __restrict__ len, uint32_t* __restrict__ n_trained,
                                                        unsigned long long* __restrict__ words) {
    if (tk_smp_reported(words)) return;  // (the same in every thread) the caller's arrays do not describe the batch: nothing is indexed with them
    const TkSmpRolesPtr t{tab.off, tab.ids, tab.train};
    uint32_t longest = 0;
    for (uint64_t s = blockIdx.x * 256ull + threadIdx.x; s < p.n_samples; s += (uint64_t)gridDim.x * 256) {
        const uint32_t l = tk_smp_sample_entry(p, sample_off, pstart, part_role, t, s, full, len, n_trained);
        longest = l > longest ? l : longest;
    }
    longest = tk_wave_max_u32(longest);  // (behind the loop: every lane is here)
    if ((threadIdx.x & 63) == 0 && longest) atomicMax(words + TK_SMP_LONGEST, (unsigned long long)longest);
}

// ids_out, labels_out, mask_out: 16-byte aligned (the library's own buffers): a lane's eight ids and eight labels leave as 16-byte stores,
// its eight mask bytes as one 8-byte store.  tokens is the caller's: eight ids arrive as two 16-byte loads where the lane's positions are
// eight body tokens of one part and their address allows it, otherwise as 4-byte loads, as in tk_k_pad_write.  What a lane computes is
// tk_smp_lane (tk_samples_rule.h), the same statements the CPU simulation runs.
__global__ __launch_bounds__(256) void tk_k_smp_write(const uint32_t* __restrict__ tokens, const uint64_t* __restrict__ tok_off, const uint64_t* __restrict__ sample_off,
                                                      const uint8_t* __restrict__ part_role, const uint64_t* __restrict__ pstart, TkSmpTable tab, TkSmp p,
                                                      uint32_t* __restrict__ ids_out, int32_t* __restrict__ labels_out, uint8_t* __restrict__ mask_out) {
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
    uint32_t id[8];
    int32_t lab[8];
    uint64_t mask;
    tk_smp_lane(p, TkTokens{tokens}, TkSmpInPtr{tok_off, sample_off, part_role, pstart}, TkSmpRolesPtr{sh_off, sh_ids, sh_train}, i0, N, id, lab, &mask);
    if (N - i0 >= 8u) {
        tk_ids_store8<false>(ids_out, i0, id);
        *(int4*)(labels_out + i0) = make_int4(lab[0], lab[1], lab[2], lab[3]);
        *(int4*)(labels_out + i0 + 4) = make_int4(lab[4], lab[5], lab[6], lab[7]);
        *(unsigned long long*)(mask_out + i0) = mask;
    } else {
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j)
            if (N - i0 > j) {
                tk_ids_store1<false>(ids_out, i0 + j, id[j]);
                labels_out[i0 + j] = lab[j];
                mask_out[i0 + j] = (uint8_t)(mask >> (8 * j));
            }
    }
}
