// Streaming decode on the device: R row slots whose state lives in HBM, fed ids [R, W] per step, W <= 64 -- a column per step of a
// generation loop, a few under speculative decoding --; every step hands back, per row, the text that became final (the rule:
// include/tiktoken_amd.h, tk_stream_step_device; its plain C++: tk_stream_rule.h).  A step is latency-bound -- tens to thousands of rows of
// a few ids each --, so it is two launches whatever R, W and the data are, and one wait of the host:
//   tk_k_stream_row    a WAVEFRONT per row, four rows per workgroup.  Lane c reads column c and the row's state; the stop id, the live
//                      range and the kept columns are ballots (the row rule of tk_decode_rows_rule.h, a column per lane); a wave prefix sum
//                      of the kept tokens' lengths places their bytes, gathered from the decode table, behind the row's held-back tail in
//                      the row's LDS buffer; the lanes search that buffer for full hits and for the first prefix that has to be held back
//                      (the stop set staged in LDS once per workgroup, as tk_k_stops_find stages it), decide (tk_stream_decide), repair
//                      what is emitted sixteen bytes per lane (tk_u8r_lane, counted, placed by a wave prefix sum, written) into the row's
//                      slot of a strided scratch, and write the row's new state into the OTHER copy of the slots.
//   tk_k_stream_pack   a thread per row, 256 rows per workgroup: returns at once when the row kernel reported a refusal; otherwise the
//                      lengths' prefix (the rows before the workgroup added up by the workgroup itself, then tk_block_exscan_256), text_off,
//                      char_off, state, hit, and the scratch slots copied into the packed text, a byte per thread and turn.
// Why a wavefront per row: a row's work is W <= 64 columns and a buffer of tens of bytes.  A wavefront covers the columns with one lane each,
// so the row rule needs no loop and no scratch, and every exchange inside the row is a ballot or a DPP prefix sum, not a barrier; a workgroup
// per row would leave three of four wavefronts idle at W = 1 .. 4 and a thread per row would serialise the gather and the search.  The
// workgroup's barriers only order LDS writes before the reads of other lanes; every thread reaches every one of them.
// The host swaps the two copies of the slots when the call is accepted, so a refused step -- TK_KEY_ERROR, begin > end, end > W -- leaves
// state and the previous outputs whole without a check pass of its own: the row kernel writes scratch and the other copy only.
// Bounds: a lane reads column c only where begin <= c < end <= W, so nothing is read outside the (R - 1) * ld + W elements; the row buffer
// holds tail + W * (longest token) bytes by the sizes refused at create, and a lane still checks before it writes.
// Included by tk_api.hip only.
#pragma once
#include "tk_decode_rows.h"  // TkIdMatrix
#include "tk_scan.h"
#include "tk_stream_rule.h"

struct TkStreamBuf {  // a row's bytes in LDS
    const uint8_t* b;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return b[i]; }
};

// ids, begin, end, p: as the decode-rows kernels take them (p.W <= 64).  op: TK_STREAM_OP_*; sel: a byte per row (null: every row) for
// flush and reset.  cap: bytes of a row's LDS buffer (a multiple of 16); dynamic LDS: TK_STREAM_SET_BYTES + 4 * cap.  scratch: a slot of
// `slot` bytes per row; out_len, out_chars: what every row emitted.
template <int MODE>
__global__ __launch_bounds__(64 * TK_STREAM_ROWS_WG) void tk_k_stream_row(const void* __restrict__ ids, const uint32_t* __restrict__ begin, const uint32_t* __restrict__ end,
                                                                          TkDrows p, uint32_t op, const uint8_t* __restrict__ sel, const uint2* __restrict__ dec, uint32_t n_ids,
                                                                          const uint8_t* __restrict__ tok_bytes, const uint8_t* __restrict__ spec_bytes,
                                                                          const uint32_t* __restrict__ d_set, uint32_t mode, uint32_t cap,
                                                                          const TkStreamRow* __restrict__ cur, TkStreamRow* __restrict__ next, uint8_t* __restrict__ scratch,
                                                                          uint64_t slot, uint32_t* __restrict__ out_len, uint32_t* __restrict__ out_chars,
                                                                          unsigned long long* __restrict__ words) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const TkStopSet& set = *(const TkStopSet*)lds;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint8_t* const buf = lds + TK_STREAM_SET_BYTES + (size_t)wave * cap;
    const TkStreamBuf B{buf};
    for (uint32_t i = threadIdx.x; i < TK_STOPS_SET_WORDS; i += 64 * TK_STREAM_ROWS_WG) ((uint32_t*)lds)[i] = d_set[i];
    const uint64_t r = (uint64_t)blockIdx.x * TK_STREAM_ROWS_WG + wave;
    const bool row = r < p.R;  // (everything below is uniform over the wavefront unless it names `lane`)
    uint32_t state = TK_STREAM_FLUSHED, hit = TK_STOPS_NO_HIT, tail_len = 0;
    uint64_t n_kept = 0, n_text = 0, n_chars = 0;
    if (row) {
        state = cur[r].state, hit = cur[r].hit, tail_len = cur[r].tail_len;
        n_kept = cur[r].n_kept, n_text = cur[r].n_text, n_chars = cur[r].n_chars;
    }
    if (tail_len > TK_STREAM_HOLD) tail_len = TK_STREAM_HOLD;  // (never: the slots are written by this kernel alone)
    const bool chosen = row && (!sel || sel[r]);
    const bool step = op == TK_STREAM_OP_STEP, live = row && state == TK_STREAM_LIVE && (step || (op == TK_STREAM_OP_FLUSH && chosen));

    // the row rule, a column per lane
    uint32_t b = 0, e = 0;
    if (live && step && !tk_drows_range(p, begin, begin != nullptr, end, end != nullptr, r, &b, &e) && lane == 0) tk_report_min(words + TK_STREAM_BAD_ROW, r);
    const bool in = live && step && lane >= b && lane < e;
    const uint64_t v = in ? TkIdMatrix<MODE>{ids}.one(r * p.ld + lane) : 0ull;
    const unsigned long long stops = __ballot(in && tk_drows_listed(p.stop, p.n_stop, v));
    const bool found_stop = stops != 0ull;
    uint32_t live_end, x = 0, len = 0;
    tk_drows_stop_col(p, found_stop ? tk_ctz64(stops) : 0xFFFFFFFFu, e, &live_end);
    const bool keep = in && lane < live_end && tk_stream_keep(p, v, dec, n_ids, &x, &len);
    const unsigned long long kept = __ballot(keep), bad = __ballot(keep && !len);
    if (bad && lane == 0) tk_report_min(words + TK_STREAM_BAD_ID, r * p.W + tk_ctz64(bad));
    if (!keep) len = 0;
    uint32_t incl = tk_wave_scan_u32(len, (int)lane);
    uint32_t n_new = __shfl(incl, 63, 64);
    if (tail_len + n_new > cap) {  // (never, by the sizes refused at create: nothing is written behind the buffer all the same)
        if (lane == 0) words[TK_STREAM_OVERFLOW] = 1ull;
        n_new = len = incl = 0;
    }
    const uint32_t L = tail_len + n_new;
    if (live) {
        for (uint32_t i = lane; i < tail_len; i += 64) buf[i] = cur[r].tail[i];
        const uint8_t* src = ((x & TK_DEC_SPEC) ? spec_bytes : tok_bytes) + (x & ~TK_DEC_SPEC);
        uint8_t* dst = buf + tail_len + incl - len;
        for (uint32_t i = 0; i < len; ++i) dst[i] = src[i];
    }
    __syncthreads();  // the stop set and the row's bytes are in LDS

    // full hits, the first prefix to hold back, what to emit
    uint32_t best = TK_STOPS_NO_HIT, e0 = L;
    if (live && step && set.n) tk_stream_find_lane(B, L, set, lane, 64u, &best, &e0);
    best = tk_wave_min_u32(best);
    e0 = tk_wave_min_u32(e0);
    TkStreamCut cut{0u, state, hit, 0u};
    if (live) cut = tk_stream_decide(B, L, best, e0, found_stop, !step, set, mode);
    if (L - cut.tail_at > TK_STREAM_HOLD && live) {  // (never: a proper prefix has at most 63 bytes, a unit in front of it at most 3)
        if (lane == 0) words[TK_STREAM_OVERFLOW] = 1ull;
        cut.tail_at = L;
    }

    // the emitted bytes, repaired, into the row's slot
    uint32_t n_out = 0, n_ch = 0;
    uint8_t* const mine = scratch + r * slot;  // (indexed only where `live`)
    if (mode == TK_STREAM_MODE_BYTES) {
        for (uint32_t i = lane; i < cut.n_emit; i += 64) mine[i] = buf[i];
        n_out = cut.n_emit;
    } else {
        for (uint32_t q = 0; q < cut.n_emit; q += 1024u) {  // (n_emit is the wavefront's: every lane takes every turn)
            TkU8rNoStream none;
            const TkU8rCounts c = tk_stream_emit_lane(B, cut.n_emit, q + 16u * lane, mode, none);
            const uint32_t upto = tk_wave_scan_u32(c.out, (int)lane);
            n_ch += tk_wave_sum_u32(c.chars);
            if (c.out) {
                TkDecStores stores{mine};
                TkU8rStream<TkDecStores> out(stores, (unsigned long long)n_out + upto - c.out);
                (void)tk_stream_emit_lane(B, cut.n_emit, q + 16u * lane, mode, out);
                out.finish();
            }
            n_out += __shfl(upto, 63, 64);
        }
    }

    // the row's new slot, in the other copy
    if (!row) return;  // (no barrier below)
    const bool reset = op == TK_STREAM_OP_RESET && chosen;
    const uint32_t new_tail = reset ? 0u : live ? L - cut.tail_at : tail_len;
    for (uint32_t i = lane; i < new_tail; i += 64) next[r].tail[i] = live ? buf[cut.tail_at + i] : cur[r].tail[i];
    if (lane == 0) {
        next[r].state = reset ? (uint32_t)TK_STREAM_LIVE : cut.state;
        next[r].hit = reset ? TK_STOPS_NO_HIT : cut.hit;
        next[r].tail_len = new_tail;
        next[r].pad = 0u;
        next[r].n_kept = reset ? 0ull : n_kept + tk_popc64(kept);
        next[r].n_text = reset ? 0ull : n_text + n_out;
        next[r].n_chars = reset ? 0ull : n_chars + n_ch;
        out_len[r] = n_out;
        out_chars[r] = n_ch;
    }
}

// len, chars: what every row emitted into its slot.  Writes nothing when the row kernel reported a refusal.  text_off, char_off: R + 1;
// state, hit: R; text: the sum of len.  words[TK_STREAM_N_TEXT], [TK_STREAM_N_CHARS]: the totals.  The grid covers R + 1 entries.
__global__ __launch_bounds__(TK_STREAM_PACK_BLOCK) void tk_k_stream_pack(uint64_t R, const uint32_t* __restrict__ len, const uint32_t* __restrict__ chars,
                                                                         const TkStreamRow* __restrict__ next, const uint8_t* __restrict__ scratch, uint64_t slot,
                                                                         unsigned long long* __restrict__ words, uint8_t* __restrict__ text, uint64_t* __restrict__ text_off,
                                                                         uint64_t* __restrict__ char_off, uint32_t* __restrict__ state, uint32_t* __restrict__ hit) {
    __shared__ uint32_t sh_a[4], sh_b[4], sh_c[8], sh_d[8];
    __shared__ uint32_t off_s[TK_STREAM_PACK_BLOCK + 1];
    if (words[TK_STREAM_BAD_ROW] != ~0ull || words[TK_STREAM_BAD_ID] != ~0ull || words[TK_STREAM_OVERFLOW]) return;  // (the same in every thread)
    const uint64_t r0 = (uint64_t)blockIdx.x * TK_STREAM_PACK_BLOCK, r = r0 + threadIdx.x;
    uint32_t before_t = 0, before_c = 0;  // (the stream's scratch is below 2^32 bytes: the sums fit)
    for (uint64_t i = threadIdx.x; i < r0; i += TK_STREAM_PACK_BLOCK) before_t += len[i], before_c += chars[i];
    const unsigned long long base_t = tk_block_sum_256(before_t, sh_a), base_c = tk_block_sum_256(before_c, sh_b);
    const uint32_t my_t = r < R ? len[r] : 0u, my_c = r < R ? chars[r] : 0u;
    uint32_t tot_t, tot_c;
    const uint32_t ex_t = tk_block_exscan_256(my_t, &tot_t, sh_c), ex_c = tk_block_exscan_256(my_c, &tot_c, sh_d);
    off_s[threadIdx.x] = ex_t;
    if (threadIdx.x == 0) off_s[TK_STREAM_PACK_BLOCK] = tot_t;
    if (r <= R) {
        text_off[r] = base_t + ex_t;
        char_off[r] = base_c + ex_c;
    }
    if (r < R) {
        state[r] = next[r].state;
        hit[r] = next[r].hit;
    }
    if (r == R) {
        words[TK_STREAM_N_TEXT] = base_t + ex_t;
        words[TK_STREAM_N_CHARS] = base_c + ex_c;
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < tot_t; j += TK_STREAM_PACK_BLOCK) {  // byte j of the workgroup's text: the last row that starts at or before it
        uint32_t lo = 0, hi = TK_STREAM_PACK_BLOCK - 1;
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (off_s[mid] <= j) lo = mid;
            else hi = mid - 1;
        }
        text[base_t + j] = scratch[(r0 + lo) * slot + (j - off_s[lo])];
    }
}
