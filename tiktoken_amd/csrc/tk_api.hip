// C ABI + host orchestration of the MI355X BPE encode path (see include/tiktoken_amd.h).
// Host code here only builds tables, moves buffers and launches kernels; every byte of
// pre-tokenisation and merging is done by the kernels in tk_fused.h / tk_kernels.h.  There is no CPU path.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <functional>
#include <algorithm>
#include <array>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/tiktoken_amd.h"
#include "tk_decode.h"
#include "tk_decode_rows.h"
#include "tk_offsets.h"
#include "tk_utf8_repair.h"
#include "tk_stop_text.h"
#include "tk_stream.h"
#include "tk_padded.h"
#include "tk_split.h"
#include "tk_fingerprint.h"
#include "tk_jsonl.h"
#include "tk_sample_rows.h"
#include "tk_samples.h"
#include "tk_rows.h"
#include "tk_train.h"
#include "tk_fused.h"
#include "tk_mid_plan.h"
#include "tk_tables.h"
#include "tk_unicode_tables.inc"
#include "tk_regex_kernels.h"

static thread_local std::string g_err;
static double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
#define HIPCHK(expr)                                                                                    \
    do {                                                                                                \
        hipError_t e__ = (expr);                                                                        \
        if (e__ != hipSuccess)                                                                          \
            return fail(TK_RUNTIME_ERROR, std::string("HIP error: ") + hipGetErrorString(e__) + " at " #expr); \
    } while (0)

// ------------------------------------------------------------------------------------------
// Owners.  Every device buffer, page-locked block, stream and event of this file belongs to one of these and goes with it: nothing
// below (the pinned pool aside) calls hipFree / hipHostFree / hipStreamDestroy / hipEventDestroy itself.  Movable, not copyable; each converts to its raw handle.
// (The owner of a host thread that sends a block after the other to the device, Feed, stands further down, beside the copies it makes.)
// ------------------------------------------------------------------------------------------
struct Buf {  // device memory
    void* p = nullptr;
    size_t cap = 0;
    Buf() = default;
    Buf(Buf&& o) noexcept : p(o.p), cap(o.cap) {
        o.p = nullptr;
        o.cap = 0;
    }
    Buf& operator=(Buf&& o) noexcept {  // (the old block goes with `o`)
        std::swap(p, o.p);
        std::swap(cap, o.cap);
        return *this;
    }
    ~Buf() { if (p) (void)hipFree(p); }
    template <class T>
    T* as() const { return (T*)p; }
};
static int ensure(Buf& b, size_t bytes) {
    if (bytes <= b.cap && b.p) return TK_OK;
    if (b.p) HIPCHK(hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
    size_t want = bytes + bytes / 8 + 256;
    HIPCHK(hipMalloc(&b.p, want));
    b.cap = want;
    return TK_OK;
}
static void release(Buf& b) { b = Buf(); }  // the explicit early free
template <class T>
struct Pinned {  // a page-locked host block (the flags are the call site's)
    T* p = nullptr;
    Pinned() = default;
    Pinned(Pinned&& o) noexcept : p(o.p) { o.p = nullptr; }
    ~Pinned() { if (p) (void)hipHostFree(p); }
    hipError_t alloc(size_t bytes, unsigned flags) { return hipHostMalloc((void**)&p, bytes, flags); }
    operator T*() const { return p; }
};
struct Stream {  // default priority, hipStreamNonBlocking: the one kind this library makes (tk_create)
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream&& o) noexcept : s(o.s) { o.s = nullptr; }
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    operator hipStream_t() const { return s; }
};
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
    ~Event() { if (e) (void)hipEventDestroy(e); }
    hipError_t create(bool timing = false) { return timing ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, hipEventDisableTiming); }
    operator hipEvent_t() const { return e; }
};
template <class T>
struct HostResult {  // a result on its way to the caller, from the pinned pool (pinned_get) or from malloc: tk_free takes either
    T* p = nullptr;
    explicit HostResult(void* q = nullptr) : p((T*)q) {}
    HostResult(HostResult&& o) noexcept : p(o.p) { o.p = nullptr; }
    HostResult& operator=(HostResult&& o) noexcept {
        std::swap(p, o.p);
        return *this;
    }
    ~HostResult() { if (p) tk_free(p); }
    T* release() { return std::exchange(p, nullptr); }  // success: the caller's from here on
    operator T*() const { return p; }
};

struct KernelStat {
    double ms = 0;
    uint64_t launches = 0;
};

#define TK_NAUX 6  // side streams of the merge kernels
#define TK_NSET 4  // chunks in flight (work sets): the front kernel of chunk k + 1 runs while chunk k is merged and its tokens are placed

// Work buffers of ONE chunk in flight.  This list is the one place that names them: it declares the members and adds them up (WorkSet::bytes).
#define TK_WORK_BUFS(X)                                                                                                                                  \
    X(text_al) X(tile_sum) X(wide_ws) X(scan_sums) X(doc_first) X(brk) X(docb) X(cand) X(ss) X(si) X(starts) X(blockcnt) X(pstart) X(res) X(staging)     \
    X(listB) X(listC) X(counters) X(total) X(g_id) X(g_rk) X(g_nx) X(g_pv) X(g_lv) X(tile_np) X(tile_nt) X(mt_keys) X(mtab) X(movf) X(mcnt) X(wbin)       \
    X(deferred) X(big) X(rx_spec) X(rx_gst) X(rx_lnk) X(rx_exit) X(merge_work) X(find)
// (Members go in reverse order: the buffers, declared last, are freed first -- hipFree waits for the device -- then the events, the
// stream and the page-locked words.)
struct WorkSet {
    Pinned<uint32_t> h_counters;  // [2][TK_CNT_N]
    Pinned<uint64_t> h_total;     // [3]: tokens, pieces of the chunk; where its first disallowed special token starts (all ones: nowhere)
    Stream sb;                    // the set's back stage in a multi-chunk batch: back stages of different chunks overlap each other too
                                  // (they are chains of short latency-bound kernels, ~2 ms however small the chunk)
    Event ev_front;               // the front kernel is done
    Event ev_cnt;                 // ... and the deferred tiles: the counters are in h_counters
    Event ev_tot;                 // the chunk's token base and total are known (tok_bases[k + 1] written)
    Event ev_done;                // the back stage is done: totals and counters are in h_total / h_counters + TK_CNT_N, the buffers are free
    Event ev_fork, ev_join[TK_NAUX];  // fork / join of the merge kernels on the side streams
#define X(name) Buf name;
    TK_WORK_BUFS(X)
#undef X
    uint64_t bytes() const {  // device memory of the set
        uint64_t t = 0;
#define X(name) t += name.cap;
        TK_WORK_BUFS(X)
#undef X
        return t;
    }
};
#define TK_GROW (-1000)  // (internal) the batch has to be repeated with a larger miss data: encode_device_locked
#define TK_RESYNC (-1001)  // (internal) a deferred tile gave up while the host was not waiting: the batch is repeated, encode_device_locked
#define TK_SPEC_HIT (-1002)  // (internal) a chunk holds a disallowed special token (c->find_hit): the entry point reports it, no tokens are handed out
#ifndef TK_MT_DIV
#define TK_MT_DIV 128  // bytes of a chunk per slot of the in-call miss table (stage_front)
#endif

// What a caller asks of the chunk pipeline (stage_front .. chunk_finish, run_chunk): one chunk (n < 4 GiB bytes) of packed documents on the device.
enum class ChunkKind {
    Batch,                // documents, pre-tokenised and encoded
    SinglePiece,          // the whole buffer is one piece (encode_single_piece), no pre-tokenisation
    SinglePieceNoLookup,  // ... and is not looked up as a whole first (_byte_pair_encode)
    PieceStarts,          // debugging / test entry and training: piece offsets only (w.pstart), no tokens
};
struct ChunkAsk {  // (call sites name the fields they set, in this order)
    ChunkKind kind = ChunkKind::Batch;
    const uint8_t* d_text = nullptr;      // chunk text, readable 64 bytes past n
    const uint64_t* d_doc_off = nullptr;  // uint64 offsets of the chunk's documents (n_docs + 1 entries, absolute: `base` is subtracted)
    uint64_t n = 0, n_docs = 0, base = 0;
    uint32_t* d_out = nullptr;            // the batch's token buffer (null: piece starts only)
    uint64_t* d_tok_off = nullptr;        // the documents' token offsets (null: not wanted; the single-piece kinds are refused with one)
    bool use_special = false;
    bool single_piece() const { return kind == ChunkKind::SinglePiece || kind == ChunkKind::SinglePieceNoLookup; }
    bool piece_starts() const { return kind == ChunkKind::PieceStarts; }
};
// What every launch of the front kernel in a chunk is given behind the tables, the text and the base (tk_k_front's parameters, in their order; the
// list of deferred tiles and the internal debug bits are the launch's own: launch_front).  Filled once, by stage_front.
struct FrontArgs {
    int pat_id = 0;
    uint32_t *brk = nullptr, *docb = nullptr, *ss = nullptr, *si = nullptr;  // (docb, ss, si: null without special tokens in the chunk)
    TkFrontOut out{};
    TkMissKey* mt = nullptr;
    uint32_t mt_mask = 0;
    const uint32_t* gapb = nullptr;  // gap chars of the generic engine's split, or null
    int dbg = 0;                     // the core's debug word without the internal bits (the piece-offsets entry: piece starts only)
};
// What the front stage of a chunk leaves for its back stage.
struct ChunkJob {
    ChunkAsk ask;
    FrontArgs front;
    uint64_t ntiles = 0;
    bool find = false;  // the chunk's text was searched for disallowed special tokens (tk_k_spec_find -> w.find)
    bool docs_in_place = false;  // tk_k_place writes the documents' token offsets (w.doc_first is filled); else, if they are wanted, the chunk is empty: tk_k_docoff
    uint32_t index = 0;  // position of the chunk in its batch
    uint32_t mt_bits = 14;
    TkMissKey* mt = nullptr;   // the in-call miss table's keys (null: no table -- every missed piece gets an overflow entry)
    uint32_t ovf_base = 0;     // slots of the table = index of the first overflow entry of the miss data
    uint32_t ovf_cap = 0;      // overflow entries there is room for
    bool optimistic = false;   // the host has not waited for the deferred tiles' counters (stage_deferred): chunk_finish looks at them
};

// the chunk's entries of distinct missed pieces, as the kernels take them
static TkMiss miss_of(WorkSet& w, const ChunkJob& job) { return TkMiss{w.mtab.as<TkMissTab>(), w.movf.as<TkMissOvf>(), job.ovf_base, w.mcnt.as<uint8_t>()}; }

struct tk_core {
    int device = 0;
    // (members go in reverse order: the streams declared here outlive every buffer declared below)
    Stream stream;
    Stream aux[TK_NAUX];     // side streams: the merge kernels are independent of each other
    Stream cs_h2d, cs_d2h;   // copy streams of the host-buffer entry points (created on first use)
    Pinned<void> stage[2];   // page-locked staging buffers of tk_decode_batch (created on its first use)
    Event ev_stage[2];
    TkHostTables H;
    TkTables D;  // device view
    Buf t_stage1, t_stage2, t_bmp, t_byte_tab, t_short, t_mid, t_dec, t_piece, t_piece_off, t_tok_bytes, t_pair, t_pair2, t_byte_rank, t_xl, t_xfilter, t_spec_bytes, t_spec_off, t_spec_id, t_spec_head;
    uint32_t spec_max_len = 0;
    bool has_rx = false;  // the pat_str runs on the generic engine (tk_regex_kernels.h)
    bool has_rx_fb = false;  // a pat_str of the scanner families, compiled for the generic engine as well: the way out of stretches without certain starts (stage_deferred)
    TkRxCompiled rx_fb;
    uint64_t st_fallbacks = 0;  // chunks that took that way
    uint64_t st_regrown = 0;    // batches repeated with a larger miss data (encode_device_locked)
    uint64_t st_resynced = 0;   // batches repeated because a deferred tile gave up its walk while the host was not waiting for the counters (stage_deferred)
    bool defer_sync = false;    // ... from then on the host waits for them in every chunk, as it did up to round 5
    uint32_t defer_ppm = 1u << 12;  // deferred tiles per 2^20 tiles of the last chunk (the grid of the kernel that finishes them; first guess: one in 256 -- 4400 empty workgroups of that kernel were 0.06 ms of a first 1 GiB call)
    TkRxDev rx{};
    Buf t_rx_ins, t_rx_sets, t_rx_ranges, t_rx_first, t_rx_s1, t_rx_s2, t_rx_dtrans, t_rx_dascii, t_rx_ds1, t_rx_ds2;
    int rx_form = TK_RX_FORM_PROGRAM;  // how the generic engine's kernels match: the pattern's DFA where it has one ($TIKTOKEN_AMD_RX_MATCHER)
    std::mutex mu;
    // workspace: per chunk in flight, and what a whole call shares
    WorkSet ws[TK_NSET];
    Buf text, doc_off, out_tokens, out_tok_off, allowed, tok_bases;  // tok_bases[k]: tokens of the chunks before chunk k (on the device)
    // The disallowed special tokens of a checked call (tk_encode_batch_checked and its kin): `disallowed` is a byte per special token, as
    // `allowed`; find_on is set by the entry point, under the mutex, for the duration of its call, and every chunk's front stage then runs
    // tk_k_spec_find.  find_hit: where in the batch the first hit starts (chunk_finish).
    Buf disallowed;
    bool find_on = false;
    uint64_t find_hit = ~0ull;
    uint64_t st_find_launches = 0;  // launches of that scan since the core was made
    uint64_t st_mark_launches = 0;  // launches of the marking pair (tk_k_spec_cand + tk_k_spec_resolve) since the core was made
    uint64_t st_train_table_moves = 0, st_train_blob_moves = 0;  // of the last tk_train_bpe: word tables rehashed into a larger one, word blobs copied into a larger one
    // Streams of the back stages of a multi-chunk batch.  HIP multiplexes its streams onto a few hardware queues (four by default), and
    // two streams that share a queue run one after the other: the back stage of chunk k, queued behind the front kernel of chunk
    // k + 1, then waits for that kernel to END instead of running beside it (seen in the kernel timeline of round 4: no overlap at all).
    // Which streams share a queue cannot be asked; it is found out once per caller's stream (pick_back_streams).
    hipStream_t back_for = nullptr;  // the front stream the choice was made for
    struct BackChoice {
        hipStream_t s[3];
        int n;
    };
    std::map<hipStream_t, BackChoice> back_known;  // ... and the choices made for other front streams before
    bool back_probed = false;
    hipStream_t back_s[3] = {};      // streams that share a queue neither with back_for nor with each other (as far as the pool has any)
    int n_back = 0;
    Pinned<uint32_t> h_probe;        // page-locked words of the probe: [0] the gate, [1 ..] one per candidate (made by the first probe)
    Buf out_tokens_alt, out_tok_off_alt;  // the other pair of result buffers of tk_encode_batch_device (tk_set_output_buffers(core, 2))
    uint32_t out_bufs = 1;
    bool ovf_full = false;  // a batch has asked for more overflow entries of the miss data than the default: room for the worst case from then on
    uint64_t chunk_bytes = 1ull << 30;  // one chunk per GiB: smaller chunks pipeline (stage_front / stage_back) but pay the merge kernels' fixed latency per chunk
    int dbg = 0;
    uint32_t n_cu = 256;             // compute units of the device
    uint32_t rx_grid_cap = 65536;    // most workgroups of tk_k_rx_speculate_staged (each walks the stretches with the stride of the grid: a chunk of more than 2 GiB, or $TIKTOKEN_AMD_RX_GRID_CAP)
    uint32_t n_dec = 0;  // entries of the device decode table (0: ids too sparse for a direct table -- decode stays on the host)
    Buf d_tok, d_lens, d_bsum, d_tboff, d_bytes, d_bytes_alt, d_boff;  // decode workspace (d_bytes_alt: the other range's bytes on their way to the host)
    // Token spans (tk_offsets.h).  t_cw: the second per-id table, beside t_dec and with its indexing (tk_char_word); d_span: byte_start and
    // char_start of every token; d_span_blk: per workgroup {chars, mark key, document start bytes / chars}; d_span_marks: document starts over
    // the tokens, d_span_bmarks: over the decoded bytes; d_span_doc: byte_off, char_off, then the TK_SPAN_WORDS report words.
    Buf t_cw, d_span, d_span_blk, d_span_marks, d_span_bmarks, d_span_doc;
    // Training rows (tk_rows.h), apart from everything above: d_rows: ids, doc and pos of every position; d_rows_seg: the TK_ROWS_WORDS report
    // words, cu_seqlens, row_seg; d_rows_marks: document starts over the stream positions; d_rows_blk: segment starts per workgroup.
    Buf d_rows, d_rows_seg, d_rows_marks, d_rows_blk;
    // Padded inputs (tk_padded.h), apart from everything above: d_pad: ids and mask of every position; d_pad_row: len, row_doc, row_tok of
    // every row; d_pad_doc: doc_row; d_pad_cnt: the TK_PAD_WORDS report words and the doc_row a call counts in until it is accepted.
    Buf d_pad, d_pad_row, d_pad_doc, d_pad_cnt;
    // Text chunks (tk_split.h), apart from everything above: d_split: the arrays of every chunk and doc_chunk; d_split_work: the report words,
    // the class planes, the cut and spec planes, exit_at / join_at of every block and the starts per count block -- everything a call computes
    // until it is accepted.  st_split: the counters of the last call (TK_SPLIT_ST_*).
    Buf d_split, d_split_work;
    // JSON Lines (tk_jsonl.h), apart from everything above: d_jsonl: text, doc_off, line, line_off and status of the last call that
    // succeeded; d_jsonl_work: the report words, the tiles' summaries and entry states, the escaped plane, the tiles' counts; d_jsonl_lines:
    // everything per line and per block of lines -- what a call computes until it is accepted; d_jsonl_in: the bytes of a host call.
    Buf d_jsonl, d_jsonl_work, d_jsonl_lines, d_jsonl_in;
    // Fingerprints (tk_fingerprint.h), apart from everything above: d_fp: the signatures of a call whose caller wants band keys without
    // them, and the four result arrays of the host entries; d_fp_in: tokens and tok_off of a host call.
    // fp_done: recorded behind every call that has used d_fp, on that call's stream; the next such call's stream waits for it first.
    Buf d_fp, d_fp_in;
    Event fp_done;
    uint64_t st_split[TK_SPLIT_STATS] = {0, 0, 0, 0};
    // Supervised samples (tk_samples.h), apart from everything above: d_smp: ids, labels and mask of every position; d_smp_row: full_len, len,
    // n_trained of every sample; d_smp_cnt: the TK_SMP_WORDS report words, the role table, pstart and the per-sample figures a call counts in
    // until it is accepted; d_smp_in: part_role and sample_off of a host-text call.
    Buf d_smp, d_smp_row, d_smp_cnt, d_smp_in;
    // Packed sample rows (tk_sample_rows.h), apart from everything above: d_srow: ids, labels, seg and pos of every position; d_srow_row: the
    // per-sample and per-row arrays and cu_seqlens; d_srow_cnt: the report words, the role table and everything a call computes until it is
    // accepted (the write pass reads pstart, c, f, row_sample and row_seg there); d_srow_in: part_role and sample_off of a host-text call.
    Buf d_srow, d_srow_row, d_srow_cnt, d_srow_in;
    // Decoded id matrices (tk_decode_rows.h), apart from everything above: d_drows_tok: the kept ids; d_drows_row: tok_off, n_kept and stop_col
    // of every row; d_drows_cnt: the TK_DROWS_WORDS report words, the rows' stop words and the tile counts a call computes until it is
    // accepted; d_drows_in: the matrix, begin and end of a host call.
    Buf d_drows_tok, d_drows_row, d_drows_cnt, d_drows_in;
    // UTF-8 repair (tk_utf8_repair.h), apart from everything above: d_u8r_text: the repaired text; d_u8r_doc: text_off, char_off, repl_off;
    // d_u8r_cnt: the TK_U8R_WORDS report words, the workgroups' sums, the lanes' places, the documents' prefixes and the bitmap of document
    // starts -- everything a call computes until it is accepted.
    Buf d_u8r_text, d_u8r_doc, d_u8r_cnt;
    // Stop strings (tk_stop_text.h), apart from everything above: d_stop_text: the cut text; d_stop_doc: text_off, hit and (id matrices)
    // n_tok; d_stop_cnt: the TK_STOPS_WORDS report words, the stop set, the documents' words, kept lengths and hits, the workgroups' sums --
    // everything a call computes until it is accepted.
    Buf d_stop_text, d_stop_doc, d_stop_cnt;
    // Small calls (tk_k_small) do not take `mu`: the reference's normal use is several threads on one Encoding (core.py:175, a thread pool
    // over encode; lib.rs:232-238 keeps a regex per thread for it), and a small call needs nothing of the shared workspace -- a slot of its
    // own (page-locked text and result buffers the kernel reads and writes directly, merge scratch, a stream) is all.  A caller takes a
    // free slot (one atomic exchange), launches, watches the slot's completion word.
    struct SmallSlot {
        std::atomic<int> busy{0};
        std::atomic<int> state{0};  // 0 idle, 1 ready (input written, waiting for a launch), 2 launched
        Pinned<uint8_t> in;       // page-locked, device-visible: text of the call
        Pinned<uint32_t> out;     // page-locked, device-visible: its result
        void *d_in = nullptr, *d_out = nullptr;
        uint32_t seq = 0, n = 0;
        Buf ws;
        Stream s;
        bool ready = false;       // every piece above has been made (set last: a first use that failed half-way is repeated by the next caller)
    };
    SmallSlot small[TK_SMALL_SLOTS];
    // Callers of small calls that arrive together go out in ONE launch (flat combining): whoever gets this mutex -- try_lock: nobody waits for
    // it -- launches every slot that is ready, his own included or not (someone else may have taken it along already); the others watch
    // their completion words.  The streams of the launches take turns so that consecutive batches overlap on the device.
    std::mutex small_launch_mu;
    std::atomic<int> small_active{0};  // callers inside encode_small / encode_mid
    std::atomic<int> mid_skip{0};     // calls that skip encode_mid (set when an attempt found the text unfit for the small kernel)
    std::atomic<int> mid_fail_run{0};  // such attempts in a row
    bool mid_cut = false;             // an ASCII letter followed by a space is a certain piece start of this pattern: documents of 2 .. 128 KiB are cut there
    uint64_t st_mid_calls = 0;
    Stream small_s[4];
    uint32_t small_turn = 0;
    uint64_t st_small_launches = 0, st_small_calls = 0;
    std::vector<uint8_t> sorted_blob;  // token_byte_values(), packed (built on first use)
    std::vector<uint64_t> sorted_off;
    // instrumentation
    bool profiling = false;
    std::map<std::string, KernelStat> stats;
    struct TimedPair {
        std::string name;
        Event a, b;
    };
    std::vector<TimedPair> pending;
    uint64_t st_bytes = 0, st_pieces = 0, st_tokens = 0, st_docs = 0, st_medium = 0, st_long = 0;
    uint64_t st_chunks = 0;
    double host_us[6] = {0, 0, 0, 0, 0, 0};  // host time of the last call: front stages, back stages (of which: waiting for the front kernel), finish waits, total
};

// ------------------------------------------------------------------------------------------
// Pinned host memory, pooled.  Results of the host-buffer entry points are returned in page-locked buffers (the D2H copy runs at PCIe
// speed and the caller reads them in place: no second copy); pinning a gigabyte costs far more than filling it, so released buffers are
// kept for the next call.  tk_free() recognises them.
// ------------------------------------------------------------------------------------------
struct PinnedBuf {
    void* p;
    size_t cap;
    bool used;
};
static std::mutex g_pin_mu;
static std::vector<PinnedBuf> g_pin;
static void* pinned_get(size_t bytes) {
    if (bytes < 64) bytes = 64;
    std::lock_guard<std::mutex> lk(g_pin_mu);
    PinnedBuf* best = nullptr;
    for (auto& b : g_pin)
        if (!b.used && b.cap >= bytes && (!best || b.cap < best->cap)) best = &b;
    if (best && best->cap <= 4 * bytes + (64u << 20)) {
        best->used = true;
        return best->p;
    }
    void* p = nullptr;
    const size_t cap = bytes + bytes / 4 + 4096;
    if (hipHostMalloc(&p, cap, hipHostMallocPortable) != hipSuccess) return nullptr;
    size_t free_bytes = 0;  // keep the pool bounded: drop idle buffers beyond 8 GiB
    for (size_t i = 0; i < g_pin.size();) {
        if (!g_pin[i].used && (free_bytes += g_pin[i].cap) > (8ull << 30)) {
            (void)hipHostFree(g_pin[i].p);
            g_pin.erase(g_pin.begin() + i);
        } else {
            ++i;
        }
    }
    g_pin.push_back(PinnedBuf{p, cap, true});
    return p;
}
static bool pinned_release(void* p) {
    if (!p) return false;
    std::lock_guard<std::mutex> lk(g_pin_mu);
    for (auto& b : g_pin)
        if (b.p == p) {
            b.used = false;
            return true;
        }
    return false;
}

template <class F>
static int timed(tk_core* c, hipStream_t s, const char* name, F&& f) {
    if (!c->profiling) {
        f();
        HIPCHK(hipGetLastError());
        return TK_OK;
    }
    tk_core::TimedPair t{name, {}, {}};
    hipError_t e = t.a.create(true);
    if (e == hipSuccess) e = t.b.create(true);
    if (e == hipSuccess) e = hipEventRecord(t.a, s);
    if (e == hipSuccess) {
        f();
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(t.b, s);
    if (e != hipSuccess) return fail(TK_RUNTIME_ERROR, std::string("HIP error: ") + hipGetErrorString(e) + " in " + name);  // (no event pair is left behind by a failed launch)
    c->pending.push_back(std::move(t));
    return TK_OK;
}
static int drain_events(tk_core* c) {
    std::vector<tk_core::TimedPair> pending;  // (every pair goes with this list, whichever wait fails)
    pending.swap(c->pending);
    for (auto& pe : pending) {
        float ms = 0;
        HIPCHK(hipEventSynchronize(pe.b));
        HIPCHK(hipEventElapsedTime(&ms, pe.a, pe.b));
        KernelStat& ks = c->stats[pe.name];
        ks.ms += ms;
        ks.launches += 1;
    }
    return TK_OK;
}
// a pass of timed launches: the timed pairs go whatever happened to it; the first error
template <class F>
static int drained(tk_core* c, F&& f) {
    const int rc = f();
    const int rc2 = drain_events(c);
    return rc != TK_OK ? rc : rc2;
}
#define TRY(x)                      \
    do {                            \
        int rc__ = (x);             \
        if (rc__ != TK_OK) return rc__; \
    } while (0)

static int upload(Buf& b, const void* src, size_t bytes) {
    TRY(ensure(b, bytes ? bytes : 16));
    if (bytes) HIPCHK(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
    return TK_OK;
}
// The opening of the entries whose batch is on the device -- tk_decode_batch_device, tk_token_spans_device, tk_pack_rows_device,
// tk_pad_batch_device, tk_assemble_samples_device (`args`: the entry's own pointers are there): run(s) under the core's mutex, on its
// device, s the caller's stream or the core's, and the timed launches drained behind it.
template <class Run>
static int device_pass(tk_core* c, bool args, void* stream, Run&& run) {
    if (!c) return fail(TK_VALUE_ERROR, "core is null");
    if (!args) return fail(TK_VALUE_ERROR, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(hipSetDevice(c->device));
    return drained(c, [&] { return run(stream ? (hipStream_t)stream : c->stream); });
}
// A buffer carved into arrays: add(bytes) gives the offset of the next one, every one at a multiple of 16 bytes (the write passes store 16
// bytes at a time); `total` is what to ask ensure() for, once; carved<T>(buf, offset) is the array.
struct Carve {
    uint64_t total = 0;
    uint64_t add(uint64_t bytes) { return std::exchange(total, total + ((bytes + 15) & ~15ull)); }
};
template <class T>
static T* carved(const Buf& b, uint64_t off) { return (T*)(b.as<uint8_t>() + off); }

extern "C" void tk_free(void* p);
extern "C" const char* tk_last_error(void) { return g_err.c_str(); }

extern "C" int tk_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int tk_create(const uint8_t* ranks_blob, const uint64_t* ranks_off, const uint32_t* ranks_ids, uint64_t n_ranks,
                         const uint8_t* spec_blob, const uint64_t* spec_off, const uint32_t* spec_ids, uint64_t n_spec,
                         const char* pat_str, int device, tk_core** out) {
    if (!out) return fail(TK_VALUE_ERROR, "out is null");
    *out = nullptr;
    {
        TkPat pp;
        TkRxCompiled prx;
        const std::string perr = tk_compile_pattern(pat_str, &pp, nullptr, &prx);
        if (!perr.empty()) return fail(TK_UNSUPPORTED, perr);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(TK_RUNTIME_ERROR, "no HIP device available: tiktoken_amd has no CPU path");
    if (device < 0 || device >= ndev) return fail(TK_VALUE_ERROR, "device ordinal out of range");
    struct Destroy {
        void operator()(tk_core* core) const { tk_destroy(core); }
    };
    std::unique_ptr<tk_core, Destroy> owner(new tk_core());  // (every early return below destroys what has been made; released into *out at the end)
    tk_core* c = owner.get();
    c->device = device;
    std::string err = tk_build_tables(ranks_blob, ranks_off, ranks_ids, n_ranks, spec_blob, spec_off, spec_ids, n_spec, pat_str, &c->H);
    if (!err.empty()) return fail(TK_VALUE_ERROR, err);
    if (hipSetDevice(device) != hipSuccess) return fail(TK_RUNTIME_ERROR, "hipSetDevice failed");
    if (c->stream.create() != hipSuccess) return fail(TK_RUNTIME_ERROR, "hipStreamCreate failed");
    // All streams at the default priority.  (Measured, profiles/r03_stream_priority.txt: the mere existence of high-priority streams
    // in the process slows the front kernel from 5.76 to 6.28 ms per GiB even while nothing runs on them.)
    for (int i = 0; i < TK_NAUX; ++i)
        if (c->aux[i].create() != hipSuccess) return fail(TK_RUNTIME_ERROR, "hipStreamCreate failed");
    for (WorkSet& w : c->ws) {
        if (w.sb.create() != hipSuccess) return fail(TK_RUNTIME_ERROR, "hipStreamCreate failed");
        for (Event* e : {&w.ev_front, &w.ev_cnt, &w.ev_tot, &w.ev_done, &w.ev_fork})
            if (e->create() != hipSuccess) return fail(TK_RUNTIME_ERROR, "hipEventCreate failed");
        for (int i = 0; i < TK_NAUX; ++i)
            if (w.ev_join[i].create() != hipSuccess) return fail(TK_RUNTIME_ERROR, "hipEventCreate failed");
        if (w.h_counters.alloc(2 * TK_CNT_N * 4 + 64, hipHostMallocDefault) != hipSuccess || w.h_total.alloc(64, hipHostMallocDefault) != hipSuccess)
            return fail(TK_RUNTIME_ERROR, "hipHostMalloc failed");
    }
    const TkHostTables& H = c->H;
    auto upload_rx = [&](const TkRxCompiled& X) -> int {  // the program of the generic engine
        TRY(upload(c->t_rx_ins, X.ins.data(), X.ins.size() * sizeof(TkRxIns)));
        TRY(upload(c->t_rx_sets, X.sets.data(), X.sets.size() * sizeof(TkRxSet)));
        TRY(upload(c->t_rx_ranges, X.ranges.data(), X.ranges.size() * 4));
        TRY(upload(c->t_rx_first, X.first.data(), X.first.size() * 4));
        TRY(upload(c->t_rx_s1, tk_rx_props_stage1(), 0x1100));
        TRY(upload(c->t_rx_s2, tk_rx_props_stage2(), (size_t)tk_rx_props_blocks() * 256));
        c->rx = TkRxDev{c->t_rx_ins.as<TkRxIns>(), c->t_rx_sets.as<TkRxSet>(), c->t_rx_ranges.as<uint32_t>(), c->t_rx_s1.as<uint8_t>(),
                        c->t_rx_s2.as<uint8_t>(), (uint32_t)X.ins.size(), (uint32_t)X.sets.size(), (uint32_t)X.ranges.size() / 2,
                        c->t_rx_first.as<uint32_t>(), (uint32_t)X.first.size() / 8, nullptr, nullptr, nullptr, nullptr, 0u, 0u, 0u};
        c->rx_form = TK_RX_FORM_PROGRAM;
        // the pattern's DFA (tk_regex_dfa.inc), where it has one: $TIKTOKEN_AMD_RX_MATCHER = program | dfa | flat (the default) chooses the
        // kernels' form -- "dfa" keeps the piece-by-piece speculative lane, "program" interprets the backtracking program as before
        const char* want = getenv("TIKTOKEN_AMD_RX_MATCHER");
        if (X.has_dfa() && !(want && !strcmp(want, "program"))) {
            std::vector<uint16_t> tr(X.dfa_trans);
            tr.resize((tr.size() + 1) & ~(size_t)1, 0);  // (whole 32-bit words: the kernels copy it to LDS word by word)
            TRY(upload(c->t_rx_dtrans, tr.data(), tr.size() * 2));
            TRY(upload(c->t_rx_dascii, X.dfa_ascii.data(), 384));
            TRY(upload(c->t_rx_ds1, X.dfa_s1.data(), X.dfa_s1.size() * 2));
            TRY(upload(c->t_rx_ds2, X.dfa_s2.data(), X.dfa_s2.size()));
            c->rx.dfa_trans = c->t_rx_dtrans.as<uint16_t>();
            c->rx.dfa_ascii = c->t_rx_dascii.as<uint8_t>();
            c->rx.dfa_s1 = c->t_rx_ds1.as<uint16_t>();
            c->rx.dfa_s2 = c->t_rx_ds2.as<uint8_t>();
            c->rx.dfa_ncls = X.dfa_ncls;
            c->rx.dfa_nstates = X.dfa_nstates;
            c->rx.dfa_flags = X.dfa_flags;
            c->rx_form = (want && !strcmp(want, "dfa")) ? TK_RX_FORM_DFA : TK_RX_FORM_DFA_FLAT;
            if (X.dfa_flags & 1u) c->rx_form += TK_RX_FORM_DFA_PREV - TK_RX_FORM_DFA;  // (a pattern that looks behind: the instantiations that read the char in front of a match)
        }
        return TK_OK;
    };
    // the class of every code point below U+10000 in one table (TkTables::uc_bmp), from the two stages
    auto upload_bmp = [&](const uint8_t* s1, const uint8_t* s2) -> int {
        std::vector<uint8_t> bmp(65536);
        for (uint32_t cp = 0; cp < 65536u; ++cp) bmp[cp] = s2[(uint32_t)s1[cp >> 8] * 256u + (cp & 255u)];
        return upload(c->t_bmp, bmp.data(), bmp.size());
    };
    if (H.rx.empty()) {
        // a pattern of the scanner families: compiled for the generic engine as well, for stretches of text without certain starts
        // (stage_deferred); a family member the generic compiler cannot take keeps its scanners alone
        if (tk_rx_compile(pat_str, &c->rx_fb).empty()) {
            TRY(upload_rx(c->rx_fb));
            c->has_rx_fb = true;
        }
        TRY(upload(c->t_stage1, tk_uc_stage1, sizeof tk_uc_stage1));
        TRY(upload(c->t_stage2, tk_uc_stage2, sizeof tk_uc_stage2));
        TRY(upload_bmp(tk_uc_stage1, tk_uc_stage2));
        uint32_t bt[256 * 2];
        tk_build_byte_table(tk_uc_stage1, tk_uc_stage2, bt);
        TRY(upload(c->t_byte_tab, bt, sizeof bt));
    } else {
        // The generic engine splits (tk_regex_kernels.h) and hands every piece start to the front kernel as a hard start; the scanners
        // then run over a class table in which every char is a lower-case letter: a piece is a run of letters up to the next hard start.
        std::vector<uint8_t> s1(0x1100, 0), s2(256, (uint8_t)TK_C_LL);
        TRY(upload(c->t_stage1, s1.data(), s1.size()));
        TRY(upload(c->t_stage2, s2.data(), s2.size()));
        TRY(upload_bmp(s1.data(), s2.data()));
        uint32_t bt[256 * 2];
        tk_build_byte_table(s1.data(), s2.data(), bt);
        TRY(upload(c->t_byte_tab, bt, sizeof bt));
        TRY(upload_rx(H.rx));
        c->has_rx = true;
    }
    TRY(upload(c->t_short, H.short_tab.data(), H.short_tab.size() * sizeof(TkShortSlot)));
    TRY(upload(c->t_mid, H.mid_tab.data(), H.mid_tab.size() * sizeof(TkPieceSlot)));
    TRY(upload(c->t_piece, H.piece.data(), H.piece.size() * sizeof(TkPieceSlot)));
    TRY(upload(c->t_piece_off, H.piece_off.data(), H.piece_off.size() * 4));
    TRY(upload(c->t_tok_bytes, H.tok_bytes.data(), H.tok_bytes.size()));
    TRY(upload(c->t_pair, H.pair8.empty() ? (const void*)H.pair.data() : (const void*)H.pair8.data(),
                     H.pair8.empty() ? H.pair.size() * sizeof(TkPairSlot) : H.pair8.size() * 8));
    TRY(upload(c->t_pair2, H.pair2.data(), H.pair2.size() * 4));
    TRY(upload(c->t_byte_rank, H.byte_rank, sizeof H.byte_rank));
    TRY(upload(c->t_xl, H.xl.data(), H.xl.size() * sizeof(TkXlSlot)));
    TRY(upload(c->t_xfilter, H.xfilter.data(), H.xfilter.size() * 4));
    TRY(upload(c->t_spec_bytes, H.spec_bytes.data(), H.spec_bytes.size()));
    TRY(upload(c->t_spec_off, H.spec_off.data(), H.spec_off.size() * 4));
    TRY(upload(c->t_spec_id, H.spec_id.data(), H.spec_id.size() * 4));
    TkTables& D = c->D;
    D.uc_stage1 = c->t_stage1.as<uint8_t>();
    D.uc_stage2 = c->t_stage2.as<uint8_t>();
    D.uc_bmp = c->t_bmp.as<uint8_t>();
    D.byte_tab = c->t_byte_tab.as<uint32_t>();
    D.short_tab = H.short_tab.empty() ? nullptr : c->t_short.as<TkShortSlot>();
    D.short_mask = H.short_mask;
    D.short_shift = H.short_shift;
    D.mid_tab = c->t_mid.as<TkPieceSlot>();
    D.mid_mask = H.mid_mask;
    D.mid_shift = H.mid_shift;
    D.piece = c->t_piece.as<TkPieceSlot>();
    D.piece_off = c->t_piece_off.as<uint32_t>();
    D.piece_mask = H.piece_mask;
    D.max_token_len = H.max_token_len;
    D.tok_bytes = c->t_tok_bytes.as<uint8_t>();
    D.pair = H.pair8.empty() ? c->t_pair.as<TkPairSlot>() : nullptr;
    D.pair8 = H.pair8.empty() ? nullptr : c->t_pair.as<uint64_t>();
    D.pair_mask = H.pair_mask;
    D.pair2 = c->t_pair2.as<uint32_t>();
    D.byte_rank = c->t_byte_rank.as<uint32_t>();
    D.xl = c->t_xl.as<TkXlSlot>();
    D.xl_mask = H.xl_mask;
    D.xfilter = c->t_xfilter.as<uint32_t>();
    D.spec_bytes = c->t_spec_bytes.as<uint8_t>();
    D.spec_off = c->t_spec_off.as<uint32_t>();
    D.spec_id = c->t_spec_id.as<uint32_t>();
    {
        std::vector<uint32_t> head;
        tk_spec_tables(H, head, D);
        TRY(upload(c->t_spec_head, head.data(), head.size() * 4));
        D.spec_head = c->t_spec_head.as<uint32_t>();
    }
    D.pattern = H.pattern;
    D.pat = H.pat;
    memcpy(D.cert, H.cert, sizeof D.cert);
    // a document of a few KiB is cut at "letter, then space" when that is a certain piece start of the pattern (encode_mid): both cases of letter,
    // in the family's table and in what was derived for this pattern
    c->mid_cut = tk_mid_cut_certain(H.cert) && !(c->dbg & TK_DBG_NO_MID_CUT);
    for (size_t k = 0; k + 1 < H.spec_off.size(); ++k) c->spec_max_len = std::max(c->spec_max_len, H.spec_off[k + 1] - H.spec_off[k]);
    {  // decode table: id -> {offset into the token / special blob, length}
        uint32_t max_id = 0;
        max_id = H.max_rank;
        for (const auto& kv : H.spec_decoder) max_id = std::max(max_id, kv.first);
        if (max_id < (1u << 26)) {
            std::vector<uint2> dec((size_t)max_id + 1, make_uint2(0, 0));
            for (const auto& kv : H.spec_decoder) dec[kv.first] = make_uint2(kv.second.first | TK_DEC_SPEC, kv.second.second);
            H.for_each_token([&](uint32_t r, uint32_t o, uint32_t l) { dec[r] = make_uint2(o, l); });  // (lib.rs:347-351: decoder first)
            TRY(upload(c->t_dec, dec.data(), dec.size() * sizeof(uint2)));
            c->n_dec = max_id + 1;
            // ... and id -> char word (core.py:330-331: what the token adds to the char count, whether it starts inside a char), special tokens from their text
            std::vector<uint32_t> cw((size_t)max_id + 1, 0u);
            for (const auto& kv : H.spec_decoder) cw[kv.first] = tk_char_word(H.spec_bytes.data() + kv.second.first, kv.second.second);
            H.for_each_token([&](uint32_t r, uint32_t o, uint32_t l) { cw[r] = tk_char_word(H.tok_bytes.data() + o, l); });
            TRY(upload(c->t_cw, cw.data(), cw.size() * sizeof(uint32_t)));
        }
    }
    if (const char* e = getenv("TIKTOKEN_AMD_CHUNK_BYTES")) {
        uint64_t v = strtoull(e, nullptr, 10);
        if (v >= 4096 && v <= (3ull << 30)) c->chunk_bytes = v;
    }
    if (const char* e = getenv("TIKTOKEN_AMD_DEBUG")) {
        c->dbg = atoi(e);
        int unknown = c->dbg;
        for (int b : TK_DBG_USER) unknown &= ~b;
        if (unknown)  // (the phase stops and merge hooks of earlier rounds are compile-time parameters now: tools/build_variant.sh)
            fprintf(stderr, "tiktoken_amd: TIKTOKEN_AMD_DEBUG: 0x%x holds no debug bits (ignored)\n", (unsigned)unknown);
    }
    if (const char* e = getenv("TIKTOKEN_AMD_RX_GRID_CAP")) {  // (tests: most workgroups of the staged speculative pass, so that a small input makes every workgroup take several stretches)
        const int k = atoi(e);
        if (k >= 1 && k <= 65536) c->rx_grid_cap = (uint32_t)k;
    }
    {
        int cu = 0;
        if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cu > 0) c->n_cu = (uint32_t)cu;
    }
    {
        // tk_k_front reads some of its arguments from the kernarg segment again, at offsets taken from TkFrontArgs (tk_fused.h, phases E and F): one launch
        // of a kernel with the same parameter list and arguments of distinct values checks that the compiler lays the segment out that way
        TkTables Tt{};
        uint64_t v = 0x1000;
        auto nextp = [&]() { v += 0x1010; return (uintptr_t)v; };
        Tt.short_tab = (const TkShortSlot*)nextp(); Tt.short_mask = (uint32_t)nextp(); Tt.short_shift = (uint32_t)nextp();
        Tt.mid_tab = (const TkPieceSlot*)nextp(); Tt.mid_mask = (uint32_t)nextp(); Tt.mid_shift = (uint32_t)nextp();
        Tt.xl = (decltype(Tt.xl))nextp(); Tt.xl_mask = (uint32_t)nextp(); Tt.max_token_len = (uint32_t)nextp();
        Tt.tok_bytes = (const uint8_t*)nextp(); Tt.piece = (const TkPieceSlot*)nextp(); Tt.piece_off = (const uint32_t*)nextp(); Tt.piece_mask = nextp();
        Tt.n_spec = (uint32_t)nextp(); Tt.spec_bytes = (const uint8_t*)nextp(); Tt.spec_id = (const uint32_t*)nextp(); Tt.spec_off = (const uint32_t*)nextp();
        TkFrontOut fo{};
        fo.starts = (uint32_t*)nextp(); fo.tile_np = (uint32_t*)nextp(); fo.res = (uint32_t*)nextp(); fo.tile_sum = (uint8_t*)nextp();
        fo.data.tab = (TkMissTab*)nextp(); fo.data.ovf = (TkMissOvf*)nextp(); fo.data.ovf_base = (uint32_t)nextp(); fo.ovf_cap = (uint32_t)nextp();
        fo.listC = (uint32_t*)nextp(); fo.counters = (uint32_t*)nextp();
        Buf okb;
        TRY(ensure(okb, 64));
        (void)hipMemsetAsync(okb.p, 0, 4, c->stream);
        hipLaunchKernelGGL(tk_k_front_args_check, dim3(1), dim3(64), 0, c->stream, Tt, (const uint8_t*)nextp(), (uint64_t)nextp(), (uint64_t)nextp(), (const uint32_t*)nextp(),
                           (const uint32_t*)nextp(), (const uint32_t*)nextp(), (const uint32_t*)nextp(), fo, (TkMissKey*)nextp(), (uint32_t)nextp(), (uint32_t*)nextp(),
                           (const uint32_t*)nextp(), (int)nextp(), okb.as<uint32_t>());
        uint32_t ok = 0;
        const bool copied = hipMemcpyAsync(&ok, okb.p, 4, hipMemcpyDeviceToHost, c->stream) == hipSuccess && hipStreamSynchronize(c->stream) == hipSuccess;
        release(okb);
        if (!copied || ok != 1u) return fail(TK_RUNTIME_ERROR, "internal error: the front kernel's arguments do not lie in the kernarg segment as TkFrontArgs says");
    }
    *out = owner.release();
    return TK_OK;
}

extern "C" void tk_destroy(tk_core* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c;  // (its members free what they own)
}

static uint32_t grid_for(uint64_t items, uint32_t per_block, uint32_t cap) {
    uint64_t g = (items + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (uint32_t)g;
}

// one launch of the front kernel for the chunk of `job`: the instance of its pattern, with the arguments stage_front has put together
template <int MODE>
static void launch_front(tk_core* c, const ChunkJob& job, dim3 grid, hipStream_t s, uint32_t* deferred, int internal_dbg) {
    const ChunkAsk& a = job.ask;
    const FrontArgs& f = job.front;
    auto go = [&](auto* kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, c->D, a.d_text, a.n, a.base, f.brk, f.docb, f.ss, f.si, f.out, f.mt, f.mt_mask, deferred, f.gapb, f.dbg | internal_dbg);
    };
    auto of_pattern = [&](auto pat) {  // (with or without special tokens in the chunk)
        if (f.ss) go(tk_k_front<decltype(pat)::value, true, MODE>);
        else go(tk_k_front<decltype(pat)::value, false, MODE>);
    };
    if (f.pat_id == TK_PAT_R50K) of_pattern(std::integral_constant<int, TK_PAT_R50K>{});
    else if (f.pat_id == TK_PAT_CL100K) of_pattern(std::integral_constant<int, TK_PAT_CL100K>{});
    else if (f.pat_id == TK_PAT_O200K) of_pattern(std::integral_constant<int, TK_PAT_O200K>{});
    else of_pattern(std::integral_constant<int, TK_PAT_GENERIC>{});  // a pattern of the family that is not one of the stock three: family and parameters are run-time values
}

// exclusive prefix sum of a uint32 array in place, total -> total_out[0]
static int scan_u32(tk_core* c, WorkSet& w, hipStream_t s, uint32_t* a, uint64_t n, uint64_t* total_out) {
    if (n <= 2 * (uint64_t)TK_SCAN_BLOCK) {  // (one workgroup walks 8 Ki values in ~7 us: cheaper than three launches of 6-8 us each; 17.5 Ki -- the tiles of 64 MiB -- took it 27 us)
        TRY(timed(c, s, "tk_k_scan_small", [&] { hipLaunchKernelGGL(tk_k_scan_small, dim3(1), dim3(TK_SCAN_THREADS), 0, s, a, n, total_out); }));
        return TK_OK;
    }
    const uint64_t nb = (n + TK_SCAN_BLOCK - 1) / TK_SCAN_BLOCK;
    TRY(ensure(w.scan_sums, (nb + 2) * 4));
    uint32_t* sums = w.scan_sums.as<uint32_t>();
    TRY(timed(c, s, "tk_k_scan_sums", [&] { hipLaunchKernelGGL(tk_k_scan_sums, dim3((uint32_t)nb), dim3(TK_SCAN_THREADS), 0, s, a, n, sums); }));
    TRY(timed(c, s, "tk_k_scan_small", [&] { hipLaunchKernelGGL(tk_k_scan_small, dim3(1), dim3(TK_SCAN_THREADS), 0, s, sums, nb, total_out); }));
    TRY(timed(c, s, "tk_k_scan_apply", [&] { hipLaunchKernelGGL(tk_k_scan_apply, dim3((uint32_t)nb), dim3(TK_SCAN_THREADS), 0, s, a, n, sums); }));
    return TK_OK;
}

// the generic pat_str engine gave up on a piece (tk_regex_split.h): which way, and where
static int rx_failure(const uint32_t* counters, uint64_t base) {
    const std::string at = std::to_string(base + (uint64_t)(~counters[TK_CNT_RXPOS]));
    if (counters[TK_CNT_ERR] & TK_RX_ERR_STACK)
        return fail(TK_VALUE_ERROR, "pat_str: a repeated group needs more backtracking state than the matcher keeps (piece at byte " + at +
                                        " of the batch); make the group possessive, e.g. (?:...)++");
    return fail(TK_VALUE_ERROR, "pat_str: backtrack limit exceeded at byte " + at +
                                    " of the batch (nested quantifiers; the reference's fancy-regex gives up after 1 000 000 backtracks as well)");
}

// The generic engine's bitmaps over a chunk of n bytes: three pairs (w.rx_spec, w.rx_gst, w.rx_lnk), in each the starts and, behind them, the
// gap chars among the starts.
struct RxPairs {
    const uint64_t nwords;  // of one bitmap, before its two words of slack
    explicit RxPairs(uint64_t n) : nwords((n + 31) / 32) {}
    uint64_t bytes() const { return 2 * (nwords + 2) * 4; }  // of one pair
    uint32_t* gap(const Buf& pair) const { return pair.as<uint32_t>() + nwords + 2; }
    static std::array<Buf*, 3> of(WorkSet& w) { return {&w.rx_spec, &w.rx_gst, &w.rx_lnk}; }
};

// The generic engine's split of a chunk (tk_regex_kernels.h): speculate, link, resolve, then brk |= the true piece starts.  The three
// pairs of bitmaps (RxPairs) are zero on entry.
static int rx_split(tk_core* c, WorkSet& w, const ChunkJob& job, hipStream_t s) {
    const uint8_t* d_text = job.ask.d_text;
    const uint64_t n = job.ask.n, nwords = (n + 31) / 32;
    uint32_t *brk = job.front.brk, *ss = job.front.ss, *si = job.front.si;
    const RxPairs rx(n);
    uint32_t* counters = w.counters.as<uint32_t>();
    const uint32_t seg_shift = n < TK_RX_SEG_SMALL_BELOW ? TK_RX_SEG_SHIFT_SMALL : TK_RX_SEG_SHIFT_LARGE;
    const uint64_t nseg = (n + (1ull << seg_shift) - 1) >> seg_shift;
    TRY(ensure(w.rx_exit, 3 * (nseg + 2) * 4));  // exit of every segment's chain; where the link met it; where the link left the segment
    uint32_t *spec = w.rx_spec.as<uint32_t>(), *gst = w.rx_gst.as<uint32_t>(), *xexit = w.rx_exit.as<uint32_t>();
    uint32_t *lnk = w.rx_lnk.as<uint32_t>(), *lmerge = xexit + nseg + 2, *lexit = xexit + 2 * (nseg + 2);
    uint32_t *spec_gap = rx.gap(w.rx_spec), *gst_gap = rx.gap(w.rx_gst), *lnk_gap = rx.gap(w.rx_lnk);
    // (the kernels' form: the pattern's DFA in LDS -- its speculative pass as one loop -- or the backtracking program; tk_regex_kernels.h)
    const uint32_t lds = c->rx_form == TK_RX_FORM_PROGRAM ? 0u : tk_rx_dfa_lds_bytes(c->rx);
    const uint32_t ahead = c->rx_form == TK_RX_FORM_PROGRAM ? TK_RX_AHEAD : TK_RX_AHEAD_DFA;
    auto by_form = [&](auto&& launch) {
        if (c->rx_form == TK_RX_FORM_DFA_FLAT) launch(std::integral_constant<int, TK_RX_FORM_DFA_FLAT>{});
        else if (c->rx_form == TK_RX_FORM_DFA) launch(std::integral_constant<int, TK_RX_FORM_DFA>{});
        else if (c->rx_form == TK_RX_FORM_DFA_FLAT_PREV) launch(std::integral_constant<int, TK_RX_FORM_DFA_FLAT_PREV>{});
        else if (c->rx_form == TK_RX_FORM_DFA_PREV) launch(std::integral_constant<int, TK_RX_FORM_DFA_PREV>{});
        else launch(std::integral_constant<int, TK_RX_FORM_PROGRAM>{});
    };
    // (the pattern's DFA without look-behind over 128-byte segments: the lanes walk codes staged in LDS -- tk_k_rx_speculate_staged; otherwise
    // the one-loop lanes over global memory)
    const bool staged = c->rx_form == TK_RX_FORM_DFA_FLAT && seg_shift == TK_RX_SEG_SHIFT_SMALL && tk_rx_staged_fits(c->rx);
    TRY(timed(c, s, "tk_k_rx_speculate", [&] {
        if (staged)
            hipLaunchKernelGGL(tk_k_rx_speculate_staged, dim3(grid_for(nseg, TK_RX_STAGE_SEGS, c->rx_grid_cap)), dim3(TK_RX_STAGE_SEGS), tk_rx_staged_lds_bytes(c->rx), s, c->rx, d_text, (uint32_t)n, brk, ss,
                               si, ahead, spec, spec_gap, xexit);
        else
            by_form([&](auto form) {
                hipLaunchKernelGGL(tk_k_rx_speculate<decltype(form)::value>, dim3(grid_for(nseg, 256, 65536)), dim3(256), lds, s, c->rx, d_text, (uint32_t)n, brk, ss, si, seg_shift,
                                   ahead, spec, spec_gap, xexit);
            });
    }));
    TRY(timed(c, s, "tk_k_rx_link", [&] {
        by_form([&](auto form) {
            hipLaunchKernelGGL(tk_k_rx_link<decltype(form)::value>, dim3(grid_for(nseg, 256, 65536)), dim3(256), lds, s, c->rx, d_text, (uint32_t)n, brk, ss, si, seg_shift,
                               ahead, spec, xexit, lnk, lnk_gap, lmerge, lexit);
        });
    }));
    const TkRxMaps maps{spec, spec_gap, xexit, lnk, lnk_gap, lmerge, lexit, seg_shift};
    TRY(timed(c, s, "tk_k_rx_resolve", [&] {  // (the wavefront form, tk_k_rx_resolve_wave: kernel times keep this name)
        by_form([&](auto form) {
            hipLaunchKernelGGL(tk_k_rx_resolve_wave<decltype(form)::value>, dim3(grid_for(job.ask.n_docs, 4, 65536)), dim3(256), lds, s, c->rx, d_text, (uint32_t)n, brk, ss, si,
                               job.ask.d_doc_off, job.ask.n_docs, job.ask.base, maps, gst, gst_gap, counters);
        });
    }));
    TRY(timed(c, s, "tk_k_rx_merge", [&] { hipLaunchKernelGGL(tk_k_rx_merge, dim3(grid_for(nwords, 256, 4096)), dim3(256), 0, s, brk, gst, nwords); }));
    return TK_OK;
}

// ------------------------------------------------------------------------------------------
// The production pipeline (kernels of tk_fused.h) on one chunk (n < 4 GiB bytes) of packed documents, everything device resident, in two
// stages so that chunks can overlap: while chunk k is merged and its tokens are placed (stage_back: latency- and memory-bound kernels,
// on their own stream), the front kernel of chunk k + 1 (bound by the vector ALU) already runs on the caller's stream.  Each chunk in
// flight has its own WorkSet.  The host never needs a chunk's token count to queue the next one: the running total stays on the device
// (c->tok_bases[k]: written by chunk k - 1's back stage as soon as it knows its token count).
//   What the caller asks for -- text, documents, where the results go, which of the entries it is -- is a ChunkAsk.
// ------------------------------------------------------------------------------------------
// The tiles the front kernel has deferred (they need the workgroup-wide scanner: long pieces, far-away piece starts; their number stays
// on the device), then the counters of both kernels -- pieces for the tree kernel, errors of the generic engine -- on their way to the host.
// A kernel of a few hundred workgroups that each take ~0.3 ms: it belongs to the back stage, beside the next chunk's front kernel.
static int stage_deferred(tk_core* c, WorkSet& w, ChunkJob& job, hipStream_t s) {
    // A stretch without certain starts ("x'llx'll...": whether 'll ends a piece depends on everything before it) makes every deferred tile
    // inside it walk from the stretch's start -- quadratic in its length, seconds for 10 MB.  A tile whose walk exceeds TKF_WALK_BUDGET
    // windows gives up instead (second list); if any did, the generic engine -- linear on exactly such text: the pieces are short, every
    // segment's guess is taken -- splits the chunk under the same pat_str, its piece starts become hard starts, and the tiles that gave up
    // run again: every piece start is certain now.  (Pieces that are already final are what they were: a hard start at the start of a
    // piece changes nothing, and the stock patterns match a piece the same way when the text ends behind it.)
    const uint64_t n = job.ask.n;
    const bool can_fall_back = c->has_rx_fb && n >= (256u << 10);
    if (n > 0 && !job.ask.single_piece()) {
        uint32_t* deferred = w.deferred.as<uint32_t>();
        // (the grid: what is resident -- or, where the host does not wait for the counters, as many workgroups as the chunks before had deferred tiles (at
        // least 64: they take their tiles from a counter).  On ordinary text no tile is deferred since round 6, and an empty grid of 768 such workgroups
        // -- 168 registers, 37 KiB of LDS, scratch -- costs 12.6 us against the 7 of 64.)
        const uint64_t defer_guess = ((job.ntiles * (uint64_t)c->defer_ppm) >> 20) * 5 / 4 + 64;
        const bool sync_now = can_fall_back && (c->defer_sync || job.ask.piece_starts());  // (the piece-offsets entry has no chunk_finish)
        job.optimistic = can_fall_back && !sync_now;
        uint64_t slow_wgs = 256u * TKF_SLOW_OCC;
        if (job.optimistic && defer_guess < slow_wgs) slow_wgs = defer_guess;
        const dim3 grid((uint32_t)(job.ntiles < slow_wgs ? job.ntiles : slow_wgs));
        // The deferred tiles in two kernels: the deferred-tile instance finds a tile's piece starts (the workgroup-wide scanner: 128 registers,
        // four workgroups per CU), the one-tile-per-workgroup instance does the rest from the starts it is given (phases E and F, at eight
        // workgroups per CU).  Its grid is the list's length where the host reads the counters (inputs of 256 KiB and more); otherwise one
        // workgroup per tile of the chunk, of which all but the list's length return at once.
        TRY(timed(c, s, "tk_k_front_slow", [&] { launch_front<TKF_MODE_STARTS>(c, job, grid, s, deferred, can_fall_back ? TK_DBG_MAY_GIVE_UP : 0); }));
        uint64_t n_given = job.ntiles;
        // (round 6) The host does not wait for the counters here any more: the wait cost every chunk ~25 us of an idle device between the two kernels
        // (3 % of a 64 MiB batch) and kept the host from queueing the next chunk -- for a decision that ordinary text never needs.  The kernel that
        // finishes the deferred tiles walks the list with a grid sized from the chunk before (the same kind of text: a quarter more than it needed),
        // and chunk_finish looks at the counter of tiles that gave up: if there is one the batch is repeated (encode_device_locked) and the core waits
        // here from then on (c->defer_sync), as it did up to round 5.  Small inputs, a pat_str without that way out: one workgroup per tile.
        if (job.optimistic) n_given = defer_guess < job.ntiles ? defer_guess : job.ntiles;
        if (sync_now) {
            HIPCHK(hipMemcpyAsync(w.h_counters, w.counters.p, TK_CNT_N * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(hipEventRecord(w.ev_cnt, s));
            HIPCHK(hipEventSynchronize(w.ev_cnt));
            if (can_fall_back && w.h_counters[TK_CNT_DEFER2]) {
                const RxPairs rx(n);
                for (Buf* b : rx.of(w)) {
                    TRY(ensure(*b, rx.bytes()));
                    HIPCHK(hipMemsetAsync(b->p, 0, rx.bytes(), s));
                }
                TRY(rx_split(c, w, job, s));
                TRY(timed(c, s, "tk_k_front_slow", [&] { launch_front<TKF_MODE_STARTS>(c, job, grid, s, deferred + job.ntiles + 2, TK_DBG_SECOND); }));
                c->st_fallbacks += 1;
            }
            n_given = w.h_counters[TK_CNT_DEFER];
        }
        if (n_given && TKF_STOP_AFTER == 0)  // (TKF_STOP_AFTER: the kernels stop after a phase, there are no starts to go on from)
            TRY(timed(c, s, "tk_k_front_given", [&] { launch_front<TKF_MODE_GIVEN>(c, job, dim3((uint32_t)n_given), s, deferred, 0); }));
    }
    HIPCHK(hipMemcpyAsync(w.h_counters, w.counters.p, TK_CNT_N * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipEventRecord(w.ev_cnt, s));
    return TK_OK;
}

static int stage_front(tk_core* c, WorkSet& w, ChunkJob& job, hipStream_t s, const ChunkAsk& ask) {
    const TkTables& T = c->D;
    const uint8_t* d_text = ask.d_text;
    const uint64_t n = ask.n, n_docs = ask.n_docs, base = ask.base;
    const bool single_piece = ask.single_piece(), pretok_only = ask.piece_starts();
    const uint64_t nwords = (n + 31) / 32;
    const uint64_t nblk = (nwords + 255) / 256;
    const uint64_t ntiles = (n && !single_piece) ? (n + TK_TILE - 1) / TK_TILE : 1;  // (single piece: one run of one piece)
    if (single_piece && ask.d_tok_off) return fail(TK_RUNTIME_ERROR, "internal error: token offsets asked of a single piece");
    job = ChunkJob();
    job.ask = ask;
    job.ntiles = ntiles;
    job.docs_in_place = n > 0 && !single_piece && ask.d_tok_off != nullptr;
    TRY(ensure(w.blockcnt, (nblk + 2) * 4));
    TRY(ensure(w.tile_np, (ntiles + 2) * 4));
    TRY(ensure(w.tile_nt, (ntiles + 2) * 4));
    TRY(ensure(w.wbin, (TK_NBIN * TKD_WAVES + 2) * 4));
    const uint64_t pid_cap = tk_pid_cap(n);
    TRY(ensure(w.res, pid_cap * 4));
    TRY(ensure(w.staging, (n + 64) * 4));
    // The entries of the distinct missed pieces (tk_fused.h, TkMiss): one per slot of the in-call de-duplication table -- which pays for
    // its reset (of the 16-byte keys: the 64-byte entries are written by whoever claims a slot, never cleared) only on real batches -- and
    // the overflow entries behind them.  The table takes what repeats; the overflow entries are sized for a sixteenth of the worst case
    // (every piece a distinct two-byte piece that is not a token) unless the chunk is small or a batch has already asked for more
    // (c->ovf_full: encode_device_locked repeats such a batch once, with room for the worst case).
    // (small chunks too: without the table every missed piece has an overflow entry, whose tokens tk_k_place copies from the staging area two
    // pieces at a time -- 92 us for a 4 KiB call, against 4 us for clearing 16 Ki keys)
    if (n >= 512 && !single_piece && !pretok_only) {
        while (job.mt_bits < TK_MT_BITS && (1ull << job.mt_bits) < n / TK_MT_DIV) ++job.mt_bits;  // 4 Mi slots from 512 MiB up
        job.ovf_base = 1u << job.mt_bits;
    }
    {
        const uint64_t worst = n / 2 + 64;
        job.ovf_cap = (uint32_t)((n <= (1u << 20) || c->ovf_full) ? worst : std::min<uint64_t>(worst, std::max<uint64_t>(n >> 4, 1u << 16)));
        if (pretok_only) job.ovf_cap = 64;
    }
    const uint64_t n_entries = (uint64_t)job.ovf_base + job.ovf_cap;
    TRY(ensure(w.mtab, (uint64_t)job.ovf_base * sizeof(TkMissTab)));
    TRY(ensure(w.mcnt, (uint64_t)job.ovf_base + 16));
    TRY(ensure(w.movf, ((uint64_t)job.ovf_cap + 1) * sizeof(TkMissOvf)));
    TRY(ensure(w.listB, (n_entries + 64) * 4));
    TRY(ensure(w.listC, (n / 1025 + 64) * 20));
    TRY(ensure(w.big, (1 + 3 * TK_BIGCOPY_CAP) * 4));
    TkClearArgs clr;
    clr.n = 0;
    // room for `bytes` (nothing to do where more was asked for above), those from `from` on filled -- from the 16-byte unit that holds
    // `from`: up to three words before it are filled too, so whoever writes those must run behind tk_k_chunk_clear on this stream
    auto clear = [&](Buf& b, uint64_t bytes, uint32_t v, uint64_t from = 0) -> int {
        if (clr.n >= TK_CLEAR_MAX) return fail(TK_RUNTIME_ERROR, "internal error: more buffers to clear than tk_k_chunk_clear takes");
        TRY(ensure(b, bytes));
        clr.p[clr.n] = b.as<uint4>() + from / 16;
        clr.n16[clr.n] = (bytes + 15) / 16 - from / 16;  // (every Buf has at least 256 bytes of slack behind what was asked for)
        clr.v[clr.n] = v;
        ++clr.n;
        return TK_OK;
    };
    TRY(clear(w.brk, (nwords + 2) * 4, 0u));
    TRY(clear(w.counters, TK_CNT_N * 4, 0u));
    TRY(clear(w.big, 4, 0u));
    TRY(clear(w.merge_work, 16 * TKM_WORK_STRIDE * 4, 0u));
    TRY(clear(w.total, 32, 0u));
    // (tk_k_place reads all 120 words of the last tile's piece starts; the front kernel, launched below behind the clears, writes those
    // below nwords, the others stay zero)
    TRY(clear(w.starts, tk_starts_words(nwords, ntiles) * 4, 0u, nwords * 4));
    uint32_t* find_docb = nullptr;  // the document starts for the disallowed scan: `docb`, or the same bitmap made for the scan alone
    // the first document that starts in every tile (tk_k_mark_docs), for tk_k_place, which writes the documents' token offsets as it passes
    // their pieces (an empty chunk has no pieces: tk_k_docoff)
    if (job.docs_in_place) TRY(clear(w.doc_first, (ntiles + 2) * 4, 0xFFFFFFFFu));
    TRY(clear(w.tile_sum, ntiles + 16, 0xFFFFFFFFu));
    FrontArgs& f = job.front;
    if (job.ovf_base) {
        TRY(clear(w.mt_keys, sizeof(TkMissKey) * job.ovf_base, 0xFFFFFFFFu));
        job.mt = w.mt_keys.as<TkMissKey>();
    }
    f.pat_id = T.pat.generic() ? TK_PAT_GENERIC : T.pattern;
    f.brk = w.brk.as<uint32_t>();
    f.out = TkFrontOut{w.starts.as<uint32_t>(), w.tile_np.as<uint32_t>(), w.res.as<uint32_t>(), w.tile_sum.as<uint8_t>(), miss_of(w, job), job.ovf_cap, w.listC.as<uint32_t>(), w.counters.as<uint32_t>()};
    f.mt = (c->dbg & TK_DBG_NO_MT) ? (TkMissKey*)nullptr : job.mt;
    f.mt_mask = (1u << job.mt_bits) - 1u;
    f.dbg = (c->dbg & ~TK_DBG_INTERNAL) | (pretok_only ? TK_DBG_STARTS_ONLY : 0);
    if (n > 0 && !single_piece) {
        if (ask.use_special) {
            for (Buf* b : {&w.docb, &w.cand}) TRY(clear(*b, (nwords + 4) * 4, 0u));  // (tk_bits64 reads two words past the one a position lies in)
            for (Buf* b : {&w.ss, &w.si}) TRY(clear(*b, (nwords + 2) * 4, 0u));
            f.docb = w.docb.as<uint32_t>();
            f.ss = w.ss.as<uint32_t>();
            f.si = w.si.as<uint32_t>();
        }
        if (c->find_on && !pretok_only) {
            job.find = true;
            TRY(clear(w.find, 16, 0xFFFFFFFFu));
            if (!f.docb) TRY(clear(w.docb, (nwords + 4) * 4, 0u));
            find_docb = w.docb.as<uint32_t>();
        }
        if (c->has_rx) {
            const RxPairs rx(n);
            for (Buf* b : rx.of(w)) TRY(clear(*b, rx.bytes(), 0u));
            f.gapb = rx.gap(w.rx_gst);
        }
        hipLaunchKernelGGL(tk_k_chunk_clear, dim3(grid_for(n / 64 + 1, 256, 2048)), dim3(256), 0, s, clr);
        clr.n = 0;
        TRY(timed(c, s, "tk_k_mark_docs", [&] {
            hipLaunchKernelGGL(tk_k_mark_docs, dim3(grid_for(n_docs, 256, 4096)), dim3(256), 0, s, ask.d_doc_off, n_docs, base, n, f.brk, f.docb ? f.docb : find_docb,
                               job.docs_in_place ? w.doc_first.as<uint32_t>() : (uint32_t*)nullptr, ntiles);
        }));
        if (ask.use_special) {
            const uint8_t* allowed = c->allowed.as<uint8_t>();
            uint32_t* cand = w.cand.as<uint32_t>();
            TRY(timed(c, s, "tk_k_spec_cand", [&] {
                hipLaunchKernelGGL(tk_k_spec_cand, dim3(grid_for(n / 16 + 1, 256, 65536)), dim3(256), 0, s, T, d_text, n, allowed, f.docb, cand);
            }));
            TRY(timed(c, s, "tk_k_spec_resolve", [&] {
                hipLaunchKernelGGL(tk_k_spec_resolve, dim3(grid_for(nwords, 256, 65536)), dim3(256), 0, s, T, d_text, n, allowed, f.docb, cand,
                                   c->spec_max_len, f.ss, f.si, f.brk);
            }));
            c->st_mark_launches += 1;
        }
        if (job.find) {
            // (a match ends inside the chunk -- tk_special_at asks for pos + len <= n -- and inside its document: the text behind the chunk, the
            // next document or the zeroed slack, is never part of one)
            TRY(timed(c, s, "tk_k_spec_find", [&] {
                hipLaunchKernelGGL(tk_k_spec_find, dim3(grid_for(n / 16 + 1, 256, 65536)), dim3(256), 0, s, T, d_text, n, c->disallowed.as<uint8_t>(), find_docb, base,
                                   w.find.as<unsigned long long>());
            }));
            c->st_find_launches += 1;
        }
        if (c->has_rx) TRY(rx_split(c, w, job, s));  // the generic engine finds the piece starts; they join the hard starts in `brk`
        TRY(ensure(w.deferred, 2 * (ntiles + 2) * 4));  // (behind the list of deferred tiles: those that gave up their walk, stage_deferred)
        TRY(timed(c, s, "tk_k_front", [&] {
            launch_front<TKF_MODE_TILE>(c, job, dim3((uint32_t)ntiles), s, w.deferred.as<uint32_t>(), (c->has_rx && !(c->dbg & TK_DBG_SCANNERS)) ? TK_DBG_HARD_ONLY : 0);
        }));
    } else if (n > 0) {
        hipLaunchKernelGGL(tk_k_chunk_clear, dim3(1), dim3(256), 0, s, clr);
        clr.n = 0;
        TRY(timed(c, s, "tk_k_single_front", [&] { hipLaunchKernelGGL(tk_k_single_front, dim3(1), dim3(64), 0, s, T, d_text, (uint32_t)n, f.out, ask.kind == ChunkKind::SinglePieceNoLookup ? 1 : 0); }));
    }
    if (clr.n) hipLaunchKernelGGL(tk_k_chunk_clear, dim3(1), dim3(256), 0, s, clr);  // (an empty chunk)
    HIPCHK(hipEventRecord(w.ev_front, s));
    return TK_OK;
}

// The piece-starts entry (debugging / test entry, training), behind the front stage and the deferred tiles of its chunk: the piece starts are
// counted and written to w.pstart (ascending, then the total byte count; bit 31 marks a gap char).  Waits: *count_out pieces.
static int piece_starts(tk_core* c, WorkSet& w, const ChunkJob& job, hipStream_t s, uint64_t* count_out) {
    const uint64_t n = job.ask.n, nwords = (n + 31) / 32, nblk = (nwords + 255) / 256;
    uint32_t *starts = w.starts.as<uint32_t>(), *blockcnt = w.blockcnt.as<uint32_t>();
    uint64_t P = 0;
    TRY(ensure(w.pstart, 16));
    if (n > 0) {
        TRY(timed(c, s, "tk_k_count", [&] { hipLaunchKernelGGL(tk_k_count, dim3((uint32_t)nblk), dim3(256), 0, s, starts, nwords, blockcnt); }));
        TRY(timed(c, s, "tk_k_scan_small", [&] { hipLaunchKernelGGL(tk_k_scan_small, dim3(1), dim3(TK_SCAN_THREADS), 0, s, blockcnt, nblk, w.total.as<uint64_t>()); }));
        HIPCHK(hipMemcpyAsync(&P, w.total.p, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (w.h_counters[TK_CNT_ERR] & (TK_RX_ERR_GAP | TK_RX_ERR_STACK | TK_RX_ERR_LIMIT)) return rx_failure(w.h_counters, job.ask.base);
        TRY(ensure(w.pstart, (P + 2) * 4));
        TRY(timed(c, s, "tk_k_emit", [&] {
            hipLaunchKernelGGL(tk_k_emit, dim3((uint32_t)nblk), dim3(256), 0, s, starts, nwords, blockcnt, w.pstart.as<uint32_t>(), P, n, job.front.gapb);
        }));
    } else {
        HIPCHK(hipMemsetAsync(w.pstart.p, 0, 4, s));
    }
    *count_out = P;
    return TK_OK;
}

// Second stage of a chunk, on stream s (the front stage's stream for a single chunk, the set's own otherwise; the caller has made it wait
// for w.ev_front).  The chunk's tokens go into the batch's token buffer (ask.d_out) behind tok_bases[job.index] of them, which the previous
// chunk's back stage writes (prev_tot: the event to wait for; none for the first chunk or on a single stream).
static int stage_back(tk_core* c, WorkSet& w, ChunkJob& job, hipStream_t s, hipEvent_t prev_tot = nullptr) {
    const TkTables& T = c->D;
    const ChunkAsk& ask = job.ask;
    const uint64_t n = ask.n, ntiles = job.ntiles;
    const uint8_t* d_text = ask.d_text;
    uint32_t *d_out = ask.d_out, *counters = w.counters.as<uint32_t>();
    uint32_t *res = w.res.as<uint32_t>(), *stg = w.staging.as<uint32_t>();
    const TkMiss data = miss_of(w, job);
    uint32_t *tile_np = w.tile_np.as<uint32_t>(), *tile_nt = w.tile_nt.as<uint32_t>();
    const unsigned long long* tok_base = c->tok_bases.as<unsigned long long>() + job.index;
    uint64_t nC = 0;
    TRY(stage_deferred(c, w, job, s));
    // (perf experiments, tools/gpu_phases.sh: a build with TKF_STOP_AFTER -- the front kernel stops after one of its phases -- its outputs
    // are incomplete, so nothing behind it runs but the chunk's end, as for an empty chunk: the call returns zero tokens and offsets that mean nothing)
    constexpr bool front_only = TKF_STOP_AFTER != 0;
    const bool encode = n > 0 && !front_only;
    if (encode) {
        uint32_t* wbin = w.wbin.as<uint32_t>();
        uint32_t* listB = w.listB.as<uint32_t>();
        // the two list passes walk the miss data (table slots + overflow entries): as many wavefronts as it has rows of 64 entries for
        // (small calls are latency-bound: a workgroup or two)
        const uint64_t n_entries = (uint64_t)job.ovf_base + job.ovf_cap;
        const uint32_t dd_blocks = grid_for(n_entries, 4 * 256, TKD_WAVES / 4);
        TRY(timed(c, s, "tk_k_bincount", [&] {
            hipLaunchKernelGGL(tk_k_bincount, dim3(dd_blocks), dim3(256), 0, s, T, d_text, data, job.mt, job.ovf_cap, counters, wbin, (c->dbg & TK_DBG_COLLIDE) ? 0 : 1);
        }));
        TRY(scan_u32(c, w, s, wbin, (uint64_t)TK_NBIN * dd_blocks * 4 + 1, w.total.as<uint64_t>()));
        TRY(timed(c, s, "tk_k_binfill", [&] {
            hipLaunchKernelGGL(tk_k_binfill, dim3(dd_blocks), dim3(256), 0, s, T, d_text, data, job.mt, job.ovf_cap, wbin, listB, counters);
        }));
        if (T.pair8 && !(c->dbg & TK_DBG_MERGE_PER_BIN)) {
            // every bin in one launch (tk_k_merge_all); TK_DBG_MERGE_PER_BIN: the kernel-per-bin form below
            uint64_t most_units = 0;
            for (int b = 0; b < TK_NBIN; ++b)
                if (n >= tk_bin_lo(b)) most_units += std::min<uint64_t>(n / tk_bin_lo(b), n_entries) / (64u >> tkm_lg_of_bin(b)) + 1;
            uint32_t wgs = (uint32_t)std::min<uint64_t>((most_units + TKM_WAVES - 1) / TKM_WAVES, (uint64_t)c->n_cu * TKM_WGS_PER_CU);
            wgs = std::max(16u / TKM_WAVES, (wgs + 16u / TKM_WAVES - 1u) / (16u / TKM_WAVES) * (16u / TKM_WAVES));  // (wavefronts: a multiple of 16, tk_k_merge_all's work counters rely on it)
            TRY(timed(c, s, "tk_k_merge_all", [&] {
                hipLaunchKernelGGL(tk_k_merge_all, dim3(wgs), dim3(64 * TKM_WAVES), TKM_LDS_BYTES, s, T, d_text, listB, counters, data, stg, w.merge_work.as<uint32_t>());
            }));
        } else
        {
            // The bins are independent: spread them over the side streams, longest-tailed kernels first.  List starts and lengths are
            // read on the device, so nothing waits for the host here; grids are sized by the most a bin can hold.
            static const char* const names[TK_NBIN] = {"tk_k_merge_llane_16", "tk_k_merge_llane_24", "tk_k_merge_llane_32", "tk_k_merge_llane_48", "tk_k_merge_llane_64",
                                                       "tk_k_merge_group_8", "tk_k_merge_group_16", "tk_k_merge_group_32", "tk_k_merge_group_64"};
            uint32_t small_counts[TK_CNT_N];
            const bool small = n <= (4u << 20);  // small calls: a round trip is cheaper than launching kernels over empty lists
            if (small) {
                HIPCHK(hipMemcpyAsync(small_counts, counters, sizeof small_counts, hipMemcpyDeviceToHost, s));
                HIPCHK(hipStreamSynchronize(s));
            }
            HIPCHK(hipEventRecord(w.ev_fork, s));
            for (int i = 0; i < TK_NAUX; ++i) HIPCHK(hipStreamWaitEvent(c->aux[i], w.ev_fork, 0));
            // (longest first; the four lane-group kernels have a stream each -- their run time is the longest piece's chain of
            // merges --, the five lane-per-piece kernels share two)
            static const int order[TK_NBIN] = {6, 8, 7, 5, 2, 4, 1, 3, 0};
            static const int stream_of[TK_NBIN] = {5, 5, 4, 4, 5, 3, 0, 2, 1};
            for (int oi = 0; oi < TK_NBIN; ++oi) {
                const int b = order[oi];
                if (n < tk_bin_lo(b) || (small && !small_counts[TK_CNT_BIN0 + b])) continue;
                const uint64_t most = std::min<uint64_t>(n / tk_bin_lo(b), n_entries);
                hipStream_t sa = c->aux[stream_of[b]];
                TRY(timed(c, sa, names[b], [&] {
                    switch (b) {
                        case 0: hipLaunchKernelGGL((tk_k_merge_llane<16, 256>), dim3(grid_for(most, 256, 8192)), dim3(256), 0, sa, T, d_text, listB, counters, b, data, stg); break;
                        case 1: hipLaunchKernelGGL((tk_k_merge_llane<24, 256>), dim3(grid_for(most, 256, 8192)), dim3(256), 0, sa, T, d_text, listB, counters, b, data, stg); break;
                        case 2: hipLaunchKernelGGL((tk_k_merge_llane<32, 256>), dim3(grid_for(most, 256, 8192)), dim3(256), 0, sa, T, d_text, listB, counters, b, data, stg); break;
                        case 3: hipLaunchKernelGGL((tk_k_merge_llane<48, 128>), dim3(grid_for(most, 128, 8192)), dim3(128), 0, sa, T, d_text, listB, counters, b, data, stg); break;
                        case 4: hipLaunchKernelGGL((tk_k_merge_llane<64, 128>), dim3(grid_for(most, 128, 8192)), dim3(128), 0, sa, T, d_text, listB, counters, b, data, stg); break;
                        case 5: hipLaunchKernelGGL((tk_k_merge_group<8>), dim3(grid_for(most, 32, 8192)), dim3(256), 0, sa, T, d_text, listB, counters, b, data, stg); break;
                        case 6: hipLaunchKernelGGL((tk_k_merge_group<16>), dim3(grid_for(most, 16, 8192)), dim3(256), 0, sa, T, d_text, listB, counters, b, data, stg); break;
                        case 7: hipLaunchKernelGGL((tk_k_merge_group<32>), dim3(grid_for(most, 8, 8192)), dim3(256), 0, sa, T, d_text, listB, counters, b, data, stg); break;
                        default: hipLaunchKernelGGL((tk_k_merge_group<64>), dim3(grid_for(most, 4, 8192)), dim3(256), 0, sa, T, d_text, listB, counters, b, data, stg); break;
                    }
                }));
            }
            for (int i = 0; i < TK_NAUX; ++i) {
                HIPCHK(hipEventRecord(w.ev_join[i], c->aux[i]));
                HIPCHK(hipStreamWaitEvent(s, w.ev_join[i], 0));
            }
        }
        // pieces longer than TK_GLANE_MAX were listed by the front kernel: their scratch is sized from its counters,
        // which were copied back while the kernels above were being queued
        {
            const double t0 = now_us();
            HIPCHK(hipEventSynchronize(w.ev_cnt));
            c->host_us[2] += now_us() - t0;
        }
        const uint32_t* hc = w.h_counters;
        nC = hc[TK_CNT_C];
        if (nC) {
            const uint64_t lb = (uint64_t)hc[TK_CNT_CBYTES] + 4 * nC, lvls = hc[TK_CNT_CLEVELS];
            TRY(ensure(w.g_id, (lb + 64) * 4));
            TRY(ensure(w.g_rk, (lb + 64) * 4));
            TRY(ensure(w.g_nx, (lb + 64) * 4));
            TRY(ensure(w.g_pv, (lb + 64) * 4));
            TRY(ensure(w.g_lv, (lvls + 64) * 8));
            const bool rounds = !(c->dbg & TK_DBG_ONE_MERGE);
            if (rounds) {
                TRY(timed(c, s, "tk_k_merge_rounds", [&] {
                    hipLaunchKernelGGL(tk_k_merge_rounds, dim3(grid_for(nC, 1, 1024)), dim3(TKB_THREADS), 0, s, T, d_text, w.listC.as<uint32_t>(),
                                       (uint32_t)nC, w.g_id.as<uint32_t>(), w.g_rk.as<uint32_t>(), w.g_nx.as<uint32_t>(), w.g_pv.as<uint32_t>(),
                                       data, stg);
                }));
            }
            if (rounds && n >= TK_WIDE_MIN) {  // (pieces of TK_WIDE_MIN bytes and more, if there are any: the whole grid on each)
                TRY(ensure(w.wide_ws, sizeof(TkWideWs)));
                HIPCHK(hipMemsetAsync(w.wide_ws.p, 0, sizeof(TkWideWs), s));
                TRY(timed(c, s, "tk_k_merge_rounds_wide", [&] {
                    hipLaunchKernelGGL(tk_k_merge_rounds_wide, dim3(TK_WIDE_BLOCKS), dim3(TKB_THREADS), 0, s, T, d_text, w.listC.as<uint32_t>(),
                                       (uint32_t)nC, w.g_id.as<uint32_t>(), w.g_rk.as<uint32_t>(), w.g_nx.as<uint32_t>(), w.g_pv.as<uint32_t>(),
                                       data, stg, w.wide_ws.as<TkWideWs>());
                }));
            }
            TRY(timed(c, s, "tk_k_merge_long", [&] {
                hipLaunchKernelGGL(tk_k_merge_long, dim3(grid_for(nC, 4, 8192)), dim3(256), 0, s, T, d_text, w.listC.as<uint32_t>(), (uint32_t)nC,
                                   w.g_id.as<uint32_t>(), w.g_rk.as<uint32_t>(), w.g_nx.as<uint32_t>(), w.g_pv.as<uint32_t>(),
                                   w.g_lv.as<uint64_t>(), data, stg, rounds ? 1 : 0);
            }));
        }
    }
    const bool small_rows = n < (8u << 20);  // (the one-row instances: a third of the code to fetch for a kernel that runs over a few tiles)
    if (encode) {
        // token count per tile (a missed piece's count from its entry), then the tiles' places (tk_fused.h: back end)
        TRY(timed(c, s, "tk_k_count_tiles", [&] {
            if (small_rows) hipLaunchKernelGGL(tk_k_count_tiles<1>, dim3(grid_for(ntiles, 4, 2048)), dim3(256), 0, s, ntiles, tile_np, res, data, tile_nt,
                               w.total.as<unsigned long long>());
            else hipLaunchKernelGGL(tk_k_count_tiles<TKP_ROWS_COUNT>, dim3(grid_for(ntiles, 4, 2048)), dim3(256), 0, s, ntiles, tile_np, res, data, tile_nt,
                               w.total.as<unsigned long long>());
        }));
        TRY(scan_u32(c, w, s, tile_nt, ntiles, w.total.as<uint64_t>()));
    } else {
        HIPCHK(hipMemsetAsync(w.total.p, 0, 32, s));  // (the scan of the bin counts is not run for an empty chunk; be explicit)
    }
    // the chunk's token count is known: the next chunk's base.  Its tokens go behind those of the chunk before it (whose back stage may be
    // running beside this one).
    if (prev_tot) HIPCHK(hipStreamWaitEvent(s, prev_tot, 0));
    hipLaunchKernelGGL(tk_k_advance, dim3(1), dim3(64), 0, s, c->tok_bases.as<unsigned long long>(), job.index, w.total.as<uint64_t>());
    HIPCHK(hipEventRecord(w.ev_tot, s));
    if (encode) {
        TRY(timed(c, s, "tk_k_place", [&] {
            // (one instance for every size: three rows per step for inputs of a few tiles measured slower -- C1 0.082 ms against 0.060 --, profiles/r05_place_experiments.txt)
            const TkPlaceDocs docs{ask.d_doc_off, ask.base, n, ask.n_docs, w.doc_first.as<uint32_t>(), w.starts.as<uint32_t>(), w.total.as<uint64_t>(), job.docs_in_place ? ask.d_tok_off : (uint64_t*)nullptr};
            // (six workgroups per CU: 80 registers, 26 688 B of LDS; a grid of four times what is resident -- 0.84 ms with 4096 workgroups, 0.81 with 1536 or 3072,
            // 0.80 with 6144 or 12 288, round 6)
            hipLaunchKernelGGL(tk_k_place<TKP_ROWS_PLACE>, dim3(grid_for(ntiles, 4, 6144)), dim3(256), 0, s, ntiles, tile_np, tile_nt, res, data, stg, d_out, tok_base, w.big.as<uint32_t>(), docs);
        }));
    }
    if (encode && n > TK_BIGCOPY)  // (a token run of TK_BIGCOPY tokens needs at least as many bytes)
        hipLaunchKernelGGL(tk_k_bigcopy, dim3(1024), dim3(256), 0, s, w.big.as<uint32_t>(), stg, d_out, tok_base);
    if (!front_only && n == 0 && ask.d_tok_off) {  // (else tk_k_place has written them)
        TRY(timed(c, s, "tk_k_docoff", [&] {
            hipLaunchKernelGGL(tk_k_docoff, dim3(grid_for(ask.n_docs + 1, 256, 4096)), dim3(256), 0, s, ask.n_docs, w.total.as<uint64_t>(), tok_base, ask.d_tok_off);
        }));
    }
    HIPCHK(hipMemcpyAsync(w.h_total, w.total.p, 16, hipMemcpyDeviceToHost, s));
    if (job.find) HIPCHK(hipMemcpyAsync(w.h_total + 2, w.find.p, 8, hipMemcpyDeviceToHost, s));  // (read where the host waits for the totals anyway: chunk_finish)
    HIPCHK(hipMemcpyAsync(w.h_counters + TK_CNT_N, counters, TK_CNT_N * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipEventRecord(w.ev_done, s));
    c->st_long += nC;
    return TK_OK;
}

// the chunk of `w` is complete: its totals, statistics and error flags (waits for its back stage)
static int chunk_finish(tk_core* c, WorkSet& w, const ChunkJob& job, uint64_t* n_tokens_out) {
    HIPCHK(hipEventSynchronize(w.ev_done));
    if (job.find && w.h_total[2] != ~0ull) {  // (before anything else: the reference refuses such text before it encodes any of it)
        c->find_hit = w.h_total[2];
        return TK_SPEC_HIT;
    }
    const uint32_t* hb = w.h_counters + TK_CNT_N;
    uint64_t nB = 0;
    for (int b = 0; b < TK_NBIN; ++b) {
        nB += hb[TK_CNT_BIN0 + b];
        if ((c->dbg & TK_DBG_VERBOSE) && hb[TK_CNT_BIN0 + b]) fprintf(stderr, "bin %d (%u..%u bytes): %u pieces\n", b, tk_bin_lo(b), tk_bin_hi(b), hb[TK_CNT_BIN0 + b]);
    }
    if (hb[TK_CNT_ERR] & (TK_RX_ERR_GAP | TK_RX_ERR_STACK | TK_RX_ERR_LIMIT)) return rx_failure(hb, job.ask.base);
    if (hb[TK_CNT_ERR]) return fail(TK_RUNTIME_ERROR, "internal error in the front kernel (scanner list overflow, code " + std::to_string(hb[TK_CNT_ERR]) + ")");
    if (job.optimistic) {  // (stage_deferred did not wait for these)
        if (hb[TK_CNT_DEFER2]) {
            c->defer_sync = true;
            return TK_RESYNC;
        }
        // (at once upwards, to a quarter per chunk downwards: chunks of two kinds of text in turn keep the larger grid)
        const uint32_t ppm = (uint32_t)std::min<uint64_t>(((uint64_t)hb[TK_CNT_DEFER] << 20) / (job.ntiles ? job.ntiles : 1), 1u << 20);
        c->defer_ppm = std::max(ppm, c->defer_ppm / 4);
    }
    if (hb[TK_CNT_OVF] > job.ovf_cap && !job.ask.piece_starts()) {  // more distinct missed pieces than the miss data has room for: the batch is repeated with room for the worst case
        c->ovf_full = true;
        return TK_GROW;
    }
    c->st_bytes += job.ask.n;
    c->st_pieces += w.h_total[1];
    c->st_tokens += w.h_total[0];
    c->st_medium += nB;
    c->st_chunks += 1;
    *n_tokens_out = w.h_total[0];
    return TK_OK;
}

// one chunk, both stages on one stream, waited for: the single-chunk entries (piece starts only, single piece).  *n_out: its tokens, or its pieces
static int run_chunk(tk_core* c, hipStream_t s, const ChunkAsk& ask, uint64_t* n_out) {
    WorkSet& w = c->ws[0];
    ChunkJob job;
    TRY(ensure(c->tok_bases, 64));
    HIPCHK(hipMemsetAsync(c->tok_bases.p, 0, 16, s));
    TRY(stage_front(c, w, job, s, ask));
    if (ask.piece_starts()) {
        TRY(stage_deferred(c, w, job, s));
        return piece_starts(c, w, job, s, n_out);
    }
    TRY(stage_back(c, w, job, s));
    return chunk_finish(c, w, job, n_out);
}

// a byte per special token on the device: 1 for those whose id is among ids[0..n)
static int prepare_mask(tk_core* c, hipStream_t s, Buf& mask, const uint32_t* ids, uint64_t n, bool* any) {
    const TkHostTables& H = c->H;
    std::vector<uint8_t> a(H.spec_id.size() + 16, 0);
    *any = false;
    for (size_t k = 0; k < H.spec_id.size(); ++k)
        for (uint64_t j = 0; j < n; ++j)
            if (H.spec_id[k] == ids[j]) {
                a[k] = 1;
                *any = true;
            }
    TRY(ensure(mask, a.size()));
    HIPCHK(hipMemcpyAsync(mask.p, a.data(), a.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));  // `a` goes out of scope
    return TK_OK;
}
static int prepare_allowed(tk_core* c, hipStream_t s, const uint32_t* allowed_ids, uint64_t n_allowed, bool* any) {
    return prepare_mask(c, s, c->allowed, allowed_ids, n_allowed, any);
}

// ---- checked calls: the disallowed special tokens of Encoding.encode / encode_batch (tiktoken/core.py:116-124) ----
struct CheckArgs {
    const uint32_t* ids;  // the disallowed special tokens
    uint64_t n;
    tk_special_hit* hit;
};
// every id names a special token of the core (host only: before anything is locked or sent)
static int check_disallowed_ids(tk_core* c, const CheckArgs* chk) {
    if (!chk || !chk->n) return TK_OK;
    if (!chk->ids || !chk->hit) return fail(TK_VALUE_ERROR, "null argument");
    for (uint64_t j = 0; j < chk->n; ++j)
        if (std::find(c->H.spec_id.begin(), c->H.spec_id.end(), chk->ids[j]) == c->H.spec_id.end())
            return fail(TK_VALUE_ERROR, "disallowed id " + std::to_string(chk->ids[j]) + " is not a special token of this encoding");
    return TK_OK;
}
// The scan is on for the calls of this scope (the core's mutex is held).
struct FindScope {
    tk_core* c;
    explicit FindScope(tk_core* core) : c(core) {}
    int begin(hipStream_t s, const CheckArgs* chk) {
        if (!chk || !chk->n) return TK_OK;
        bool any = false;
        TRY(prepare_mask(c, s, c->disallowed, chk->ids, chk->n, &any));
        c->find_on = any;
        c->find_hit = ~0ull;
        return TK_OK;
    }
    ~FindScope() { c->find_on = false; }
};
// A pass has ended with TK_SPEC_HIT: which document c->find_hit lies in and which token it is -- the longest disallowed one that matches
// there inside the document -- from the few bytes at the hit (`at`: the batch's text from the hit on, at least min(spec_max_len,
// bytes left in the batch) of it, on the host).  Returns TK_DISALLOWED_SPECIAL.
static int report_hit(tk_core* c, const uint8_t* at, const uint64_t* doc_off, uint64_t n_docs, const CheckArgs* chk) {
    const TkHostTables& H = c->H;
    const uint64_t pos = c->find_hit;
    const uint64_t doc = (uint64_t)(std::upper_bound(doc_off, doc_off + n_docs + 1, pos) - doc_off) - 1;  // (the last document that starts at or before pos: not an empty one)
    if (doc >= n_docs) return fail(TK_RUNTIME_ERROR, "internal error: a special token was found outside every document");
    const uint64_t room = doc_off[doc + 1] - pos;
    uint32_t best = 0, id = 0;
    for (size_t k = 0; k < H.spec_id.size(); ++k) {
        const uint32_t o = H.spec_off[k], len = H.spec_off[k + 1] - o;
        if (len <= best || len > room || memcmp(at, H.spec_bytes.data() + o, len) != 0) continue;
        if (std::find(chk->ids, chk->ids + chk->n, H.spec_id[k]) == chk->ids + chk->n) continue;
        best = len;
        id = H.spec_id[k];
    }
    if (!best) return fail(TK_RUNTIME_ERROR, "internal error: no disallowed special token at the position the device reported");
    *chk->hit = tk_special_hit{doc, pos - doc_off[doc], id, best};
    return fail(TK_DISALLOWED_SPECIAL, "disallowed special token " + std::to_string(id) + " (" + std::string((const char*)at, best) + ") in document " + std::to_string(doc) +
                                           " at byte " + std::to_string(pos - doc_off[doc]));
}

// ---- which of the library's streams run BESIDE a given stream (see tk_core::back_s) ----
// A gate kernel spins on `on` until the host opens the gate (or 4 ms have passed: 100 MHz counter); a one-thread kernel on every
// candidate stream sets a word of its own.  Candidates whose word arrives while the gate is closed do not share `on`'s hardware queue.
// (the probe's words live in mapped host memory: system-scope atomics, so that neither side looks at a cached copy)
__global__ void tk_k_gate(volatile uint32_t* gate, uint64_t max_ticks) {
    const uint64_t t0 = wall_clock64();
    while (!__hip_atomic_load((const uint32_t*)gate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) && wall_clock64() - t0 < max_ticks) __builtin_amdgcn_s_sleep(16);
}
__global__ void tk_k_touch(uint32_t* p) { __hip_atomic_store(p, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM); }

static int streams_beside(tk_core* c, hipStream_t on, const std::vector<hipStream_t>& cand, std::vector<hipStream_t>* beside) {
    beside->clear();
    if (cand.empty()) return TK_OK;
    if (!c->h_probe) HIPCHK(c->h_probe.alloc(64 * 4, hipHostMallocCoherent | hipHostMallocMapped));
    volatile uint32_t* h = c->h_probe;
    uint32_t* d = nullptr;
    HIPCHK(hipHostGetDevicePointer((void**)&d, c->h_probe, 0));
    for (int i = 0; i < 64; ++i) h[i] = 0;
    hipLaunchKernelGGL(tk_k_gate, dim3(1), dim3(1), 0, on, (volatile uint32_t*)d, (uint64_t)400000);
    for (size_t i = 0; i < cand.size(); ++i) hipLaunchKernelGGL(tk_k_touch, dim3(1), dim3(1), 0, cand[i], d + 1 + i);
    // wait until the words have stopped arriving (a launch reaches the device within tens of microseconds)
    const double t0 = now_us();
    size_t seen = 0;
    double t_last = t0;
    for (;;) {
        size_t n = 0;
        for (size_t i = 0; i < cand.size(); ++i) n += h[1 + i] ? 1 : 0;
        const double t = now_us();
        if (n != seen) {
            seen = n;
            t_last = t;
        }
        if (n == cand.size() || (t - t0 > 200.0 && t - t_last > 100.0) || t - t0 > 2000.0) break;
    }
    std::vector<bool> ok(cand.size());
    for (size_t i = 0; i < cand.size(); ++i) ok[i] = h[1 + i] != 0;
    h[0] = 1u;  // open the gate
    HIPCHK(hipStreamSynchronize(on));
    for (hipStream_t q : cand) HIPCHK(hipStreamSynchronize(q));
    for (size_t i = 0; i < cand.size(); ++i)
        if (ok[i]) beside->push_back(cand[i]);
    return TK_OK;
}

// back-stage streams for front stream s: first those that run beside s, among them those that run beside each other
static int pick_back_streams(tk_core* c, hipStream_t s) {
    if (c->back_probed && c->back_for == s) return TK_OK;
    {  // (a caller that alternates between streams: what was found for a stream is kept)
        auto it = c->back_known.find(s);
        if (it != c->back_known.end()) {
            c->n_back = it->second.n;
            for (int i = 0; i < 3; ++i) c->back_s[i] = it->second.s[i];
            c->back_for = s;
            c->back_probed = true;
            return TK_OK;
        }
    }
    std::vector<hipStream_t> pool, f;
    for (WorkSet& w : c->ws) pool.push_back(w.sb);
    for (int i = 0; i < TK_NAUX; ++i) pool.push_back(c->aux[i]);
    c->n_back = 0;
    hipStream_t on = s;
    for (int r = 0; r < 3 && !pool.empty(); ++r) {
        TRY(streams_beside(c, on, pool, &f));
        if (f.empty()) break;
        c->back_s[c->n_back++] = on = f[0];
        pool.assign(f.begin() + 1, f.end());
    }
    if (c->n_back == 0) c->back_s[c->n_back++] = c->ws[0].sb;  // (nothing runs beside s: the stages take turns, as before)
    c->back_for = s;
    c->back_probed = true;
    tk_core::BackChoice bc{};
    bc.n = c->n_back;
    for (int i = 0; i < 3; ++i) bc.s[i] = c->back_s[i];
    if (c->back_known.size() < 64) c->back_known[s] = bc;
    return TK_OK;
}

// Hooks of the host-buffer entry point: the text of a chunk must have arrived before its kernels start, and its tokens can start
// their way back while the next chunk is being encoded.
struct ChunkHooks {
    std::function<int(uint64_t /*byte_end*/)> before;                                   // text [0, byte_end) has to be on the device
    std::function<int(uint64_t /*tok_begin*/, uint64_t /*n_tok*/, bool /*last*/)> after;  // a chunk's tokens are final (stream idle)
};

// Device-resident batch: cut into chunks at document boundaries and pipelined -- the front stage of chunk k + 1 is queued (on the
// caller's stream) before the back stage of chunk k (on the back-stage stream), so the two overlap on the device; TK_NSET work sets.
static int encode_device_pass(tk_core* c, hipStream_t s, const uint8_t* d_utf8, uint64_t n_bytes, const uint64_t* d_doc_off,
                              const uint64_t* h_doc_off, uint64_t n_docs, bool use_special, uint64_t* n_tokens_out,
                              uint64_t chunk_bytes, const ChunkHooks* hooks) {
    if (!chunk_bytes) chunk_bytes = c->chunk_bytes;
    c->st_bytes = c->st_pieces = c->st_tokens = c->st_medium = c->st_long = c->st_chunks = 0;
    c->st_docs = n_docs;
    TRY(ensure(c->out_tokens, (n_bytes + 64) * 4));  // (a token is at least one byte of text)
    TRY(ensure(c->out_tok_off, (n_docs + 2) * 8));
    uint32_t* d_out = c->out_tokens.as<uint32_t>();
    uint64_t* d_tok_off = c->out_tok_off.as<uint64_t>();
    // chunks: document ranges [d0, d1) of at most chunk_bytes (a longer document is a chunk of its own); cuts prefer documents that
    // start at a 16-byte aligned address (the kernels read the text with aligned 4- and 16-byte loads, some of them through the scalar
    // unit, which ignores the low address bits: any other chunk is first copied to an aligned buffer, ~0.1 ms per 128 MiB)
    struct Cut {
        uint64_t d0, d1, b, nn;
    };
    std::vector<Cut> cuts;
    if (n_bytes <= chunk_bytes || !h_doc_off) {
        if (n_bytes > chunk_bytes && n_bytes >= (3ull << 30)) return fail(TK_VALUE_ERROR, "h_doc_off is required when n_bytes exceeds the chunk size");
        cuts.push_back(Cut{0, n_docs, 0, n_bytes});
    } else {
        // (chunks of equal size, cut at the document boundaries next to j * n / N: a last chunk of a few KiB would still pay the back
        // stage's fixed latencies, about a millisecond; a chunk may exceed chunk_bytes by less than a document)
        const uint64_t n_cuts = (n_bytes + chunk_bytes - 1) / chunk_bytes;
        uint64_t d0 = 0;
        while (d0 < n_docs) {
            uint64_t d1 = d0 + 1;
            const uint64_t j = cuts.size() + 1;
            const uint64_t until = j >= n_cuts ? n_bytes : (uint64_t)((unsigned __int128)n_bytes * j / n_cuts);
            while (d1 < n_docs && h_doc_off[d1] < until && h_doc_off[d1 + 1] - h_doc_off[d0] <= chunk_bytes + (chunk_bytes >> 3)) ++d1;
            if (d1 < n_docs)  // an aligned cut a little earlier saves the next chunk its copy
                for (uint64_t q = d1; q > d0 + 1 && d1 - q < 256; --q)
                    if ((((uintptr_t)d_utf8 + h_doc_off[q]) & 15u) == 0) {
                        d1 = q;
                        break;
                    }
            const uint64_t b = h_doc_off[d0], nn = h_doc_off[d1] - b;
            if (nn >= (4ull << 30) - 65536) return fail(TK_VALUE_ERROR, "a single document of 4 GiB or more is not supported");
            cuts.push_back(Cut{d0, d1, b, nn});
            d0 = d1;
        }
        if (cuts.empty()) cuts.push_back(Cut{0, 0, 0, 0});
    }
    const size_t N = cuts.size();
    if (N > 1) TRY(pick_back_streams(c, s));
    TRY(ensure(c->tok_bases, (N + 2) * 8));
    HIPCHK(hipMemsetAsync(c->tok_bases.p, 0, 8, s));  // (before the first front stage on the same stream, which every back stage waits for)
    ChunkJob jobs[TK_NSET];
    auto front = [&](size_t k) -> int {
        WorkSet& w = c->ws[k % TK_NSET];
        const Cut& q = cuts[k];
        if (k >= TK_NSET) HIPCHK(hipStreamWaitEvent(s, w.ev_done, 0));  // the set's previous chunk has left its buffers
        if (hooks && hooks->before) TRY(hooks->before(q.b + q.nn));
        const uint8_t* tx = d_utf8 + q.b;
        if (((uintptr_t)tx & 15u) != 0 && q.nn) {
            TRY(ensure(w.text_al, q.nn + 256));
            HIPCHK(hipMemcpyAsync(w.text_al.p, tx, q.nn, hipMemcpyDeviceToDevice, s));
            HIPCHK(hipMemsetAsync((uint8_t*)w.text_al.p + q.nn, 0, 128, s));
            tx = w.text_al.as<uint8_t>();
        }
        const ChunkAsk ask{.kind = ChunkKind::Batch, .d_text = tx, .d_doc_off = d_doc_off + q.d0, .n = q.nn, .n_docs = q.d1 - q.d0, .base = q.b, .d_out = d_out,
                           .d_tok_off = d_tok_off + q.d0, .use_special = use_special};
        TRY(stage_front(c, w, jobs[k % TK_NSET], s, ask));
        jobs[k % TK_NSET].index = (uint32_t)k;
        return TK_OK;
    };
    uint64_t total = 0;
    auto finish = [&](size_t k) -> int {
        uint64_t t = 0;
        TRY(chunk_finish(c, c->ws[k % TK_NSET], jobs[k % TK_NSET], &t));
        if (hooks && hooks->after) TRY(hooks->after(total, t, k + 1 == N));
        total += t;
        return TK_OK;
    };
    for (double& x : c->host_us) x = 0;
    const double t_call = now_us();
    TRY(front(0));
    for (size_t k = 0; k < N; ++k) {
        if (k + 1 < N) {
            double t0 = now_us();
            if (k + 1 >= TK_NSET) TRY(finish(k + 1 - TK_NSET));  // (its totals are read before the set is handed to chunk k + 1)
            c->host_us[3] += now_us() - t0;
            t0 = now_us();
            TRY(front(k + 1));
            c->host_us[0] += now_us() - t0;
        }
        const double tb0 = now_us();
        // a single chunk keeps both stages on the caller's stream; otherwise every set's back stage has a stream of its own
        WorkSet& w = c->ws[k % TK_NSET];
        hipStream_t sb = N > 1 ? c->back_s[k % (size_t)c->n_back] : s;
        if (N > 1) HIPCHK(hipStreamWaitEvent(sb, w.ev_front, 0));
        TRY(stage_back(c, w, jobs[k % TK_NSET], sb, (N > 1 && k > 0) ? c->ws[(k - 1) % TK_NSET].ev_tot : (hipEvent_t) nullptr));
        c->host_us[1] += now_us() - tb0;
    }
    const double t_tail = now_us();
    for (size_t k = N > TK_NSET ? N - TK_NSET : 0; k < N; ++k) TRY(finish(k));
    HIPCHK(hipStreamSynchronize(s));
    c->host_us[4] = now_us() - t_tail;
    c->host_us[5] = now_us() - t_call;
    TRY(drain_events(c));
    *n_tokens_out = total;
    return TK_OK;
}

// The miss data's overflow entries are sized for ordinary text (stage_front).  A batch with more distinct missed pieces than that -- the
// counter on the device says so when a chunk is finished -- is run once more from its first chunk, with room for the worst case from
// then on (c->ovf_full).  Everything a pass writes is written again by the next one, and the hooks are idempotent (text already sent
// is not sent again; token ranges are copied again).
static int encode_device_locked(tk_core* c, hipStream_t s, const uint8_t* d_utf8, uint64_t n_bytes, const uint64_t* d_doc_off,
                                const uint64_t* h_doc_off, uint64_t n_docs, bool use_special, uint64_t* n_tokens_out,
                                uint64_t chunk_bytes = 0, const ChunkHooks* hooks = nullptr) {
    // (round 6) ... and so is a batch in which a deferred tile gave up its walk while the host was not waiting for the counters (TK_RESYNC,
    // stage_deferred): once more, waiting -- at most one repeat of either kind.
    int rc = encode_device_pass(c, s, d_utf8, n_bytes, d_doc_off, h_doc_off, n_docs, use_special, n_tokens_out, chunk_bytes, hooks);
    for (int again = 0; (rc == TK_GROW || rc == TK_RESYNC) && again < 2; ++again) {
        HIPCHK(hipDeviceSynchronize());  // (chunks of the abandoned pass may still be in flight on the sets' streams)
        (void)drain_events(c);
        if (rc == TK_GROW) c->st_regrown += 1;
        else c->st_resynced += 1;
        rc = encode_device_pass(c, s, d_utf8, n_bytes, d_doc_off, h_doc_off, n_docs, use_special, n_tokens_out, chunk_bytes, hooks);
    }
    if (rc == TK_SPEC_HIT) {  // (chunks are finished in document order: the first chunk with a hit holds the batch's first; those behind it are abandoned)
        HIPCHK(hipDeviceSynchronize());
        (void)drain_events(c);
        return rc;
    }
    if (rc == TK_GROW) return fail(TK_RUNTIME_ERROR, "internal error: the miss data overflowed at its largest size");
    if (rc == TK_RESYNC) return fail(TK_RUNTIME_ERROR, "internal error: a deferred tile gave up although the host was waiting");
    return rc;
}

static int encode_batch_device_impl(tk_core* c, const void* d_utf8, uint64_t n_bytes, const void* d_doc_off, const uint64_t* h_doc_off, uint64_t n_docs,
                                    int use_special, const uint32_t* allowed_ids, uint64_t n_allowed, void* stream, const uint32_t** d_tokens_out,
                                    uint64_t* n_tokens_out, const uint64_t** d_tok_off_out, const CheckArgs* chk, bool locked = false) {
    if (!c) return fail(TK_VALUE_ERROR, "core is null");
    TRY(check_disallowed_ids(c, chk));
    std::unique_lock<std::mutex> lk(c->mu, std::defer_lock);
    if (!locked) lk.lock();  // (locked: the caller holds c->mu -- tk_encode_jsonl, whose text is the core's own)
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    bool any = false;
    if (use_special) TRY(prepare_allowed(c, s, allowed_ids, n_allowed, &any));
    FindScope find(c);
    TRY(find.begin(s, chk));
    uint64_t total = 0;
    if (c->out_bufs == 2) {  // (the previous call's result stays where it is: a consumer on another stream may still be reading it)
        std::swap(c->out_tokens, c->out_tokens_alt);
        std::swap(c->out_tok_off, c->out_tok_off_alt);
    }
    const int rc = encode_device_locked(c, s, (const uint8_t*)d_utf8, n_bytes, (const uint64_t*)d_doc_off, h_doc_off, n_docs, use_special && any, &total);
    if (rc == TK_SPEC_HIT) {  // the few bytes at the hit, and the offsets where the caller has not given them, come to the host
        std::vector<uint8_t> at((size_t)std::min<uint64_t>(c->spec_max_len, n_bytes - c->find_hit));
        HIPCHK(hipMemcpy(at.data(), (const uint8_t*)d_utf8 + c->find_hit, at.size(), hipMemcpyDeviceToHost));
        std::vector<uint64_t> off;
        if (!h_doc_off) {
            off.resize(n_docs + 1);
            HIPCHK(hipMemcpy(off.data(), d_doc_off, (n_docs + 1) * 8, hipMemcpyDeviceToHost));
            h_doc_off = off.data();
        }
        return report_hit(c, at.data(), h_doc_off, n_docs, chk);
    }
    TRY(rc);
    if (d_tokens_out) *d_tokens_out = c->out_tokens.as<uint32_t>();
    if (d_tok_off_out) *d_tok_off_out = c->out_tok_off.as<uint64_t>();
    if (n_tokens_out) *n_tokens_out = total;
    return TK_OK;
}
extern "C" int tk_encode_batch_device(tk_core* c, const void* d_utf8, uint64_t n_bytes, const void* d_doc_off,
                                      const uint64_t* h_doc_off, uint64_t n_docs, int use_special, const uint32_t* allowed_ids,
                                      uint64_t n_allowed, void* stream, const uint32_t** d_tokens_out, uint64_t* n_tokens_out,
                                      const uint64_t** d_tok_off_out) {
    return encode_batch_device_impl(c, d_utf8, n_bytes, d_doc_off, h_doc_off, n_docs, use_special, allowed_ids, n_allowed, stream, d_tokens_out, n_tokens_out,
                                    d_tok_off_out, nullptr);
}
extern "C" int tk_encode_batch_device_checked(tk_core* c, const void* d_utf8, uint64_t n_bytes, const void* d_doc_off, const uint64_t* h_doc_off,
                                              uint64_t n_docs, int use_special, const uint32_t* allowed_ids, uint64_t n_allowed, void* stream,
                                              const uint32_t** d_tokens_out, uint64_t* n_tokens_out, const uint64_t** d_tok_off_out,
                                              const uint32_t* disallowed_ids, uint64_t n_disallowed, tk_special_hit* hit) {
    const CheckArgs chk{disallowed_ids, n_disallowed, hit};
    return encode_batch_device_impl(c, d_utf8, n_bytes, d_doc_off, h_doc_off, n_docs, use_special, allowed_ids, n_allowed, stream, d_tokens_out, n_tokens_out,
                                    d_tok_off_out, &chk);
}

// Host-buffer batches: the text goes to the device by DMA on a copy stream, straight from the caller's buffer, while earlier chunks are
// being encoded, and every chunk's tokens start their way back to a page-locked result buffer on a second copy stream while the next chunk
// is being encoded.  PCIe is the ceiling of this path (about 50 GB/s per direction).
#define TK_STAGE_BYTES (64ull << 20)  // a block of text on its way to the device; a staging buffer of tk_decode_batch

// host threads of the staging copies (ids into / bytes and regrown results out of page-locked buffers): the copy, not the link, bounds
// them (round 4: 8 threads, 25-34 GB/s of text; a GPU box gives the container 16 cores)
static unsigned copy_threads(unsigned hw) { return hw == 0 ? 4u : (hw > 16u ? 16u : hw); }

// the copy streams of the host-buffer entry points
static int ensure_copy_streams(tk_core* c) {
    for (Stream* cs : {&c->cs_h2d, &c->cs_d2h})
        if (!*cs) HIPCHK(cs->create());
    return TK_OK;
}

// offsets of a batch's documents: [0] is 0 and none is below the one before it (`name`: the argument's name in the message)
static int check_offsets(const uint64_t* off, uint64_t n_docs, const char* name) {
    if (off[0] != 0) return fail(TK_VALUE_ERROR, std::string(name) + "[0] must be 0");
    for (uint64_t d = 0; d < n_docs; ++d)
        if (off[d + 1] < off[d]) return fail(TK_VALUE_ERROR, std::string(name) + " must be non-decreasing");
    return TK_OK;
}
static void parallel_memcpy(void* dst, const void* src, size_t n, unsigned nth) {
    if (n < (8u << 20) || nth <= 1) {
        memcpy(dst, src, n);
        return;
    }
    std::vector<std::thread> th;
    const size_t per = ((n + nth - 1) / nth + 4095) & ~(size_t)4095;
    for (unsigned t = 0; t < nth; ++t) {
        const size_t a = (size_t)t * per;
        if (a >= n) break;
        const size_t len = a + per < n ? per : n - a;
        th.emplace_back([=]() { memcpy((uint8_t*)dst + a, (const uint8_t*)src + a, len); });
    }
    for (auto& t : th) t.join();
}

// One more owner (see the top of the file): a host array on its way to the device in blocks, sent on c->cs_h2d by a thread of its own
// while the caller's thread consumes the blocks.  The thread, its events and its flags go with this object, and it leaves no scope
// before the thread has ended and the copy stream is idle: an early return of the consumer cannot outlive either.
// staged: the source is pageable and the caller wants it copied through the core's two page-locked staging blocks (c->stage, c->ev_stage:
// made by the caller, a block of this feed fits into one) by a few host threads; otherwise the copy takes the source as it is.
struct Feed {
    tk_core* const c;
    uint8_t* const dst;
    const uint8_t* const src;
    const uint64_t n, block, n_blocks;
    const bool staged;
    std::vector<Event> ev;  // one per block: it has arrived
    std::atomic<int> rc{TK_OK};
    std::atomic<uint64_t> sent{0};
    std::thread th;
    Feed(tk_core* c_, void* dst_, const void* src_, uint64_t bytes, uint64_t block_, bool staged_ = false)
        : c(c_), dst((uint8_t*)dst_), src((const uint8_t*)src_), n(bytes), block(block_), n_blocks((bytes + block_ - 1) / block_), staged(staged_), ev(n_blocks) {}
    ~Feed() { if (th.joinable()) (void)finish(); }
    int start() {
        for (auto& e : ev) HIPCHK(e.create());
        th = std::thread([this]() {
            (void)hipSetDevice(c->device);
            const unsigned nth = copy_threads(std::thread::hardware_concurrency());
            for (uint64_t k = 0; k < n_blocks; ++k) {
                const uint64_t a = k * block, len = a + block < n ? block : n - a;
                const int slot = (int)(k & 1);
                const void* from = src + a;
                if (staged) {
                    if (k >= 2 && hipEventSynchronize(c->ev_stage[slot]) != hipSuccess) rc = TK_RUNTIME_ERROR;
                    parallel_memcpy(c->stage[slot], from, len, nth);
                    from = c->stage[slot];
                }
                if (hipMemcpyAsync(dst + a, from, len, hipMemcpyHostToDevice, c->cs_h2d) != hipSuccess) rc = TK_RUNTIME_ERROR;
                if (staged) (void)hipEventRecord(c->ev_stage[slot], c->cs_h2d);
                (void)hipEventRecord(ev[k], c->cs_h2d);
                sent.store(k + 1, std::memory_order_release);
            }
        });
        return TK_OK;
    }
    // the consumer: block k (and every one before it) has been sent, and stream `s` goes on once it has arrived
    int wait(uint64_t k, hipStream_t s) {
        while (sent.load(std::memory_order_acquire) <= k) std::this_thread::yield();
        if (rc.load() != TK_OK) return fail(TK_RUNTIME_ERROR, "host-to-device copy failed");
        HIPCHK(hipStreamWaitEvent(s, ev[k], 0));
        return TK_OK;
    }
    // every block has been sent and has arrived (or not: the copy stream's error)
    hipError_t finish() {
        if (th.joinable()) th.join();
        return hipStreamSynchronize(c->cs_h2d);
    }
};

// a result array on its way to the caller: page-locked from a MiB on (the copy back runs at the link's rate)
static void* result_alloc(size_t bytes) { return bytes >= (1u << 20) ? pinned_get(bytes) : malloc(bytes ? bytes : 1); }
// ... made for n elements that are on the device and filled with them (the caller lets go of it once every array of its call is there)
template <class T>
static int result_from_device(HostResult<T>& host, const void* d_src, uint64_t n) {
    host = HostResult<T>(result_alloc(n * sizeof(T)));
    if (!host) return fail(TK_RUNTIME_ERROR, "out of host memory");
    if (n) HIPCHK(hipMemcpy(host, d_src, n * sizeof(T), hipMemcpyDeviceToHost));
    return TK_OK;
}
// The result arrays of one call: fetch() makes each and fills it from the device, give() hands them all to the caller's out-pointers --
// called once every fetch has succeeded; a bag that goes without it frees what it has fetched.
struct ResultBag {
    HostResult<uint8_t> host[12];
    void* out[12];  // the caller's pointers, a T* each: set[i] knows which T
    void (*set[12])(void*, void*);
    int n = 0;
    template <class T>
    int fetch(T** o, const void* d_src, uint64_t count) {
        out[n] = o, set[n] = [](void* where, void* p) { *(T**)where = (T*)p; };
        return result_from_device(host[n++], d_src, count * sizeof(T));
    }
    void give() { for (int i = 0; i < n; ++i) set[i](out[i], host[i].release()); }
};
// A result array that is filled while its final size is not known yet, sized by the density so far: `done` of the call's `all` input units
// have made `need` elements (`filled` of them are in the array or on their way into it on c->cs_d2h, the others follow once this returns).
// An array that turns out too small is replaced by one of the new estimate and what it holds is copied over.
struct GrowRule {
    double slack;     // the estimate: the density so far times this ...
    uint64_t extra;   // ... plus so many elements
    bool pinned;      // page-locked whatever the size (otherwise: result_alloc's rule)
    const char* oom;  // the message when there is no memory
};
template <class T>
static int result_grow(tk_core* c, HostResult<T>& host, uint64_t& cap, uint64_t filled, uint64_t need, uint64_t done, uint64_t all, bool last, const GrowRule& g) {
    if (need <= cap && host) return TK_OK;
    uint64_t est = last ? need : (uint64_t)((double)need / (double)(done ? done : 1) * (double)all * g.slack) + g.extra;
    if (est < need) est = need;
    HostResult<T> nh(g.pinned ? pinned_get((est ? est : 1) * sizeof(T)) : result_alloc(est * sizeof(T)));
    if (!nh) return fail(TK_RUNTIME_ERROR, g.oom);
    if (host) {
        HIPCHK(hipStreamSynchronize(c->cs_d2h));
        if (filled) parallel_memcpy(nh, host, filled * sizeof(T), copy_threads(std::thread::hardware_concurrency()));
    }
    host = std::move(nh);  // (the old array goes with `nh`)
    cap = est;
    return TK_OK;
}

static int encode_batch_impl(tk_core* c, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, int use_special, const uint32_t* allowed_ids,
                             uint64_t n_allowed, uint32_t** tokens_out, uint64_t* n_tokens_out, uint64_t* tok_off_out, bool device_result, bool no_small,
                             const CheckArgs* chk = nullptr, bool locked = false);
// ---- the slots of the small-call path (tk_core::SmallSlot) ----
static int small_slot_init(tk_core* c, tk_core::SmallSlot* sl) {
    if (sl->ready) return TK_OK;  // (a first use that failed: what it did make is kept, the rest is made now)
    if (!sl->in) {
        HIPCHK(sl->in.alloc(TK_SMALL_MAX + 64, hipHostMallocCoherent | hipHostMallocMapped));
        memset(sl->in, 0, TK_SMALL_MAX + 64);
    }
    if (!sl->out) {
        HIPCHK(sl->out.alloc((TK_SMALL_HDR + TK_SMALL_MAX + 16) * 4, hipHostMallocCoherent | hipHostMallocMapped));
        memset(sl->out, 0, (TK_SMALL_HDR + TK_SMALL_MAX + 16) * 4);
    }
    TRY(ensure(sl->ws, 256 * TK_SMALL_PIECE * 4));
    HIPCHK(hipHostGetDevicePointer(&sl->d_in, sl->in, 0));
    HIPCHK(hipHostGetDevicePointer(&sl->d_out, sl->out, 0));
    sl->ready = true;
    return TK_OK;
}
// text -> the slot, marked ready: whoever launches next takes it along
static void small_slot_submit(tk_core::SmallSlot* sl, const uint8_t* utf8, uint32_t n, bool no_long = false) {
    memcpy(sl->in, utf8, n);
    memset(sl->in + n, 0, 8);
    sl->seq = ++sl->seq ? sl->seq : ++sl->seq;  // (never 0: the buffer starts zeroed)
    sl->n = n | (no_long ? TK_SMALL_NO_LONG : 0u);
    sl->state.store(1, std::memory_order_release);
}
// Hands a slot back on any exit path.  A slot that was submitted and never launched goes from "ready" to idle by compare-and-swap: a launcher
// that is taking it along at this very moment (1 -> 2) either loses that race or is seen.  A slot in state 2 whose kernel has not written
// the call's sequence number yet is IN FLIGHT on this call's buffers (the owner left early: its time-out); the next owner's text must not
// meet that kernel, so the slot is waited for (bounded) and, if the kernel never completes, stays busy for good (quarantined: the
// other slots remain).
static void small_slot_release(tk_core::SmallSlot* sl) {
    int st = 1;
    if (!sl->state.compare_exchange_strong(st, 0, std::memory_order_acq_rel)) {
        if (st == 2 && sl->out && __atomic_load_n(&sl->out[2], __ATOMIC_ACQUIRE) != sl->seq) {
            const auto t0 = std::chrono::steady_clock::now();
            while (__atomic_load_n(&sl->out[2], __ATOMIC_ACQUIRE) != sl->seq) {
                if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) return;  // (quarantined: busy stays set)
                std::this_thread::yield();
            }
        }
        sl->state.store(0, std::memory_order_release);
    }
    sl->busy.store(0, std::memory_order_release);
}
// Waits until every one of the caller's slots has completed (the kernel's last store is the slot's sequence number, system scope: watched
// instead of a stream); while one of them has not been launched, tries to be the one who launches -- EVERY ready slot of the core, the
// caller's or not (flat combining: try_lock, nobody waits for the mutex).
static int small_wait(tk_core* c, tk_core::SmallSlot* const* mine, uint32_t k) {
    const auto t0 = std::chrono::steady_clock::now();
    uint32_t spins = 0;
    for (;;) {
        bool all = true, unlaunched = false;
        for (uint32_t i = 0; i < k; ++i) {
            if (__atomic_load_n(&mine[i]->out[2], __ATOMIC_ACQUIRE) != mine[i]->seq) all = false;
            if (mine[i]->state.load(std::memory_order_acquire) == 1) unlaunched = true;
        }
        if (all) break;
        if (unlaunched && c->small_launch_mu.try_lock()) {
            std::lock_guard<std::mutex> lk(c->small_launch_mu, std::adopt_lock);
            TkSmallReqs R{};
            uint32_t cnt = 0;
            for (uint32_t j = 0; j < TK_SMALL_SLOTS && cnt < TK_SMALL_BATCH; ++j) {
                tk_core::SmallSlot& q = c->small[j];
                int expect = 1;
                if (q.state.load(std::memory_order_acquire) == 1 && q.state.compare_exchange_strong(expect, 2, std::memory_order_acq_rel))
                    R.r[cnt++] = TkSmallReq{(const uint8_t*)q.d_in, (uint32_t*)q.d_out, q.ws.as<uint32_t>(), q.n, q.seq};
            }
            if (cnt) {
                Stream& ls = c->small_s[c->small_turn++ & 3u];
                if (!ls) HIPCHK(ls.create());
                hipLaunchKernelGGL(tk_k_small, dim3(cnt), dim3(256), 0, ls, c->D, R);
                const hipError_t le = hipGetLastError();
                if (le != hipSuccess) {
                    // (the slots this launcher took go back to "ready": their owners try the launch themselves instead of waiting two seconds)
                    for (uint32_t j = 0; j < TK_SMALL_SLOTS; ++j) {
                        int two = 2;
                        for (uint32_t q = 0; q < cnt; ++q)
                            if (R.r[q].out == (uint32_t*)c->small[j].d_out) c->small[j].state.compare_exchange_strong(two, 1, std::memory_order_acq_rel);
                    }
                    return fail(TK_RUNTIME_ERROR, std::string("HIP error: ") + hipGetErrorString(le) + " in tk_k_small");
                }
                c->st_small_launches += 1;
                c->st_small_calls += cnt;
            }
            continue;
        }
        if ((++spins & 0xFFFu) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
            (void)hipDeviceSynchronize();
            for (uint32_t i = 0; i < k; ++i)
                if (__atomic_load_n(&mine[i]->out[2], __ATOMIC_ACQUIRE) != mine[i]->seq) return fail(TK_RUNTIME_ERROR, "the small-call kernel did not complete");
            break;
        }
        if ((spins & 127u) == 127u && c->small_active.load(std::memory_order_relaxed) > 8) std::this_thread::yield();  // (many callers, maybe more than cores: a spinning waiter must not keep the launcher off its core; a lone caller never yields)
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    for (uint32_t i = 0; i < k; ++i) mine[i]->state.store(0, std::memory_order_release);
    return TK_OK;
}

// One document of 2 .. 128 KiB without special tokens: cut into segments of at most TK_SMALL_MAX bytes at piece starts that are certain whatever
// stands on either side (an ASCII letter followed by a space, where the pattern's table says so: c->mid_cut), the segments encoded as so
// many small calls in ONE launch (a workgroup each), their tokens put together on the host.  The general pipeline costs a dozen dependent
// launches -- 0.15 ms for 4 KiB; this is one.  *handled = false: no cut where one is needed, not enough free slots, or a segment
// the small kernel does not do (a long piece that is not a token): the general path takes the call.
static int encode_mid(tk_core* c, const uint8_t* utf8, uint32_t n, uint32_t** tokens_out, uint64_t* n_tokens_out, bool* handled) {
    *handled = false;
    auto why = [&](const char* r) {
        if (c->dbg & TK_DBG_VERBOSE) fprintf(stderr, "encode_mid: %u bytes not taken: %s\n", n, r);
        return TK_OK;
    };
    if (!c->mid_cut) return why("letter -> space is not a certain start of this pattern");
    // (text full of long pieces that are not tokens -- URLs, runs of a script without spaces -- is not for the small kernel: after a call that
    // found that out, the next 16 .. 64 go straight to the general pipeline instead of paying for a launch first)
    if (c->mid_skip.load(std::memory_order_relaxed) > 0) {
        c->mid_skip.fetch_sub(1, std::memory_order_relaxed);
        return why("the last attempt met a long piece that is not a token");
    }
    // cuts: about equal segments, each from one certain piece start to the next (tk_mid_plan.h)
    static_assert(TK_MID_SEGMENT_MAX == TK_SMALL_MAX && TK_SMALL_SLOTS == TK_SMALL_BATCH, "a segment is one small call; one launch carries every slot");
    uint32_t cuts[TK_SMALL_SLOTS + 1];
    const char* reason = nullptr;
    const uint32_t k = tk_mid_plan(utf8, n, cuts, &reason);
    if (!k) return why(reason);
    // k free slots, or none
    tk_core::SmallSlot* mine[TK_SMALL_SLOTS];
    uint32_t got = 0;
    for (uint32_t j = 0; j < TK_SMALL_SLOTS && got < k; ++j) {
        tk_core::SmallSlot& cand = c->small[j];
        if (!cand.busy.load(std::memory_order_relaxed) && !cand.busy.exchange(1, std::memory_order_acquire)) mine[got++] = &cand;
    }
    struct Release {
        tk_core::SmallSlot** s;
        uint32_t* n;
        std::atomic<int>* active;
        ~Release() {
            for (uint32_t i = 0; i < *n; ++i) small_slot_release(s[i]);  // (also when small_wait left early -- a failed launch, its time-out: the next owner must not be launched with this call's text)
            active->fetch_sub(1, std::memory_order_relaxed);
        }
    } release_slots{mine, &got, &c->small_active};
    c->small_active.fetch_add(1, std::memory_order_relaxed);
    if (got < k) return why("not enough free slots");  // (other callers hold them: the general path)
    HIPCHK(hipSetDevice(c->device));
    for (uint32_t i = 0; i < k; ++i) TRY(small_slot_init(c, mine[i]));
    // (segments leave EVERY piece of more than TK_SMALL_PIECE bytes that is not a token to the general pipeline: sixty-four workgroups each
    // waiting for its longest chain of merges cost more than the pipeline, whose merge kernel runs all the chains of the document side by side
    // -- measured on web text, profiles/r04_mid_calls_corpus.txt)
    // (documents of up to 6 KiB: the segments merge their long pieces themselves -- 4 KiB of web text 140 us against 162 when a segment gives the
    // document up at such a piece, and 170 through the general pipeline; from 16 KiB on the pipeline wins on such text either way:
    // profiles/r05_small_variants.txt.  TK_DBG_KEEP_LONG: always.)
    const bool keep_long = n <= 6144u || (c->dbg & TK_DBG_KEEP_LONG);
    for (uint32_t i = 0; i < k; ++i) small_slot_submit(mine[i], utf8 + cuts[i], cuts[i + 1] - cuts[i], !keep_long);
    TRY(small_wait(c, mine, k));
    // the segments' tokens, one after the other.  A segment the small kernel did not do sends the WHOLE document to the general pipeline (one pass
    // over 64 KiB costs it little more than one over 2 KiB; segment by segment it was 1.4x the pipeline on web text), and the next calls do not
    // even try: 16 of them after the first such document, 32 and then 64 after further ones in a row, 16 again after a success
    uint64_t nt = 0;
    bool all_done = true;
    for (uint32_t i = 0; i < k; ++i) {
        if (mine[i]->out[0] != 1u) all_done = false;
        else nt += mine[i]->out[1];
    }
    if (!all_done) {
        const int run = std::min(std::max(c->mid_fail_run.load(std::memory_order_relaxed), 0), 2);  // (a lost update between two threads costs a launch, no more)
        c->mid_fail_run.store(std::min(run + 1, 2), std::memory_order_relaxed);
        c->mid_skip.store(16 << run, std::memory_order_relaxed);
        return why("a segment with a long piece that is not a token");
    }
    c->mid_fail_run.store(0, std::memory_order_relaxed);
    uint32_t* host = (uint32_t*)malloc((nt ? nt : 1) * 4);
    if (!host) return fail(TK_RUNTIME_ERROR, "out of host memory");
    uint64_t at = 0;
    for (uint32_t i = 0; i < k; ++i) {
        const uint32_t cnt = mine[i]->out[1];
        if (cnt) memcpy(host + at, mine[i]->out + TK_SMALL_HDR, (size_t)cnt * 4);
        at += cnt;
    }
    __atomic_store_n(&c->st_bytes, (uint64_t)n, __ATOMIC_RELAXED);
    __atomic_store_n(&c->st_tokens, nt, __ATOMIC_RELAXED);
    __atomic_store_n(&c->st_docs, (uint64_t)1, __ATOMIC_RELAXED);
    __atomic_store_n(&c->st_pieces, (uint64_t)0, __ATOMIC_RELAXED);
    __atomic_fetch_add(&c->st_mid_calls, (uint64_t)1, __ATOMIC_RELAXED);
    *tokens_out = host;
    *n_tokens_out = nt;
    *handled = true;
    return TK_OK;
}

// One short document without special tokens: one launch, no copies, no stream synchronisation (tk_k_small, tk_fused.h), and no lock: the
// call runs on a slot of its own (tk_core::SmallSlot), so the threads of a caller's pool overlap (core.py:175).
// Returns TK_OK with *handled = false when the call has to take the general path.
static int encode_small(tk_core* c, const uint8_t* utf8, uint32_t n, uint32_t** tokens_out, uint64_t* n_tokens_out, bool* handled) {
    *handled = false;
    // a free slot: start at a place of this thread's own, so that a pool of callers does not fight over slot 0
    static std::atomic<uint32_t> next_thread{0};
    static thread_local uint32_t home = next_thread.fetch_add(1, std::memory_order_relaxed);
    tk_core::SmallSlot* sl = nullptr;
    for (uint32_t spins = 0; !sl; ++spins) {
        for (uint32_t k = 0; k < TK_SMALL_SLOTS && !sl; ++k) {
            tk_core::SmallSlot& cand = c->small[(home + k) % TK_SMALL_SLOTS];
            if (!cand.busy.load(std::memory_order_relaxed) && !cand.busy.exchange(1, std::memory_order_acquire)) sl = &cand;
        }
        if (!sl) {
            if (spins > 64) std::this_thread::yield();  // (more callers than slots: a slot is held for some tens of microseconds)
#if defined(__x86_64__)
            else __builtin_ia32_pause();
#endif
        }
    }
    struct Release {
        tk_core::SmallSlot* s;
        std::atomic<int>* active;
        ~Release() {
            small_slot_release(s);  // (see encode_mid's guard)
            active->fetch_sub(1, std::memory_order_relaxed);
        }
    } release_slot{sl, &c->small_active};
    c->small_active.fetch_add(1, std::memory_order_relaxed);
    HIPCHK(hipSetDevice(c->device));
    TRY(small_slot_init(c, sl));
    if (c->profiling) {  // (kernel times are collected in the core's shared list: one caller at a time then, every call a launch of its own)
        std::lock_guard<std::mutex> lk(c->mu);
        memcpy(sl->in, utf8, n);
        memset(sl->in + n, 0, 8);
        sl->seq = ++sl->seq ? sl->seq : ++sl->seq;
        sl->n = n;
        if (!sl->s) HIPCHK(sl->s.create());
        TkSmallReqs R{};
        R.r[0] = TkSmallReq{(const uint8_t*)sl->d_in, (uint32_t*)sl->d_out, sl->ws.as<uint32_t>(), n, sl->seq};
        TRY(timed(c, sl->s, "tk_k_small", [&] { hipLaunchKernelGGL(tk_k_small, dim3(1), dim3(256), 0, sl->s, c->D, R); }));
        HIPCHK(hipStreamSynchronize(sl->s));
        TRY(drain_events(c));
    } else {
        small_slot_submit(sl, utf8, n);
    }
    TRY(small_wait(c, &sl, 1));
    if (sl->out[0] != 1u) return TK_OK;  // a long piece that is not a token: general path
    const uint64_t nt = sl->out[1];
    uint32_t* host = (uint32_t*)malloc((nt ? nt : 1) * 4);
    if (!host) return fail(TK_RUNTIME_ERROR, "out of host memory");
    memcpy(host, sl->out + TK_SMALL_HDR, nt * 4);
    // (statistics of the last call: plain words, written without the lock -- with several callers "the last call" is whoever came last)
    __atomic_store_n(&c->st_bytes, (uint64_t)n, __ATOMIC_RELAXED);
    __atomic_store_n(&c->st_tokens, nt, __ATOMIC_RELAXED);
    __atomic_store_n(&c->st_docs, (uint64_t)1, __ATOMIC_RELAXED);
    __atomic_store_n(&c->st_pieces, (uint64_t)0, __ATOMIC_RELAXED);
    __atomic_store_n(&c->st_medium, (uint64_t)0, __ATOMIC_RELAXED);
    __atomic_store_n(&c->st_long, (uint64_t)0, __ATOMIC_RELAXED);
    *tokens_out = host;
    *n_tokens_out = nt;
    *handled = true;
    return TK_OK;
}

// Host text in.  device_result = false: the contract of tk_encode_batch (ids in a host buffer the caller frees).  device_result = true: the ids
// stay on the device (c->out_tokens, c->out_tok_off: valid until the core's next call) and only the text crosses PCIe -- what the
// several-GPU gather needs; the one-launch small path (which writes straight to host memory) is not taken then.
static int encode_batch_impl(tk_core* c, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, int use_special,
                             const uint32_t* allowed_ids, uint64_t n_allowed, uint32_t** tokens_out, uint64_t* n_tokens_out,
                             uint64_t* tok_off_out, bool device_result, bool no_small, const CheckArgs* chk, bool locked /* the caller holds c->mu (and passes no_small) */) {
    if (!c) return fail(TK_VALUE_ERROR, "core is null");
    if (!doc_off || (!device_result && !tokens_out) || !n_tokens_out) return fail(TK_VALUE_ERROR, "null argument");
    TRY(check_offsets(doc_off, n_docs, "doc_off"));
    TRY(check_disallowed_ids(c, chk));
    if (chk && chk->n) no_small = true;  // (the one-launch paths do not search: a checked call takes the general pipeline)
    const uint64_t n_bytes = doc_off[n_docs];
    if (!no_small && !device_result && n_docs == 1 && n_bytes > 0 && n_bytes <= (uint64_t)TK_SMALL_MAX * TK_MID_SEGMENTS && !(use_special && n_allowed) && !(c->dbg & TK_DBG_NO_SMALL) && !c->has_rx &&
        (n_bytes <= TK_SMALL_MAX || !c->profiling)) {
        bool handled = false;  // (before the lock: small calls of several threads run side by side)
        if (n_bytes <= TK_SMALL_MAX) TRY(encode_small(c, utf8, (uint32_t)n_bytes, tokens_out, n_tokens_out, &handled));
        else TRY(encode_mid(c, utf8, (uint32_t)n_bytes, tokens_out, n_tokens_out, &handled));
        if (handled) {
            if (tok_off_out) {
                tok_off_out[0] = 0;
                tok_off_out[1] = *n_tokens_out;
            }
            return TK_OK;
        }
    }
    std::unique_lock<std::mutex> lk(c->mu, std::defer_lock);
    if (!locked) lk.lock();
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    TRY(ensure(c->text, n_bytes + 256));
    TRY(ensure(c->doc_off, (n_docs + 2) * 8));
    HIPCHK(hipMemsetAsync((uint8_t*)c->text.p + n_bytes, 0, 128, s));
    HIPCHK(hipMemcpyAsync(c->doc_off.p, doc_off, (n_docs + 1) * 8, hipMemcpyHostToDevice, s));
    bool any = false;
    if (use_special) TRY(prepare_allowed(c, s, allowed_ids, n_allowed, &any));
    FindScope find(c);
    TRY(find.begin(s, chk));
    uint64_t total = 0;
    if (n_bytes < 2 * TK_STAGE_BYTES) {
        // small batches: one copy each way (latency matters more than overlap)
        if (n_bytes) HIPCHK(hipMemcpyAsync(c->text.p, utf8, n_bytes, hipMemcpyHostToDevice, s));
        const int rc = encode_device_locked(c, s, c->text.as<uint8_t>(), n_bytes, c->doc_off.as<uint64_t>(), doc_off, n_docs, use_special && any, &total);
        if (rc == TK_SPEC_HIT) return report_hit(c, utf8 + c->find_hit, doc_off, n_docs, chk);
        TRY(rc);
        if (device_result) {
            *n_tokens_out = total;
            return TK_OK;
        }
        HostResult<uint32_t> host;
        TRY(result_from_device(host, c->out_tokens.p, total));
        if (tok_off_out) HIPCHK(hipMemcpy(tok_off_out, c->out_tok_off.p, (n_docs + 1) * 8, hipMemcpyDeviceToHost));
        *tokens_out = host.release();
        *n_tokens_out = total;
        return TK_OK;
    }
    // ---- pipelined
    TRY(ensure_copy_streams(c));
    // How the text gets to the device.  Round 6 measured the link on the bench's box (tools/ubench/pcie_rates.hip, profiles/r06_pcie_link.txt):
    // 57 GB/s either way alone, 48 GB/s each way with both directions busy -- and hipMemcpyAsync straight from PAGEABLE memory at 56.5 GB/s,
    // the runtime's own staging.  So the text takes that copy, in blocks of 64 MiB (smaller ones cost the copy its rate: 28 ms with 16 MiB), and
    // chunks of 32 MiB: 25 ms per GiB = 0.88 of what the link gives in both directions at once, where the staging buffers of rounds 2-5
    // (filled by host threads, 64 MiB at a time, chunks of 128 MiB) took 32 ms.
    HostResult<uint32_t> host;
    uint64_t host_cap = 0;  // tokens
    Feed feed(c, c->text.p, utf8, n_bytes, TK_STAGE_BYTES);
    TRY(feed.start());
    ChunkHooks hooks;
    hooks.before = [&](uint64_t byte_end) -> int { return byte_end ? feed.wait((byte_end - 1) / feed.block, s) : TK_OK; };  // the blocks up to byte_end
    const GrowRule grow{1.08, 4096, true, "out of page-locked host memory"};
    if (!device_result) hooks.after = [&](uint64_t tok_begin, uint64_t n_tok, bool last) -> int {
        // (c->st_bytes: bytes encoded so far -- the density of the chunks seen sizes the result buffer)
        TRY(result_grow(c, host, host_cap, tok_begin, tok_begin + n_tok, c->st_bytes, n_bytes, last, grow));
        if (n_tok) HIPCHK(hipMemcpyAsync(host + tok_begin, c->out_tokens.as<uint32_t>() + tok_begin, n_tok * 4, hipMemcpyDeviceToHost, c->cs_d2h));
        return TK_OK;
    };
    int rc = encode_device_locked(c, s, c->text.as<uint8_t>(), n_bytes, c->doc_off.as<uint64_t>(), doc_off, n_docs, use_special && any, &total,
                                  32ull << 20, &hooks);
    hipError_t e = feed.finish();
    if (e == hipSuccess) e = hipStreamSynchronize(c->cs_d2h);
    if (rc == TK_SPEC_HIT) {  // (the text has arrived and nothing is on its way back: the caller's buffers are his again)
        if (e != hipSuccess) return fail(TK_RUNTIME_ERROR, std::string("HIP error: ") + hipGetErrorString(e));
        return report_hit(c, utf8 + c->find_hit, doc_off, n_docs, chk);
    }
    if (rc == TK_OK && e != hipSuccess) rc = fail(TK_RUNTIME_ERROR, std::string("HIP error: ") + hipGetErrorString(e));
    if (rc == TK_OK && tok_off_out && !device_result) {
        e = hipMemcpy(tok_off_out, c->out_tok_off.p, (n_docs + 1) * 8, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(TK_RUNTIME_ERROR, std::string("HIP error: ") + hipGetErrorString(e));
    }
    TRY(rc);
    *n_tokens_out = total;
    if (device_result) return TK_OK;
    *tokens_out = host ? host.release() : (uint32_t*)pinned_get(64);
    return TK_OK;
}

// encode, keep the ids on the device (c->out_tokens, c->out_tok_off) for a pass over them; the caller holds c->mu
static int encode_batch_kept(tk_core* c, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, int use_special, const uint32_t* allowed_ids,
                             uint64_t n_allowed, const CheckArgs& chk, uint64_t* n_tokens_out) {
    return encode_batch_impl(c, utf8, doc_off, n_docs, use_special, allowed_ids, n_allowed, nullptr, n_tokens_out, nullptr, /* device_result */ true, /* no_small */ true,
                             chk.n ? &chk : nullptr, /* locked */ true);
}
// The host-text entries that run a pass over the ids of the batch they have just encoded (tk_encode_batch_spans, _rows, _padded), under
// the core's mutex from the encode to the end: `outs`: the entry's own pointers are there; check(): what of its arguments can be refused
// before anything is encoded; pass(n): the device pass over c->out_tokens (n ids) and c->out_tok_off; tail(n): its results to the caller.
template <class Check, class Pass, class Tail>
static int encode_batch_pass(tk_core* c, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, int use_special, const uint32_t* allowed_ids, uint64_t n_allowed,
                             const uint32_t* disallowed_ids, uint64_t n_disallowed, tk_special_hit* hit, bool outs, Check&& check, Pass&& pass, Tail&& tail) {
    if (!c) return fail(TK_VALUE_ERROR, "core is null");
    if (!outs || (n_disallowed && !hit)) return fail(TK_VALUE_ERROR, "null argument");
    TRY(check());
    const CheckArgs chk{disallowed_ids, n_disallowed, hit};
    std::lock_guard<std::mutex> lk(c->mu);
    uint64_t n = 0;
    TRY(encode_batch_kept(c, utf8, doc_off, n_docs, use_special, allowed_ids, n_allowed, chk, &n));
    TRY(drained(c, [&] { return pass(n); }));
    return tail(n);
}

extern "C" int tk_encode_batch(tk_core* c, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, int use_special,
                               const uint32_t* allowed_ids, uint64_t n_allowed, uint32_t** tokens_out, uint64_t* n_tokens_out,
                               uint64_t* tok_off_out) {
    return encode_batch_impl(c, utf8, doc_off, n_docs, use_special, allowed_ids, n_allowed, tokens_out, n_tokens_out, tok_off_out, false, false);
}
// The same with Encoding.encode_batch's disallowed_special (tiktoken/core.py:116-124) checked in the same call, on the text it has moved to
// the device: see include/tiktoken_amd.h.
extern "C" int tk_encode_batch_checked(tk_core* c, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, int use_special, const uint32_t* allowed_ids,
                                       uint64_t n_allowed, const uint32_t* disallowed_ids, uint64_t n_disallowed, uint32_t** tokens_out,
                                       uint64_t* n_tokens_out, uint64_t* tok_off_out, tk_special_hit* hit) {
    const CheckArgs chk{disallowed_ids, n_disallowed, hit};
    return encode_batch_impl(c, utf8, doc_off, n_docs, use_special, allowed_ids, n_allowed, tokens_out, n_tokens_out, tok_off_out, false, false, &chk);
}

// Debug / test entry: the piece-start offsets the GPU pre-tokeniser produces for a packed batch
// (what regex.find_iter yields at src/lib.rs:365 and :405).  *starts_out gets n_pieces+1 uint32
// values (ascending piece starts, then the total byte count); release with tk_free.
extern "C" int tk_pretokenize_batch(tk_core* c, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, int use_special,
                                    const uint32_t* allowed_ids, uint64_t n_allowed, uint32_t** starts_out, uint64_t* n_out) {
    if (!c) return fail(TK_VALUE_ERROR, "core is null");
    if (!doc_off || !starts_out || !n_out) return fail(TK_VALUE_ERROR, "null argument");
    TRY(check_offsets(doc_off, n_docs, "doc_off"));
    const uint64_t n_bytes = doc_off[n_docs];
    if (n_bytes > c->chunk_bytes) return fail(TK_VALUE_ERROR, "tk_pretokenize_batch handles a single chunk only");
    if (n_bytes >= (1ull << 31)) return fail(TK_VALUE_ERROR, "tk_pretokenize_batch: less than 2 GiB per call (bit 31 of an offset marks a gap char)");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    TRY(ensure(c->text, n_bytes + 256));
    TRY(ensure(c->doc_off, (n_docs + 2) * 8));
    if (n_bytes) HIPCHK(hipMemcpyAsync(c->text.p, utf8, n_bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync((uint8_t*)c->text.p + n_bytes, 0, 128, s));
    HIPCHK(hipMemcpyAsync(c->doc_off.p, doc_off, (n_docs + 1) * 8, hipMemcpyHostToDevice, s));
    bool any = false;
    if (use_special) TRY(prepare_allowed(c, s, allowed_ids, n_allowed, &any));
    uint64_t P = 0;
    const ChunkAsk ask{.kind = ChunkKind::PieceStarts, .d_text = c->text.as<uint8_t>(), .d_doc_off = c->doc_off.as<uint64_t>(), .n = n_bytes, .n_docs = n_docs,
                       .use_special = use_special && any};
    TRY(run_chunk(c, s, ask, &P));
    HIPCHK(hipStreamSynchronize(s));
    TRY(drain_events(c));
    HostResult<uint32_t> host(malloc((P + 1) * 4));
    if (!host) return fail(TK_RUNTIME_ERROR, "out of host memory");
    HIPCHK(hipMemcpy(host, c->ws[0].pstart.p, (P + 1) * 4, hipMemcpyDeviceToHost));
    *starts_out = host.release();
    *n_out = P + 1;
    return TK_OK;
}

extern "C" int tk_encode_ordinary(tk_core* c, const uint8_t* utf8, uint64_t len, uint32_t** tokens_out, uint64_t* n_tokens_out) {
    uint64_t off[2] = {0, len};
    return tk_encode_batch(c, utf8, off, 1, 0, nullptr, 0, tokens_out, n_tokens_out, nullptr);
}

extern "C" int tk_encode(tk_core* c, const uint8_t* utf8, uint64_t len, const uint32_t* allowed_ids, uint64_t n_allowed,
                         uint32_t** tokens_out, uint64_t* n_tokens_out) {
    uint64_t off[2] = {0, len};
    return tk_encode_batch(c, utf8, off, 1, 1, allowed_ids, n_allowed, tokens_out, n_tokens_out, nullptr);
}

static int single_piece(tk_core* c, const uint8_t* piece, uint64_t len, ChunkKind kind, uint32_t** tokens_out, uint64_t* n_tokens_out) {
    if (!c) return fail(TK_VALUE_ERROR, "core is null");
    if (!tokens_out || !n_tokens_out) return fail(TK_VALUE_ERROR, "null argument");
    if (len >= (4ull << 30) - 65536) return fail(TK_VALUE_ERROR, "piece too long");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    c->st_bytes = c->st_pieces = c->st_tokens = c->st_medium = c->st_long = c->st_chunks = 0;
    TRY(ensure(c->text, len + 256));
    if (len) HIPCHK(hipMemcpyAsync(c->text.p, piece, len, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync((uint8_t*)c->text.p + len, 0, 128, s));
    TRY(ensure(c->out_tokens, (len + 64) * 4));
    uint64_t total = 0;
    const ChunkAsk ask{.kind = kind, .d_text = c->text.as<uint8_t>(), .n = len, .d_out = c->out_tokens.as<uint32_t>()};
    TRY(run_chunk(c, s, ask, &total));
    HIPCHK(hipStreamSynchronize(s));
    TRY(drain_events(c));
    HostResult<uint32_t> host(malloc((total ? total : 1) * 4));
    if (!host) return fail(TK_RUNTIME_ERROR, "out of host memory");
    if (total) HIPCHK(hipMemcpy(host, c->out_tokens.p, total * 4, hipMemcpyDeviceToHost));
    *tokens_out = host.release();
    *n_tokens_out = total;
    return TK_OK;
}

extern "C" int tk_encode_single_piece(tk_core* c, const uint8_t* piece, uint64_t len, uint32_t** tokens_out, uint64_t* n_tokens_out) {
    return single_piece(c, piece, len, ChunkKind::SinglePiece, tokens_out, n_tokens_out);
}

extern "C" int tk_byte_pair_encode(tk_core* c, const uint8_t* piece, uint64_t len, uint32_t** tokens_out, uint64_t* n_tokens_out) {
    return single_piece(c, piece, len, ChunkKind::SinglePieceNoLookup, tokens_out, n_tokens_out);
}

extern "C" int tk_encode_single_token(tk_core* c, const uint8_t* piece, uint64_t len, uint32_t* token_out) {
    if (!c) return fail(TK_VALUE_ERROR, "core is null");
    uint32_t r = len < 0xFFFFFFFFull ? c->H.lookup_piece(piece, (uint32_t)len) : TK_RANK_MAX;
    if (r == TK_RANK_MAX) {
        const TkHostTables& H = c->H;
        for (size_t k = 0; k + 1 < H.spec_off.size(); ++k)
            if (H.spec_off[k + 1] - H.spec_off[k] == len && memcmp(H.spec_bytes.data() + H.spec_off[k], piece, len) == 0) r = H.spec_id[k];
    }
    if (r == TK_RANK_MAX) return fail(TK_KEY_ERROR, "token not found");
    *token_out = r;
    return TK_OK;
}

extern "C" int tk_decode_single_token_bytes(tk_core* c, uint32_t token, const uint8_t** bytes_out, uint64_t* len_out) {
    if (!c) return fail(TK_VALUE_ERROR, "core is null");
    if (const auto* e = c->H.find_token(token)) {
        *bytes_out = c->H.tok_bytes.data() + e->first;
        *len_out = e->second;
        return TK_OK;
    }
    auto it = c->H.spec_decoder.find(token);
    if (it != c->H.spec_decoder.end()) {
        *bytes_out = c->H.spec_bytes.data() + it->second.first;
        *len_out = it->second.second;
        return TK_OK;
    }
    return fail(TK_KEY_ERROR, std::to_string(token));
}

// the reference's KeyError for an id that has no bytes: ids[pos], ids on the device or on the host
static int invalid_token(const uint32_t* ids, uint64_t pos, bool on_device) {
    uint32_t bad_tok = 0;
    if (on_device) (void)hipMemcpy(&bad_tok, ids + pos, 4, hipMemcpyDeviceToHost);
    else bad_tok = ids[pos];
    return fail(TK_KEY_ERROR, "Invalid token for decoding: " + std::to_string(bad_tok));
}

extern "C" int tk_decode_bytes(tk_core* c, const uint32_t* tokens, uint64_t n, uint8_t** bytes_out, uint64_t* len_out) {
    if (!c) return fail(TK_VALUE_ERROR, "core is null");
    if (n >= 8192 && c->n_dec) {  // long inputs: on the device (short ones are quicker on the host than a launch)
        const uint64_t off[2] = {0, n};
        return tk_decode_batch(c, tokens, off, 1, bytes_out, len_out, nullptr);
    }
    std::string acc;
    acc.reserve(n * 4);
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t* p;
        uint64_t l;
        if (tk_decode_single_token_bytes(c, tokens[i], &p, &l) != TK_OK) return invalid_token(tokens, i, false);
        acc.append((const char*)p, l);
    }
    uint8_t* host = (uint8_t*)malloc(acc.size() ? acc.size() : 1);
    memcpy(host, acc.data(), acc.size());
    *bytes_out = host;
    *len_out = acc.size();
    return TK_OK;
}

// CoreBPE.decode_bytes over a packed batch (Encoding.decode_bytes_batch / decode_batch, tiktoken/core.py:331-350), on the device.
static int decode_table_check(tk_core* c) { return c->n_dec ? TK_OK : fail(TK_UNSUPPORTED, "token ids are too sparse for the device decode table"); }
constexpr uint64_t ID_RANGE = TK_STAGE_BYTES / 4;  // ids per range of a host batch that is decoded in ranges (a multiple of TK_DEC_BLOCK)
static uint64_t id_ranges(uint64_t n) { return (n + ID_RANGE - 1) / ID_RANGE; }

struct DecodeView {  // the decode workspace of the core, valid until its next decode or spans call
    uint32_t* lens = nullptr;                             // bytes of every token
    unsigned long long *bsum = nullptr, *tots = nullptr;  // bytes per workgroup; the report words {bytes, first invalid position}: the batch's, then every range's
    unsigned long long* tboff = nullptr;                  // byte offset of every token (null unless asked for)
    uint64_t *tok_off = nullptr, *byte_off = nullptr;     // n_docs + 1 each (null unless asked for)
};
// ... made for n ids in n_ranges ranges; tboff, docs: with the token offsets, with the two arrays over the n_docs documents
static int decode_view(tk_core* c, uint64_t n, uint64_t n_ranges, bool tboff, bool docs, uint64_t n_docs, DecodeView* v) {
    const uint64_t nb = n / TK_DEC_BLOCK + 1;  // (workgroups over the positions 0 .. n: the span passes have one more position than tk_k_dec_len)
    Carve sums, doc;
    const uint64_t at_bsum = sums.add(nb * 8), at_tots = sums.add((n_ranges + 1) * 16);
    const uint64_t at_tok_off = doc.add((n_docs + 1) * 8), at_byte_off = doc.add((n_docs + 1) * 8);
    TRY(ensure(c->d_lens, (n + 1) * 4));
    TRY(ensure(c->d_bsum, sums.total));
    if (tboff) TRY(ensure(c->d_tboff, (n + 1) * 8));
    if (docs) TRY(ensure(c->d_boff, doc.total));
    *v = DecodeView{c->d_lens.as<uint32_t>(), carved<unsigned long long>(c->d_bsum, at_bsum), carved<unsigned long long>(c->d_bsum, at_tots),
                    tboff ? c->d_tboff.as<unsigned long long>() : nullptr, docs ? carved<uint64_t>(c->d_boff, at_tok_off) : nullptr,
                    docs ? carved<uint64_t>(c->d_boff, at_byte_off) : nullptr};
    return TK_OK;
}

// One range of a packed batch on the device: lengths and their block sums, the scan, then (decode_range_copy) the bytes, and the tokens'
// byte offsets if the view has them.
//   d_tok: the batch's ids on the device; [a, a + cnt) the range (a: a multiple of TK_DEC_BLOCK); `tot`: two device words {bytes of the
//   range, first invalid position (the caller sets it to ~0 once)}
static int decode_range_len(tk_core* c, hipStream_t s, const DecodeView& v, const uint32_t* d_tok, uint64_t a, uint64_t cnt, unsigned long long* tot) {
    const uint64_t nb = (cnt + TK_DEC_BLOCK - 1) / TK_DEC_BLOCK;
    unsigned long long* bsum = v.bsum + a / TK_DEC_BLOCK;
    TRY(timed(c, s, "tk_k_dec_len", [&] {
        hipLaunchKernelGGL(tk_k_dec_len, dim3((uint32_t)nb), dim3(256), 0, s, d_tok + a, cnt, c->t_dec.as<uint2>(), c->n_dec, v.lens + a, bsum, tot + 1, a);
    }));
    hipLaunchKernelGGL(tk_k_dec_scan64, dim3(1), dim3(1024), 0, s, bsum, nb, tot);
    return TK_OK;
}
static int decode_range_copy(tk_core* c, hipStream_t s, const DecodeView& v, const uint32_t* d_tok, uint64_t a, uint64_t cnt, uint8_t* d_out, uint64_t byte_base) {
    const uint64_t nb = (cnt + TK_DEC_BLOCK - 1) / TK_DEC_BLOCK;
    TRY(timed(c, s, "tk_k_dec_copy", [&] {
        hipLaunchKernelGGL(tk_k_dec_copy, dim3((uint32_t)nb), dim3(256), 0, s, d_tok + a, cnt, c->t_dec.as<uint2>(), v.lens + a, v.bsum + a / TK_DEC_BLOCK, c->D.tok_bytes,
                           c->D.spec_bytes, d_out, v.tboff ? v.tboff + a : nullptr, (unsigned long long)byte_base);
    }));
    return TK_OK;
}
// A batch of n host ids through the device in its ranges, as tk_decode_batch and tk_decode_batch_spans run a large one: the ids travel into
// c->d_tok on c->cs_h2d, a range at a time (`staged`: through the core's staging blocks, see Feed); step(k, a, cnt) is called once the ids
// [a, a + cnt) of range k have been sent and `s` waits for them: it queues the range's work on `s` and what goes back to the host on
// c->cs_d2h, so the ids of range k + 1 travel in while range k is computed and the results of range k - 1 travel out.  after(): queued behind
// the last range.  The first error ends the ranges; however they ended, the three streams are idle when this returns: nothing is on its way
// into the caller's result buffers when they are let go.
template <class Step, class After>
static int ranged_ids_pass(tk_core* c, hipStream_t s, const uint32_t* ids, uint64_t n, bool staged, Step&& step, After&& after) {
    TRY(ensure_copy_streams(c));
    Feed feed(c, c->d_tok.p, ids, n * 4, ID_RANGE * 4, staged);
    TRY(feed.start());
    int rc = TK_OK;
    for (uint64_t k = 0; k < id_ranges(n) && rc == TK_OK; ++k) {
        const uint64_t a = k * ID_RANGE;
        rc = feed.wait(k, s);
        if (rc == TK_OK) rc = step(k, a, std::min(ID_RANGE, n - a));
    }
    hipError_t e = feed.finish();
    if (rc == TK_OK) rc = after();
    const hipError_t e_s = hipStreamSynchronize(s), e_out = hipStreamSynchronize(c->cs_d2h);  // (both, whatever came before)
    if (e == hipSuccess) e = e_s != hipSuccess ? e_s : e_out;
    if (e == hipSuccess) e = hipGetLastError();
    if (rc == TK_OK && e != hipSuccess) rc = fail(TK_RUNTIME_ERROR, std::string("HIP error: ") + hipGetErrorString(e));
    return rc;
}

// Device-resident decode: ids and token offsets in HBM in, bytes and byte offsets in HBM out (library-owned buffers, valid until the core's
// next decode call).  The host learns the byte count (one 16-byte copy): the output buffer is sized by it.
// decode_device_run: the caller holds c->mu (tk_decode_batch_device, and the decode-rows entries behind their own passes).
static int decode_device_run(tk_core* c, hipStream_t s, const uint32_t* d_tok, uint64_t n, const uint64_t* d_tok_off, uint64_t n_docs, DecodeView* v, uint64_t* nbytes) {
    TRY(decode_table_check(c));
    TRY(decode_view(c, n, 0, d_tok_off != nullptr, true, n_docs, v));
    unsigned long long h_tot[2] = {0, ~0ull};
    HIPCHK(hipMemcpyAsync(v->tots, h_tot, 16, hipMemcpyHostToDevice, s));
    if (n) TRY(decode_range_len(c, s, *v, d_tok, 0, n, v->tots));
    HIPCHK(hipMemcpyAsync(h_tot, v->tots, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (h_tot[1] != ~0ull) return invalid_token(d_tok, h_tot[1], true);
    *nbytes = h_tot[0];
    TRY(ensure(c->d_bytes, *nbytes + 16));
    if (n) TRY(decode_range_copy(c, s, *v, d_tok, 0, n, c->d_bytes.as<uint8_t>(), 0));
    if (d_tok_off)
        hipLaunchKernelGGL(tk_k_dec_docoff, dim3(grid_for(n_docs + 1, 256, 4096)), dim3(256), 0, s, d_tok_off, n_docs, n, v->tboff, v->tots, v->byte_off);
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    return TK_OK;
}
extern "C" int tk_decode_batch_device(tk_core* c, const void* d_tokens, uint64_t n_tokens, const void* d_tok_off, uint64_t n_docs, void* stream,
                                      const uint8_t** d_bytes_out, uint64_t* n_bytes_out, const uint64_t** d_byte_off_out) {
    DecodeView v;
    uint64_t nbytes = 0;
    TRY(device_pass(c, n_bytes_out && (d_tokens || !n_tokens), stream, [&](hipStream_t s) -> int {
        return decode_device_run(c, s, (const uint32_t*)d_tokens, n_tokens, (const uint64_t*)d_tok_off, n_docs, &v, &nbytes);
    }));
    if (d_bytes_out) *d_bytes_out = c->d_bytes.as<uint8_t>();
    if (d_byte_off_out) *d_byte_off_out = d_tok_off ? v.byte_off : nullptr;
    *n_bytes_out = nbytes;
    return TK_OK;
}

// Host buffers in, host buffers out.  The batch is decoded in ranges of 16 Mi ids (ranged_ids_pass): the ids travel through two page-locked
// staging buffers filled by a few host threads, or straight from the caller's buffer when that is page-locked itself (the result of an
// encode call is); the bytes of a range travel back from one of two buffers while the next range is decoded into the other.  The result
// buffer is page-locked and sized by the density of the ranges seen so far (grown by a copy if a later range is denser).
extern "C" int tk_decode_batch(tk_core* c, const uint32_t* tokens, const uint64_t* tok_off, uint64_t n_docs, uint8_t** bytes_out,
                               uint64_t* n_bytes_out, uint64_t* byte_off_out) {
    if (!c) return fail(TK_VALUE_ERROR, "core is null");
    if (!tok_off || !bytes_out || !n_bytes_out) return fail(TK_VALUE_ERROR, "null argument");
    TRY(check_offsets(tok_off, n_docs, "tok_off"));
    TRY(decode_table_check(c));
    const uint64_t n = tok_off[n_docs], n_ranges = id_ranges(n);
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    DecodeView v;
    TRY(decode_view(c, n, n_ranges, byte_off_out != nullptr, true, n_docs, &v));
    TRY(ensure(c->d_tok, (n + 1) * 4));
    const uint32_t* d_tok = c->d_tok.as<uint32_t>();
    for (int i = 0; i < 2; ++i) {  // the staging buffers (this entry's own: the text of tk_encode_batch goes straight from the caller's buffer)
        if (!c->stage[i]) HIPCHK(c->stage[i].alloc(TK_STAGE_BYTES, hipHostMallocPortable));
        if (!c->ev_stage[i]) HIPCHK(c->ev_stage[i].create());
    }
    // is the caller's buffer page-locked (then the DMA engine reads it directly)?
    bool src_pinned = false;
    {
        hipPointerAttribute_t at;
        if (n && hipPointerGetAttributes(&at, tokens) == hipSuccess) src_pinned = at.type == hipMemoryTypeHost;
        else (void)hipGetLastError();
    }
    std::vector<Event> ev_out(2);
    for (auto& e : ev_out) HIPCHK(e.create());
    Event ev_copy;
    HIPCHK(ev_copy.create());
    HostResult<uint8_t> host;
    uint64_t host_cap = 0, base = 0;
    const GrowRule grow{1.06, 4096, n_ranges > 1, "out of host memory"};
    Buf* dout[2] = {&c->d_bytes, &c->d_bytes_alt};
    // every pair's position word to all ones = no id offends (the byte counts are written before they are read: tk_k_dec_scan64, doc_offsets below)
    HIPCHK(hipMemsetAsync(v.tots, 0xFF, (n_ranges + 1) * 16, s));
    const double t_call = now_us();
    double t_0 = t_call;  // when the wait for a range's ids began: the end of the step before
    unsigned long long h_total = 0;
    auto step = [&](uint64_t k, uint64_t a, uint64_t cnt) -> int {
        const double t_1 = now_us();
        unsigned long long* tot = v.tots + 2 * (k + 1);
        TRY(decode_range_len(c, s, v, d_tok, a, cnt, tot));
        unsigned long long h_tot[2] = {0, ~0ull};
        HIPCHK(hipMemcpyAsync(h_tot, tot, 16, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (h_tot[1] != ~0ull) return invalid_token(tokens, h_tot[1], false);
        const uint64_t nbk = h_tot[0];
        const double t_2 = now_us();
        Buf& d = *dout[k & 1];
        if (k >= 2) HIPCHK(hipEventSynchronize(ev_out[k & 1]));  // the buffer's previous bytes have left
        TRY(ensure(d, nbk + 16));
        TRY(decode_range_copy(c, s, v, d_tok, a, cnt, d.as<uint8_t>(), base));
        HIPCHK(hipEventRecord(ev_copy, s));
        // the result buffer: sized by the density so far
        const uint64_t need = base + nbk, done = a + cnt;
        TRY(result_grow(c, host, host_cap, base, need, done, n, done == n, grow));
        const double t_3 = now_us();
        if (c->dbg & TK_DBG_VERBOSE)
            fprintf(stderr, "decode range %llu: at %.0f us; ids waited %.0f us, lengths %.0f us, buffers %.0f us\n", (unsigned long long)k, t_0 - t_call, t_1 - t_0,
                    t_2 - t_1, t_3 - t_2);
        HIPCHK(hipStreamWaitEvent(c->cs_d2h, ev_copy, 0));
        if (nbk) HIPCHK(hipMemcpyAsync(host + base, d.p, nbk, hipMemcpyDeviceToHost, c->cs_d2h));
        HIPCHK(hipEventRecord(ev_out[k & 1], c->cs_d2h));
        base = need;
        t_0 = now_us();
        return TK_OK;
    };
    auto doc_offsets = [&]() -> int {
        if (!byte_off_out) return TK_OK;
        h_total = base;
        HIPCHK(hipMemcpyAsync(v.tots, &h_total, 8, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(v.tok_off, tok_off, (n_docs + 1) * 8, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(tk_k_dec_docoff, dim3(grid_for(n_docs + 1, 256, 4096)), dim3(256), 0, s, v.tok_off, n_docs, n, v.tboff, v.tots, v.byte_off);
        HIPCHK(hipMemcpyAsync(byte_off_out, v.byte_off, (n_docs + 1) * 8, hipMemcpyDeviceToHost, s));
        return TK_OK;
    };
    TRY(drained(c, [&] {  // (before the outputs are published: a caller that gets an error owns nothing)
        const int rc = ranged_ids_pass(c, s, tokens, n, !src_pinned, step, doc_offsets);
        if (c->dbg & TK_DBG_VERBOSE) fprintf(stderr, "decode: %llu ranges, ids %s, %.0f us\n", (unsigned long long)n_ranges, src_pinned ? "page-locked" : "staged", now_us() - t_call);
        return rc;
    }));
    *bytes_out = host ? host.release() : (uint8_t*)malloc(1);
    *n_bytes_out = base;
    return TK_OK;
}

// ------------------------------------------------------------------------------------------
// Token spans (tk_offsets.h): Encoding.decode_with_offsets (tiktoken/core.py:312-335) and decode_tokens_bytes (:303-310) for packed batches.
// ------------------------------------------------------------------------------------------
struct SpanView {  // device buffers of the core, valid until its next decode or spans call
    uint32_t *byte_start = nullptr, *char_start = nullptr;
    uint64_t *byte_off = nullptr, *char_off = nullptr;
    uint64_t n_bytes = 0, n_chars = 0;
    uint64_t bad_doc = ~0ull;  // the first document that is not well-formed UTF-8 (when asked for)
    DecodeView dec;            // the lengths and the workgroups' byte bases, where tk_k_dec_copy reads them
};
// The span passes in their parts; the caller holds c->mu.  spans_begin: the buffers of a batch of n tokens in n_docs documents, the report
// words, the document starts over the tokens.  spans_range: the three passes over the tokens [a, a + cnt) (a: a multiple of TK_DEC_BLOCK;
// ranges in order, the last one ends at n).  spans_end: the per-document pass, then the host waits and looks at the report words.
static int spans_begin(tk_core* c, hipStream_t s, uint64_t n, const uint64_t* d_tok_off, uint64_t n_docs, SpanView* out, unsigned long long** words_out) {
    TRY(decode_table_check(c));
    const uint64_t nb = n / TK_DEC_BLOCK + 1;  // (workgroups over the positions 0 .. n)
    TRY(decode_view(c, n, 0, false, false, 0, &out->dec));
    TRY(ensure(c->d_span, (n + 1) * 8));
    TRY(ensure(c->d_span_blk, nb * 8 * 4));
    TRY(ensure(c->d_span_marks, (n / 32 + 4) * 4));
    TRY(ensure(c->d_span_doc, ((n_docs + 1) * 2 + TK_SPAN_WORDS) * 8));
    out->byte_start = c->d_span.as<uint32_t>();
    out->char_start = out->byte_start + n + 1;
    out->byte_off = c->d_span_doc.as<uint64_t>();
    out->char_off = out->byte_off + n_docs + 1;
    unsigned long long* words = (unsigned long long*)(out->char_off + n_docs + 1);
    const unsigned long long h_words[TK_SPAN_WORDS] = {~0ull, ~0ull, ~0ull, ~0ull, 0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(words, h_words, sizeof h_words, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(c->d_span_marks.p, 0, (n / 32 + 4) * 4, s));
    TRY(timed(c, s, "tk_k_span_mark", [&] {
        hipLaunchKernelGGL(tk_k_span_mark, dim3(grid_for(n_docs + 1, 256, 4096)), dim3(256), 0, s, d_tok_off, n_docs + 1, n, c->d_span_marks.as<uint32_t>());
    }));
    *words_out = words;
    return TK_OK;
}
static int spans_range(tk_core* c, hipStream_t s, const uint32_t* d_tok, uint64_t n, uint64_t a, uint64_t cnt, const uint64_t* d_tok_off, uint64_t n_docs,
                       const SpanView* v, unsigned long long* words) {
    const uint32_t end = a + cnt == n ? 1u : 0u;
    const uint64_t nb_all = n / TK_DEC_BLOCK + 1, b0 = a / TK_DEC_BLOCK, nb = (cnt + end + TK_DEC_BLOCK - 1) / TK_DEC_BLOCK;
    unsigned long long* bsum = v->dec.bsum + b0;
    unsigned long long *csum = c->d_span_blk.as<unsigned long long>() + b0, *mkey = csum + nb_all, *doc_b = mkey + nb_all, *doc_c = doc_b + nb_all;
    uint32_t* lens = v->dec.lens + a;
    const uint8_t* marks = c->d_span_marks.as<uint8_t>() + a / 8;
    const uint32_t* cw = c->t_cw.as<uint32_t>();
    if (nb)
        TRY(timed(c, s, "tk_k_span_len", [&] {
            hipLaunchKernelGGL(tk_k_span_len, dim3((uint32_t)nb), dim3(256), 0, s, d_tok + a, cnt, end, a, c->t_dec.as<uint2>(), cw, c->n_dec, marks, lens, bsum, csum, mkey, words);
        }));
    TRY(timed(c, s, "tk_k_span_scan", [&] { hipLaunchKernelGGL(tk_k_span_scan, dim3(1), dim3(1024), 0, s, bsum, csum, mkey, nb, doc_b, doc_c, words); }));
    if (nb)
        TRY(timed(c, s, "tk_k_span_write", [&] {
            hipLaunchKernelGGL(tk_k_span_write, dim3((uint32_t)nb), dim3(256), 0, s, d_tok + a, cnt, end, a, cw, c->n_dec, lens, marks, d_tok_off, n_docs, bsum, csum, doc_b, doc_c,
                               v->byte_start + a, v->char_start + a, v->byte_off, v->char_off);
        }));
    return TK_OK;
}
static int spans_end(tk_core* c, hipStream_t s, const uint32_t* d_tok, const uint64_t* d_tok_off, uint64_t n_docs, const uint64_t* d_doc_off, SpanView* out,
                     unsigned long long* words) {
    TRY(timed(c, s, "tk_k_span_docs", [&] {
        hipLaunchKernelGGL(tk_k_span_docs, dim3(grid_for(n_docs + 1, 256, 4096)), dim3(256), 0, s, d_tok_off, out->byte_off, out->char_off, d_doc_off, n_docs, words);
    }));
    unsigned long long h_words[TK_SPAN_WORDS];
    HIPCHK(hipMemcpyAsync(h_words, words, sizeof h_words, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    if (h_words[TK_SPAN_BAD_TOKEN] != ~0ull) return invalid_token(d_tok, h_words[TK_SPAN_BAD_TOKEN], true);  // (reported as tk_k_dec_len's: the first id without an entry)
    if (h_words[TK_SPAN_BIG_DOC] != ~0ull)
        return fail(TK_VALUE_ERROR, "document " + std::to_string(h_words[TK_SPAN_BIG_DOC]) + " decodes to 4 GiB or more: token spans are 32-bit offsets into a document");
    if (h_words[TK_SPAN_GAP_DOC] != ~0ull)
        return fail(TK_UNSUPPORTED, "document " + std::to_string(h_words[TK_SPAN_GAP_DOC]) +
                                        ": its tokens do not add up to its text -- the pat_str leaves characters unmatched (they yield no token); token spans "
                                        "across such gaps are not supported");
    out->n_bytes = h_words[TK_SPAN_BYTES];
    out->n_chars = h_words[TK_SPAN_CHARS];
    return TK_OK;
}
// the strict UTF-8 check over the batch's bytes in c->d_bytes (queued; out->bad_doc is there once the stream has been waited for)
static int spans_validate(tk_core* c, hipStream_t s, uint64_t n_docs, SpanView* out, unsigned long long* words) {
    const uint64_t nbytes = out->n_bytes;
    if (!nbytes) return TK_OK;
    TRY(ensure(c->d_span_bmarks, (nbytes / 32 + 4) * 4));
    HIPCHK(hipMemsetAsync(c->d_span_bmarks.p, 0, (nbytes / 32 + 4) * 4, s));
    TRY(timed(c, s, "tk_k_span_mark", [&] {
        hipLaunchKernelGGL(tk_k_span_mark, dim3(grid_for(n_docs + 1, 256, 4096)), dim3(256), 0, s, out->byte_off, n_docs + 1, nbytes, c->d_span_bmarks.as<uint32_t>());
    }));
    const uint64_t lanes = (nbytes + 15) / 16;
    TRY(timed(c, s, "tk_k_utf8_docs", [&] {
        hipLaunchKernelGGL(tk_k_utf8_docs, dim3((uint32_t)((lanes + 255) / 256)), dim3(256), 0, s, c->d_bytes.as<uint8_t>(), nbytes, c->d_span_bmarks.as<uint32_t>(), out->byte_off,
                           n_docs, words);
    }));
    HIPCHK(hipMemcpyAsync(&out->bad_doc, words + TK_SPAN_BAD_UTF8, 8, hipMemcpyDeviceToHost, s));
    return TK_OK;
}
// A whole batch that is on the device.  d_doc_off (may be null): the offsets of the documents' text -- the tokens of every document must
// add up to its length.  want_bytes: the decoded bytes in c->d_bytes as well; validate: ... and checked (they are decoded for that in any case).
static int spans_run(tk_core* c, hipStream_t s, const uint32_t* d_tok, uint64_t n, const uint64_t* d_tok_off, uint64_t n_docs, const uint64_t* d_doc_off,
                     bool want_bytes, bool validate, SpanView* out) {
    unsigned long long* words = nullptr;
    TRY(spans_begin(c, s, n, d_tok_off, n_docs, out, &words));
    TRY(spans_range(c, s, d_tok, n, 0, n, d_tok_off, n_docs, out, words));
    TRY(spans_end(c, s, d_tok, d_tok_off, n_docs, d_doc_off, out, words));
    if (want_bytes || validate) {
        TRY(ensure(c->d_bytes, out->n_bytes + 16));
        if (n) TRY(decode_range_copy(c, s, out->dec, d_tok, 0, n, c->d_bytes.as<uint8_t>(), 0));
        if (validate) TRY(spans_validate(c, s, n_docs, out, words));
        HIPCHK(hipStreamSynchronize(s));
        HIPCHK(hipGetLastError());
    }
    return TK_OK;
}

extern "C" int tk_token_spans_device(tk_core* c, const void* d_tokens, uint64_t n_tokens, const void* d_tok_off, uint64_t n_docs, const void* d_doc_off, void* stream,
                                     const uint32_t** d_byte_start_out, const uint32_t** d_char_start_out, const uint64_t** d_byte_off_out,
                                     const uint64_t** d_char_off_out) {
    SpanView v;
    TRY(device_pass(c, d_tok_off && (d_tokens || !n_tokens), stream, [&](hipStream_t s) {
        return spans_run(c, s, (const uint32_t*)d_tokens, n_tokens, (const uint64_t*)d_tok_off, n_docs, (const uint64_t*)d_doc_off, false, false, &v);
    }));
    if (d_byte_start_out) *d_byte_start_out = v.byte_start;
    if (d_char_start_out) *d_char_start_out = v.char_start;
    if (d_byte_off_out) *d_byte_off_out = v.byte_off;
    if (d_char_off_out) *d_char_off_out = v.char_off;
    return TK_OK;
}

// Host buffers in and out.  A batch of less than two ranges of 16 Mi ids takes one copy each way.  A larger one runs in those ranges
// (ranged_ids_pass; the ids straight from the caller's buffer): the spans of a range travel back while the next one is scanned; the scan's
// carry (sums and last document start) stays on the device between the ranges.  Then the bytes, range by range: the copy kernel of range k + 1
// runs while the bytes of range k travel (by then the byte count is known: the result buffer has its size at once), and the UTF-8 check behind them.
static int decode_spans_ranges(tk_core* c, hipStream_t s, const uint32_t* tokens, uint64_t n, const uint64_t* d_tok_off, uint64_t n_docs, bool want_bytes, bool validate,
                               SpanView* v, HostResult<uint32_t>& bs, HostResult<uint32_t>& cs, HostResult<uint8_t>& host) {
    const uint64_t n_ranges = id_ranges(n);
    const uint32_t* d_tok = c->d_tok.as<uint32_t>();
    std::vector<Event> ev_out(n_ranges), ev_bytes(want_bytes ? n_ranges : 0);  // the spans of a range are there; so are its bytes
    for (auto& e : ev_out) HIPCHK(e.create());
    for (auto& e : ev_bytes) HIPCHK(e.create());
    bs = HostResult<uint32_t>(pinned_get(n * 4));
    cs = HostResult<uint32_t>(pinned_get(n * 4));
    Pinned<unsigned long long> cum;  // bytes of the batch up to the end of every range
    HIPCHK(cum.alloc((n_ranges + 1) * 8, hipHostMallocPortable));
    if (!bs || !cs) return fail(TK_RUNTIME_ERROR, "out of page-locked host memory");
    unsigned long long* words = nullptr;
    TRY(spans_begin(c, s, n, d_tok_off, n_docs, v, &words));
    auto step = [&](uint64_t k, uint64_t a, uint64_t cnt) -> int {
        TRY(spans_range(c, s, d_tok, n, a, cnt, d_tok_off, n_docs, v, words));
        HIPCHK(hipMemcpyAsync(cum + k + 1, words + TK_SPAN_BYTES, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(hipEventRecord(ev_out[k], s));
        HIPCHK(hipStreamWaitEvent(c->cs_d2h, ev_out[k], 0));
        HIPCHK(hipMemcpyAsync(bs + a, v->byte_start + a, cnt * 4, hipMemcpyDeviceToHost, c->cs_d2h));
        HIPCHK(hipMemcpyAsync(cs + a, v->char_start + a, cnt * 4, hipMemcpyDeviceToHost, c->cs_d2h));
        return TK_OK;
    };
    auto bytes_by_range = [&]() -> int {
        TRY(spans_end(c, s, d_tok, d_tok_off, n_docs, nullptr, v, words));
        if (!want_bytes && !validate) return TK_OK;
        cum[0] = 0;
        TRY(ensure(c->d_bytes, v->n_bytes + 16));
        if (want_bytes) {
            host = HostResult<uint8_t>(pinned_get(v->n_bytes));
            if (!host) return fail(TK_RUNTIME_ERROR, "out of page-locked host memory");
        }
        for (uint64_t k = 0; k < n_ranges; ++k) {
            const uint64_t a = k * ID_RANGE;
            TRY(decode_range_copy(c, s, v->dec, d_tok, a, std::min(ID_RANGE, n - a), c->d_bytes.as<uint8_t>(), 0));  // (the bases are the batch's: every range writes at its place)
            if (!want_bytes) continue;
            HIPCHK(hipEventRecord(ev_bytes[k], s));
            HIPCHK(hipStreamWaitEvent(c->cs_d2h, ev_bytes[k], 0));
            if (cum[k + 1] > cum[k]) HIPCHK(hipMemcpyAsync(host + cum[k], c->d_bytes.as<uint8_t>() + cum[k], cum[k + 1] - cum[k], hipMemcpyDeviceToHost, c->cs_d2h));
        }
        if (validate) TRY(spans_validate(c, s, n_docs, v, words));
        return TK_OK;
    };
    return ranged_ids_pass(c, s, tokens, n, /* staged */ false, step, bytes_by_range);
}

extern "C" int tk_decode_batch_spans(tk_core* c, const uint32_t* tokens, const uint64_t* tok_off, uint64_t n_docs, int validate, uint8_t** bytes_out,
                                     uint64_t* n_bytes_out, uint32_t** byte_start_out, uint32_t** char_start_out, uint64_t* byte_off_out, uint64_t* char_off_out,
                                     uint64_t* invalid_doc_out) {
    if (!c) return fail(TK_VALUE_ERROR, "core is null");
    if (!tok_off || !byte_start_out || !char_start_out || (validate && !invalid_doc_out)) return fail(TK_VALUE_ERROR, "null argument");
    TRY(check_offsets(tok_off, n_docs, "tok_off"));
    TRY(decode_table_check(c));
    const uint64_t n = tok_off[n_docs];
    if (n && !tokens) return fail(TK_VALUE_ERROR, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    SpanView v;
    TRY(ensure(c->d_tok, (n + 1) * 4));
    TRY(decode_view(c, n, 0, false, true, n_docs, &v.dec));
    uint64_t* const d_tok_off = v.dec.tok_off;  // (spans_begin makes the view again, without the documents' arrays)
    HIPCHK(hipMemcpyAsync(d_tok_off, tok_off, (n_docs + 1) * 8, hipMemcpyHostToDevice, s));
    HostResult<uint32_t> bs, cs;
    HostResult<uint8_t> host;
    if (n >= 2 * ID_RANGE) {
        TRY(drained(c, [&] { return decode_spans_ranges(c, s, tokens, n, d_tok_off, n_docs, bytes_out != nullptr, validate != 0, &v, bs, cs, host); }));
    } else {
        if (n) HIPCHK(hipMemcpyAsync(c->d_tok.p, tokens, n * 4, hipMemcpyHostToDevice, s));
        TRY(drained(c, [&] { return spans_run(c, s, c->d_tok.as<uint32_t>(), n, d_tok_off, n_docs, nullptr, bytes_out != nullptr, validate != 0, &v); }));
        TRY(result_from_device(bs, v.byte_start, n));
        TRY(result_from_device(cs, v.char_start, n));
        if (bytes_out) TRY(result_from_device(host, c->d_bytes.p, v.n_bytes));
    }
    if (byte_off_out) HIPCHK(hipMemcpy(byte_off_out, v.byte_off, (n_docs + 1) * 8, hipMemcpyDeviceToHost));
    if (char_off_out) HIPCHK(hipMemcpy(char_off_out, v.char_off, (n_docs + 1) * 8, hipMemcpyDeviceToHost));
    if (invalid_doc_out) *invalid_doc_out = v.bad_doc;
    if (n_bytes_out) *n_bytes_out = v.n_bytes;
    if (bytes_out) *bytes_out = host.release();
    *byte_start_out = bs.release();
    *char_start_out = cs.release();
    return TK_OK;
}

// tk_encode_batch (tk_encode_batch_checked with disallowed ids) with the spans of the tokens it has just produced: the span pass runs over
// the ids while they are still on the device, against the offsets of the documents' text.
extern "C" int tk_encode_batch_spans(tk_core* c, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, int use_special, const uint32_t* allowed_ids,
                                     uint64_t n_allowed, const uint32_t* disallowed_ids, uint64_t n_disallowed, uint32_t** tokens_out, uint64_t* n_tokens_out,
                                     uint64_t* tok_off_out, uint32_t** byte_start_out, uint32_t** char_start_out, tk_special_hit* hit) {
    SpanView v;
    return encode_batch_pass(
        c, utf8, doc_off, n_docs, use_special, allowed_ids, n_allowed, disallowed_ids, n_disallowed, hit, tokens_out && n_tokens_out && byte_start_out && char_start_out,
        [] { return TK_OK; },
        [&](uint64_t n) { return spans_run(c, c->stream, c->out_tokens.as<uint32_t>(), n, c->out_tok_off.as<uint64_t>(), n_docs, c->doc_off.as<uint64_t>(), false, false, &v); },
        [&](uint64_t n) -> int {
            ResultBag bag;
            TRY(bag.fetch(tokens_out, c->out_tokens.p, n));
            TRY(bag.fetch(byte_start_out, v.byte_start, n));
            TRY(bag.fetch(char_start_out, v.char_start, n));
            if (tok_off_out) HIPCHK(hipMemcpy(tok_off_out, c->out_tok_off.p, (n_docs + 1) * 8, hipMemcpyDeviceToHost));
            bag.give();
            *n_tokens_out = n;
            return TK_OK;
        });
}

// ------------------------------------------------------------------------------------------
// Training rows (tk_rows.h): a packed batch on the device -> rows of seq_len with document ids, positions and segment boundaries.
// ------------------------------------------------------------------------------------------
struct RowsView {  // device buffers of the core, valid until its next rows call
    void* ids = nullptr;
    uint32_t *doc = nullptr, *pos = nullptr, *cu = nullptr, *row_seg = nullptr;
    uint64_t n_rows = 0, n_segs = 0, n_stream = 0, n_tail = 0, n_pos = 0;  // n_pos: positions written (M)
    bool ids16 = false;
};
// 16-bit ids (TK_ROWS_IDS16, TK_PAD_IDS16): every id of the vocabulary, the special tokens, bos_id, eos_id and pad_id must fit
static int ids16_check(tk_core* c, uint32_t bos_id, uint32_t eos_id, uint32_t pad_id) {
    uint32_t max_id = c->H.max_rank;
    for (const auto& kv : c->H.spec_decoder) max_id = std::max(max_id, kv.first);
    if (max_id > 0xFFFFu) return fail(TK_VALUE_ERROR, "16-bit ids: the vocabulary has ids up to " + std::to_string(max_id));
    const uint32_t extra[3] = {bos_id, eos_id, pad_id};
    const char* names[3] = {"bos_id", "eos_id", "pad_id"};
    for (int i = 0; i < 3; ++i)
        if (extra[i] > 0xFFFFu && (i == 2 || extra[i] != TK_ROWS_NO_TOKEN)) return fail(TK_VALUE_ERROR, std::string("16-bit ids: ") + names[i] + " does not fit");
    return TK_OK;
}
// The report words of the row and the padded passes (device memory); word TK_BAD_OFF is what the check of the caller's tok_off found.
// Before the passes: all ones = no entry offends (the other words are the passes' to write, or the caller's to clear)
static int report_arm(unsigned long long* words, hipStream_t s) {
    HIPCHK(hipMemsetAsync(words + TK_BAD_OFF, 0xFF, 8, s));
    return TK_OK;
}
// TK_OK, or the refusal of an offsets array that does not describe the batch (`word`: its report word, a tk_rows_bad_key): the first
// offending entry and what is wrong with it.  ("tok_off", "document", "n_tokens") and ("sample_off", "sample", "n_parts").
static int offsets_refusal(unsigned long long word, const char* array, const char* entry, const char* count) {
    if (word == ~0ull) return TK_OK;
    const std::string a = array, e = std::string(entry) + " " + std::to_string(word >> 2);
    switch (word & 3u) {
        case 1: return fail(TK_VALUE_ERROR, a + "[0] must be 0 (" + e + ")");
        case 2: return fail(TK_VALUE_ERROR, a + " must be non-decreasing: " + e + " ends before it starts");
        default: return fail(TK_VALUE_ERROR, a + " must end at " + count + ": " + e + " ends elsewhere");
    }
}
// Behind the passes: the stream is waited for, the n words come over (synchronous: nothing is on its way into `got` when this returns,
// however it returns), and an offending tok_off is refused
static int report_read(const unsigned long long* words, unsigned long long* got, size_t n, hipStream_t s) {
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(got, words, n * 8, hipMemcpyDeviceToHost));
    return offsets_refusal(got[TK_BAD_OFF], "tok_off", "document", "n_tokens");
}
// What of a tk_rows_spec can be refused without looking at the batch (the host-text entry asks before it encodes anything).
static int rows_check_spec(tk_core* c, const tk_rows_spec* spec) {
    if (!spec) return fail(TK_VALUE_ERROR, "null argument");
    if (spec->flags & ~(TK_ROWS_DROP_LAST | TK_ROWS_IDS16)) return fail(TK_VALUE_ERROR, "tk_rows_spec: unknown flag");
    if (!spec->seq_len) return fail(TK_VALUE_ERROR, "seq_len must be at least 1");
    if (spec->flags & TK_ROWS_IDS16) TRY(ids16_check(c, spec->bos_id, spec->eos_id, spec->pad_id));
    return TK_OK;
}
// rows_run: the caller holds c->mu.  Everything but the number of segments follows from the arguments; the host waits once, at the end, for
// that number and for what tk_k_rows_mark has to say about tok_off.
static int rows_run(tk_core* c, hipStream_t s, const uint32_t* d_tok, uint64_t n, const uint64_t* d_tok_off, uint64_t n_docs, const tk_rows_spec* spec, RowsView* out) {
    TRY(rows_check_spec(c, spec));
    TkRows r;
    switch (tk_rows_shape(n, n_docs, spec->seq_len, spec->bos_id, spec->eos_id, spec->pad_id, (spec->flags & TK_ROWS_DROP_LAST) != 0, &r)) {
        case 0: break;
        case 1: return fail(TK_VALUE_ERROR, "seq_len must be at least 1");
        case 3: return fail(TK_VALUE_ERROR, "too many documents: the document indices of the rows are 32-bit");
        default: return fail(TK_VALUE_ERROR, "the stream has 2^32 positions or more: the positions of the rows are 32-bit");
    }
    const bool ids16 = (spec->flags & TK_ROWS_IDS16) != 0;
    const uint64_t m8 = (r.M + 7) & ~7ull, nb = (r.M + TK_DEC_BLOCK - 1) / TK_DEC_BLOCK;  // (m8: room for whole lanes of eight)
    Carve rows, seg;
    const uint64_t at_ids = rows.add(m8 * (ids16 ? 2 : 4)), at_doc = rows.add(m8 * 4), at_pos = rows.add(m8 * 4);
    const uint64_t at_words = seg.add(TK_ROWS_WORDS * 8), at_cu = seg.add((n_docs + r.R + 4) * 4), at_rs = seg.add((r.R + 1) * 4);
    TRY(ensure(c->d_rows, rows.total + 64));
    TRY(ensure(c->d_rows_seg, seg.total));
    TRY(ensure(c->d_rows_marks, (r.M / 32 + 4) * 4));
    TRY(ensure(c->d_rows_blk, (nb + 1) * 8));
    out->ids = carved<void>(c->d_rows, at_ids);
    out->doc = carved<uint32_t>(c->d_rows, at_doc);
    out->pos = carved<uint32_t>(c->d_rows, at_pos);
    unsigned long long* words = carved<unsigned long long>(c->d_rows_seg, at_words);
    out->cu = carved<uint32_t>(c->d_rows_seg, at_cu);
    out->row_seg = carved<uint32_t>(c->d_rows_seg, at_rs);
    out->ids16 = ids16;
    out->n_rows = r.R;
    out->n_stream = r.S;
    out->n_pos = r.M;
    out->n_tail = (spec->flags & TK_ROWS_DROP_LAST) ? r.S - r.R * r.seq_len : 0;
    unsigned long long* cnt = c->d_rows_blk.as<unsigned long long>();
    TRY(report_arm(words, s));  // (tk_k_rows_scan writes the other word)
    HIPCHK(hipMemsetAsync(c->d_rows_marks.p, 0, (r.M / 32 + 4) * 4, s));
    TRY(timed(c, s, "tk_k_rows_mark", [&] {
        hipLaunchKernelGGL(tk_k_rows_mark, dim3(grid_for(n_docs + 1, 256, 4096)), dim3(256), 0, s, d_tok_off, r, c->d_rows_marks.as<uint32_t>(), words);
    }));
    if (nb)
        TRY(timed(c, s, "tk_k_rows_count", [&] { hipLaunchKernelGGL(tk_k_rows_count, dim3((uint32_t)nb), dim3(256), 0, s, c->d_rows_marks.as<uint8_t>(), r, cnt); }));
    TRY(timed(c, s, "tk_k_rows_scan", [&] { hipLaunchKernelGGL(tk_k_rows_scan, dim3(1), dim3(1024), 0, s, cnt, nb, r, out->cu, out->row_seg, words); }));
    if (nb)
        TRY(timed(c, s, "tk_k_rows_write", [&] {
            if (ids16) hipLaunchKernelGGL(tk_k_rows_write<true>, dim3((uint32_t)nb), dim3(256), 0, s, d_tok, d_tok_off, r, cnt, words, out->ids, out->doc, out->pos, out->cu, out->row_seg);
            else hipLaunchKernelGGL(tk_k_rows_write<false>, dim3((uint32_t)nb), dim3(256), 0, s, d_tok, d_tok_off, r, cnt, words, out->ids, out->doc, out->pos, out->cu, out->row_seg);
        }));
    unsigned long long got[TK_ROWS_WORDS];
    TRY(report_read(words, got, TK_ROWS_WORDS, s));
    out->n_segs = got[TK_ROWS_NSEGS];
    return TK_OK;
}

extern "C" int tk_pack_rows_device(tk_core* c, const void* d_tokens, uint64_t n_tokens, const void* d_tok_off, uint64_t n_docs, const tk_rows_spec* spec, void* stream,
                                   const void** d_ids_out, const uint32_t** d_doc_out, const uint32_t** d_pos_out, const uint32_t** d_cu_seqlens_out,
                                   const uint32_t** d_row_seg_out, uint64_t* n_rows_out, uint64_t* n_segs_out, uint64_t* n_stream_out, uint64_t* n_tail_out) {
    RowsView v;
    TRY(device_pass(c, d_tok_off && (d_tokens || !n_tokens) && spec, stream,
                    [&](hipStream_t s) { return rows_run(c, s, (const uint32_t*)d_tokens, n_tokens, (const uint64_t*)d_tok_off, n_docs, spec, &v); }));
    if (d_ids_out) *d_ids_out = v.ids;
    if (d_doc_out) *d_doc_out = v.doc;
    if (d_pos_out) *d_pos_out = v.pos;
    if (d_cu_seqlens_out) *d_cu_seqlens_out = v.cu;
    if (d_row_seg_out) *d_row_seg_out = v.row_seg;
    if (n_rows_out) *n_rows_out = v.n_rows;
    if (n_segs_out) *n_segs_out = v.n_segs;
    if (n_stream_out) *n_stream_out = v.n_stream;
    if (n_tail_out) *n_tail_out = v.n_tail;
    return TK_OK;
}

// tk_encode_batch (tk_encode_batch_checked with disallowed ids) with the rows of the tokens it has just produced: the row passes run over
// the ids while they are still on the device, and only the row arrays travel back.
extern "C" int tk_encode_batch_rows(tk_core* c, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, int use_special, const uint32_t* allowed_ids,
                                    uint64_t n_allowed, const uint32_t* disallowed_ids, uint64_t n_disallowed, const tk_rows_spec* spec, void** ids_out,
                                    uint32_t** doc_out, uint32_t** pos_out, uint32_t** cu_seqlens_out, uint32_t** row_seg_out, uint64_t* n_rows_out,
                                    uint64_t* n_segs_out, uint64_t* n_stream_out, uint64_t* n_tail_out, tk_special_hit* hit) {
    RowsView v;
    return encode_batch_pass(
        c, utf8, doc_off, n_docs, use_special, allowed_ids, n_allowed, disallowed_ids, n_disallowed, hit,
        spec && ids_out && doc_out && pos_out && cu_seqlens_out && row_seg_out && n_rows_out && n_segs_out,
        [&] { return rows_check_spec(c, spec); },  // (before the encode, not after it)
        [&](uint64_t n) { return rows_run(c, c->stream, c->out_tokens.as<uint32_t>(), n, c->out_tok_off.as<uint64_t>(), n_docs, spec, &v); },
        [&](uint64_t) -> int {
            ResultBag bag;
            TRY(bag.fetch((uint8_t**)ids_out, v.ids, v.n_pos * (v.ids16 ? 2 : 4)));
            TRY(bag.fetch(doc_out, v.doc, v.n_pos));
            TRY(bag.fetch(pos_out, v.pos, v.n_pos));
            TRY(bag.fetch(cu_seqlens_out, v.cu, v.n_segs + 1));
            TRY(bag.fetch(row_seg_out, v.row_seg, v.n_rows + 1));
            bag.give();
            *n_rows_out = v.n_rows;
            *n_segs_out = v.n_segs;
            if (n_stream_out) *n_stream_out = v.n_stream;
            if (n_tail_out) *n_tail_out = v.n_tail;
            return TK_OK;
        });
}

// ------------------------------------------------------------------------------------------
// Padded model inputs (tk_padded.h): a packed batch on the device -> one row per document or overlapping windows, ids and mask as [R, W].
// ------------------------------------------------------------------------------------------
static_assert(TK_PAD_WINDOWS == TK_PADF_WINDOWS && TK_PAD_KEEP_TAIL == TK_PADF_KEEP_TAIL && TK_PAD_LEFT == TK_PADF_LEFT && TK_PAD_IDS16 == TK_PADF_IDS16, "tk_pad_spec flags");
struct PadView {  // device buffers of the core, valid until its next padded call
    void* ids = nullptr;
    uint8_t* mask = nullptr;
    uint32_t *len = nullptr, *row_doc = nullptr, *row_tok = nullptr, *doc_row = nullptr;
    uint64_t n_rows = 0, width = 0;
    bool ids16 = false;
};
static int pad_refusal(int why) {
    switch (why) {
        case 0: return TK_OK;
        case 1: return fail(TK_VALUE_ERROR, "max_len must be at least 1 and leave room for a body token beside bos_id / eos_id");
        case 2: return fail(TK_VALUE_ERROR, "stride must be less than max_len minus the bos / eos elements");
        case 3: return fail(TK_VALUE_ERROR, "stride without TK_PAD_WINDOWS");
        case 4: return fail(TK_VALUE_ERROR, "TK_PAD_KEEP_TAIL together with TK_PAD_WINDOWS");
        case 5: return fail(TK_VALUE_ERROR, "too many documents: the document indices of the rows are 32-bit");
        case 6: return fail(TK_VALUE_ERROR, "2^32 tokens or more: the token indices of the rows are 32-bit");
        case 7: return fail(TK_VALUE_ERROR, "2^32 rows or more: the row indices are 32-bit");
        default: return fail(TK_VALUE_ERROR, "rows times width reaches 2^32: the positions are 32-bit");
    }
}
// What of a tk_pad_spec can be refused without looking at the batch (the host-text entry asks before it encodes anything).
static int pad_check_spec(tk_core* c, const tk_pad_spec* spec) {
    if (!spec) return fail(TK_VALUE_ERROR, "null argument");
    if (spec->flags & ~(TK_PAD_WINDOWS | TK_PAD_KEEP_TAIL | TK_PAD_LEFT | TK_PAD_IDS16)) return fail(TK_VALUE_ERROR, "tk_pad_spec: unknown flag");
    TkPad p;
    TRY(pad_refusal(tk_pad_shape(0, 0, spec->max_len, spec->stride, spec->width_multiple, spec->bos_id, spec->eos_id, spec->pad_id, spec->flags, &p)));
    if (spec->flags & TK_PAD_IDS16) TRY(ids16_check(c, spec->bos_id, spec->eos_id, spec->pad_id));
    return TK_OK;
}
// pad_run: the caller holds c->mu.  The host waits twice: for R, the longest row and what tk_k_pad_count has to say about tok_off -- W and
// the sizes of the outputs follow from them --, and at the end.  A call that is refused has written into d_pad_cnt only: the previous
// result, doc_row included, stays whole.
static int pad_run(tk_core* c, hipStream_t s, const uint32_t* d_tok, uint64_t n, const uint64_t* d_tok_off, uint64_t n_docs, const tk_pad_spec* spec, PadView* out) {
    TRY(pad_check_spec(c, spec));
    TkPad p;
    TRY(pad_refusal(tk_pad_shape(n, n_docs, spec->max_len, spec->stride, spec->width_multiple, spec->bos_id, spec->eos_id, spec->pad_id, spec->flags, &p)));
    Carve cnt;
    const uint64_t at_words = cnt.add(TK_PAD_WORDS * 8), at_counted = cnt.add((n_docs + 1) * 4);
    TRY(ensure(c->d_pad_cnt, cnt.total));
    unsigned long long* words = carved<unsigned long long>(c->d_pad_cnt, at_words);
    uint32_t* counted = carved<uint32_t>(c->d_pad_cnt, at_counted);  // (the result's doc_row is written once the call is accepted)
    TRY(report_arm(words, s));  // (tk_k_pad_scan writes the second word)
    HIPCHK(hipMemsetAsync(words + TK_PAD_LONGEST, 0, 8, s));
    TRY(timed(c, s, "tk_k_pad_count", [&] { hipLaunchKernelGGL(tk_k_pad_count, dim3(grid_for(n_docs + 1, 256, 4096)), dim3(256), 0, s, d_tok_off, p, counted, words); }));
    TRY(timed(c, s, "tk_k_pad_scan", [&] { hipLaunchKernelGGL(tk_k_pad_scan, dim3(1), dim3(1024), 0, s, counted, n_docs, words); }));
    unsigned long long got[TK_PAD_WORDS];
    TRY(report_read(words, got, TK_PAD_WORDS, s));
    TRY(pad_refusal(tk_pad_size(&p, got[TK_PAD_NROWS], (uint32_t)got[TK_PAD_LONGEST])));
    const bool ids16 = (spec->flags & TK_PAD_IDS16) != 0;
    const uint64_t N = p.R * p.W, n8 = (N + 7) & ~7ull, nb = (N + TK_DEC_BLOCK - 1) / TK_DEC_BLOCK;  // (n8: room for whole lanes of eight)
    Carve pos, row;
    const uint64_t at_ids = pos.add(n8 * (ids16 ? 2 : 4)), at_mask = pos.add(n8);
    const uint64_t at_len = row.add(p.R * 4), at_rd = row.add(p.R * 4), at_rt = row.add(p.R * 4);
    TRY(ensure(c->d_pad, pos.total));
    TRY(ensure(c->d_pad_row, row.total));
    TRY(ensure(c->d_pad_doc, (n_docs + 1) * 4));
    uint32_t* doc_row = c->d_pad_doc.as<uint32_t>();
    HIPCHK(hipMemcpyAsync(doc_row, counted, (n_docs + 1) * 4, hipMemcpyDeviceToDevice, s));
    out->ids = carved<void>(c->d_pad, at_ids);
    out->mask = carved<uint8_t>(c->d_pad, at_mask);
    out->len = carved<uint32_t>(c->d_pad_row, at_len);
    out->row_doc = carved<uint32_t>(c->d_pad_row, at_rd);
    out->row_tok = carved<uint32_t>(c->d_pad_row, at_rt);
    out->doc_row = doc_row;
    out->n_rows = p.R;
    out->width = p.W;
    out->ids16 = ids16;
    if (p.R)
        TRY(timed(c, s, "tk_k_pad_rows", [&] {
            hipLaunchKernelGGL(tk_k_pad_rows, dim3(grid_for(p.R, 256, 4096)), dim3(256), 0, s, d_tok_off, doc_row, p, out->len, out->row_doc, out->row_tok);
        }));
    if (nb)
        TRY(timed(c, s, "tk_k_pad_write", [&] {
            if (ids16) hipLaunchKernelGGL(tk_k_pad_write<true>, dim3((uint32_t)nb), dim3(256), 0, s, d_tok, d_tok_off, doc_row, p, out->ids, out->mask);
            else hipLaunchKernelGGL(tk_k_pad_write<false>, dim3((uint32_t)nb), dim3(256), 0, s, d_tok, d_tok_off, doc_row, p, out->ids, out->mask);
        }));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    return TK_OK;
}

extern "C" int tk_pad_batch_device(tk_core* c, const void* d_tokens, uint64_t n_tokens, const void* d_tok_off, uint64_t n_docs, const tk_pad_spec* spec, void* stream,
                                   const void** d_ids_out, const uint8_t** d_mask_out, const uint32_t** d_len_out, const uint32_t** d_row_doc_out,
                                   const uint32_t** d_row_tok_out, const uint32_t** d_doc_row_out, uint64_t* n_rows_out, uint64_t* width_out) {
    PadView v;
    TRY(device_pass(c, d_tok_off && (d_tokens || !n_tokens) && spec, stream,
                    [&](hipStream_t s) { return pad_run(c, s, (const uint32_t*)d_tokens, n_tokens, (const uint64_t*)d_tok_off, n_docs, spec, &v); }));
    if (d_ids_out) *d_ids_out = v.ids;
    if (d_mask_out) *d_mask_out = v.mask;
    if (d_len_out) *d_len_out = v.len;
    if (d_row_doc_out) *d_row_doc_out = v.row_doc;
    if (d_row_tok_out) *d_row_tok_out = v.row_tok;
    if (d_doc_row_out) *d_doc_row_out = v.doc_row;
    if (n_rows_out) *n_rows_out = v.n_rows;
    if (width_out) *width_out = v.width;
    return TK_OK;
}

// tk_encode_batch (tk_encode_batch_checked with disallowed ids) with the padded rows of the tokens it has just produced: the passes run
// over the ids while they are still on the device, and only the padded arrays travel back.
extern "C" int tk_encode_batch_padded(tk_core* c, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, int use_special, const uint32_t* allowed_ids,
                                      uint64_t n_allowed, const uint32_t* disallowed_ids, uint64_t n_disallowed, const tk_pad_spec* spec, void** ids_out,
                                      uint8_t** mask_out, uint32_t** len_out, uint32_t** row_doc_out, uint32_t** row_tok_out, uint32_t** doc_row_out,
                                      uint64_t* n_rows_out, uint64_t* width_out, tk_special_hit* hit) {
    PadView v;
    return encode_batch_pass(
        c, utf8, doc_off, n_docs, use_special, allowed_ids, n_allowed, disallowed_ids, n_disallowed, hit,
        spec && ids_out && mask_out && len_out && row_doc_out && row_tok_out && doc_row_out && n_rows_out && width_out,
        [&] { return pad_check_spec(c, spec); },  // (before the encode, not after it)
        [&](uint64_t n) { return pad_run(c, c->stream, c->out_tokens.as<uint32_t>(), n, c->out_tok_off.as<uint64_t>(), n_docs, spec, &v); },
        [&](uint64_t) -> int {
            const uint64_t N = v.n_rows * v.width;
            ResultBag bag;
            TRY(bag.fetch((uint8_t**)ids_out, v.ids, N * (v.ids16 ? 2 : 4)));
            TRY(bag.fetch(mask_out, v.mask, N));
            TRY(bag.fetch(len_out, v.len, v.n_rows));
            TRY(bag.fetch(row_doc_out, v.row_doc, v.n_rows));
            TRY(bag.fetch(row_tok_out, v.row_tok, v.n_rows));
            TRY(bag.fetch(doc_row_out, v.doc_row, n_docs + 1));
            bag.give();
            *n_rows_out = v.n_rows;
            *width_out = v.width;
            return TK_OK;
        });
}

// ------------------------------------------------------------------------------------------
// Text chunks (tk_split.h): a packed batch and its text on the device -> every document cut at separators under a token budget.
// ------------------------------------------------------------------------------------------
static_assert(TK_SPLIT_HARD == TK_SPLITC_HARD && TK_SPLIT_FORCED == TK_SPLITC_FORCED && TK_SPLIT_END == TK_SPLITC_END, "tk_split cut values");
static_assert(sizeof(tk_split_sep) == sizeof(TkSplitSep) && sizeof(tk_split_sep) == 34, "tk_split_sep layout");
struct SplitView {  // device buffers of the core, valid until its next split call that succeeds
    TkSplitOut out = {};
    uint32_t* doc_chunk = nullptr;
    uint64_t n_chunks = 0;
};
static int split_refusal(int why) {
    switch (why) {
        case 0: return TK_OK;
        case 1: return fail(TK_VALUE_ERROR, "min_tokens must be at least 1");
        case 2: return fail(TK_VALUE_ERROR, "max_tokens must be at least min_tokens + 3 (a char is at most four tokens of one byte)");
        case 3: return fail(TK_VALUE_ERROR, "overlap must be less than min_tokens");
        case 4: return fail(TK_VALUE_ERROR, "n_levels: at most 4 levels of separators");
        case 5: return fail(TK_VALUE_ERROR, "n_seps: at most 4 separators in a level");
        case 6: return fail(TK_VALUE_ERROR, "separators: a part (tail, head) is at most 16 bytes");
        case 7: return fail(TK_VALUE_ERROR, "separators: tail and head of a separator are both empty");
        case 8: return fail(TK_VALUE_ERROR, "seg_tokens must be 0 or a multiple of 64");
        case 9: return fail(TK_VALUE_ERROR, "n_tokens: 2^32 tokens or more: the token indices of the chunks are 32-bit");
        case 10: return fail(TK_VALUE_ERROR, "n_docs: too many documents: the document indices of the chunks are 32-bit");
        default: return fail(TK_VALUE_ERROR, "tk_split_spec: unknown flag");
    }
}
static int split_shape(const tk_split_spec* spec, uint64_t n, uint64_t n_docs, TkSplit* p) {
    return split_refusal(tk_split_shape(n, n_docs, spec->max_tokens, spec->min_tokens, spec->overlap, spec->n_levels, spec->n_seps, spec->sep, spec->seg_tokens, spec->flags, p));
}
// What of a tk_split_spec can be refused without looking at the batch (the host-text entry asks before it encodes anything).
static int split_check_spec(const tk_split_spec* spec) {
    if (!spec) return fail(TK_VALUE_ERROR, "null argument");
    TkSplit p;
    return split_shape(spec, 0, 0, &p);
}
// split_run: the caller holds c->mu.  The host waits for what tk_k_split_check has to say about tok_off (nothing is indexed with it before),
// inside the span passes, and once in the split passes proper: for C, before the outputs are sized.  A call that is refused has written
// into d_split_work (and the span buffers) only: the previous result stays whole.
static int split_run(tk_core* c, hipStream_t s, const uint32_t* d_tok, uint64_t n, const uint64_t* d_tok_off, uint64_t n_docs, const uint8_t* d_utf8,
                     const uint64_t* d_doc_off, const tk_split_spec* spec, SplitView* out) {
    TkSplit p;
    TRY(split_shape(spec, n, n_docs, &p));  // (spec is not null: device_pass's arguments, split_check_spec before the encode)
    const uint64_t n_blocks = (n + p.K - 1) / p.K, nb = (p.W + TK_SPLIT_CB_WORDS - 1) / TK_SPLIT_CB_WORDS;
    Carve work;
    const uint64_t at_words = work.add(TK_SPLIT_WORDS * 8), at_planes = work.add((p.L + 1) * p.W * 8), at_cut = work.add(p.W * 8), at_spec = work.add(p.W * 8);
    const uint64_t at_exit = work.add((n_blocks + 1) * 4), at_join = work.add((n_blocks + 1) * 4), at_cnt = work.add((nb + 1) * 4);
    TRY(ensure(c->d_split_work, work.total));
    unsigned long long* words = carved<unsigned long long>(c->d_split_work, at_words);
    unsigned long long *planes = carved<unsigned long long>(c->d_split_work, at_planes), *cut = carved<unsigned long long>(c->d_split_work, at_cut);
    unsigned long long* spec_plane = carved<unsigned long long>(c->d_split_work, at_spec);
    uint32_t *exit_at = carved<uint32_t>(c->d_split_work, at_exit), *join_at = carved<uint32_t>(c->d_split_work, at_join), *cnt = carved<uint32_t>(c->d_split_work, at_cnt);
    HIPCHK(hipMemsetAsync(words, 0, TK_SPLIT_WORDS * 8, s));
    TRY(report_arm(words, s));
    TRY(timed(c, s, "tk_k_split_check", [&] { hipLaunchKernelGGL(tk_k_split_check, dim3(grid_for(n_docs + 1, 256, 4096)), dim3(256), 0, s, d_tok_off, n_docs, n, words); }));
    unsigned long long got[TK_SPLIT_WORDS];
    TRY(report_read(words, got, TK_SPLIT_WORDS, s));
    SpanView v;
    TRY(spans_run(c, s, d_tok, n, d_tok_off, n_docs, d_doc_off, false, false, &v));
    // (cut and spec lie one behind the other, exit_at and join_at too: one memset each)
    HIPCHK(hipMemsetAsync(cut, 0, (at_exit - at_cut), s));
    HIPCHK(hipMemsetAsync(exit_at, 0xFF, (at_cnt - at_exit), s));
    TRY(timed(c, s, "tk_k_split_class", [&] {
        hipLaunchKernelGGL(tk_k_split_class, dim3((uint32_t)((p.W * 64 + 255) / 256)), dim3(256), 0, s, p, d_utf8, d_doc_off, d_tok_off, v.byte_start, planes);
    }));
    if (n_blocks)
        TRY(timed(c, s, "tk_k_split_walk", [&] {
            hipLaunchKernelGGL(tk_k_split_walk, dim3((uint32_t)((n_blocks + 3) / 4)), dim3(256), 0, s, p, planes, d_tok_off, n_blocks, cut, spec_plane, exit_at, words);
        }));
    if (n_blocks > 1)
        TRY(timed(c, s, "tk_k_split_stitch", [&] {
            hipLaunchKernelGGL(tk_k_split_stitch, dim3(grid_for(n_docs, 4, 65536)), dim3(256), 0, s, p, planes, d_tok_off, cut, spec_plane, exit_at, join_at, words);
        }));
    TRY(timed(c, s, "tk_k_split_count", [&] {
        hipLaunchKernelGGL(tk_k_split_count, dim3((uint32_t)((p.W + 255) / 256)), dim3(256), 0, s, p, cut, spec_plane, join_at, cnt);
    }));
    TRY(timed(c, s, "tk_k_split_scan", [&] { hipLaunchKernelGGL(tk_k_split_scan, dim3(1), dim3(1024), 0, s, cnt, nb, words); }));
    TRY(report_read(words, got, TK_SPLIT_WORDS, s));
    const uint64_t C = got[TK_SPLIT_NCHUNKS];  // (below 2^32: a chunk owns a token)
    for (int i = 0; i < TK_SPLIT_STATS; ++i) c->st_split[i] = got[TK_SPLIT_STAT0 + i];
    Carve res;
    uint64_t at[7];
    for (uint64_t& a : at) a = res.add(C * 4);
    const uint64_t at_cutv = res.add(C), at_dc = res.add((n_docs + 1) * 4);
    TRY(ensure(c->d_split, res.total + 16));
    out->out = TkSplitOut{carved<uint32_t>(c->d_split, at[0]), carved<uint32_t>(c->d_split, at[1]), carved<uint32_t>(c->d_split, at[2]), carved<uint32_t>(c->d_split, at[3]),
                          carved<uint32_t>(c->d_split, at[4]), carved<uint32_t>(c->d_split, at[5]), carved<uint32_t>(c->d_split, at[6]), carved<uint8_t>(c->d_split, at_cutv)};
    out->doc_chunk = carved<uint32_t>(c->d_split, at_dc);
    out->n_chunks = C;
    if (C)
        TRY(timed(c, s, "tk_k_split_write", [&] {
            hipLaunchKernelGGL(tk_k_split_write, dim3((uint32_t)((p.W + 255) / 256)), dim3(256), 0, s, p, planes, cut, cnt, d_tok_off, v.byte_start, v.char_start, v.byte_off,
                               v.char_off, out->out);
        }));
    TRY(timed(c, s, "tk_k_split_docs", [&] {
        hipLaunchKernelGGL(tk_k_split_docs, dim3(grid_for(n_docs + 1, 256, 4096)), dim3(256), 0, s, p, cut, cnt, d_tok_off, out->doc_chunk);
    }));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    return TK_OK;
}
static void split_give(const SplitView& v, const uint32_t** doc, const uint32_t** tok_begin, const uint32_t** tok_end, const uint32_t** byte_begin, const uint32_t** byte_end,
                       const uint32_t** char_begin, const uint32_t** char_end, const uint8_t** cut, const uint32_t** doc_chunk, uint64_t* n_chunks) {
    if (doc) *doc = v.out.doc;
    if (tok_begin) *tok_begin = v.out.tok_begin;
    if (tok_end) *tok_end = v.out.tok_end;
    if (byte_begin) *byte_begin = v.out.byte_begin;
    if (byte_end) *byte_end = v.out.byte_end;
    if (char_begin) *char_begin = v.out.char_begin;
    if (char_end) *char_end = v.out.char_end;
    if (cut) *cut = v.out.cut;
    if (doc_chunk) *doc_chunk = v.doc_chunk;
    if (n_chunks) *n_chunks = v.n_chunks;
}

extern "C" int tk_split_device(tk_core* c, const void* d_tokens, uint64_t n_tokens, const void* d_tok_off, uint64_t n_docs, const void* d_utf8, const void* d_doc_off,
                               const tk_split_spec* spec, void* stream, const uint32_t** d_doc_out, const uint32_t** d_tok_begin_out, const uint32_t** d_tok_end_out,
                               const uint32_t** d_byte_begin_out, const uint32_t** d_byte_end_out, const uint32_t** d_char_begin_out, const uint32_t** d_char_end_out,
                               const uint8_t** d_cut_out, const uint32_t** d_doc_chunk_out, uint64_t* n_chunks_out) {
    SplitView v;
    TRY(device_pass(c, d_tok_off && d_doc_off && (d_tokens || !n_tokens) && (d_utf8 || !n_tokens) && spec, stream, [&](hipStream_t s) {
        return split_run(c, s, (const uint32_t*)d_tokens, n_tokens, (const uint64_t*)d_tok_off, n_docs, (const uint8_t*)d_utf8, (const uint64_t*)d_doc_off, spec, &v);
    }));
    split_give(v, d_doc_out, d_tok_begin_out, d_tok_end_out, d_byte_begin_out, d_byte_end_out, d_char_begin_out, d_char_end_out, d_cut_out, d_doc_chunk_out, n_chunks_out);
    return TK_OK;
}

// tk_encode_batch (tk_encode_batch_checked with disallowed ids) with the chunks of the text it has just encoded: the passes run over the
// ids and the text while both are on the device; the chunk arrays and the ids travel back.
extern "C" int tk_encode_batch_split(tk_core* c, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, int use_special, const uint32_t* allowed_ids,
                                     uint64_t n_allowed, const uint32_t* disallowed_ids, uint64_t n_disallowed, const tk_split_spec* spec, uint32_t** doc_out,
                                     uint32_t** tok_begin_out, uint32_t** tok_end_out, uint32_t** byte_begin_out, uint32_t** byte_end_out, uint32_t** char_begin_out,
                                     uint32_t** char_end_out, uint8_t** cut_out, uint32_t** doc_chunk_out, uint64_t* n_chunks_out, uint32_t** tokens_out,
                                     uint64_t* n_tokens_out, uint64_t* tok_off_out, tk_special_hit* hit) {
    SplitView v;
    return encode_batch_pass(
        c, utf8, doc_off, n_docs, use_special, allowed_ids, n_allowed, disallowed_ids, n_disallowed, hit,
        spec && doc_out && tok_begin_out && tok_end_out && byte_begin_out && byte_end_out && char_begin_out && char_end_out && cut_out && doc_chunk_out && n_chunks_out &&
            tokens_out && n_tokens_out,
        [&] { return split_check_spec(spec); },  // (before the encode, not after it)
        [&](uint64_t n) {
            return split_run(c, c->stream, c->out_tokens.as<uint32_t>(), n, c->out_tok_off.as<uint64_t>(), n_docs, c->text.as<uint8_t>(), c->doc_off.as<uint64_t>(), spec, &v);
        },
        [&](uint64_t n) -> int {
            const uint64_t C = v.n_chunks;
            ResultBag bag;
            TRY(bag.fetch(doc_out, v.out.doc, C));
            TRY(bag.fetch(tok_begin_out, v.out.tok_begin, C));
            TRY(bag.fetch(tok_end_out, v.out.tok_end, C));
            TRY(bag.fetch(byte_begin_out, v.out.byte_begin, C));
            TRY(bag.fetch(byte_end_out, v.out.byte_end, C));
            TRY(bag.fetch(char_begin_out, v.out.char_begin, C));
            TRY(bag.fetch(char_end_out, v.out.char_end, C));
            TRY(bag.fetch(cut_out, v.out.cut, C));
            TRY(bag.fetch(doc_chunk_out, v.doc_chunk, n_docs + 1));
            TRY(bag.fetch(tokens_out, c->out_tokens.p, n));
            if (tok_off_out) HIPCHK(hipMemcpy(tok_off_out, c->out_tok_off.p, (n_docs + 1) * 8, hipMemcpyDeviceToHost));
            bag.give();
            *n_chunks_out = C;
            *n_tokens_out = n;
            return TK_OK;
        });
}

// ------------------------------------------------------------------------------------------
// JSON Lines (tk_jsonl.h): a buffer of lines on the device -> the unescaped text of one field per line as (text, doc_off), line statuses.
// ------------------------------------------------------------------------------------------
static_assert(TK_JSONL_OK == TK_JSONL_ST_OK && TK_JSONL_BLANK == TK_JSONL_ST_BLANK && TK_JSONL_MISSING == TK_JSONL_ST_MISSING &&
                  TK_JSONL_NOT_STRING == TK_JSONL_ST_NOT_STRING && TK_JSONL_BAD == TK_JSONL_ST_BAD,
              "tk_jsonl statuses");
static_assert(TK_JSONL_RAISE == TK_JSONL_M_RAISE && TK_JSONL_SKIP == TK_JSONL_M_SKIP && TK_JSONL_EMPTY == TK_JSONL_M_EMPTY, "tk_jsonl modes");
struct JsonlView {  // device buffers of the core, valid until its next JSON Lines call that succeeds
    uint8_t *text = nullptr, *status = nullptr;
    uint64_t *doc_off = nullptr, *line = nullptr, *line_off = nullptr;
    uint64_t n_docs = 0, n_lines = 0, n_text = 0;
};
static int jsonl_refusal(int why) {
    switch (why) {
        case 0: return TK_OK;
        case 1: return fail(TK_VALUE_ERROR, "field must be 1 .. 64 bytes");
        case 2: return fail(TK_VALUE_ERROR, "field must not hold a quote, a backslash or a byte below 0x20 (keys are compared as raw bytes)");
        case 3: return fail(TK_VALUE_ERROR, "flags: TK_JSONL_RAISE, TK_JSONL_SKIP or TK_JSONL_EMPTY");
        case 4: return fail(TK_VALUE_ERROR, "n_bytes: a JSON Lines buffer is at most 0xFFFF0000 bytes (positions are 32-bit)");
        default: return fail(TK_VALUE_ERROR, "tile must be a multiple of 64");
    }
}
static const char* jsonl_status_name(unsigned st) {
    static const char* names[] = {"ok", "blank", "the field is missing", "the field's value is not a string", "not a JSON object the pass can read"};
    return st < 5 ? names[st] : "?";
}
// jsonl_run: the caller holds c->mu.  The host waits twice: for the number of lines, and for documents, text bytes and the first line
// TK_JSONL_RAISE refuses.  A call that is refused has written into d_jsonl_work and d_jsonl_lines only: the previous result stays whole.
static int jsonl_run(tk_core* c, hipStream_t s, const uint8_t* d_bytes, uint64_t n, const uint8_t* field, uint64_t flen, uint32_t flags, JsonlView* out, tk_jsonl_bad* bad) {
    if (!field) return fail(TK_VALUE_ERROR, "null argument");
    TkJsonl j;
    TRY(jsonl_refusal(tk_jsonl_shape(n, field, flen, flags, TK_JSONL_TILE, &j)));
    uint8_t head[3] = {0, 0, 0}, last = '\n';
    if (n >= 3) HIPCHK(hipMemcpyAsync(head, d_bytes, 3, hipMemcpyDeviceToHost, s));
    if (n) HIPCHK(hipMemcpyAsync(&last, d_bytes + n - 1, 1, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    j.p = d_bytes;
    j.bom = n >= 3 && head[0] == 0xEF && head[1] == 0xBB && head[2] == 0xBF ? 3u : 0u;
    j.eof_nl = n && last != '\n' ? 1u : 0u;
    const uint64_t nt = j.n_tiles, W = nt * (TK_JSONL_TILE / 64);
    Carve work;
    const uint64_t at_words = work.add(TK_JSONL_WORDS * 8);
    uint64_t at_t[14];
    for (uint64_t& a : at_t) a = work.add(nt * 4);
    const uint64_t at_entry = work.add(nt * sizeof(TkJsonlCarry)), at_ep = work.add(W * 8), at_cnt = work.add(nt * 4);
    TRY(ensure(c->d_jsonl_work, work.total));
    unsigned long long* words = carved<unsigned long long>(c->d_jsonl_work, at_words);
    auto tu = [&](int i) { return carved<uint32_t>(c->d_jsonl_work, at_t[i]); };
    auto ti = [&](int i) { return carved<int32_t>(c->d_jsonl_work, at_t[i]); };
    const TkJsonlTiles T{tu(0), tu(1), tu(2), tu(3), tu(4), tu(5), ti(6), tu(7), tu(8), ti(9), ti(10), ti(11), ti(12), tu(13)};
    TkJsonlCarry* entry = carved<TkJsonlCarry>(c->d_jsonl_work, at_entry);
    unsigned long long* ep = carved<unsigned long long>(c->d_jsonl_work, at_ep);
    uint32_t* cnt = carved<uint32_t>(c->d_jsonl_work, at_cnt);
    HIPCHK(hipMemsetAsync(words, 0, TK_JSONL_WORDS * 8, s));
    HIPCHK(hipMemsetAsync(words + TK_JSONL_W_BADLINE, 0xFF, 8, s));
    const dim3 tiles((uint32_t)((nt + 3) / 4));
    TRY(timed(c, s, "tk_k_jsonl_sum", [&] { hipLaunchKernelGGL(tk_k_jsonl_sum, tiles, dim3(256), 0, s, j, T); }));
    TRY(timed(c, s, "tk_k_jsonl_carry", [&] { hipLaunchKernelGGL(tk_k_jsonl_carry, dim3(1), dim3(1024), 0, s, j, T, entry, words); }));
    unsigned long long got[TK_JSONL_WORDS];
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(got, words, sizeof got, hipMemcpyDeviceToHost));
    const uint64_t n_lines = got[TK_JSONL_W_LINES], nb = (n_lines + TK_JSONL_LB - 1) / TK_JSONL_LB;
    Carve lines;
    uint64_t at_l[7];
    for (uint64_t& a : at_l) a = lines.add((n_lines + 1) * 4);
    const uint64_t at_vmax = lines.add((n_lines + 1) * 8), at_status = lines.add(n_lines + 1), at_loff = lines.add((n_lines + 1) * 8);
    const uint64_t at_blen = lines.add((nb + 1) * 4), at_bdocs = lines.add((nb + 1) * 4);
    TRY(ensure(c->d_jsonl_lines, lines.total));
    HIPCHK(hipMemsetAsync(c->d_jsonl_lines.p, 0, lines.total, s));
    auto lu = [&](int i) { return carved<uint32_t>(c->d_jsonl_lines, at_l[i]); };
    const TkJsonlLines L{lu(0), lu(1), lu(2), lu(3), lu(4), lu(5), lu(6), carved<uint64_t>(c->d_jsonl_lines, at_vmax), carved<uint8_t>(c->d_jsonl_lines, at_status)};
    uint64_t* w_loff = carved<uint64_t>(c->d_jsonl_lines, at_loff);
    uint32_t *blen = carved<uint32_t>(c->d_jsonl_lines, at_blen), *bdocs = carved<uint32_t>(c->d_jsonl_lines, at_bdocs);
    TRY(timed(c, s, "tk_k_jsonl_select", [&] { hipLaunchKernelGGL(tk_k_jsonl_select, tiles, dim3(256), 0, s, j, entry, L, w_loff, ep); }));
    TRY(timed(c, s, "tk_k_jsonl_count", [&] { hipLaunchKernelGGL(tk_k_jsonl_count, tiles, dim3(256), 0, s, j, entry, ep, L, cnt); }));
    TRY(timed(c, s, "tk_k_jsonl_tile_scan", [&] { hipLaunchKernelGGL(tk_k_jsonl_tile_scan, dim3(1), dim3(1024), 0, s, cnt, (uint32_t)nt); }));
    if (nb) TRY(timed(c, s, "tk_k_jsonl_lines", [&] { hipLaunchKernelGGL(tk_k_jsonl_lines, dim3((uint32_t)nb), dim3(256), 0, s, j, L, cnt, (uint32_t)n_lines, blen, bdocs, words); }));
    TRY(timed(c, s, "tk_k_jsonl_line_scan", [&] { hipLaunchKernelGGL(tk_k_jsonl_line_scan, dim3(1), dim3(1024), 0, s, blen, bdocs, (uint32_t)nb, words); }));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(got, words, sizeof got, hipMemcpyDeviceToHost));
    if (got[TK_JSONL_W_BADLINE] != ~0ull) {  // TK_JSONL_RAISE: the first line that is neither a record nor blank
        const uint64_t line = got[TK_JSONL_W_BADLINE];
        uint64_t pos = 0;
        uint8_t st = 0;
        HIPCHK(hipMemcpy(&pos, w_loff + line, 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(&st, L.status + line, 1, hipMemcpyDeviceToHost));
        if (bad) *bad = tk_jsonl_bad{line, pos, st, 0};
        return fail(TK_JSONL_ERROR, "line " + std::to_string(line) + " (byte " + std::to_string(pos) + "): " + jsonl_status_name(st));
    }
    const uint64_t n_docs = got[TK_JSONL_W_DOCS], n_text = got[TK_JSONL_W_TEXT];
    Carve res;
    const uint64_t at_text = res.add(n_text + 64), at_doff = res.add((n_docs + 1) * 8), at_line = res.add((n_docs + 1) * 8), at_rloff = res.add((n_lines + 1) * 8);
    const uint64_t at_rst = res.add(n_lines + 1);
    TRY(ensure(c->d_jsonl, res.total));
    out->text = carved<uint8_t>(c->d_jsonl, at_text), out->status = carved<uint8_t>(c->d_jsonl, at_rst);
    out->doc_off = carved<uint64_t>(c->d_jsonl, at_doff), out->line = carved<uint64_t>(c->d_jsonl, at_line), out->line_off = carved<uint64_t>(c->d_jsonl, at_rloff);
    out->n_docs = n_docs, out->n_lines = n_lines, out->n_text = n_text;
    HIPCHK(hipMemsetAsync(out->text + n_text, 0, 64, s));  // (the encode entries read up to 64 bytes behind the text)
    TRY(timed(c, s, "tk_k_jsonl_docs", [&] {
        hipLaunchKernelGGL(tk_k_jsonl_docs, dim3((uint32_t)(nb ? nb : 1)), dim3(256), 0, s, j, L, (uint32_t)n_lines, blen, bdocs, n_docs, n_text, out->doc_off, out->line);
    }));
    if (n_text) TRY(timed(c, s, "tk_k_jsonl_write", [&] { hipLaunchKernelGGL(tk_k_jsonl_write, tiles, dim3(256), 0, s, j, entry, ep, L, cnt, out->doc_off, out->text); }));
    HIPCHK(hipMemcpyAsync(out->line_off, w_loff, (n_lines + 1) * 8, hipMemcpyDeviceToDevice, s));
    if (n_lines) HIPCHK(hipMemcpyAsync(out->status, L.status, n_lines, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    return TK_OK;
}

extern "C" int tk_jsonl_extract_device(tk_core* c, const void* d_bytes, uint64_t n_bytes, const uint8_t* field, uint64_t field_len, uint32_t flags, void* stream,
                                       const uint8_t** d_text_out, const uint64_t** d_doc_off_out, const uint64_t** d_line_out, const uint64_t** d_line_off_out,
                                       const uint8_t** d_status_out, uint64_t* n_docs_out, uint64_t* n_lines_out, uint64_t* n_text_out, tk_jsonl_bad* bad) {
    JsonlView v;
    TRY(device_pass(c, d_bytes || !n_bytes, stream, [&](hipStream_t s) { return jsonl_run(c, s, (const uint8_t*)d_bytes, n_bytes, field, field_len, flags, &v, bad); }));
    if (d_text_out) *d_text_out = v.text;
    if (d_doc_off_out) *d_doc_off_out = v.doc_off;
    if (d_line_out) *d_line_out = v.line;
    if (d_line_off_out) *d_line_off_out = v.line_off;
    if (d_status_out) *d_status_out = v.status;
    if (n_docs_out) *n_docs_out = v.n_docs;
    if (n_lines_out) *n_lines_out = v.n_lines;
    if (n_text_out) *n_text_out = v.n_text;
    return TK_OK;
}
// the bytes of a host call on their way to d_jsonl_in, block by block on the copy stream (the caller holds c->mu), then jsonl_run
static int jsonl_run_host(tk_core* c, const uint8_t* bytes, uint64_t n, const uint8_t* field, uint64_t flen, uint32_t flags, JsonlView* v, tk_jsonl_bad* bad) {
    if (n > TK_JSONL_MAX_BYTES) return jsonl_refusal(4);
    HIPCHK(hipSetDevice(c->device));
    TRY(ensure_copy_streams(c));
    TRY(ensure(c->d_jsonl_in, n + 64));
    if (n) {
        Feed feed(c, c->d_jsonl_in.p, bytes, n, TK_STAGE_BYTES);
        TRY(feed.start());
        TRY(feed.wait(feed.n_blocks - 1, c->stream));
        const hipError_t e = feed.finish();
        if (e != hipSuccess) return fail(TK_RUNTIME_ERROR, std::string("HIP error: ") + hipGetErrorString(e));
    }
    return drained(c, [&] { return jsonl_run(c, c->stream, c->d_jsonl_in.as<uint8_t>(), n, field, flen, flags, v, bad); });
}
extern "C" int tk_jsonl_extract(tk_core* c, const uint8_t* bytes, uint64_t n_bytes, const uint8_t* field, uint64_t field_len, uint32_t flags, uint8_t** text_out,
                                uint64_t** doc_off_out, uint64_t** line_out, uint64_t** line_off_out, uint8_t** status_out, uint64_t* n_docs_out, uint64_t* n_lines_out,
                                uint64_t* n_text_out, tk_jsonl_bad* bad) {
    if (!c) return fail(TK_VALUE_ERROR, "core is null");
    if ((!bytes && n_bytes) || !text_out || !doc_off_out || !line_out || !line_off_out || !status_out || !n_docs_out || !n_lines_out || !n_text_out)
        return fail(TK_VALUE_ERROR, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    JsonlView v;
    TRY(jsonl_run_host(c, bytes, n_bytes, field, field_len, flags, &v, bad));
    ResultBag bag;
    TRY(bag.fetch(text_out, v.text, v.n_text));
    TRY(bag.fetch(doc_off_out, v.doc_off, v.n_docs + 1));
    TRY(bag.fetch(line_out, v.line, v.n_docs));
    TRY(bag.fetch(line_off_out, v.line_off, v.n_lines + 1));
    TRY(bag.fetch(status_out, v.status, v.n_lines));
    bag.give();
    *n_docs_out = v.n_docs, *n_lines_out = v.n_lines, *n_text_out = v.n_text;
    return TK_OK;
}
// Extract, then the batch encode of the device entries on the text where it is: the text never visits the host.
extern "C" int tk_encode_jsonl(tk_core* c, const uint8_t* bytes, uint64_t n_bytes, const uint8_t* field, uint64_t field_len, uint32_t flags, int use_special,
                               const uint32_t* allowed_ids, uint64_t n_allowed, const uint32_t* disallowed_ids, uint64_t n_disallowed, uint32_t** tokens_out,
                               uint64_t* n_tokens_out, uint64_t** tok_off_out, uint64_t** line_out, uint8_t** status_out, uint64_t* n_docs_out, uint64_t* n_lines_out,
                               tk_special_hit* hit, tk_jsonl_bad* bad) {
    if (!c) return fail(TK_VALUE_ERROR, "core is null");
    if ((!bytes && n_bytes) || !tokens_out || !n_tokens_out || !tok_off_out || !line_out || !status_out || !n_docs_out || !n_lines_out || (n_disallowed && !hit))
        return fail(TK_VALUE_ERROR, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    JsonlView v;
    TRY(jsonl_run_host(c, bytes, n_bytes, field, field_len, flags, &v, bad));
    const CheckArgs chk{disallowed_ids, n_disallowed, hit};
    const uint32_t* d_tok = nullptr;
    const uint64_t* d_tok_off = nullptr;
    uint64_t n_tok = 0;
    std::vector<uint64_t> h_doc_off(v.n_docs + 1);  // (a batch of several chunks is cut by the host's copy of the offsets)
    HIPCHK(hipMemcpy(h_doc_off.data(), v.doc_off, (v.n_docs + 1) * 8, hipMemcpyDeviceToHost));
    TRY(encode_batch_device_impl(c, v.text, v.n_text, v.doc_off, h_doc_off.data(), v.n_docs, use_special, allowed_ids, n_allowed, nullptr, &d_tok, &n_tok, &d_tok_off,
                                 n_disallowed ? &chk : nullptr, /* locked */ true));
    ResultBag bag;
    TRY(bag.fetch(tokens_out, d_tok, n_tok));
    TRY(bag.fetch(tok_off_out, d_tok_off, v.n_docs + 1));
    TRY(bag.fetch(line_out, v.line, v.n_docs));
    TRY(bag.fetch(status_out, v.status, v.n_lines));
    bag.give();
    *n_tokens_out = n_tok, *n_docs_out = v.n_docs, *n_lines_out = v.n_lines;
    return TK_OK;
}

// ------------------------------------------------------------------------------------------
// Fingerprints (tk_fingerprint.h): a packed batch on the device -> MinHash signatures, LSH band keys, exact hashes, shingle counts.
// ------------------------------------------------------------------------------------------
struct FpOuts {  // the caller's arrays (device memory for fp_run, host memory for fp_to_host); any may be null
    uint32_t* sig;
    uint64_t *band, *exact, *n_shingles;
};
static int fp_shape(const tk_fingerprint_spec* spec, uint64_t n, uint64_t n_docs, TkFp* p) {
    switch (tk_fp_shape(spec->ngram, spec->n_perm, spec->bands, spec->seed, n, n_docs, p)) {
        case 0: return TK_OK;
        case 1: return fail(TK_VALUE_ERROR, "ngram must be 1 .. 32");
        case 2: return fail(TK_VALUE_ERROR, "n_perm must be 1 .. 256");
        default: return fail(TK_VALUE_ERROR, "bands must be 1 .. n_perm and divide n_perm");
    }
}
// What of a tk_fingerprint_spec can be refused without looking at the batch (the host-text entry asks before it encodes anything).
static int fp_check_spec(const tk_fingerprint_spec* spec) {
    if (!spec) return fail(TK_VALUE_ERROR, "null argument");
    TkFp p;
    return fp_shape(spec, 0, 0, &p);
}
// fp_run: the caller holds c->mu.  Three launches on s, and no wait of the host: the results are there when the stream has got to them.
// in_core: the outputs lie in c->d_fp.  A call that uses c->d_fp -- that, or band keys without signatures -- may follow one that is still
// running on another stream: its stream waits for that call's event first.
static int fp_run(tk_core* c, hipStream_t s, const uint32_t* d_tok, uint64_t n, const uint64_t* d_tok_off, uint64_t n_docs, const tk_fingerprint_spec* spec, FpOuts o,
                  bool in_core = false) {
    TkFp p;
    TRY(fp_shape(spec, n, n_docs, &p));
    if (n >= (1ull << 41)) return fail(TK_VALUE_ERROR, "n_tokens: 2^41 tokens or more");
    if (!n_docs || !(o.sig || o.band || o.exact || o.n_shingles)) return TK_OK;
    const bool core_buf = in_core || (o.band && !o.sig);
    if (core_buf) {
        if (!c->fp_done.e) HIPCHK(c->fp_done.create());
        HIPCHK(hipStreamWaitEvent(s, c->fp_done, 0));  // (an event nothing has recorded yet holds nobody up)
    }
    if (o.band && !o.sig) {  // (the band keys are made from the signatures)
        TRY(ensure(c->d_fp, n_docs * p.P * 4));
        o.sig = c->d_fp.as<uint32_t>();
    }
    const TkFpOut out{o.sig, (unsigned long long*)o.exact, (unsigned long long*)o.n_shingles};
    TRY(timed(c, s, "tk_k_fp_fill", [&] { hipLaunchKernelGGL(tk_k_fp_fill, dim3(grid_for(n_docs * (o.sig ? p.P : 1), 256, 65536)), dim3(256), 0, s, p, out); }));
    if (n)
        TRY(timed(c, s, "tk_k_fp_tile", [&] {
            hipLaunchKernelGGL(tk_k_fp_tile, dim3((uint32_t)((n + TK_FP_TILE - 1) / TK_FP_TILE)), dim3(TK_FP_THREADS), 0, s, p, d_tok, d_tok_off, out);
        }));
    if (o.band || o.exact)
        TRY(timed(c, s, "tk_k_fp_finish", [&] {
            hipLaunchKernelGGL(tk_k_fp_finish, dim3(grid_for(n_docs * p.B, 256, 65536)), dim3(256), 0, s, p, d_tok_off, o.sig, o.band, o.exact);
        }));
    if (core_buf) HIPCHK(hipEventRecord(c->fp_done, s));
    return TK_OK;
}
// fp_run into buffers of the core, then every array the caller asked for to the host (the caller holds c->mu; the stream is waited for)
static int fp_to_host(tk_core* c, hipStream_t s, const uint32_t* d_tok, uint64_t n, const uint64_t* d_tok_off, uint64_t n_docs, const tk_fingerprint_spec* spec, FpOuts h) {
    TkFp p;
    TRY(fp_shape(spec, n, n_docs, &p));
    Carve res;
    const uint64_t at_sig = res.add(n_docs * p.P * 4), at_band = res.add(n_docs * p.B * 8), at_exact = res.add(n_docs * 8), at_nsh = res.add(n_docs * 8);
    TRY(ensure(c->d_fp, res.total + 16));
    const FpOuts d{h.sig || h.band ? carved<uint32_t>(c->d_fp, at_sig) : nullptr, h.band ? carved<uint64_t>(c->d_fp, at_band) : nullptr,
                   h.exact ? carved<uint64_t>(c->d_fp, at_exact) : nullptr, h.n_shingles ? carved<uint64_t>(c->d_fp, at_nsh) : nullptr};
    TRY(fp_run(c, s, d_tok, n, d_tok_off, n_docs, spec, d, /* in_core */ true));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    if (!n_docs) return TK_OK;
    if (h.sig) HIPCHK(hipMemcpy(h.sig, d.sig, n_docs * p.P * 4, hipMemcpyDeviceToHost));
    if (h.band) HIPCHK(hipMemcpy(h.band, d.band, n_docs * p.B * 8, hipMemcpyDeviceToHost));
    if (h.exact) HIPCHK(hipMemcpy(h.exact, d.exact, n_docs * 8, hipMemcpyDeviceToHost));
    if (h.n_shingles) HIPCHK(hipMemcpy(h.n_shingles, d.n_shingles, n_docs * 8, hipMemcpyDeviceToHost));
    return TK_OK;
}

extern "C" int tk_fingerprint_device(tk_core* c, const void* d_tokens, uint64_t n_tokens, const void* d_tok_off, uint64_t n_docs, const tk_fingerprint_spec* spec, void* stream,
                                     uint32_t* d_sig, uint64_t* d_band, uint64_t* d_exact, uint64_t* d_n_shingles) {
    // This entry does not wait, so its stream must be one the caller can wait on: `stream` as it is, null being HIP's null stream (not
    // the core's own stream, which device_pass hands to the entries that wait before they return).
    return device_pass(c, d_tok_off && (d_tokens || !n_tokens) && spec, stream, [&](hipStream_t) {
        return fp_run(c, (hipStream_t)stream, (const uint32_t*)d_tokens, n_tokens, (const uint64_t*)d_tok_off, n_docs, spec, FpOuts{d_sig, d_band, d_exact, d_n_shingles});
    });
}

extern "C" int tk_fingerprint(tk_core* c, const uint32_t* tokens, const uint64_t* tok_off, uint64_t n_docs, const tk_fingerprint_spec* spec, uint32_t* sig_out,
                              uint64_t* band_out, uint64_t* exact_out, uint64_t* n_shingles_out) {
    if (!c) return fail(TK_VALUE_ERROR, "core is null");
    if (!tok_off || !spec) return fail(TK_VALUE_ERROR, "null argument");
    TRY(fp_check_spec(spec));
    TRY(check_offsets(tok_off, n_docs, "tok_off"));
    const uint64_t n = tok_off[n_docs];
    if (n && !tokens) return fail(TK_VALUE_ERROR, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(hipSetDevice(c->device));
    Carve in;
    const uint64_t at_off = in.add((n_docs + 1) * 8), at_tok = in.add(n * 4);
    TRY(ensure(c->d_fp_in, in.total + 16));
    uint64_t* d_off = carved<uint64_t>(c->d_fp_in, at_off);
    uint32_t* d_tok = carved<uint32_t>(c->d_fp_in, at_tok);
    HIPCHK(hipMemcpyAsync(d_off, tok_off, (n_docs + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (n) HIPCHK(hipMemcpyAsync(d_tok, tokens, n * 4, hipMemcpyHostToDevice, c->stream));
    return drained(c, [&] { return fp_to_host(c, c->stream, d_tok, n, d_off, n_docs, spec, FpOuts{sig_out, band_out, exact_out, n_shingles_out}); });
}

// tk_encode_batch (tk_encode_batch_checked with disallowed ids) with the fingerprints of the ids it has just produced: the passes run over
// the ids while they are on the device; the ids travel back only when tokens_out is there.
extern "C" int tk_encode_batch_fingerprint(tk_core* c, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, int use_special, const uint32_t* allowed_ids,
                                           uint64_t n_allowed, const uint32_t* disallowed_ids, uint64_t n_disallowed, const tk_fingerprint_spec* spec, uint32_t* sig_out,
                                           uint64_t* band_out, uint64_t* exact_out, uint64_t* n_shingles_out, uint64_t* tok_off_out, uint32_t** tokens_out,
                                           uint64_t* n_tokens_out, tk_special_hit* hit) {
    return encode_batch_pass(
        c, utf8, doc_off, n_docs, use_special, allowed_ids, n_allowed, disallowed_ids, n_disallowed, hit, spec && (!tokens_out || n_tokens_out),
        [&] { return fp_check_spec(spec); },  // (before the encode, not after it)
        [&](uint64_t n) {
            return fp_to_host(c, c->stream, c->out_tokens.as<uint32_t>(), n, c->out_tok_off.as<uint64_t>(), n_docs, spec, FpOuts{sig_out, band_out, exact_out, n_shingles_out});
        },
        [&](uint64_t n) -> int {
            ResultBag bag;
            if (tokens_out) TRY(bag.fetch(tokens_out, c->out_tokens.p, n));
            if (tok_off_out) HIPCHK(hipMemcpy(tok_off_out, c->out_tok_off.p, (n_docs + 1) * 8, hipMemcpyDeviceToHost));
            bag.give();
            if (n_tokens_out) *n_tokens_out = n;
            return TK_OK;
        });
}

// ------------------------------------------------------------------------------------------
// Supervised samples (tk_samples.h): a packed batch of parts on the device -> one row per sample, ids, mask and labels as [R, W].
// ------------------------------------------------------------------------------------------
static_assert(TK_SMP_KEEP_TAIL == TK_SMPF_KEEP_TAIL && TK_SMP_LEFT == TK_SMPF_LEFT, "tk_smp_spec flags");
struct SmpRoles {  // the role table as the caller gave it (host memory)
    uint32_t n_roles;
    const uint32_t *ids, *off;
    const uint8_t* train;
};
struct SmpView {  // device buffers of the core, valid until its next samples call that succeeds
    uint32_t* ids = nullptr;
    uint8_t* mask = nullptr;
    int32_t* labels = nullptr;
    uint32_t *len = nullptr, *n_trained = nullptr;
    uint64_t* full = nullptr;
    uint64_t n_rows = 0, width = 0;
};
static int smp_refusal(int why) {
    switch (why) {
        case 0: return TK_OK;
        case 1: return fail(TK_VALUE_ERROR, "max_len must be at least 1");
        case 2: return fail(TK_VALUE_ERROR, "n_roles is 0 while there are parts");
        case 3: return fail(TK_VALUE_ERROR, "the role table holds at most 256 roles");
        case 4: return fail(TK_VALUE_ERROR, "role_off must ascend from 0");
        case 5: return fail(TK_VALUE_ERROR, "the role table holds at most 4096 ids");
        case 6: return fail(TK_VALUE_ERROR, "2^32 tokens or more: the positions of the rows are 32-bit");
        case 7: return fail(TK_VALUE_ERROR, "too many parts: part indices are 32-bit");
        case 8: return fail(TK_VALUE_ERROR, "too many samples: the row indices are 32-bit");
        case 9: return fail(TK_VALUE_ERROR, "the parts have 2^32 elements or more: the positions of the rows are 32-bit");
        default: return fail(TK_VALUE_ERROR, "rows times width reaches 2^32: the positions are 32-bit");
    }
}
// What of a samples call can be refused without looking at the batch (the host-text entry asks before it encodes anything).
static int smp_check_spec(const tk_smp_spec* spec, const SmpRoles& roles, uint64_t n_tokens, uint64_t n_parts, uint64_t n_samples, TkSmp* p) {
    if (!spec) return fail(TK_VALUE_ERROR, "null argument");
    if (spec->flags & ~(TK_SMP_KEEP_TAIL | TK_SMP_LEFT)) return fail(TK_VALUE_ERROR, "tk_smp_spec: unknown flag");
    if (roles.n_roles && (!roles.off || !roles.train)) return fail(TK_VALUE_ERROR, "null argument");
    TRY(smp_refusal(tk_smp_shape(n_tokens, n_parts, n_samples, roles.n_roles, roles.off, spec->max_len, spec->width_multiple, spec->bos_id, spec->eos_id, spec->pad_id,
                                 spec->ignore_index, spec->flags, p)));
    if (roles.n_roles && roles.off[2 * roles.n_roles] && !roles.ids) return fail(TK_VALUE_ERROR, "null argument");
    return TK_OK;
}
// smp_run: the caller holds c->mu.  The host waits twice, as pad_run does: for the report words -- what the count pass has to say about
// the caller's arrays, the elements of all parts, the longest row: W and the sizes of the outputs follow from them --, and at the end.  A
// call that is refused has written into d_smp_cnt only: the previous result stays whole.
static int smp_run(tk_core* c, hipStream_t s, const uint32_t* d_tok, uint64_t n, const uint64_t* d_tok_off, uint64_t n_parts, const uint8_t* d_part_role,
                   const uint64_t* d_sample_off, uint64_t n_samples, const SmpRoles& roles, const tk_smp_spec* spec, SmpView* out) {
    TkSmp p;
    TRY(smp_check_spec(spec, roles, n, n_parts, n_samples, &p));
    // scratch: the report words | role_off, role_ids, role_train | pstart | full | len | n_trained
    const uint32_t n_off = 2 * roles.n_roles + 1, n_ids = roles.n_roles ? roles.off[2 * roles.n_roles] : 0;
    Carve cnt;
    const uint64_t at_words = cnt.add(TK_SMP_WORDS * 8), at_off = cnt.add(n_off * 4ull), at_ids = cnt.add(n_ids * 4ull), at_train = cnt.add(roles.n_roles);
    const uint64_t at_ps = cnt.add((n_parts + 1) * 8), at_full = cnt.add(n_samples * 8), at_len = cnt.add(n_samples * 4), at_ntr = cnt.add(n_samples * 4);
    TRY(ensure(c->d_smp_cnt, cnt.total));
    unsigned long long* words = carved<unsigned long long>(c->d_smp_cnt, at_words);
    uint64_t *pstart = carved<uint64_t>(c->d_smp_cnt, at_ps), *full = carved<uint64_t>(c->d_smp_cnt, at_full);
    uint32_t *len = carved<uint32_t>(c->d_smp_cnt, at_len), *ntr = carved<uint32_t>(c->d_smp_cnt, at_ntr);
    const TkSmpTable tab{carved<uint32_t>(c->d_smp_cnt, at_off), carved<uint32_t>(c->d_smp_cnt, at_ids), carved<uint8_t>(c->d_smp_cnt, at_train), n_ids};
    std::vector<uint8_t> table(at_ps - at_off, 0);  // (the table as it lies on the device, from at_off on; role_off of no roles: one 0)
    if (roles.n_roles) {
        memcpy(table.data(), roles.off, n_off * 4ull);
        if (n_ids) memcpy(table.data() + (at_ids - at_off), roles.ids, n_ids * 4ull);
        memcpy(table.data() + (at_train - at_off), roles.train, roles.n_roles);
    }
    HIPCHK(hipMemcpyAsync(carved<uint8_t>(c->d_smp_cnt, at_off), table.data(), table.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(words, 0xFF, 8 * (TK_SMP_BAD_ROLE + 1), s));  // (the three words that keep the lowest offender: all ones = none)
    HIPCHK(hipMemsetAsync(words + TK_SMP_TOTAL, 0, 16, s));
    const uint64_t n_entries = std::max(n_parts, n_samples) + 1;
    TRY(timed(c, s, "tk_k_smp_count", [&] {
        hipLaunchKernelGGL(tk_k_smp_count, dim3(grid_for(n_entries, 256, 4096)), dim3(256), 0, s, d_tok_off, d_sample_off, d_part_role, tab, p, pstart, words);
    }));
    TRY(timed(c, s, "tk_k_smp_scan", [&] { hipLaunchKernelGGL(tk_k_smp_scan, dim3(1), dim3(1024), 0, s, pstart, n_parts, words); }));
    if (n_samples)
        TRY(timed(c, s, "tk_k_smp_samples", [&] {
            hipLaunchKernelGGL(tk_k_smp_samples, dim3(grid_for(n_samples, 256, 4096)), dim3(256), 0, s, d_sample_off, d_part_role, pstart, tab, p, full, len, ntr, words);
        }));
    unsigned long long got[TK_SMP_WORDS];
    TRY(report_read(words, got, TK_SMP_WORDS, s));  // (waits for the table's copy too: `table` may go)
    TRY(offsets_refusal(got[TK_SMP_BAD_SOFF], "sample_off", "sample", "n_parts"));
    if (got[TK_SMP_BAD_ROLE] != ~0ull) return fail(TK_VALUE_ERROR, "part_role must be below n_roles: part " + std::to_string(got[TK_SMP_BAD_ROLE]) + " has no such role");
    TRY(smp_refusal(tk_smp_size(&p, got[TK_SMP_TOTAL], (uint32_t)got[TK_SMP_LONGEST])));
    const uint64_t N = p.R * p.W, n8 = (N + 7) & ~7ull, nb = (N + TK_DEC_BLOCK - 1) / TK_DEC_BLOCK;  // (n8: room for whole lanes of eight)
    Carve pos, row;
    const uint64_t at_out_ids = pos.add(n8 * 4), at_labels = pos.add(n8 * 4), at_mask = pos.add(n8);
    const uint64_t at_out_full = row.add(p.R * 8), at_out_len = row.add(p.R * 4), at_out_ntr = row.add(p.R * 4);
    TRY(ensure(c->d_smp, pos.total));
    TRY(ensure(c->d_smp_row, row.total));
    out->ids = carved<uint32_t>(c->d_smp, at_out_ids);
    out->labels = carved<int32_t>(c->d_smp, at_labels);
    out->mask = carved<uint8_t>(c->d_smp, at_mask);
    out->full = carved<uint64_t>(c->d_smp_row, at_out_full);
    out->len = carved<uint32_t>(c->d_smp_row, at_out_len);
    out->n_trained = carved<uint32_t>(c->d_smp_row, at_out_ntr);
    out->n_rows = p.R;
    out->width = p.W;
    if (p.R) {
        HIPCHK(hipMemcpyAsync(out->full, full, p.R * 8, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(out->len, len, p.R * 4, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(out->n_trained, ntr, p.R * 4, hipMemcpyDeviceToDevice, s));
    }
    if (nb)
        TRY(timed(c, s, "tk_k_smp_write", [&] {
            hipLaunchKernelGGL(tk_k_smp_write, dim3((uint32_t)nb), dim3(256), 0, s, d_tok, d_tok_off, d_sample_off, d_part_role, pstart, tab, p, out->ids, out->labels, out->mask);
        }));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    return TK_OK;
}

extern "C" int tk_assemble_samples_device(tk_core* c, const void* d_tokens, uint64_t n_tokens, const void* d_tok_off, uint64_t n_parts, const void* d_part_role,
                                          const void* d_sample_off, uint64_t n_samples, uint32_t n_roles, const uint32_t* role_ids, const uint32_t* role_off,
                                          const uint8_t* role_train, const tk_smp_spec* spec, void* stream, const uint32_t** d_ids_out, const uint8_t** d_mask_out,
                                          const int32_t** d_labels_out, const uint32_t** d_len_out, const uint64_t** d_full_len_out, const uint32_t** d_n_trained_out,
                                          uint64_t* n_rows_out, uint64_t* width_out) {
    SmpView v;
    const SmpRoles roles{n_roles, role_ids, role_off, role_train};
    TRY(device_pass(c, d_tok_off && d_sample_off && (d_tokens || !n_tokens) && (d_part_role || !n_parts) && spec, stream, [&](hipStream_t s) {
        return smp_run(c, s, (const uint32_t*)d_tokens, n_tokens, (const uint64_t*)d_tok_off, n_parts, (const uint8_t*)d_part_role, (const uint64_t*)d_sample_off, n_samples,
                       roles, spec, &v);
    }));
    if (d_ids_out) *d_ids_out = v.ids;
    if (d_mask_out) *d_mask_out = v.mask;
    if (d_labels_out) *d_labels_out = v.labels;
    if (d_len_out) *d_len_out = v.len;
    if (d_full_len_out) *d_full_len_out = v.full;
    if (d_n_trained_out) *d_n_trained_out = v.n_trained;
    if (n_rows_out) *n_rows_out = v.n_rows;
    if (width_out) *width_out = v.width;
    return TK_OK;
}

// tk_encode_batch (tk_encode_batch_checked with disallowed ids) over the parts' text with the samples assembled from the tokens it has just
// produced: the passes run over the ids while they are still on the device, and only the sample arrays travel back.
extern "C" int tk_encode_batch_samples(tk_core* c, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_parts, int use_special, const uint32_t* allowed_ids,
                                       uint64_t n_allowed, const uint32_t* disallowed_ids, uint64_t n_disallowed, const uint8_t* part_role, const uint64_t* sample_off,
                                       uint64_t n_samples, uint32_t n_roles, const uint32_t* role_ids, const uint32_t* role_off, const uint8_t* role_train,
                                       const tk_smp_spec* spec, uint32_t** ids_out, uint8_t** mask_out, int32_t** labels_out, uint32_t** len_out, uint64_t** full_len_out,
                                       uint32_t** n_trained_out, uint64_t* n_rows_out, uint64_t* width_out, tk_special_hit* hit) {
    SmpView v;
    const SmpRoles roles{n_roles, role_ids, role_off, role_train};
    return encode_batch_pass(
        c, utf8, doc_off, n_parts, use_special, allowed_ids, n_allowed, disallowed_ids, n_disallowed, hit,
        spec && sample_off && (part_role || !n_parts) && ids_out && mask_out && labels_out && len_out && full_len_out && n_trained_out && n_rows_out && width_out,
        [&] {  // (before the encode, not after it)
            TkSmp p;
            return smp_check_spec(spec, roles, 0, n_parts, n_samples, &p);
        },
        [&](uint64_t n) {
            Carve in;
            const uint64_t at_role = in.add(n_parts), at_so = in.add((n_samples + 1) * 8);
            TRY(ensure(c->d_smp_in, in.total));
            uint8_t* d_role = carved<uint8_t>(c->d_smp_in, at_role);
            uint64_t* d_so = carved<uint64_t>(c->d_smp_in, at_so);
            if (n_parts) HIPCHK(hipMemcpyAsync(d_role, part_role, n_parts, hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(d_so, sample_off, (n_samples + 1) * 8, hipMemcpyHostToDevice, c->stream));
            return smp_run(c, c->stream, c->out_tokens.as<uint32_t>(), n, c->out_tok_off.as<uint64_t>(), n_parts, d_role, d_so, n_samples, roles, spec, &v);
        },
        [&](uint64_t) -> int {
            const uint64_t N = v.n_rows * v.width;
            ResultBag bag;
            TRY(bag.fetch(ids_out, v.ids, N));
            TRY(bag.fetch(mask_out, v.mask, N));
            TRY(bag.fetch(labels_out, v.labels, N));
            TRY(bag.fetch(len_out, v.len, v.n_rows));
            TRY(bag.fetch(full_len_out, v.full, v.n_rows));
            TRY(bag.fetch(n_trained_out, v.n_trained, v.n_rows));
            bag.give();
            *n_rows_out = v.n_rows;
            *width_out = v.width;
            return TK_OK;
        });
}

// ------------------------------------------------------------------------------------------
// Packed sample rows (tk_sample_rows.h): a packed batch of parts on the device -> several whole samples per row of max_len, with labels,
// the sample and the position of every element, and the segment boundaries.
// ------------------------------------------------------------------------------------------
static_assert(TK_SMP_SKIP_LONG == TK_SMPF_SKIP_LONG && TK_SMP_IGNORE_FIRST == TK_SMPF_IGNORE_FIRST, "tk_smp_spec flags");
struct SrowView {  // device buffers of the core, valid until its next packed-samples call that succeeds
    uint32_t *ids = nullptr, *seg = nullptr, *pos = nullptr, *cu = nullptr, *row_seg = nullptr, *row_sample = nullptr;
    int32_t* labels = nullptr;
    uint32_t *len = nullptr, *n_trained = nullptr, *sample_row = nullptr, *sample_col = nullptr;
    uint64_t* full = nullptr;
    uint64_t n_rows = 0, n_segs = 0, width = 0;
};
static int srow_refusal(int why) {
    switch (why) {
        case 11: return fail(TK_VALUE_ERROR, "packed sample rows are max_len wide: width_multiple must be 0");
        case 12: return fail(TK_VALUE_ERROR, "packed sample rows are padded behind their samples: TK_SMP_LEFT does not apply");
        default: return smp_refusal(why);
    }
}
// What of a packed-samples call can be refused without looking at the batch (the host-text entry asks before it encodes anything).
static int srow_check_spec(const tk_smp_spec* spec, const SmpRoles& roles, uint64_t n_tokens, uint64_t n_parts, uint64_t n_samples, TkSmp* p) {
    if (!spec) return fail(TK_VALUE_ERROR, "null argument");
    if (spec->flags & ~(TK_SMP_KEEP_TAIL | TK_SMP_LEFT | TK_SMP_SKIP_LONG | TK_SMP_IGNORE_FIRST)) return fail(TK_VALUE_ERROR, "tk_smp_spec: unknown flag");
    if (roles.n_roles && (!roles.off || !roles.train)) return fail(TK_VALUE_ERROR, "null argument");
    TRY(srow_refusal(tk_srow_shape(n_tokens, n_parts, n_samples, roles.n_roles, roles.off, spec->max_len, spec->width_multiple, spec->bos_id, spec->eos_id, spec->pad_id,
                                   spec->ignore_index, spec->flags, p)));
    if (roles.n_roles && roles.off[2 * roles.n_roles] && !roles.ids) return fail(TK_VALUE_ERROR, "null argument");
    return TK_OK;
}
// srow_run: the caller holds c->mu.  The host waits twice, as smp_run does: for the report words -- what the count pass has to say about
// the caller's arrays, the elements of all parts, R and the number of segments: the sizes of the outputs follow from them --, and at the
// end.  A call that is refused has written into d_srow_cnt only: the previous result stays whole.
static int srow_run(tk_core* c, hipStream_t s, const uint32_t* d_tok, uint64_t n, const uint64_t* d_tok_off, uint64_t n_parts, const uint8_t* d_part_role,
                    const uint64_t* d_sample_off, uint64_t n_samples, const SmpRoles& roles, const tk_smp_spec* spec, SrowView* out) {
    TkSmp p;
    TRY(srow_check_spec(spec, roles, n, n_parts, n_samples, &p));
    // scratch: the report words | role_off, role_ids, role_train | pstart | full | c | f | len | n_trained | succ | two jump arrays | mark
    // (then ex) | sample_row | sample_col | row_sample | row_pad (then row_seg)
    const uint32_t n_off = 2 * roles.n_roles + 1, n_ids = roles.n_roles ? roles.off[2 * roles.n_roles] : 0;
    const uint64_t ns = n_samples;
    Carve cnt;
    const uint64_t at_words = cnt.add(TK_SROW_WORDS * 8), at_off = cnt.add(n_off * 4ull), at_ids = cnt.add(n_ids * 4ull), at_train = cnt.add(roles.n_roles);
    const uint64_t at_ps = cnt.add((n_parts + 1) * 8), at_full = cnt.add(ns * 8), at_c = cnt.add((ns + 1) * 8), at_f = cnt.add((ns + 1) * 8);
    const uint64_t at_len = cnt.add(ns * 4), at_ntr = cnt.add(ns * 4), at_succ = cnt.add((ns + 1) * 4), at_j0 = cnt.add((ns + 1) * 4), at_j1 = cnt.add((ns + 1) * 4);
    const uint64_t at_mark = cnt.add((ns + 1) * 4), at_srow = cnt.add(ns * 4), at_scol = cnt.add(ns * 4), at_rsmp = cnt.add((ns + 1) * 4), at_rpad = cnt.add((ns + 1) * 4);
    TRY(ensure(c->d_srow_cnt, cnt.total));
    const Buf& B = c->d_srow_cnt;
    unsigned long long* words = carved<unsigned long long>(B, at_words);
    uint64_t *pstart = carved<uint64_t>(B, at_ps), *full = carved<uint64_t>(B, at_full), *cs = carved<uint64_t>(B, at_c), *fs = carved<uint64_t>(B, at_f);
    uint32_t *len = carved<uint32_t>(B, at_len), *ntr = carved<uint32_t>(B, at_ntr), *succ = carved<uint32_t>(B, at_succ), *mark = carved<uint32_t>(B, at_mark);
    uint32_t* jump[2] = {carved<uint32_t>(B, at_j0), carved<uint32_t>(B, at_j1)};
    uint32_t *srow = carved<uint32_t>(B, at_srow), *scol = carved<uint32_t>(B, at_scol), *rsmp = carved<uint32_t>(B, at_rsmp), *rpad = carved<uint32_t>(B, at_rpad);
    const TkSmpTable tab{carved<uint32_t>(B, at_off), carved<uint32_t>(B, at_ids), carved<uint8_t>(B, at_train), n_ids};
    std::vector<uint8_t> table(at_ps - at_off, 0);  // (the table as it lies on the device, from at_off on; role_off of no roles: one 0)
    if (roles.n_roles) {
        memcpy(table.data(), roles.off, n_off * 4ull);
        if (n_ids) memcpy(table.data() + (at_ids - at_off), roles.ids, n_ids * 4ull);
        memcpy(table.data() + (at_train - at_off), roles.train, roles.n_roles);
    }
    HIPCHK(hipMemcpyAsync(carved<uint8_t>(B, at_off), table.data(), table.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(words, 0xFF, 8 * (TK_SMP_BAD_ROLE + 1), s));  // (the three words that keep the lowest offender: all ones = none)
    HIPCHK(hipMemsetAsync(words + TK_SMP_TOTAL, 0, 8 * (TK_SROW_WORDS - TK_SMP_TOTAL), s));
    const uint64_t n_entries = std::max(n_parts, n_samples) + 1;
    const uint32_t g_smp = grid_for(ns + 1, 256, 4096);
    TRY(timed(c, s, "tk_k_smp_count", [&] {
        hipLaunchKernelGGL(tk_k_smp_count, dim3(grid_for(n_entries, 256, 4096)), dim3(256), 0, s, d_tok_off, d_sample_off, d_part_role, tab, p, pstart, words);
    }));
    TRY(timed(c, s, "tk_k_smp_scan", [&] { hipLaunchKernelGGL(tk_k_smp_scan, dim3(1), dim3(1024), 0, s, pstart, n_parts, words); }));
    if (ns) {
        TRY(timed(c, s, "tk_k_smp_samples", [&] {
            hipLaunchKernelGGL(tk_k_smp_samples, dim3(g_smp), dim3(256), 0, s, d_sample_off, d_part_role, pstart, tab, p, full, len, ntr, words);
        }));
        TRY(timed(c, s, "tk_k_srow_plen", [&] {
            hipLaunchKernelGGL(tk_k_srow_plen, dim3(g_smp), dim3(256), 0, s, d_tok_off, d_sample_off, d_part_role, pstart, tab, p, full, len, ntr, cs, fs, words);
        }));
    }
    TRY(timed(c, s, "tk_k_srow_sums", [&] { hipLaunchKernelGGL(tk_k_srow_sums, dim3(1), dim3(1024), 0, s, cs, fs, ns, words); }));
    TRY(timed(c, s, "tk_k_srow_succ", [&] { hipLaunchKernelGGL(tk_k_srow_succ, dim3(g_smp), dim3(256), 0, s, cs, fs, ns, p.max_len, succ, mark, words); }));
    const uint32_t rounds = tk_srow_rounds(ns);
    for (uint32_t k = 0; k < rounds; ++k) {
        const uint32_t* jin = k ? jump[(k - 1) & 1] : succ;
        TRY(timed(c, s, "tk_k_srow_double", [&] { hipLaunchKernelGGL(tk_k_srow_double, dim3(g_smp), dim3(256), 0, s, jin, jump[k & 1], mark, ns, words); }));
    }
    TRY(timed(c, s, "tk_k_srow_rows", [&] { hipLaunchKernelGGL(tk_k_srow_rows, dim3(1), dim3(1024), 0, s, mark, ns, words); }));
    TRY(timed(c, s, "tk_k_srow_place", [&] { hipLaunchKernelGGL(tk_k_srow_place, dim3(g_smp), dim3(256), 0, s, mark, cs, succ, ns, p.max_len, srow, scol, rsmp, rpad, words); }));
    TRY(timed(c, s, "tk_k_srow_segs", [&] { hipLaunchKernelGGL(tk_k_srow_segs, dim3(1), dim3(1024), 0, s, mark, fs, rsmp, ns, rpad, words); }));
    unsigned long long got[TK_SROW_WORDS];
    TRY(report_read(words, got, TK_SROW_WORDS, s));  // (waits for the table's copy too: `table` may go)
    TRY(offsets_refusal(got[TK_SMP_BAD_SOFF], "sample_off", "sample", "n_parts"));
    if (got[TK_SMP_BAD_ROLE] != ~0ull) return fail(TK_VALUE_ERROR, "part_role must be below n_roles: part " + std::to_string(got[TK_SMP_BAD_ROLE]) + " has no such role");
    TRY(srow_refusal(tk_srow_size(&p, got[TK_SMP_TOTAL], got[TK_SROW_R])));
    const uint64_t R = p.R, n_segs = got[TK_SROW_NSEGS], N = R * p.W, n8 = (N + 7) & ~7ull, nb = (N + TK_DEC_BLOCK - 1) / TK_DEC_BLOCK;  // (n8: room for whole lanes of eight)
    Carve pos, row;
    const uint64_t at_out_ids = pos.add(n8 * 4), at_labels = pos.add(n8 * 4), at_seg = pos.add(n8 * 4), at_pos = pos.add(n8 * 4);
    const uint64_t at_out_full = row.add(ns * 8), at_out_len = row.add(ns * 4), at_out_ntr = row.add(ns * 4), at_out_srow = row.add(ns * 4), at_out_scol = row.add(ns * 4);
    const uint64_t at_out_rsmp = row.add((R + 1) * 4), at_out_rseg = row.add((R + 1) * 4), at_cu = row.add((n_segs + 1) * 4);
    TRY(ensure(c->d_srow, pos.total));
    TRY(ensure(c->d_srow_row, row.total));
    out->ids = carved<uint32_t>(c->d_srow, at_out_ids);
    out->labels = carved<int32_t>(c->d_srow, at_labels);
    out->seg = carved<uint32_t>(c->d_srow, at_seg);
    out->pos = carved<uint32_t>(c->d_srow, at_pos);
    out->full = carved<uint64_t>(c->d_srow_row, at_out_full);
    out->len = carved<uint32_t>(c->d_srow_row, at_out_len);
    out->n_trained = carved<uint32_t>(c->d_srow_row, at_out_ntr);
    out->sample_row = carved<uint32_t>(c->d_srow_row, at_out_srow);
    out->sample_col = carved<uint32_t>(c->d_srow_row, at_out_scol);
    out->row_sample = carved<uint32_t>(c->d_srow_row, at_out_rsmp);
    out->row_seg = carved<uint32_t>(c->d_srow_row, at_out_rseg);
    out->cu = carved<uint32_t>(c->d_srow_row, at_cu);
    out->n_rows = R;
    out->n_segs = n_segs;
    out->width = p.W;
    if (ns) {
        HIPCHK(hipMemcpyAsync(out->full, full, ns * 8, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(out->len, len, ns * 4, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(out->n_trained, ntr, ns * 4, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(out->sample_row, srow, ns * 4, hipMemcpyDeviceToDevice, s));
        HIPCHK(hipMemcpyAsync(out->sample_col, scol, ns * 4, hipMemcpyDeviceToDevice, s));
    }
    HIPCHK(hipMemcpyAsync(out->row_sample, rsmp, (R + 1) * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(out->row_seg, rpad, (R + 1) * 4, hipMemcpyDeviceToDevice, s));
    if (nb) {
        const TkSrowInPtr rw{cs, fs, rsmp, rpad};
        TRY(timed(c, s, "tk_k_srow_write", [&] {
            hipLaunchKernelGGL(tk_k_srow_write, dim3((uint32_t)nb), dim3(256), 0, s, d_tok, d_tok_off, d_sample_off, d_part_role, pstart, rw, tab, p, (uint32_t)n_segs, out->ids,
                               out->labels, out->seg, out->pos, out->cu);
        }));
    } else {
        HIPCHK(hipMemsetAsync(out->cu, 0, 4, s));  // (no row: cu_seqlens is its closing entry, R * L = 0)
    }
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    return TK_OK;
}

extern "C" int tk_pack_samples_device(tk_core* c, const void* d_tokens, uint64_t n_tokens, const void* d_tok_off, uint64_t n_parts, const void* d_part_role,
                                      const void* d_sample_off, uint64_t n_samples, uint32_t n_roles, const uint32_t* role_ids, const uint32_t* role_off,
                                      const uint8_t* role_train, const tk_smp_spec* spec, void* stream, const uint32_t** d_ids_out, const int32_t** d_labels_out,
                                      const uint32_t** d_seg_out, const uint32_t** d_pos_out, const uint32_t** d_cu_seqlens_out, const uint32_t** d_row_seg_out,
                                      const uint32_t** d_row_sample_out, const uint32_t** d_len_out, const uint64_t** d_full_len_out, const uint32_t** d_n_trained_out,
                                      const uint32_t** d_sample_row_out, const uint32_t** d_sample_col_out, uint64_t* n_rows_out, uint64_t* n_segs_out) {
    SrowView v;
    const SmpRoles roles{n_roles, role_ids, role_off, role_train};
    TRY(device_pass(c, d_tok_off && d_sample_off && (d_tokens || !n_tokens) && (d_part_role || !n_parts) && spec, stream, [&](hipStream_t s) {
        return srow_run(c, s, (const uint32_t*)d_tokens, n_tokens, (const uint64_t*)d_tok_off, n_parts, (const uint8_t*)d_part_role, (const uint64_t*)d_sample_off, n_samples,
                        roles, spec, &v);
    }));
    if (d_ids_out) *d_ids_out = v.ids;
    if (d_labels_out) *d_labels_out = v.labels;
    if (d_seg_out) *d_seg_out = v.seg;
    if (d_pos_out) *d_pos_out = v.pos;
    if (d_cu_seqlens_out) *d_cu_seqlens_out = v.cu;
    if (d_row_seg_out) *d_row_seg_out = v.row_seg;
    if (d_row_sample_out) *d_row_sample_out = v.row_sample;
    if (d_len_out) *d_len_out = v.len;
    if (d_full_len_out) *d_full_len_out = v.full;
    if (d_n_trained_out) *d_n_trained_out = v.n_trained;
    if (d_sample_row_out) *d_sample_row_out = v.sample_row;
    if (d_sample_col_out) *d_sample_col_out = v.sample_col;
    if (n_rows_out) *n_rows_out = v.n_rows;
    if (n_segs_out) *n_segs_out = v.n_segs;
    return TK_OK;
}

// tk_encode_batch (tk_encode_batch_checked with disallowed ids) over the parts' text with the samples packed into rows from the tokens it
// has just produced: the passes run over the ids while they are still on the device, and only the row arrays travel back.
extern "C" int tk_encode_batch_sample_rows(tk_core* c, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_parts, int use_special, const uint32_t* allowed_ids,
                                           uint64_t n_allowed, const uint32_t* disallowed_ids, uint64_t n_disallowed, const uint8_t* part_role, const uint64_t* sample_off,
                                           uint64_t n_samples, uint32_t n_roles, const uint32_t* role_ids, const uint32_t* role_off, const uint8_t* role_train,
                                           const tk_smp_spec* spec, uint32_t** ids_out, int32_t** labels_out, uint32_t** seg_out, uint32_t** pos_out,
                                           uint32_t** cu_seqlens_out, uint32_t** row_seg_out, uint32_t** row_sample_out, uint32_t** len_out, uint64_t** full_len_out,
                                           uint32_t** n_trained_out, uint32_t** sample_row_out, uint32_t** sample_col_out, uint64_t* n_rows_out, uint64_t* n_segs_out,
                                           tk_special_hit* hit) {
    SrowView v;
    const SmpRoles roles{n_roles, role_ids, role_off, role_train};
    return encode_batch_pass(
        c, utf8, doc_off, n_parts, use_special, allowed_ids, n_allowed, disallowed_ids, n_disallowed, hit,
        spec && sample_off && (part_role || !n_parts) && ids_out && labels_out && seg_out && pos_out && cu_seqlens_out && row_seg_out && row_sample_out && len_out &&
            full_len_out && n_trained_out && sample_row_out && sample_col_out && n_rows_out && n_segs_out,
        [&] {  // (before the encode, not after it)
            TkSmp p;
            return srow_check_spec(spec, roles, 0, n_parts, n_samples, &p);
        },
        [&](uint64_t n) {
            Carve in;
            const uint64_t at_role = in.add(n_parts), at_so = in.add((n_samples + 1) * 8);
            TRY(ensure(c->d_srow_in, in.total));
            uint8_t* d_role = carved<uint8_t>(c->d_srow_in, at_role);
            uint64_t* d_so = carved<uint64_t>(c->d_srow_in, at_so);
            if (n_parts) HIPCHK(hipMemcpyAsync(d_role, part_role, n_parts, hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(d_so, sample_off, (n_samples + 1) * 8, hipMemcpyHostToDevice, c->stream));
            return srow_run(c, c->stream, c->out_tokens.as<uint32_t>(), n, c->out_tok_off.as<uint64_t>(), n_parts, d_role, d_so, n_samples, roles, spec, &v);
        },
        [&](uint64_t) -> int {
            const uint64_t N = v.n_rows * v.width;
            ResultBag bag;
            TRY(bag.fetch(ids_out, v.ids, N));
            TRY(bag.fetch(labels_out, v.labels, N));
            TRY(bag.fetch(seg_out, v.seg, N));
            TRY(bag.fetch(pos_out, v.pos, N));
            TRY(bag.fetch(cu_seqlens_out, v.cu, v.n_segs + 1));
            TRY(bag.fetch(row_seg_out, v.row_seg, v.n_rows + 1));
            TRY(bag.fetch(row_sample_out, v.row_sample, v.n_rows + 1));
            TRY(bag.fetch(len_out, v.len, n_samples));
            TRY(bag.fetch(full_len_out, v.full, n_samples));
            TRY(bag.fetch(n_trained_out, v.n_trained, n_samples));
            TRY(bag.fetch(sample_row_out, v.sample_row, n_samples));
            TRY(bag.fetch(sample_col_out, v.sample_col, n_samples));
            bag.give();
            *n_rows_out = v.n_rows;
            *n_segs_out = v.n_segs;
            return TK_OK;
        });
}

// ------------------------------------------------------------------------------------------
// Decoding id matrices (tk_decode_rows.h): an id matrix on the device -> the compact ids of its rows' live ranges, then the decode passes.
// ------------------------------------------------------------------------------------------
static_assert(TK_DROWS_KEEP_STOP == TK_DROWSF_KEEP_STOP && TK_DROWS_SKIP_SPECIAL == TK_DROWSF_SKIP_SPECIAL && TK_DROWS_I32 == TK_DROWSF_I32 && TK_DROWS_I64 == TK_DROWSF_I64,
              "tk_drows_spec flags");
static_assert(sizeof(((tk_drows_spec*)nullptr)->stop_ids) == TK_DROWS_LIST * 4 && sizeof(((tk_drows_spec*)nullptr)->skip_ids) == TK_DROWS_LIST * 4, "tk_drows_spec lists");
struct DrowsView {  // device buffers of the core: the first four valid until its next decode-rows call that succeeds, the last two until its next decode call
    const uint32_t* tokens = nullptr;
    const uint64_t* tok_off = nullptr;
    const uint32_t *n_kept = nullptr, *stop_col = nullptr;
    const uint8_t* bytes = nullptr;
    const uint64_t* byte_off = nullptr;
    uint64_t n_tokens = 0, n_bytes = 0;
    const unsigned long long* tok_byte = nullptr;  // the byte position of every kept token in `bytes` (the decode passes leave it: valid as long as they are)
};
static int drows_refusal(int why) {
    switch (why) {
        case 0: return TK_OK;
        case 1: return fail(TK_VALUE_ERROR, "more than 16 stop ids");
        case 2: return fail(TK_VALUE_ERROR, "more than 16 skip ids");
        case 3: return fail(TK_VALUE_ERROR, "TK_DROWS_I32 together with TK_DROWS_I64");
        case 4: return fail(TK_VALUE_ERROR, "ld must be at least the width");
        case 5: return fail(TK_VALUE_ERROR, "too many rows: the row indices are 32-bit");
        case 6: return fail(TK_VALUE_ERROR, "2^32 columns or more: the column indices are 32-bit");
        case 7: return fail(TK_VALUE_ERROR, "tk_drows_spec: unknown flag");
        default: return fail(TK_VALUE_ERROR, "the matrix spans 2^60 elements or more");
    }
}
// What can be refused without looking at the matrix
static int drows_check_spec(tk_core* c, const tk_drows_spec* spec, uint64_t R, uint64_t W, uint64_t ld, TkDrows* p) {
    if (!spec) return fail(TK_VALUE_ERROR, "null argument");
    TRY(drows_refusal(tk_drows_shape(R, W, ld, spec->flags, spec->n_stop, spec->stop_ids, spec->n_skip, spec->skip_ids, TK_DEC_BLOCK, p)));
    return decode_table_check(c);
}
// the kernels of a matrix's element type: f(std::integral_constant<int, MODE>) with TkIdMatrix's MODE
template <class F>
static void drows_by_type(uint32_t flags, F&& f) {
    if (flags & TK_DROWS_I64) f(std::integral_constant<int, 2>());
    else if (flags & TK_DROWS_I32) f(std::integral_constant<int, 1>());
    else f(std::integral_constant<int, 0>());
}
// the reference's KeyError for element (r, c) of the matrix, which has no bytes
static int drows_invalid_token(const void* d_ids, const TkDrows& p, uint64_t pos) {
    const uint64_t r = pos / p.W, col = pos - r * p.W;  // (W != 0: there is an element)
    const uint32_t es = tk_drows_elem_size(p.flags);
    int64_t wide = 0;
    uint32_t narrow = 0;
    (void)hipMemcpy(es == 8 ? (void*)&wide : (void*)&narrow, (const uint8_t*)d_ids + (r * p.ld + col) * es, es, hipMemcpyDeviceToHost);
    const std::string n = es == 8 ? std::to_string(wide) : (p.flags & TK_DROWS_I32) ? std::to_string((int32_t)narrow) : std::to_string(narrow);
    return fail(TK_KEY_ERROR, "Invalid token for decoding: " + n + " (row " + std::to_string(r) + ", column " + std::to_string(col) + ")");
}
// drows_run: the caller holds c->mu.  The host waits once for the report words -- the first offending row, the first kept id without entry,
// K --, refuses or sizes the outputs, and hands (tokens, tok_off) to the decode passes.  A call that is refused has written into
// d_drows_cnt only: the previous result stays whole.
static int drows_run(tk_core* c, hipStream_t s, const void* d_ids, uint64_t R, uint64_t W, uint64_t ld, const uint32_t* d_begin, const uint32_t* d_end,
                     const tk_drows_spec* spec, DrowsView* out) {
    TkDrows p;
    TRY(drows_check_spec(c, spec, R, W, ld, &p));
    const uint64_t nt = tk_drows_n_tiles(p);
    Carve scratch;
    const uint64_t at_words = scratch.add(TK_DROWS_WORDS * 8), at_found = scratch.add(R * 4), at_cnt = scratch.add(nt * 8);
    TRY(ensure(c->d_drows_cnt, scratch.total));
    unsigned long long* words = carved<unsigned long long>(c->d_drows_cnt, at_words);
    uint32_t* found = carved<uint32_t>(c->d_drows_cnt, at_found);
    unsigned long long* cnt = carved<unsigned long long>(c->d_drows_cnt, at_cnt);
    HIPCHK(hipMemsetAsync(words, 0xFF, (TK_DROWS_K - TK_DROWS_BAD_ROW) * 8, s));  // (no row, no id offends; tk_k_drows_scan writes K)
    if (R) HIPCHK(hipMemsetAsync(found, 0xFF, R * 4, s));
    const dim3 grid((uint32_t)std::min<uint64_t>(nt, 1u << 20)), block(256);
    const uint2* dec = c->t_dec.as<uint2>();
    if (nt && (p.n_stop || d_begin || d_end))  // (nothing to find, nothing to check otherwise)
        TRY(timed(c, s, "tk_k_drows_stop", [&] {
            drows_by_type(p.flags, [&](auto m) { hipLaunchKernelGGL(tk_k_drows_stop<decltype(m)::value>, grid, block, 0, s, d_ids, d_begin, d_end, p, nt, found, words); });
        }));
    if (nt)
        TRY(timed(c, s, "tk_k_drows_count", [&] {
            drows_by_type(p.flags, [&](auto m) {
                hipLaunchKernelGGL(tk_k_drows_count<decltype(m)::value>, grid, block, 0, s, d_ids, d_begin, d_end, p, nt, found, dec, c->n_dec, cnt, words);
            });
        }));
    TRY(timed(c, s, "tk_k_drows_scan", [&] { hipLaunchKernelGGL(tk_k_drows_scan, dim3(1), dim3(1024), 0, s, cnt, nt, words); }));
    unsigned long long got[TK_DROWS_WORDS];
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(got, words, sizeof(got), hipMemcpyDeviceToHost));
    if (got[TK_DROWS_BAD_ROW] != ~0ull)
        return fail(TK_VALUE_ERROR, "begin and end must satisfy begin <= end <= width: row " + std::to_string(got[TK_DROWS_BAD_ROW]) + " does not");
    if (got[TK_DROWS_BAD_ID] != ~0ull) return drows_invalid_token(d_ids, p, got[TK_DROWS_BAD_ID]);
    const uint64_t K = got[TK_DROWS_K];
    if (K >> 32) return fail(TK_VALUE_ERROR, "2^32 kept ids or more: decode the matrix in parts");
    Carve row;
    const uint64_t at_off = row.add((R + 1) * 8), at_kept = row.add(R * 4), at_stop = row.add(R * 4);
    TRY(ensure(c->d_drows_tok, (K + 1) * 4));
    TRY(ensure(c->d_drows_row, row.total));
    uint32_t* tokens = c->d_drows_tok.as<uint32_t>();
    uint64_t* tok_off = carved<uint64_t>(c->d_drows_row, at_off);
    uint32_t *n_kept = carved<uint32_t>(c->d_drows_row, at_kept), *stop_col = carved<uint32_t>(c->d_drows_row, at_stop);
    TRY(timed(c, s, "tk_k_drows_rows", [&] {
        hipLaunchKernelGGL(tk_k_drows_rows, dim3(grid_for(R + 1, 256, 4096)), block, 0, s, d_begin, d_end, p, cnt, found, K, tok_off, n_kept, stop_col);
    }));
    if (nt && K)
        TRY(timed(c, s, "tk_k_drows_write", [&] {
            drows_by_type(p.flags, [&](auto m) {
                hipLaunchKernelGGL(tk_k_drows_write<decltype(m)::value>, grid, block, 0, s, d_ids, d_begin, d_end, p, nt, found, dec, c->n_dec, cnt, tokens);
            });
        }));
    DecodeView dv;
    TRY(decode_device_run(c, s, tokens, K, tok_off, R, &dv, &out->n_bytes));  // (waits for the stream at its end)
    out->tokens = tokens;
    out->tok_off = tok_off;
    out->n_kept = n_kept;
    out->stop_col = stop_col;
    out->bytes = c->d_bytes.as<uint8_t>();
    out->byte_off = dv.byte_off;
    out->tok_byte = dv.tboff;
    out->n_tokens = K;
    return TK_OK;
}

extern "C" int tk_decode_rows_device(tk_core* c, const void* d_ids, uint64_t n_rows, uint64_t width, uint64_t ld, const void* d_begin, const void* d_end,
                                     const tk_drows_spec* spec, void* stream, const uint32_t** d_tokens_out, const uint64_t** d_tok_off_out, const uint32_t** d_n_kept_out,
                                     const uint32_t** d_stop_col_out, const uint8_t** d_bytes_out, const uint64_t** d_byte_off_out, uint64_t* n_tokens_out,
                                     uint64_t* n_bytes_out) {
    DrowsView v;
    TRY(device_pass(c, spec && n_tokens_out && n_bytes_out && (d_ids || !n_rows || !width), stream,
                    [&](hipStream_t s) { return drows_run(c, s, d_ids, n_rows, width, ld, (const uint32_t*)d_begin, (const uint32_t*)d_end, spec, &v); }));
    if (d_tokens_out) *d_tokens_out = v.tokens;
    if (d_tok_off_out) *d_tok_off_out = v.tok_off;
    if (d_n_kept_out) *d_n_kept_out = v.n_kept;
    if (d_stop_col_out) *d_stop_col_out = v.stop_col;
    if (d_bytes_out) *d_bytes_out = v.bytes;
    if (d_byte_off_out) *d_byte_off_out = v.byte_off;
    *n_tokens_out = v.n_tokens;
    *n_bytes_out = v.n_bytes;
    return TK_OK;
}

// A matrix in host memory: its (R - 1) * ld + W elements travel to the device as they lie (a slice keeps its row stride), begin and end behind
// them (drows_host_in), and the six arrays travel back.
static int drows_host_in(tk_core* c, hipStream_t s, const void* ids, uint64_t n_rows, uint64_t width, uint64_t ld, const uint32_t* begin, const uint32_t* end,
                         const TkDrows& p, void** d_ids, uint32_t** d_begin, uint32_t** d_end) {
    const uint64_t n_elems = n_rows && width ? (n_rows - 1) * ld + width : 0;
    Carve in;
    const uint64_t at_ids = in.add(n_elems * tk_drows_elem_size(p.flags)), at_begin = in.add(n_rows * 4), at_end = in.add(n_rows * 4);
    TRY(ensure(c->d_drows_in, in.total + 16));
    *d_ids = carved<void>(c->d_drows_in, at_ids);
    *d_begin = begin ? carved<uint32_t>(c->d_drows_in, at_begin) : nullptr;
    *d_end = end ? carved<uint32_t>(c->d_drows_in, at_end) : nullptr;
    if (n_elems) HIPCHK(hipMemcpyAsync(*d_ids, ids, n_elems * tk_drows_elem_size(p.flags), hipMemcpyHostToDevice, s));
    if (begin && n_rows) HIPCHK(hipMemcpyAsync(*d_begin, begin, n_rows * 4, hipMemcpyHostToDevice, s));
    if (end && n_rows) HIPCHK(hipMemcpyAsync(*d_end, end, n_rows * 4, hipMemcpyHostToDevice, s));
    return TK_OK;
}
extern "C" int tk_decode_rows(tk_core* c, const void* ids, uint64_t n_rows, uint64_t width, uint64_t ld, const uint32_t* begin, const uint32_t* end,
                              const tk_drows_spec* spec, uint32_t** tokens_out, uint64_t** tok_off_out, uint32_t** n_kept_out, uint32_t** stop_col_out, uint8_t** bytes_out,
                              uint64_t** byte_off_out, uint64_t* n_tokens_out, uint64_t* n_bytes_out) {
    if (!c) return fail(TK_VALUE_ERROR, "core is null");
    if (!spec || !tokens_out || !tok_off_out || !n_kept_out || !stop_col_out || !bytes_out || !byte_off_out || !n_tokens_out || !n_bytes_out || (!ids && n_rows && width))
        return fail(TK_VALUE_ERROR, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(hipSetDevice(c->device));
    return drained(c, [&]() -> int {
        TkDrows p;
        TRY(drows_check_spec(c, spec, n_rows, width, ld, &p));  // (before anything is copied)
        hipStream_t s = c->stream;
        void* d_ids;
        uint32_t *d_begin, *d_end;
        TRY(drows_host_in(c, s, ids, n_rows, width, ld, begin, end, p, &d_ids, &d_begin, &d_end));
        DrowsView v;
        TRY(drows_run(c, s, d_ids, n_rows, width, ld, d_begin, d_end, spec, &v));
        ResultBag bag;
        TRY(bag.fetch(tokens_out, v.tokens, v.n_tokens));
        TRY(bag.fetch(tok_off_out, v.tok_off, n_rows + 1));
        TRY(bag.fetch(n_kept_out, v.n_kept, n_rows));
        TRY(bag.fetch(stop_col_out, v.stop_col, n_rows));
        TRY(bag.fetch(bytes_out, v.bytes, v.n_bytes));
        TRY(bag.fetch(byte_off_out, v.byte_off, n_rows + 1));
        bag.give();
        *n_tokens_out = v.n_tokens;
        *n_bytes_out = v.n_bytes;
        return TK_OK;
    });
}

// ------------------------------------------------------------------------------------------
// UTF-8 repair (tk_utf8_repair.h; the rule: include/tiktoken_amd.h): packed text on the device -> what errors="replace" / "ignore" makes of
// every document, and the packed decode entries that hand out text instead of bytes.
// ------------------------------------------------------------------------------------------
static_assert(TK_U8_REPLACE == TK_U8R_REPLACE && TK_U8_IGNORE == TK_U8R_IGNORE, "repair modes");
struct RepairView {  // device buffers of the core, valid until its next repair call (text / text_off: the INPUT where nothing was replaced)
    const uint8_t* text = nullptr;
    const uint64_t *text_off = nullptr, *char_off = nullptr, *repl_off = nullptr;
    uint64_t n_text = 0, n_chars = 0, n_replaced = 0;
};
// repair_run: the caller holds c->mu.  The host waits once, for the report words -- the first offending offset, the three totals --, refuses
// or sizes the outputs.  A call that is refused has written into d_u8r_cnt only: the previous result stays whole.
static int repair_run(tk_core* c, hipStream_t s, const uint8_t* d_bytes, uint64_t n, const uint64_t* d_off, uint64_t n_docs, uint32_t mode, RepairView* out) {
    if (mode != TK_U8_REPLACE && mode != TK_U8_IGNORE) return fail(TK_VALUE_ERROR, "mode must be TK_U8_REPLACE or TK_U8_IGNORE");
    if (!d_off || (n && !d_bytes)) return fail(TK_VALUE_ERROR, "null argument");
    if (((uintptr_t)d_bytes & 15u) || ((uintptr_t)d_off & 7u)) return fail(TK_VALUE_ERROR, "d_bytes must be 16-byte aligned and d_byte_off 8-byte aligned");
    if (n_docs >= (1ull << 60)) return fail(TK_VALUE_ERROR, "2^60 documents or more");
    if (n / TK_U8R_BLOCK >= 0x7FFFFFFFull) return fail(TK_VALUE_ERROR, "2^43 bytes or more: a workgroup per 4096 bytes is more than a grid holds -- repair the text in parts");
    const uint64_t nb = n / TK_U8R_BLOCK + 1, lanes = n / 16 + 1, bm_bytes = (n / 32 + 4) * 4;
    Carve scratch;
    const uint64_t at_words = scratch.add(TK_U8R_WORDS * 8), at_sums = scratch.add(3 * nb * 8), at_rel = scratch.add(3 * (n_docs + 1) * 4), at_place = scratch.add(lanes * 2),
                   at_bm = scratch.add(bm_bytes);
    TRY(ensure(c->d_u8r_cnt, scratch.total));
    unsigned long long *words = carved<unsigned long long>(c->d_u8r_cnt, at_words), *sums = carved<unsigned long long>(c->d_u8r_cnt, at_sums);
    uint32_t *rel = carved<uint32_t>(c->d_u8r_cnt, at_rel), *docb = carved<uint32_t>(c->d_u8r_cnt, at_bm);
    uint16_t* place = carved<uint16_t>(c->d_u8r_cnt, at_place);
    const unsigned long long h_words[TK_U8R_WORDS] = {~0ull, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(words, h_words, sizeof h_words, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(docb, 0, bm_bytes, s));
    const dim3 per_doc(grid_for(n_docs + 1, 256, 4096)), block(256);
    TRY(timed(c, s, "tk_k_u8r_check", [&] { hipLaunchKernelGGL(tk_k_u8r_check, per_doc, block, 0, s, d_off, n_docs, n, words); }));
    TRY(timed(c, s, "tk_k_span_mark", [&] { hipLaunchKernelGGL(tk_k_span_mark, per_doc, block, 0, s, d_off, n_docs + 1, n, docb); }));
    TRY(timed(c, s, "tk_k_u8r_count", [&] {
        hipLaunchKernelGGL(tk_k_u8r_count, dim3((uint32_t)nb), block, 0, s, d_bytes, n, docb, d_off, n_docs, mode, nb, sums, place, rel);
    }));
    TRY(timed(c, s, "tk_k_u8r_scan", [&] { hipLaunchKernelGGL(tk_k_u8r_scan, dim3(3), dim3(1024), 0, s, sums, nb, words); }));
    unsigned long long got[TK_U8R_WORDS];
    HIPCHK(hipMemcpyAsync(got, words, sizeof got, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    if (got[TK_U8R_BAD_DOC] != ~0ull)
        return fail(TK_VALUE_ERROR, "byte_off must ascend from 0 to n_bytes: document " + std::to_string(got[TK_U8R_BAD_DOC]) + " does not");
    const uint64_t n_text = got[TK_U8R_OUT], n_repl = got[TK_U8R_REPL];
    TRY(ensure(c->d_u8r_doc, 3 * (n_docs + 1) * 8));
    uint64_t* doc = c->d_u8r_doc.as<uint64_t>();
    TRY(timed(c, s, "tk_k_u8r_docs", [&] { hipLaunchKernelGGL(tk_k_u8r_docs, per_doc, block, 0, s, d_off, n_docs, nb, sums, rel, doc); }));
    if (n_repl) {
        TRY(ensure(c->d_u8r_text, n_text + 16));
        if (n)
            TRY(timed(c, s, "tk_k_u8r_write", [&] {
                hipLaunchKernelGGL(tk_k_u8r_write, dim3((uint32_t)((n + TK_U8R_BLOCK - 1) / TK_U8R_BLOCK)), block, 0, s, d_bytes, n, docb, mode, sums, place,
                                   c->d_u8r_text.as<uint8_t>());
            }));
    }
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    out->text = n_repl ? c->d_u8r_text.as<uint8_t>() : d_bytes;
    out->text_off = n_repl ? doc : d_off;
    out->char_off = doc + (n_docs + 1);
    out->repl_off = doc + 2 * (n_docs + 1);
    out->n_text = n_text;
    out->n_chars = got[TK_U8R_CHARS];
    out->n_replaced = n_repl;
    return TK_OK;
}

extern "C" int tk_utf8_repair_device(tk_core* c, const void* d_bytes, uint64_t n_bytes, const void* d_byte_off, uint64_t n_docs, uint32_t mode, void* stream,
                                     const uint8_t** d_text_out, uint64_t* n_text_out, const uint64_t** d_text_off_out, const uint64_t** d_char_off_out,
                                     const uint64_t** d_repl_off_out, uint64_t* n_replaced_out) {
    RepairView v;
    TRY(device_pass(c, n_text_out && n_replaced_out, stream,
                    [&](hipStream_t s) { return repair_run(c, s, (const uint8_t*)d_bytes, n_bytes, (const uint64_t*)d_byte_off, n_docs, mode, &v); }));
    if (d_text_out) *d_text_out = v.text;
    if (d_text_off_out) *d_text_off_out = v.text_off;
    if (d_char_off_out) *d_char_off_out = v.char_off;
    if (d_repl_off_out) *d_repl_off_out = v.repl_off;
    *n_text_out = v.n_text;
    *n_replaced_out = v.n_replaced;
    return TK_OK;
}

// Host ids in, host text out: the ids and their offsets in one copy, decode_device_run, the repair over its bytes, one copy out.  One pass:
// the overlapped ranges of tk_decode_batch are not built for it.
extern "C" int tk_decode_batch_text(tk_core* c, const uint32_t* tokens, const uint64_t* tok_off, uint64_t n_docs, uint32_t mode, uint8_t** text_out, uint64_t* n_text_out,
                                    uint64_t** text_off_out, uint64_t** char_off_out, uint64_t** repl_off_out, uint64_t* n_replaced_out) {
    if (!c) return fail(TK_VALUE_ERROR, "core is null");
    if (!tok_off || !text_out || !n_text_out || !text_off_out || !char_off_out || !repl_off_out || !n_replaced_out) return fail(TK_VALUE_ERROR, "null argument");
    TRY(check_offsets(tok_off, n_docs, "tok_off"));
    TRY(decode_table_check(c));
    const uint64_t n = tok_off[n_docs];
    if (n && !tokens) return fail(TK_VALUE_ERROR, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(hipSetDevice(c->device));
    return drained(c, [&]() -> int {
        hipStream_t s = c->stream;
        DecodeView dv;
        TRY(ensure(c->d_tok, (n + 1) * 4));
        TRY(decode_view(c, n, 0, true, true, n_docs, &dv));  // (decode_device_run makes the same view again)
        uint64_t* const d_tok_off = dv.tok_off;
        HIPCHK(hipMemcpyAsync(d_tok_off, tok_off, (n_docs + 1) * 8, hipMemcpyHostToDevice, s));
        if (n) HIPCHK(hipMemcpyAsync(c->d_tok.p, tokens, n * 4, hipMemcpyHostToDevice, s));
        uint64_t n_bytes = 0;
        TRY(decode_device_run(c, s, c->d_tok.as<uint32_t>(), n, d_tok_off, n_docs, &dv, &n_bytes));  // (TK_KEY_ERROR names the id from its device copy)
        RepairView v;
        TRY(repair_run(c, s, c->d_bytes.as<uint8_t>(), n_bytes, dv.byte_off, n_docs, mode, &v));
        ResultBag bag;
        TRY(bag.fetch(text_out, v.text, v.n_text));
        TRY(bag.fetch(text_off_out, v.text_off, n_docs + 1));
        TRY(bag.fetch(char_off_out, v.char_off, n_docs + 1));
        TRY(bag.fetch(repl_off_out, v.repl_off, n_docs + 1));
        bag.give();
        *n_text_out = v.n_text;
        *n_replaced_out = v.n_replaced;
        return TK_OK;
    });
}

// The decode-rows passes unchanged, then the repair over their bytes.
extern "C" int tk_decode_rows_text_device(tk_core* c, const void* d_ids, uint64_t n_rows, uint64_t width, uint64_t ld, const void* d_begin, const void* d_end,
                                          const tk_drows_spec* spec, uint32_t mode, void* stream, const uint32_t** d_tokens_out, const uint64_t** d_tok_off_out,
                                          const uint32_t** d_n_kept_out, const uint32_t** d_stop_col_out, const uint8_t** d_text_out, const uint64_t** d_text_off_out,
                                          const uint64_t** d_char_off_out, const uint64_t** d_repl_off_out, uint64_t* n_tokens_out, uint64_t* n_text_out,
                                          uint64_t* n_replaced_out) {
    if (mode != TK_U8_REPLACE && mode != TK_U8_IGNORE) return fail(TK_VALUE_ERROR, "mode must be TK_U8_REPLACE or TK_U8_IGNORE");  // (before the rows passes write)
    DrowsView v;
    RepairView t;
    TRY(device_pass(c, spec && n_tokens_out && n_text_out && n_replaced_out && (d_ids || !n_rows || !width), stream, [&](hipStream_t s) -> int {
        TRY(drows_run(c, s, d_ids, n_rows, width, ld, (const uint32_t*)d_begin, (const uint32_t*)d_end, spec, &v));
        return repair_run(c, s, v.bytes, v.n_bytes, v.byte_off, n_rows, mode, &t);
    }));
    if (d_tokens_out) *d_tokens_out = v.tokens;
    if (d_tok_off_out) *d_tok_off_out = v.tok_off;
    if (d_n_kept_out) *d_n_kept_out = v.n_kept;
    if (d_stop_col_out) *d_stop_col_out = v.stop_col;
    if (d_text_out) *d_text_out = t.text;
    if (d_text_off_out) *d_text_off_out = t.text_off;
    if (d_char_off_out) *d_char_off_out = t.char_off;
    if (d_repl_off_out) *d_repl_off_out = t.repl_off;
    *n_tokens_out = v.n_tokens;
    *n_text_out = t.n_text;
    *n_replaced_out = t.n_replaced;
    return TK_OK;
}
extern "C" int tk_decode_rows_text(tk_core* c, const void* ids, uint64_t n_rows, uint64_t width, uint64_t ld, const uint32_t* begin, const uint32_t* end,
                                   const tk_drows_spec* spec, uint32_t mode, uint32_t** tokens_out, uint64_t** tok_off_out, uint32_t** n_kept_out, uint32_t** stop_col_out,
                                   uint8_t** text_out, uint64_t** text_off_out, uint64_t** char_off_out, uint64_t** repl_off_out, uint64_t* n_tokens_out,
                                   uint64_t* n_text_out, uint64_t* n_replaced_out) {
    if (!c) return fail(TK_VALUE_ERROR, "core is null");
    if (!spec || !tokens_out || !tok_off_out || !n_kept_out || !stop_col_out || !text_out || !text_off_out || !char_off_out || !repl_off_out || !n_tokens_out || !n_text_out ||
        !n_replaced_out || (!ids && n_rows && width))
        return fail(TK_VALUE_ERROR, "null argument");
    if (mode != TK_U8_REPLACE && mode != TK_U8_IGNORE) return fail(TK_VALUE_ERROR, "mode must be TK_U8_REPLACE or TK_U8_IGNORE");
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(hipSetDevice(c->device));
    return drained(c, [&]() -> int {
        TkDrows p;
        TRY(drows_check_spec(c, spec, n_rows, width, ld, &p));  // (before anything is copied)
        hipStream_t s = c->stream;
        void* d_ids;
        uint32_t *d_begin, *d_end;
        TRY(drows_host_in(c, s, ids, n_rows, width, ld, begin, end, p, &d_ids, &d_begin, &d_end));
        DrowsView v;
        TRY(drows_run(c, s, d_ids, n_rows, width, ld, d_begin, d_end, spec, &v));
        RepairView t;
        TRY(repair_run(c, s, v.bytes, v.n_bytes, v.byte_off, n_rows, mode, &t));
        ResultBag bag;
        TRY(bag.fetch(tokens_out, v.tokens, v.n_tokens));
        TRY(bag.fetch(tok_off_out, v.tok_off, n_rows + 1));
        TRY(bag.fetch(n_kept_out, v.n_kept, n_rows));
        TRY(bag.fetch(stop_col_out, v.stop_col, n_rows));
        TRY(bag.fetch(text_out, t.text, t.n_text));
        TRY(bag.fetch(text_off_out, t.text_off, n_rows + 1));
        TRY(bag.fetch(char_off_out, t.char_off, n_rows + 1));
        TRY(bag.fetch(repl_off_out, t.repl_off, n_rows + 1));
        bag.give();
        *n_tokens_out = v.n_tokens;
        *n_text_out = t.n_text;
        *n_replaced_out = t.n_replaced;
        return TK_OK;
    });
}

// ------------------------------------------------------------------------------------------
// Stop strings (tk_stop_text.h; the rule: include/tiktoken_amd.h): packed text on the device -> every document cut at its first stop
// string, and the decode-rows entries that cut their rows so before the repair.
// ------------------------------------------------------------------------------------------
static_assert(TK_STOPS_KEEP == TK_STOPSF_KEEP, "stop flags");
struct StopsView {  // device buffers of the core, valid until its next stop-string call (text / text_off: the INPUT where no document has a hit)
    const uint8_t* text = nullptr;
    const uint64_t* text_off = nullptr;
    const uint32_t* hit = nullptr;
    uint32_t* n_tok = nullptr;  // room for a count per document behind hit, for the entries over id matrices
    uint64_t n_text = 0, n_hit = 0;
};
// What can be refused without looking at the text
static int stops_check(const tk_stops* stops, uint32_t flags, TkStopSet* set) {
    if (!stops || (stops->n && (!stops->blob || !stops->off))) return fail(TK_VALUE_ERROR, "null argument");
    switch (tk_stops_make(stops->n, stops->blob, stops->off, flags, set)) {
        case 0: return TK_OK;
        case 1: return fail(TK_VALUE_ERROR, "more than 16 stop strings");
        case 2: return fail(TK_VALUE_ERROR, "an empty stop string");
        case 3: return fail(TK_VALUE_ERROR, "a stop string of more than 64 bytes");
        case 4: return fail(TK_VALUE_ERROR, "the offsets of the stop strings must ascend from 0");
        default: return fail(TK_VALUE_ERROR, "stop strings: unknown flag");
    }
}
// stops_run: the caller holds c->mu.  The host waits once, for the report words -- the first offending offset, the bytes kept, the documents
// with a hit --, refuses, hands back the input or sizes the outputs.  A call that is refused has written into d_stop_cnt only.
static int stops_run(tk_core* c, hipStream_t s, const uint8_t* d_bytes, uint64_t n, const uint64_t* d_off, uint64_t n_docs, const TkStopSet& set, StopsView* out) {
    if (!d_off || (n && !d_bytes)) return fail(TK_VALUE_ERROR, "null argument");
    if (((uintptr_t)d_bytes & 15u) || ((uintptr_t)d_off & 7u)) return fail(TK_VALUE_ERROR, "d_bytes must be 16-byte aligned and d_byte_off 8-byte aligned");
    if (n_docs >= (1ull << 40)) return fail(TK_VALUE_ERROR, "2^40 documents or more");
    if (n / TK_STOPS_BLOCK >= 0x7FFFFFFFull) return fail(TK_VALUE_ERROR, "2^43 bytes or more: a workgroup per 4096 bytes is more than a grid holds -- search the text in parts");
    const uint64_t nb_find = (n + TK_STOPS_BLOCK - 1) / TK_STOPS_BLOCK, nb_rows = (n_docs + TK_STOPS_ROWS_BLOCK - 1) / TK_STOPS_ROWS_BLOCK;
    Carve scratch;
    const uint64_t at_words = scratch.add(TK_STOPS_WORDS * 8), at_set = scratch.add(sizeof(TkStopSet)), at_word = scratch.add(n_docs * 8), at_rel = scratch.add(n_docs * 8),
                   at_hit = scratch.add(n_docs * 4), at_bsum = scratch.add(nb_rows * 8);
    TRY(ensure(c->d_stop_cnt, scratch.total));
    unsigned long long *words = carved<unsigned long long>(c->d_stop_cnt, at_words), *word = carved<unsigned long long>(c->d_stop_cnt, at_word),
                       *rel = carved<unsigned long long>(c->d_stop_cnt, at_rel), *bsum = carved<unsigned long long>(c->d_stop_cnt, at_bsum);
    uint32_t *d_set = carved<uint32_t>(c->d_stop_cnt, at_set), *hit_s = carved<uint32_t>(c->d_stop_cnt, at_hit);
    const unsigned long long h_words[TK_STOPS_WORDS] = {~0ull, 0, 0};
    HIPCHK(hipMemcpyAsync(words, h_words, sizeof h_words, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_set, &set, sizeof set, hipMemcpyHostToDevice, s));
    if (n_docs) HIPCHK(hipMemsetAsync(word, 0xFF, n_docs * 8, s));
    const dim3 per_doc(grid_for(n_docs + 1, 256, 4096)), block(256);
    TRY(timed(c, s, "tk_k_u8r_check", [&] { hipLaunchKernelGGL(tk_k_u8r_check, per_doc, block, 0, s, d_off, n_docs, n, words); }));
    if (n && n_docs && set.n)
        TRY(timed(c, s, "tk_k_stops_find", [&] { hipLaunchKernelGGL(tk_k_stops_find, dim3((uint32_t)nb_find), block, 0, s, d_bytes, n, d_off, n_docs, d_set, word); }));
    if (n_docs)
        TRY(timed(c, s, "tk_k_stops_rows", [&] {
            hipLaunchKernelGGL(tk_k_stops_rows, dim3((uint32_t)nb_rows), dim3(TK_STOPS_ROWS_BLOCK), 0, s, d_off, n_docs, word, d_set, rel, hit_s, bsum, words);
        }));
    TRY(timed(c, s, "tk_k_stops_scan", [&] { hipLaunchKernelGGL(tk_k_stops_scan, dim3(1), dim3(1024), 0, s, bsum, nb_rows, words); }));
    unsigned long long got[TK_STOPS_WORDS];
    HIPCHK(hipMemcpyAsync(got, words, sizeof got, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    if (got[TK_STOPS_BAD_DOC] != ~0ull)
        return fail(TK_VALUE_ERROR, "byte_off must ascend from 0 to n_bytes: document " + std::to_string(got[TK_STOPS_BAD_DOC]) + " does not");
    const uint64_t n_text = got[TK_STOPS_OUT], n_hit = got[TK_STOPS_N_HIT];
    Carve doc;
    const uint64_t at_off = doc.add((n_docs + 1) * 8), at_out_hit = doc.add(n_docs * 4), at_ntok = doc.add(n_docs * 4);
    TRY(ensure(c->d_stop_doc, doc.total + 16));
    uint64_t* text_off = carved<uint64_t>(c->d_stop_doc, at_off);
    uint32_t* hit = carved<uint32_t>(c->d_stop_doc, at_out_hit);
    TRY(timed(c, s, "tk_k_stops_docs", [&] { hipLaunchKernelGGL(tk_k_stops_docs, per_doc, block, 0, s, n_docs, bsum, rel, hit_s, words, n_hit ? text_off : nullptr, hit); }));
    if (n_hit) {
        TRY(ensure(c->d_stop_text, n_text + 16));
        if (n_text)
            TRY(timed(c, s, "tk_k_stops_cut", [&] {
                hipLaunchKernelGGL(tk_k_stops_cut, dim3(grid_for((n_text + 15) / 16, 256, 1u << 16)), block, 0, s, d_bytes, d_off, text_off, n_docs, n_text,
                                   c->d_stop_text.as<uint8_t>());
            }));
    }
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    out->text = n_hit ? c->d_stop_text.as<uint8_t>() : d_bytes;
    out->text_off = n_hit ? text_off : d_off;
    out->hit = hit;
    out->n_tok = carved<uint32_t>(c->d_stop_doc, at_ntok);
    out->n_text = n_text;
    out->n_hit = n_hit;
    return TK_OK;
}

extern "C" int tk_stop_text_device(tk_core* c, const void* d_bytes, uint64_t n_bytes, const void* d_byte_off, uint64_t n_docs, const tk_stops* stops, uint32_t flags,
                                   void* stream, const uint8_t** d_text_out, uint64_t* n_text_out, const uint64_t** d_text_off_out, const uint32_t** d_hit_out,
                                   uint64_t* n_hit_out) {
    TkStopSet set;
    TRY(stops_check(stops, flags, &set));
    StopsView v;
    TRY(device_pass(c, n_text_out && n_hit_out, stream,
                    [&](hipStream_t s) { return stops_run(c, s, (const uint8_t*)d_bytes, n_bytes, (const uint64_t*)d_byte_off, n_docs, set, &v); }));
    if (d_text_out) *d_text_out = v.text;
    if (d_text_off_out) *d_text_off_out = v.text_off;
    if (d_hit_out) *d_hit_out = v.hit;
    *n_text_out = v.n_text;
    *n_hit_out = v.n_hit;
    return TK_OK;
}

// The decode-rows passes unchanged, the search and the cut over their bytes, the rows' token counts, then the repair (mode TK_U8_BYTES: none)
static int until_mode_check(uint32_t mode) {
    return mode == TK_U8_REPLACE || mode == TK_U8_IGNORE || mode == TK_U8_BYTES ? TK_OK : fail(TK_VALUE_ERROR, "mode must be TK_U8_REPLACE, TK_U8_IGNORE or TK_U8_BYTES");
}
static int until_run(tk_core* c, hipStream_t s, const void* d_ids, uint64_t R, uint64_t W, uint64_t ld, const uint32_t* d_begin, const uint32_t* d_end, const tk_drows_spec* spec,
                     const TkStopSet& set, uint32_t mode, DrowsView* v, StopsView* t, RepairView* u) {
    TRY(drows_run(c, s, d_ids, R, W, ld, d_begin, d_end, spec, v));
    TRY(stops_run(c, s, v->bytes, v->n_bytes, v->byte_off, R, set, t));
    if (R)
        TRY(timed(c, s, "tk_k_stops_ntok", [&] {
            hipLaunchKernelGGL(tk_k_stops_ntok, dim3(grid_for(R, 256, 4096)), dim3(256), 0, s, v->tok_off, v->byte_off, t->text_off, v->tok_byte, R, t->n_tok);
        }));
    if (mode != TK_U8_BYTES) return repair_run(c, s, t->text, t->n_text, t->text_off, R, mode, u);  // (waits for the stream at its end)
    *u = RepairView{t->text, t->text_off, nullptr, nullptr, t->n_text, 0, 0};
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    return TK_OK;
}
extern "C" int tk_decode_rows_until_device(tk_core* c, const void* d_ids, uint64_t n_rows, uint64_t width, uint64_t ld, const void* d_begin, const void* d_end,
                                           const tk_drows_spec* spec, const tk_stops* stops, uint32_t stop_flags, uint32_t mode, void* stream,
                                           const uint32_t** d_tokens_out, const uint64_t** d_tok_off_out, const uint32_t** d_n_kept_out, const uint32_t** d_stop_col_out,
                                           const uint8_t** d_text_out, const uint64_t** d_text_off_out, const uint64_t** d_char_off_out, const uint64_t** d_repl_off_out,
                                           const uint32_t** d_hit_out, const uint32_t** d_n_tok_out, uint64_t* n_tokens_out, uint64_t* n_text_out,
                                           uint64_t* n_replaced_out, uint64_t* n_hit_out) {
    TRY(until_mode_check(mode));  // (both before the rows passes write)
    TkStopSet set;
    TRY(stops_check(stops, stop_flags, &set));
    DrowsView v;
    StopsView t;
    RepairView u;
    TRY(device_pass(c, spec && n_tokens_out && n_text_out && n_replaced_out && n_hit_out && (d_ids || !n_rows || !width), stream, [&](hipStream_t s) -> int {
        return until_run(c, s, d_ids, n_rows, width, ld, (const uint32_t*)d_begin, (const uint32_t*)d_end, spec, set, mode, &v, &t, &u);
    }));
    if (d_tokens_out) *d_tokens_out = v.tokens;
    if (d_tok_off_out) *d_tok_off_out = v.tok_off;
    if (d_n_kept_out) *d_n_kept_out = v.n_kept;
    if (d_stop_col_out) *d_stop_col_out = v.stop_col;
    if (d_text_out) *d_text_out = u.text;
    if (d_text_off_out) *d_text_off_out = u.text_off;
    if (d_char_off_out) *d_char_off_out = u.char_off;
    if (d_repl_off_out) *d_repl_off_out = u.repl_off;
    if (d_hit_out) *d_hit_out = t.hit;
    if (d_n_tok_out) *d_n_tok_out = t.n_tok;
    *n_tokens_out = v.n_tokens;
    *n_text_out = u.n_text;
    *n_replaced_out = u.n_replaced;
    *n_hit_out = t.n_hit;
    return TK_OK;
}
extern "C" int tk_decode_rows_until(tk_core* c, const void* ids, uint64_t n_rows, uint64_t width, uint64_t ld, const uint32_t* begin, const uint32_t* end,
                                    const tk_drows_spec* spec, const tk_stops* stops, uint32_t stop_flags, uint32_t mode, uint32_t** tokens_out, uint64_t** tok_off_out,
                                    uint32_t** n_kept_out, uint32_t** stop_col_out, uint8_t** text_out, uint64_t** text_off_out, uint64_t** char_off_out,
                                    uint64_t** repl_off_out, uint32_t** hit_out, uint32_t** n_tok_out, uint64_t* n_tokens_out, uint64_t* n_text_out,
                                    uint64_t* n_replaced_out, uint64_t* n_hit_out) {
    if (!c) return fail(TK_VALUE_ERROR, "core is null");
    if (!spec || !tokens_out || !tok_off_out || !n_kept_out || !stop_col_out || !text_out || !text_off_out || !char_off_out || !repl_off_out || !hit_out || !n_tok_out ||
        !n_tokens_out || !n_text_out || !n_replaced_out || !n_hit_out || (!ids && n_rows && width))
        return fail(TK_VALUE_ERROR, "null argument");
    TRY(until_mode_check(mode));
    TkStopSet set;
    TRY(stops_check(stops, stop_flags, &set));
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(hipSetDevice(c->device));
    return drained(c, [&]() -> int {
        TkDrows p;
        TRY(drows_check_spec(c, spec, n_rows, width, ld, &p));  // (before anything is copied)
        hipStream_t s = c->stream;
        void* d_ids;
        uint32_t *d_begin, *d_end;
        TRY(drows_host_in(c, s, ids, n_rows, width, ld, begin, end, p, &d_ids, &d_begin, &d_end));
        DrowsView v;
        StopsView t;
        RepairView u;
        TRY(until_run(c, s, d_ids, n_rows, width, ld, d_begin, d_end, spec, set, mode, &v, &t, &u));
        ResultBag bag;
        TRY(bag.fetch(tokens_out, v.tokens, v.n_tokens));
        TRY(bag.fetch(tok_off_out, v.tok_off, n_rows + 1));
        TRY(bag.fetch(n_kept_out, v.n_kept, n_rows));
        TRY(bag.fetch(stop_col_out, v.stop_col, n_rows));
        TRY(bag.fetch(text_out, u.text, u.n_text));
        TRY(bag.fetch(text_off_out, u.text_off, n_rows + 1));
        if (mode != TK_U8_BYTES) {
            TRY(bag.fetch(char_off_out, u.char_off, n_rows + 1));
            TRY(bag.fetch(repl_off_out, u.repl_off, n_rows + 1));
        }
        TRY(bag.fetch(hit_out, t.hit, n_rows));
        TRY(bag.fetch(n_tok_out, t.n_tok, n_rows));
        bag.give();
        if (mode == TK_U8_BYTES) *char_off_out = *repl_off_out = nullptr;
        *n_tokens_out = v.n_tokens;
        *n_text_out = u.n_text;
        *n_replaced_out = u.n_replaced;
        *n_hit_out = t.n_hit;
        return TK_OK;
    });
}

// ------------------------------------------------------------------------------------------
// Streaming decode (tk_stream.h; the rule: include/tiktoken_amd.h): row slots in HBM, fed a few columns per step.  Every buffer of a stream
// belongs to its tk_stream and goes with it; a call holds the core's mutex.  A call is two launches and one wait: the row kernel writes
// scratch and the other copy of the slots, the pack pass writes the outputs unless the row kernel reported a refusal, and the host swaps the
// copies once it has read the report words.
// ------------------------------------------------------------------------------------------
static_assert(TK_U8_BYTES == TK_STREAM_MODE_BYTES, "stream modes");
struct tk_stream {
    tk_core* c = nullptr;
    int device = 0;
    uint64_t R = 0, slot = 0;
    uint32_t w_max = 0, mode = 0, cap = 0, dtype = 0;
    tk_drows_spec spec{};
    int cur = 0;  // which copy of the slots holds the state
    uint64_t n_text = 0, n_chars = 0;  // of the last accepted call
    bool fetched = false;
    Pinned<unsigned long long> h_words;  // [0, TK_STREAM_WORDS): what a call starts from; [8, 8 + TK_STREAM_WORDS): what it reported
    std::vector<uint8_t> h_text;         // the last accepted call's outputs on the host (stream_fetch)
    std::vector<uint64_t> h_text_off, h_char_off;
    std::vector<uint32_t> h_state, h_hit;
    Buf rows[2], set, scratch, len, text, doc, out, words, in;
};
struct StreamView {  // device buffers of the stream, valid until its next call
    const uint8_t* text = nullptr;
    const uint64_t *text_off = nullptr, *char_off = nullptr;
    const uint32_t *state = nullptr, *hit = nullptr;
};
static StreamView stream_view(const tk_stream* st) {
    const uint64_t* doc = st->doc.as<uint64_t>();
    const uint32_t* out = st->out.as<uint32_t>();
    return StreamView{st->text.as<uint8_t>(), doc, st->mode == TK_U8_BYTES ? nullptr : doc + (st->R + 1), out, out + st->R};
}
// stream_run: the caller holds the core's mutex.  op: TK_STREAM_OP_*; d_sel: a byte per row for flush and reset (null: every row).
static int stream_run(tk_stream* st, hipStream_t s, uint32_t op, const void* d_ids, uint64_t W, uint64_t ld, const uint32_t* d_begin, const uint32_t* d_end,
                      const uint8_t* d_sel) {
    tk_core* c = st->c;
    TkDrows p;
    const uint32_t flags = (st->spec.flags & ~(TK_DROWS_I32 | TK_DROWS_I64)) | st->dtype;
    TRY(drows_refusal(tk_drows_shape(st->R, W, ld, flags, st->spec.n_stop, st->spec.stop_ids, st->spec.n_skip, st->spec.skip_ids, TK_DEC_BLOCK, &p)));
    if (W > st->w_max) return fail(TK_VALUE_ERROR, "a step of " + std::to_string(W) + " columns: the stream was created with w_max = " + std::to_string(st->w_max));
    if (W && st->R && !d_ids) return fail(TK_VALUE_ERROR, "null argument");
    unsigned long long* words = st->words.as<unsigned long long>();
    HIPCHK(hipMemcpyAsync(words, st->h_words.p, TK_STREAM_WORDS * 8, hipMemcpyHostToDevice, s));
    const TkStreamRow* cur = st->rows[st->cur].as<TkStreamRow>();
    TkStreamRow* next = st->rows[st->cur ^ 1].as<TkStreamRow>();
    uint32_t *len = st->len.as<uint32_t>(), *chars = len + st->R;
    const dim3 grid_row((uint32_t)std::max<uint64_t>((st->R + TK_STREAM_ROWS_WG - 1) / TK_STREAM_ROWS_WG, 1)), grid_pack((uint32_t)(st->R / TK_STREAM_PACK_BLOCK + 1));
    const size_t lds = TK_STREAM_SET_BYTES + (size_t)TK_STREAM_ROWS_WG * st->cap;
    TRY(timed(c, s, "tk_k_stream_row", [&] {
        drows_by_type(p.flags, [&](auto m) {
            hipLaunchKernelGGL(tk_k_stream_row<decltype(m)::value>, grid_row, dim3(64 * TK_STREAM_ROWS_WG), lds, s, d_ids, d_begin, d_end, p, op, d_sel, c->t_dec.as<uint2>(), c->n_dec,
                               c->D.tok_bytes, c->D.spec_bytes, st->set.as<uint32_t>(), st->mode, st->cap, cur, next, st->scratch.as<uint8_t>(), st->slot, len, chars, words);
        });
    }));
    uint64_t* doc = st->doc.as<uint64_t>();
    uint32_t* out = st->out.as<uint32_t>();
    TRY(timed(c, s, "tk_k_stream_pack", [&] {
        hipLaunchKernelGGL(tk_k_stream_pack, grid_pack, dim3(TK_STREAM_PACK_BLOCK), 0, s, st->R, len, chars, next, st->scratch.as<uint8_t>(), st->slot, words,
                           st->text.as<uint8_t>(), doc, doc + (st->R + 1), out, out + st->R);
    }));
    unsigned long long* got = st->h_words.p + 8;
    HIPCHK(hipMemcpyAsync(got, words, TK_STREAM_WORDS * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    if (got[TK_STREAM_BAD_ROW] != ~0ull)
        return fail(TK_VALUE_ERROR, "begin and end must satisfy begin <= end <= width: row " + std::to_string(got[TK_STREAM_BAD_ROW]) + " does not");
    if (got[TK_STREAM_BAD_ID] != ~0ull) return drows_invalid_token(d_ids, p, got[TK_STREAM_BAD_ID]);
    if (got[TK_STREAM_OVERFLOW]) return fail(TK_RUNTIME_ERROR, "a row of the stream outgrew its buffer");
    st->cur ^= 1;
    st->n_text = got[TK_STREAM_N_TEXT];
    st->n_chars = got[TK_STREAM_N_CHARS];
    st->fetched = false;
    return TK_OK;
}
// the opening of a stream's entries: run(s) under the core's mutex, on its device, the timed launches drained behind it
template <class Run>
static int stream_pass(tk_stream* st, void* stream, Run&& run) {
    if (!st) return fail(TK_VALUE_ERROR, "stream is null");
    return device_pass(st->c, true, stream, run);
}
// rows (null: all) as the byte per row the row kernel takes, in st->in; *d_sel null for all
static int stream_select(tk_stream* st, hipStream_t s, const uint32_t* rows, uint64_t n, const uint8_t** d_sel) {
    *d_sel = nullptr;
    if (!rows) return TK_OK;
    std::vector<uint8_t> sel(st->R + 1, 0);
    for (uint64_t i = 0; i < n; ++i) {
        if (rows[i] >= st->R) return fail(TK_VALUE_ERROR, "row " + std::to_string(rows[i]) + ": the stream has " + std::to_string(st->R) + " rows");
        sel[rows[i]] = 1;
    }
    TRY(ensure(st->in, sel.size()));
    HIPCHK(hipMemcpyAsync(st->in.p, sel.data(), sel.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));  // (sel goes with this frame)
    *d_sel = st->in.as<uint8_t>();
    return TK_OK;
}
// the last accepted call's outputs as host arrays of the stream
static int stream_fetch(tk_stream* st, const uint8_t** text, uint64_t* n_text, const uint64_t** text_off, const uint64_t** char_off, const uint32_t** state,
                        const uint32_t** hit) {
    if (!st->fetched) {
        const StreamView v = stream_view(st);
        st->h_text.resize(st->n_text + 1);
        st->h_text_off.resize(st->R + 1);
        st->h_char_off.resize(st->R + 1);
        st->h_state.resize(st->R + 1);
        st->h_hit.resize(st->R + 1);
        if (st->n_text) HIPCHK(hipMemcpy(st->h_text.data(), v.text, st->n_text, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(st->h_text_off.data(), v.text_off, (st->R + 1) * 8, hipMemcpyDeviceToHost));
        if (v.char_off) HIPCHK(hipMemcpy(st->h_char_off.data(), v.char_off, (st->R + 1) * 8, hipMemcpyDeviceToHost));
        if (st->R) {
            HIPCHK(hipMemcpy(st->h_state.data(), v.state, st->R * 4, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(st->h_hit.data(), v.hit, st->R * 4, hipMemcpyDeviceToHost));
        }
        st->fetched = true;
    }
    if (text) *text = st->h_text.data();
    if (n_text) *n_text = st->n_text;
    if (text_off) *text_off = st->h_text_off.data();
    if (char_off) *char_off = st->mode == TK_U8_BYTES ? nullptr : st->h_char_off.data();
    if (state) *state = st->h_state.data();
    if (hit) *hit = st->h_hit.data();
    return TK_OK;
}

extern "C" void tk_stream_destroy(tk_stream* st) {
    if (!st) return;
    (void)hipSetDevice(st->device);
    delete st;
}
extern "C" int tk_stream_create(tk_core* c, uint64_t n_rows, uint32_t w_max, const tk_drows_spec* spec, const tk_stops* stops, uint32_t stop_flags, uint32_t mode,
                                tk_stream** stream_out) {
    if (!c) return fail(TK_VALUE_ERROR, "core is null");
    if (!stream_out) return fail(TK_VALUE_ERROR, "null argument");
    TRY(until_mode_check(mode));
    TkStopSet set;
    TRY(stops_check(stops, stop_flags, &set));
    TkDrows p;
    TRY(drows_check_spec(c, spec, n_rows, w_max, w_max, &p));
    const uint64_t max_tok = std::max<uint64_t>(c->H.max_token_len, c->spec_max_len);
    switch (tk_stream_shape(n_rows, w_max, max_tok, mode)) {
        case 0: break;
        case 1: return fail(TK_VALUE_ERROR, "w_max must be 1 .. 64: decode wider matrices with decode_rows_until");
        case 2: return fail(TK_VALUE_ERROR, "more than 65536 rows in a stream");
        case 3:
            return fail(TK_VALUE_ERROR, "w_max = " + std::to_string(w_max) + " columns of tokens of up to " + std::to_string(max_tok) +
                                            " bytes do not fit a row's buffer on the device: use decode_rows_until for such input");
        default: return fail(TK_VALUE_ERROR, "mode must be TK_U8_REPLACE, TK_U8_IGNORE or TK_U8_BYTES");
    }
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHK(hipSetDevice(c->device));
    std::unique_ptr<tk_stream, void (*)(tk_stream*)> st(new tk_stream, tk_stream_destroy);
    st->c = c;
    st->device = c->device;
    st->R = n_rows;
    st->w_max = w_max;
    st->mode = mode;
    st->spec = *spec;
    st->dtype = spec->flags & (TK_DROWS_I32 | TK_DROWS_I64);
    const uint64_t cap = tk_stream_cap(w_max, max_tok);
    st->cap = (uint32_t)((cap + 15) & ~15ull);
    st->slot = tk_stream_slot(cap, mode);
    HIPCHK(st->h_words.alloc(16 * 8, hipHostMallocDefault));
    const unsigned long long start[TK_STREAM_WORDS] = {~0ull, ~0ull, 0, 0, 0};
    memcpy(st->h_words.p, start, sizeof start);
    for (Buf& b : st->rows) {
        TRY(ensure(b, n_rows * sizeof(TkStreamRow) + 16));
        HIPCHK(hipMemset(b.p, 0, n_rows * sizeof(TkStreamRow) + 16));
    }
    TRY(upload(st->set, &set, sizeof set));
    TRY(ensure(st->scratch, n_rows * st->slot + 16));
    TRY(ensure(st->text, n_rows * st->slot + 16));
    TRY(ensure(st->len, 2 * n_rows * 4 + 16));
    TRY(ensure(st->doc, 2 * (n_rows + 1) * 8));
    TRY(ensure(st->out, 2 * n_rows * 4 + 16));
    TRY(ensure(st->words, TK_STREAM_WORDS * 8));
    TRY(drained(c, [&] { return stream_run(st.get(), c->stream, TK_STREAM_OP_RESET, nullptr, 0, 0, nullptr, nullptr, nullptr); }));
    *stream_out = st.release();
    return TK_OK;
}
extern "C" int tk_stream_dtype(tk_stream* st, uint32_t dtype_flags) {
    if (!st) return fail(TK_VALUE_ERROR, "stream is null");
    if ((dtype_flags & ~(TK_DROWS_I32 | TK_DROWS_I64)) || dtype_flags == (TK_DROWS_I32 | TK_DROWS_I64)) return fail(TK_VALUE_ERROR, "dtype: 0, TK_DROWS_I32 or TK_DROWS_I64");
    std::lock_guard<std::mutex> lk(st->c->mu);
    st->dtype = dtype_flags;
    return TK_OK;
}
extern "C" int tk_stream_step_device(tk_stream* st, const void* d_ids, uint64_t width, uint64_t ld, const void* d_begin, const void* d_end, void* stream,
                                     const uint8_t** d_text_out, uint64_t* n_text_out, const uint64_t** d_text_off_out, const uint64_t** d_char_off_out,
                                     const uint32_t** d_state_out, const uint32_t** d_hit_out) {
    TRY(stream_pass(st, stream, [&](hipStream_t s) {
        return stream_run(st, s, TK_STREAM_OP_STEP, d_ids, width, ld, (const uint32_t*)d_begin, (const uint32_t*)d_end, nullptr);
    }));
    const StreamView v = stream_view(st);
    if (d_text_out) *d_text_out = v.text;
    if (n_text_out) *n_text_out = st->n_text;
    if (d_text_off_out) *d_text_off_out = v.text_off;
    if (d_char_off_out) *d_char_off_out = v.char_off;
    if (d_state_out) *d_state_out = v.state;
    if (d_hit_out) *d_hit_out = v.hit;
    return TK_OK;
}
extern "C" int tk_stream_fetch(tk_stream* st, const uint8_t** text_out, uint64_t* n_text_out, const uint64_t** text_off_out, const uint64_t** char_off_out,
                               const uint32_t** state_out, const uint32_t** hit_out) {
    return stream_pass(st, nullptr, [&](hipStream_t) { return stream_fetch(st, text_out, n_text_out, text_off_out, char_off_out, state_out, hit_out); });
}
extern "C" int tk_stream_step(tk_stream* st, const void* ids, uint64_t width, uint64_t ld, const uint32_t* begin, const uint32_t* end, const uint8_t** text_out,
                              uint64_t* n_text_out, const uint64_t** text_off_out, const uint64_t** char_off_out, const uint32_t** state_out, const uint32_t** hit_out) {
    return stream_pass(st, nullptr, [&](hipStream_t s) -> int {
        if (width > st->w_max) return fail(TK_VALUE_ERROR, "a step of " + std::to_string(width) + " columns: the stream was created with w_max = " + std::to_string(st->w_max));
        if (ld < width) return fail(TK_VALUE_ERROR, "ld must be at least the width");
        if (!ids && st->R && width) return fail(TK_VALUE_ERROR, "null argument");
        const uint64_t R = st->R, es = tk_drows_elem_size(st->dtype), n_elems = R && width ? (R - 1) * ld + width : 0;
        if (ld >= (1ull << 40)) return fail(TK_VALUE_ERROR, "the matrix spans 2^60 elements or more");
        Carve in;
        const uint64_t at_ids = in.add(n_elems * es), at_begin = in.add(R * 4), at_end = in.add(R * 4);
        TRY(ensure(st->in, in.total + 16));
        if (n_elems) HIPCHK(hipMemcpyAsync(carved<void>(st->in, at_ids), ids, n_elems * es, hipMemcpyHostToDevice, s));
        if (begin && R) HIPCHK(hipMemcpyAsync(carved<void>(st->in, at_begin), begin, R * 4, hipMemcpyHostToDevice, s));
        if (end && R) HIPCHK(hipMemcpyAsync(carved<void>(st->in, at_end), end, R * 4, hipMemcpyHostToDevice, s));
        TRY(stream_run(st, s, TK_STREAM_OP_STEP, carved<void>(st->in, at_ids), width, ld, begin ? carved<uint32_t>(st->in, at_begin) : nullptr,
                       end ? carved<uint32_t>(st->in, at_end) : nullptr, nullptr));
        return stream_fetch(st, text_out, n_text_out, text_off_out, char_off_out, state_out, hit_out);
    });
}
extern "C" int tk_stream_flush(tk_stream* st, const uint32_t* rows, uint64_t n_listed, const uint8_t** text_out, uint64_t* n_text_out, const uint64_t** text_off_out,
                               const uint64_t** char_off_out, const uint32_t** state_out, const uint32_t** hit_out) {
    return stream_pass(st, nullptr, [&](hipStream_t s) -> int {
        const uint8_t* d_sel;
        TRY(stream_select(st, s, rows, n_listed, &d_sel));
        TRY(stream_run(st, s, TK_STREAM_OP_FLUSH, nullptr, 0, 0, nullptr, nullptr, d_sel));
        return stream_fetch(st, text_out, n_text_out, text_off_out, char_off_out, state_out, hit_out);
    });
}
extern "C" int tk_stream_reset(tk_stream* st, const uint32_t* rows, uint64_t n_listed) {
    return stream_pass(st, nullptr, [&](hipStream_t s) -> int {
        const uint8_t* d_sel;
        TRY(stream_select(st, s, rows, n_listed, &d_sel));
        return stream_run(st, s, TK_STREAM_OP_RESET, nullptr, 0, 0, nullptr, nullptr, d_sel);
    });
}
extern "C" int tk_stream_rows(tk_stream* st, uint32_t* state, uint32_t* hit, uint64_t* n_kept, uint64_t* n_text, uint64_t* n_chars) {
    return stream_pass(st, nullptr, [&](hipStream_t) -> int {
        std::vector<TkStreamRow> rows(st->R + 1);
        if (st->R) HIPCHK(hipMemcpy(rows.data(), st->rows[st->cur].p, st->R * sizeof(TkStreamRow), hipMemcpyDeviceToHost));
        for (uint64_t r = 0; r < st->R; ++r) {
            if (state) state[r] = rows[r].state;
            if (hit) hit[r] = rows[r].hit;
            if (n_kept) n_kept[r] = rows[r].n_kept;
            if (n_text) n_text[r] = rows[r].n_text;
            if (n_chars) n_chars[r] = rows[r].n_chars;
        }
        return TK_OK;
    });
}

// ------------------------------------------------------------------------------------------
// BPE training (tk_train.h; the rule: include/tiktoken_amd.h).  Every buffer of a call belongs to its TrainRun and goes with it.
// ------------------------------------------------------------------------------------------
struct TrainRun {
    Buf key, weight, first;  // the word table
    uint64_t slots = 0;
    Buf blob;                // the distinct words' bytes
    Buf cells;
    Buf sym[2], wid[2], pos[2], dec, pair, blk_mark, blk_cnt, merges, counts;
    uint64_t pair_slots = 0;
    TkTrainTab tab() const { return TkTrainTab{key.as<unsigned long long>(), weight.as<unsigned long long>(), first.as<unsigned long long>(), slots - 1}; }
    TkTrainStep step(uint32_t k) const {  // merge k: it reads the symbol arrays of set k & 1
        return TkTrainStep{.sym = {sym[0].as<uint32_t>(), sym[1].as<uint32_t>()},
                           .wid = {wid[0].as<uint32_t>(), wid[1].as<uint32_t>()},
                           .pos = {pos[0].as<unsigned long long>(), pos[1].as<unsigned long long>()},
                           .weight = weight.as<unsigned long long>(), .pair = pair.as<TkTrainPair>(), .pair_mask = pair_slots - 1, .dec = dec.as<uint8_t>(),
                           .blk_mark = blk_mark.as<uint32_t>(), .blk_cnt = blk_cnt.as<unsigned long long>(), .cells = cells.as<unsigned long long>(),
                           .merges = merges.as<uint32_t>(), .counts = counts.as<unsigned long long>(), .step = k, .par = k & 1u};
    }
};
// the slots of a hash table: the power of two times `floor` that is at least x
static uint64_t pow2_at_least(uint64_t floor, uint64_t x) {
    while (floor < x) floor <<= 1;
    return floor;
}

static int train_tab_alloc(tk_core* c, hipStream_t s, TrainRun& r, uint64_t slots) {
    TRY(ensure(r.key, slots * 8));
    TRY(ensure(r.weight, slots * 8));
    TRY(ensure(r.first, slots * 8));
    r.slots = slots;
    return timed(c, s, "tk_k_train_tab_init", [&] { hipLaunchKernelGGL(tk_k_train_tab_init, dim3(grid_for(slots, 256, 65536)), dim3(256), 0, s, r.tab()); });
}

// room for `words` distinct words at a load of at most one half: the slot count follows from the number of pieces, known before they go in
static int train_tab_reserve(tk_core* c, hipStream_t s, TrainRun& r, uint64_t words) {
    const uint64_t want = pow2_at_least(1024, 2 * words);
    if (want <= r.slots) return TK_OK;
    if (want > (1ull << 32)) return fail(TK_VALUE_ERROR, "tk_train_bpe: more than 2^31 pieces");
    if (!r.slots) return train_tab_alloc(c, s, r, want);
    TrainRun old;
    std::swap(old.key, r.key);
    std::swap(old.weight, r.weight);
    std::swap(old.first, r.first);
    old.slots = r.slots;
    TRY(train_tab_alloc(c, s, r, want));
    TRY(timed(c, s, "tk_k_train_rehash", [&] {
        hipLaunchKernelGGL(tk_k_train_rehash, dim3(grid_for(old.slots, 256, 65536)), dim3(256), 0, s, old.tab(), r.tab(), r.blob.as<uint8_t>(), (uint64_t)TK_HASH_SEED,
                           r.cells.as<unsigned long long>());
    }));
    HIPCHK(hipStreamSynchronize(s));  // (the old table goes with `old`)
    c->st_train_table_moves += 1;
    return TK_OK;
}

static int train_blob_reserve(tk_core* c, hipStream_t s, TrainRun& r, uint64_t used, uint64_t bytes) {
    if (bytes <= r.blob.cap && r.blob.p) return TK_OK;
    Buf bigger;
    TRY(ensure(bigger, bytes + bytes / 2));
    if (used) {
        HIPCHK(hipMemcpyAsync(bigger.p, r.blob.p, used, hipMemcpyDeviceToDevice, s));
        c->st_train_blob_moves += 1;
    }
    HIPCHK(hipStreamSynchronize(s));
    r.blob = std::move(bigger);
    return TK_OK;
}

// The word table, chunk by chunk: document ranges [d0, d1) of at most `limit` bytes; offsets stay global (doc_off[d0] + place in the chunk).
// `cells`: the host's copy of the run's cells, as they stand behind the last chunk (cells[TKT_BLOB]: the bytes of the distinct words).
static int train_words(tk_core* c, hipStream_t s, TrainRun& r, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, unsigned long long (&cells)[TKT_CELLS]) {
    TRY(ensure(r.cells, TKT_CELLS * 8));
    HIPCHK(hipMemsetAsync(r.cells.p, 0, TKT_CELLS * 8, s));
    unsigned long long* d_cells = r.cells.as<unsigned long long>();
    const uint64_t limit = std::min<uint64_t>(c->chunk_bytes, (1ull << 31) - 4096);  // (bit 31 of a piece start marks a gap char)
    std::vector<uint64_t> local;
    for (uint64_t d0 = 0; d0 < n_docs;) {
        uint64_t d1 = d0;
        while (d1 < n_docs && doc_off[d1 + 1] - doc_off[d0] <= limit) ++d1;
        if (d1 == d0)
            return fail(TK_VALUE_ERROR, "tk_train_bpe: document " + std::to_string(d0) + " has " + std::to_string(doc_off[d0 + 1] - doc_off[d0]) +
                                            " bytes, more than a chunk of " + std::to_string(limit) + ": split it into documents");
        const uint64_t base = doc_off[d0], n = doc_off[d1] - base, nd = d1 - d0;
        if (n) {
            local.resize(nd + 1);
            for (uint64_t d = 0; d <= nd; ++d) local[d] = doc_off[d0 + d] - base;
            TRY(ensure(c->text, n + 256));
            TRY(ensure(c->doc_off, (nd + 2) * 8));
            HIPCHK(hipMemcpyAsync(c->text.p, utf8 + base, n, hipMemcpyHostToDevice, s));
            HIPCHK(hipMemsetAsync((uint8_t*)c->text.p + n, 0, 128, s));
            HIPCHK(hipMemcpyAsync(c->doc_off.p, local.data(), (nd + 1) * 8, hipMemcpyHostToDevice, s));
            uint64_t P = 0;
            const ChunkAsk ask{.kind = ChunkKind::PieceStarts, .d_text = c->text.as<uint8_t>(), .d_doc_off = c->doc_off.as<uint64_t>(), .n = n, .n_docs = nd};
            TRY(run_chunk(c, s, ask, &P));  // (waits: P is known)
            if (P) {
                TRY(train_blob_reserve(c, s, r, cells[TKT_BLOB], cells[TKT_BLOB] + n + 64));
                if ((cells[TKT_BLOB] + n) >> 32) return fail(TK_VALUE_ERROR, "tk_train_bpe: more than 4 GiB of distinct words");
                TRY(train_tab_reserve(c, s, r, cells[TKT_NWORDS] + P));
                const TkTrainTab t = r.tab();
                TRY(timed(c, s, "tk_k_train_words", [&] {
                    hipLaunchKernelGGL(tk_k_train_words, dim3(grid_for(P, 256, 65536)), dim3(256), 0, s, c->text.as<uint8_t>(), c->ws[0].pstart.as<uint32_t>(), P, base,
                                       r.blob.as<uint8_t>(), t, (uint64_t)TK_HASH_SEED, d_cells);
                }));
                TRY(timed(c, s, "tk_k_train_blob", [&] {
                    hipLaunchKernelGGL(tk_k_train_blob, dim3(grid_for(r.slots, 256, 65536)), dim3(256), 0, s, c->text.as<uint8_t>(), r.blob.as<uint8_t>(), (uint64_t)r.blob.cap, t,
                                       d_cells);
                }));
                HIPCHK(hipMemcpyAsync(cells, d_cells, sizeof(cells), hipMemcpyDeviceToHost, s));
                HIPCHK(hipStreamSynchronize(s));
                if (cells[TKT_FULL]) return fail(TK_RUNTIME_ERROR, "tk_train_bpe: internal error: the word table or the word blob ran full");
            }
        }
        d0 = d1;
    }
    return TK_OK;
}

// The `steps` merges over the N symbols of the distinct words (a byte each at first), and their pairs and counts into the caller's arrays.
static int train_steps(tk_core* c, hipStream_t s, TrainRun& r, unsigned long long (&cells)[TKT_CELLS], uint64_t steps, uint32_t* pairs, uint64_t* counts) {
    const uint64_t N = cells[TKT_BLOB];
    if (N < 2) return fail(TK_VALUE_ERROR, "tk_train_bpe: no pair left to merge after 0 of " + std::to_string(steps) + " merges: the text has no piece of two bytes");
    // The symbol arrays (two sets: a step writes its survivors into the other one), the pair table, the per-workgroup words.
    const uint64_t nb = (N + TKT_BLOCK - 1) / TKT_BLOCK;
    r.pair_slots = pow2_at_least(1024, 2 * N);
    for (int p = 0; p < 2; ++p) {
        TRY(ensure(r.sym[p], N * 4));
        TRY(ensure(r.wid[p], N * 4));
        TRY(ensure(r.pos[p], N * 8));
    }
    TRY(ensure(r.dec, N));
    TRY(ensure(r.pair, r.pair_slots * sizeof(TkTrainPair)));
    TRY(ensure(r.blk_mark, nb * 4));
    TRY(ensure(r.blk_cnt, nb * 8));
    TRY(ensure(r.merges, steps * 8));
    TRY(ensure(r.counts, steps * 8));
    TRY(timed(c, s, "tk_k_train_expand", [&] {
        hipLaunchKernelGGL(tk_k_train_expand, dim3(grid_for(r.slots, 256, 65536)), dim3(256), 0, s, r.tab(), r.blob.as<uint8_t>(), N, r.sym[0].as<uint32_t>(),
                           r.wid[0].as<uint32_t>(), r.pos[0].as<unsigned long long>());
    }));
    cells[TKT_LIVE] = N;
    cells[TKT_LIVE + 1] = 0;
    cells[TKT_CMAX] = 0;
    cells[TKT_BEST] = ~0ull;
    cells[TKT_WIN] = 0;
    cells[TKT_DONE] = 0;
    HIPCHK(hipMemcpyAsync(r.cells.p, cells, sizeof(cells), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));  // (`cells` is pageable memory and is written again below)

    const dim3 grid((uint32_t)nb), one(1);
    // The merge loop: no host wait inside -- the live count, the winner and the "no pair left" flag stay in the cells.
    for (uint64_t k = 0; k < steps; ++k) {
        const TkTrainStep st = r.step((uint32_t)k);
        TRY(timed(c, s, "tk_train_pair_clear", [&] { (void)hipMemsetAsync(r.pair.p, 0, r.pair_slots * sizeof(TkTrainPair), s); }));
        TRY(timed(c, s, "tk_k_train_count", [&] { hipLaunchKernelGGL(tk_k_train_count, grid, dim3(TKT_BLOCK), 0, s, st); }));
        TRY(timed(c, s, "tk_k_train_best", [&] { hipLaunchKernelGGL(tk_k_train_best, grid, dim3(TKT_BLOCK), 0, s, st); }));
        TRY(timed(c, s, "tk_k_train_pick", [&] { hipLaunchKernelGGL(tk_k_train_pick, grid, dim3(TKT_BLOCK), 0, s, st); }));
        TRY(timed(c, s, "tk_k_train_breaks", [&] { hipLaunchKernelGGL(tk_k_train_breaks, grid, dim3(TKT_BLOCK), 0, s, st); }));
        TRY(timed(c, s, "tk_k_train_carry", [&] { hipLaunchKernelGGL(tk_k_train_carry, one, dim3(1024), 0, s, st); }));
        TRY(timed(c, s, "tk_k_train_decide", [&] { hipLaunchKernelGGL(tk_k_train_decide, grid, dim3(TKT_BLOCK), 0, s, st); }));
        TRY(timed(c, s, "tk_k_train_offsets", [&] { hipLaunchKernelGGL(tk_k_train_offsets, one, dim3(1024), 0, s, st); }));
        TRY(timed(c, s, "tk_k_train_rewrite", [&] { hipLaunchKernelGGL(tk_k_train_rewrite, grid, dim3(TKT_BLOCK), 0, s, st); }));
    }
    HIPCHK(hipMemcpyAsync(cells, r.cells.p, sizeof(cells), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(pairs, r.merges.p, steps * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(counts, r.counts.p, steps * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (cells[TKT_DONE])
        return fail(TK_VALUE_ERROR, "tk_train_bpe: no pair left to merge after " + std::to_string(cells[TKT_DONE] - 1) + " of " + std::to_string(steps) +
                                        " merges: vocab_size is too large for this text");
    return TK_OK;
}

extern "C" int tk_train_bpe(tk_core* c, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, uint32_t vocab_size, uint32_t** pairs_out,
                            uint64_t** counts_out, uint64_t* n_out) {
    if (!c) return fail(TK_VALUE_ERROR, "core is null");
    if (!doc_off || !pairs_out || !counts_out || !n_out) return fail(TK_VALUE_ERROR, "null argument");
    if (vocab_size < 256) return fail(TK_VALUE_ERROR, "vocab_size must be at least 256, so that every byte is a token");
    if (vocab_size > (1u << 30)) return fail(TK_VALUE_ERROR, "vocab_size must be at most 2^30");
    TRY(check_offsets(doc_off, n_docs, "doc_off"));
    const uint64_t steps = vocab_size - 256u;
    HostResult<uint32_t> pairs(malloc(steps * 8 + 8));
    HostResult<uint64_t> counts(malloc(steps * 8 + 8));
    if (!pairs || !counts) return fail(TK_RUNTIME_ERROR, "out of host memory");
    if (steps) {
        if (!utf8 && doc_off[n_docs]) return fail(TK_VALUE_ERROR, "null argument");
        std::lock_guard<std::mutex> lk(c->mu);
        HIPCHK(hipSetDevice(c->device));
        TrainRun r;
        c->st_train_table_moves = c->st_train_blob_moves = 0;
        unsigned long long cells[TKT_CELLS] = {};
        TRY(drained(c, [&] { return train_words(c, c->stream, r, utf8, doc_off, n_docs, cells); }));
        TRY(drained(c, [&] { return train_steps(c, c->stream, r, cells, steps, pairs, counts); }));
    }
    *pairs_out = pairs.release();
    *counts_out = counts.release();
    *n_out = steps;
    return TK_OK;
}

// ------------------------------------------------------------------------------------------
// Several GPUs of one node, one process: the documents of a batch are split into contiguous ranges of about equal
// byte counts (documents never interact: tiktoken/core.py:174-176 maps a pure function), every core encodes its range on its own
// device from its own host thread, and the token ids are gathered in document order -- on the host, or on the first core's device
// through peer copies over xGMI.  No collective on the data path.
// ------------------------------------------------------------------------------------------
// RCCL, loaded on demand (a 570 MB library nobody pays for who uses one GPU): the gather of the several-GPU entry runs on it when the
// group's devices are pairwise distinct -- grouped ncclSend / ncclRecv of the shards' id buffers to the first core's device
// (rccl.h:700-722; a gather with per-rank counts).  Virtual ranks (a device named twice) and a missing library use peer copies.
struct TkRccl {
    void* lib = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    bool tried = false, ok = false;
    bool load() {  // (the answer of the first call, whatever it was: a library without one of the symbols is not asked again)
        if (tried) return ok;
        tried = true;
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (lib) break;
        }
        if (!lib) return false;
        CommInitAll = (decltype(CommInitAll))dlsym(lib, "ncclCommInitAll");
        CommDestroy = (decltype(CommDestroy))dlsym(lib, "ncclCommDestroy");
        GroupStart = (decltype(GroupStart))dlsym(lib, "ncclGroupStart");
        GroupEnd = (decltype(GroupEnd))dlsym(lib, "ncclGroupEnd");
        Send = (decltype(Send))dlsym(lib, "ncclSend");
        Recv = (decltype(Recv))dlsym(lib, "ncclRecv");
        GetErrorString = (decltype(GetErrorString))dlsym(lib, "ncclGetErrorString");
        ok = CommInitAll && CommDestroy && GroupStart && GroupEnd && Send && Recv;
        if (!ok) {
            dlclose(lib);
            lib = nullptr;
        }
        return ok;
    }
};
static TkRccl g_rccl;
static std::mutex g_rccl_mu;

struct tk_group {
    std::vector<tk_core*> cores;
    std::mutex mu;
    Buf root_tokens, root_off, root_raw;  // gathered results on cores[0]'s device; root_raw: the shards' own offsets before rebasing
    std::vector<Stream> gs;               // one copy stream per core, on the core's device (made by the first device gather)
    std::vector<Event> ge;
    std::vector<ncclComm_t> comms;        // RCCL communicators (one per core), empty: peer copies
    bool rccl_tried = false;
    uint64_t gathers_rccl = 0, gathers_peer = 0;
};

extern "C" int tk_group_create(tk_core** cores, uint32_t n, tk_group** out) {
    if (!cores || !out || n == 0) return fail(TK_VALUE_ERROR, "tk_group_create needs at least one core");
    for (uint32_t i = 0; i < n; ++i)
        if (!cores[i]) return fail(TK_VALUE_ERROR, "null core");
    tk_group* g = new tk_group();
    g->cores.assign(cores, cores + n);
    *out = g;
    return TK_OK;
}
extern "C" void tk_group_destroy(tk_group* g) {
    if (!g) return;
    while (!g->gs.empty()) {  // every core's stream and event with its device selected
        (void)hipSetDevice(g->cores[g->gs.size() - 1]->device);
        g->gs.pop_back();
        g->ge.pop_back();
    }
    for (ncclComm_t cm : g->comms)
        if (cm) (void)g_rccl.CommDestroy(cm);
    if (!g->cores.empty()) (void)hipSetDevice(g->cores[0]->device);
    delete g;  // (the gathered results: on the first core's device)
}
extern "C" uint32_t tk_group_size(tk_group* g) { return g ? (uint32_t)g->cores.size() : 0; }
// 1: the device gather of the last tk_group_encode_batch_device ran on RCCL, 0: on peer copies
extern "C" uint64_t tk_group_stat(tk_group* g, const char* name) {
    if (!g || !name) return 0;
    if (!strcmp(name, "gathers_rccl")) return g->gathers_rccl;
    if (!strcmp(name, "gathers_peer")) return g->gathers_peer;
    return 0;
}

// document ranges [first[r], first[r + 1]) of about equal byte counts (contiguous: the order of the results is the order of the input)
static std::vector<uint64_t> partition_by_bytes(const uint64_t* doc_off, uint64_t n_docs, uint32_t parts) {
    std::vector<uint64_t> first(parts + 1, n_docs);
    first[0] = 0;
    const uint64_t total = doc_off[n_docs];
    uint64_t d = 0;
    for (uint32_t r = 1; r < parts; ++r) {
        const uint64_t want = total / parts * r + (total % parts) * r / parts;
        while (d < n_docs && doc_off[d] < want) ++d;
        first[r] = d;
    }
    return first;
}

struct ShardResult {
    int rc = TK_OK;
    std::string err;
    uint32_t* tokens = nullptr;
    uint64_t n_tokens = 0;
    std::vector<uint64_t> tok_off;
    tk_special_hit hit{};  // (a checked call, rc == TK_DISALLOWED_SPECIAL) in the shard's own document numbers
};

// every core encodes its document range from its own host thread; on_device: the ids stay in each core's out_tokens / out_tok_off
static int group_encode(tk_group* g, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, int use_special, const uint32_t* allowed_ids,
                        uint64_t n_allowed, std::vector<ShardResult>& res, std::vector<uint64_t>& first, bool on_device, const CheckArgs* chk = nullptr) {
    if (!g) return fail(TK_VALUE_ERROR, "group is null");
    if (chk && chk->n && !chk->hit) return fail(TK_VALUE_ERROR, "null argument");
    if (!doc_off) return fail(TK_VALUE_ERROR, "null argument");
    TRY(check_offsets(doc_off, n_docs, "doc_off"));
    const uint32_t R = (uint32_t)g->cores.size();
    first = partition_by_bytes(doc_off, n_docs, R);
    res.assign(R, ShardResult());
    std::vector<std::thread> th;
    for (uint32_t r = 0; r < R; ++r) {
        th.emplace_back([&, r]() {
            const uint64_t d0 = first[r], nd = first[r + 1] - d0;
            std::vector<uint64_t> off(nd + 1);
            for (uint64_t k = 0; k <= nd; ++k) off[k] = doc_off[d0 + k] - doc_off[d0];
            ShardResult& o = res[r];
            if (!on_device) o.tok_off.assign(nd + 1, 0);
            const CheckArgs shard_chk{chk ? chk->ids : nullptr, chk ? chk->n : 0, &o.hit};
            o.rc = encode_batch_impl(g->cores[r], utf8 + doc_off[d0], off.data(), nd, use_special, allowed_ids, n_allowed, &o.tokens, &o.n_tokens,
                                     on_device ? nullptr : o.tok_off.data(), on_device, false, shard_chk.n ? &shard_chk : nullptr);
            if (o.rc != TK_OK) o.err = tk_last_error();  // (thread-local message of this worker)
        });
    }
    for (auto& t : th) t.join();
    for (uint32_t r = 0; r < R; ++r)
        if (res[r].rc != TK_OK) {
            const int rc = res[r].rc;
            std::string msg = "device " + std::to_string(g->cores[r]->device) + ": " + res[r].err;
            if (rc == TK_DISALLOWED_SPECIAL) {  // shards are document ranges in order: the first shard that reports one holds the batch's first
                *chk->hit = res[r].hit;
                chk->hit->doc += first[r];
                msg = "disallowed special token " + std::to_string(chk->hit->id) + " in document " + std::to_string(chk->hit->doc) + " at byte " + std::to_string(chk->hit->pos);
            }
            for (auto& o : res) tk_free(o.tokens);
            return fail(rc, msg);
        }
    return TK_OK;
}

// Encoding.encode_ordinary_batch / encode_batch over several GPUs; same contract as tk_encode_batch.
static int group_encode_batch_impl(tk_group* g, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, int use_special, const uint32_t* allowed_ids,
                                   uint64_t n_allowed, uint32_t** tokens_out, uint64_t* n_tokens_out, uint64_t* tok_off_out, const CheckArgs* chk) {
    if (!tokens_out || !n_tokens_out) return fail(TK_VALUE_ERROR, "null argument");
    if (!g) return fail(TK_VALUE_ERROR, "group is null");
    std::lock_guard<std::mutex> lk(g->mu);
    std::vector<ShardResult> res;
    std::vector<uint64_t> first;
    TRY(group_encode(g, utf8, doc_off, n_docs, use_special, allowed_ids, n_allowed, res, first, false, chk));
    uint64_t total = 0;
    std::vector<uint64_t> base(res.size() + 1, 0);
    for (size_t r = 0; r < res.size(); ++r) {
        base[r] = total;
        total += res[r].n_tokens;
    }
    uint32_t* host = (uint32_t*)malloc((total ? total : 1) * 4);
    if (!host) {
        for (auto& o : res) tk_free(o.tokens);
        return fail(TK_RUNTIME_ERROR, "out of host memory");
    }
    std::vector<std::thread> th;
    for (size_t r = 0; r < res.size(); ++r)
        th.emplace_back([&, r]() {
            if (res[r].n_tokens) memcpy(host + base[r], res[r].tokens, res[r].n_tokens * 4);
            if (tok_off_out)
                for (uint64_t k = 0; k + 1 < res[r].tok_off.size() || (r + 1 == res.size() && k < res[r].tok_off.size()); ++k)
                    tok_off_out[first[r] + k] = base[r] + res[r].tok_off[k];
            tk_free(res[r].tokens);
        });
    for (auto& t : th) t.join();
    *tokens_out = host;
    *n_tokens_out = total;
    return TK_OK;
}

extern "C" int tk_group_encode_batch(tk_group* g, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, int use_special,
                                     const uint32_t* allowed_ids, uint64_t n_allowed, uint32_t** tokens_out, uint64_t* n_tokens_out,
                                     uint64_t* tok_off_out) {
    return group_encode_batch_impl(g, utf8, doc_off, n_docs, use_special, allowed_ids, n_allowed, tokens_out, n_tokens_out, tok_off_out, nullptr);
}
// ... with the disallowed special tokens checked on every shard's device: the hit with the lowest document index, in the batch's numbering
extern "C" int tk_group_encode_batch_checked(tk_group* g, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, int use_special,
                                             const uint32_t* allowed_ids, uint64_t n_allowed, uint32_t** tokens_out, uint64_t* n_tokens_out,
                                             uint64_t* tok_off_out, const uint32_t* disallowed_ids, uint64_t n_disallowed, tk_special_hit* hit) {
    const CheckArgs chk{disallowed_ids, n_disallowed, hit};
    return group_encode_batch_impl(g, utf8, doc_off, n_docs, use_special, allowed_ids, n_allowed, tokens_out, n_tokens_out, tok_off_out, &chk);
}

// raw[0 .. n]: a shard's own token offsets; out[k] = raw[k] + base for its documents (k < n), and out[n] as well when `last`
__global__ __launch_bounds__(256) void tk_k_group_rebase(const uint64_t* __restrict__ raw, uint64_t n, uint64_t base, uint64_t* __restrict__ out, int last) {
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (k < n || (last && k == n)) out[k] = raw[k] + base;
}

// The same with the results gathered on the FIRST core's device and nothing but the text crossing PCIe: every core encodes its shard with
// the ids left on its own device, then all shards travel to the first device at the same time -- RCCL send / recv over xGMI when the
// devices are distinct, concurrent peer copies (one stream per source device) otherwise -- and their document offsets are rebased
// there.  *d_tokens_out / *d_tok_off_out are owned by the group (valid until its next call).
extern "C" int tk_group_encode_batch_device(tk_group* g, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, int use_special,
                                            const uint32_t* allowed_ids, uint64_t n_allowed, const uint32_t** d_tokens_out,
                                            uint64_t* n_tokens_out, const uint64_t** d_tok_off_out) {
    if (!d_tokens_out || !n_tokens_out) return fail(TK_VALUE_ERROR, "null argument");
    if (!g) return fail(TK_VALUE_ERROR, "group is null");
    std::lock_guard<std::mutex> lk(g->mu);
    std::vector<ShardResult> res;
    std::vector<uint64_t> first;
    TRY(group_encode(g, utf8, doc_off, n_docs, use_special, allowed_ids, n_allowed, res, first, true));
    const size_t R = res.size();
    uint64_t total = 0;
    std::vector<uint64_t> base(R + 1, 0);
    for (size_t r = 0; r < R; ++r) {
        base[r] = total;
        total += res[r].n_tokens;
    }
    tk_core* root = g->cores[0];
    if (g->gs.empty()) {  // (the group gets them when all have been made: a first use that failed half-way is repeated by the next call)
        std::vector<Stream> gs(R);
        std::vector<Event> ge(R);
        for (size_t r = 0; r < R; ++r) {
            HIPCHK(hipSetDevice(g->cores[r]->device));
            HIPCHK(gs[r].create());
            HIPCHK(ge[r].create());
        }
        g->gs = std::move(gs);
        g->ge = std::move(ge);
    }
    if (!g->rccl_tried) {  // communicators once per group, when no device is named twice
        g->rccl_tried = true;
        std::vector<int> devs;
        bool distinct = R > 1 && !getenv("TIKTOKEN_AMD_NO_RCCL");
        for (size_t r = 0; r < R; ++r) {
            for (int d : devs) distinct = distinct && d != g->cores[r]->device;
            devs.push_back(g->cores[r]->device);
        }
        if (distinct) {
            std::lock_guard<std::mutex> lr(g_rccl_mu);
            if (g_rccl.load()) {
                g->comms.assign(R, nullptr);
                if (g_rccl.CommInitAll(g->comms.data(), (int)R, devs.data()) != ncclSuccess) g->comms.clear();
            }
        }
    }
    HIPCHK(hipSetDevice(root->device));
    TRY(ensure(g->root_tokens, (total + 1) * 4));
    TRY(ensure(g->root_off, (n_docs + 2) * 8));
    TRY(ensure(g->root_raw, (n_docs + R + 2) * 8));
    uint32_t* rt = g->root_tokens.as<uint32_t>();
    uint64_t* raw = g->root_raw.as<uint64_t>();
    bool by_rccl = !g->comms.empty();
    if (by_rccl) {
        ncclResult_t nr = g_rccl.GroupStart();
        for (size_t r = 1; r < R && nr == ncclSuccess; ++r) {
            if (!res[r].n_tokens) continue;
            (void)hipSetDevice(g->cores[r]->device);
            nr = g_rccl.Send(g->cores[r]->out_tokens.p, res[r].n_tokens, ncclUint32, 0, g->comms[r], g->gs[r]);
            (void)hipSetDevice(root->device);
            if (nr == ncclSuccess) nr = g_rccl.Recv(rt + base[r], res[r].n_tokens, ncclUint32, (int)r, g->comms[0], g->gs[0]);
        }
        const ncclResult_t ne = g_rccl.GroupEnd();
        if (nr == ncclSuccess) nr = ne;
        if (nr != ncclSuccess)
            return fail(TK_RUNTIME_ERROR, std::string("RCCL gather failed: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(nr) : "?"));
        HIPCHK(hipSetDevice(root->device));
        if (res[0].n_tokens) HIPCHK(hipMemcpyAsync(rt, root->out_tokens.p, res[0].n_tokens * 4, hipMemcpyDeviceToDevice, g->gs[0]));
        ++g->gathers_rccl;
    }
    for (size_t r = 0; r < R; ++r) {  // offsets (and, without RCCL, the ids): one peer copy per shard, each on its source device's stream
        tk_core* c = g->cores[r];
        const uint64_t nd = first[r + 1] - first[r];
        HIPCHK(hipSetDevice(c->device));
        if (!by_rccl && res[r].n_tokens)
            HIPCHK(hipMemcpyPeerAsync(rt + base[r], root->device, c->out_tokens.p, c->device, res[r].n_tokens * 4, g->gs[r]));
        HIPCHK(hipMemcpyPeerAsync(raw + first[r] + r, root->device, c->out_tok_off.p, c->device, (nd + 1) * 8, g->gs[r]));
        HIPCHK(hipEventRecord(g->ge[r], g->gs[r]));
    }
    if (!by_rccl) ++g->gathers_peer;
    HIPCHK(hipSetDevice(root->device));
    hipStream_t s0 = g->gs[0];
    for (size_t r = 1; r < R; ++r) HIPCHK(hipStreamWaitEvent(s0, g->ge[r], 0));
    for (size_t r = 0; r < R; ++r) {
        const uint64_t nd = first[r + 1] - first[r];
        hipLaunchKernelGGL(tk_k_group_rebase, dim3((uint32_t)((nd + 1 + 255) / 256)), dim3(256), 0, s0, raw + first[r] + r, nd, base[r],
                           g->root_off.as<uint64_t>() + first[r], r + 1 == R ? 1 : 0);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s0));
    *d_tokens_out = rt;
    if (d_tok_off_out) *d_tok_off_out = g->root_off.as<uint64_t>();
    *n_tokens_out = total;
    return TK_OK;
}

extern "C" uint64_t tk_n_tokens(tk_core* c) { return c ? c->H.n_ranks : 0; }

extern "C" int tk_sorted_token(tk_core* c, uint64_t i, const uint8_t** bytes_out, uint64_t* len_out, uint32_t* rank_out) {
    if (!c || i >= c->H.sorted_ranks().size()) return fail(TK_VALUE_ERROR, "index out of range");
    uint32_t r = c->H.sorted_ranks()[i];
    if (rank_out) *rank_out = r;
    return tk_decode_single_token_bytes(c, r, bytes_out, len_out);
}

// token_byte_values() in one call: all token byte strings in lexicographic order, packed (src/lib.rs:648-650, py.rs:178-183).
// The arrays are owned by the core (built on first use) and stay valid until tk_destroy.
extern "C" int tk_sorted_tokens_packed(tk_core* c, const uint8_t** blob_out, const uint64_t** off_out, uint64_t* n_out) {
    if (!c || !blob_out || !off_out || !n_out) return fail(TK_VALUE_ERROR, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->sorted_off.empty()) {
        const TkHostTables& H = c->H;
        c->sorted_off.reserve(H.sorted_ranks().size() + 1);
        c->sorted_off.push_back(0);
        for (uint32_t r : H.sorted_ranks()) {
            const auto& e = *H.find_token(r);
            c->sorted_blob.insert(c->sorted_blob.end(), H.tok_bytes.begin() + e.first, H.tok_bytes.begin() + e.first + e.second);
            c->sorted_off.push_back(c->sorted_blob.size());
        }
        if (c->sorted_blob.empty()) c->sorted_blob.push_back(0);
    }
    *blob_out = c->sorted_blob.data();
    *off_out = c->sorted_off.data();
    *n_out = c->sorted_off.size() - 1;
    return TK_OK;
}

// Vocabulary wire format: the contents of a `.tiktoken` file -> packed arrays in the layout tk_create takes (release each with tk_free).
extern "C" int tk_parse_tiktoken_bpe(const uint8_t* text, uint64_t len, uint8_t** blob_out, uint64_t** off_out, uint32_t** ids_out,
                                     uint64_t* n_out) {
    if (!blob_out || !off_out || !ids_out || !n_out || (!text && len)) return fail(TK_VALUE_ERROR, "null argument");
    std::vector<uint8_t> blob;
    std::vector<uint64_t> off;
    std::vector<uint32_t> ids;
    const std::string err = tk_parse_tiktoken(text, len, &blob, &off, &ids);
    if (!err.empty()) return fail(TK_VALUE_ERROR, err);
    uint8_t* b = (uint8_t*)malloc(blob.size() ? blob.size() : 1);
    uint64_t* o = (uint64_t*)malloc(off.size() * 8);
    uint32_t* r = (uint32_t*)malloc(ids.size() ? ids.size() * 4 : 4);
    if (!b || !o || !r) {
        free(b);
        free(o);
        free(r);
        return fail(TK_RUNTIME_ERROR, "out of host memory");
    }
    if (!blob.empty()) memcpy(b, blob.data(), blob.size());
    memcpy(o, off.data(), off.size() * 8);
    if (!ids.empty()) memcpy(r, ids.data(), ids.size() * 4);
    *blob_out = b;
    *off_out = o;
    *ids_out = r;
    *n_out = ids.size();
    return TK_OK;
}

extern "C" void tk_free(void* p) {
    if (!pinned_release(p)) free(p);
}

// Well-formed UTF-8 (Unicode 15, table 3-7): what the reference gets for free from &str.  Eight ASCII bytes per step where there are any.
extern "C" int tk_validate_utf8(const uint8_t* s, uint64_t n, uint64_t* bad_pos) {
    if (!s && n) return fail(TK_VALUE_ERROR, "null argument");
    uint64_t i = 0;
    auto bad = [&](uint64_t at) {
        if (bad_pos) *bad_pos = at;
        return fail(TK_VALUE_ERROR, "invalid UTF-8 at byte " + std::to_string(at));
    };
    while (i < n) {
        if (i + 8 <= n) {
            uint64_t w;
            memcpy(&w, s + i, 8);
            if (!(w & 0x8080808080808080ull)) {
                i += 8;
                continue;
            }
        }
        const uint8_t b = s[i];
        if (b < 0x80) {
            ++i;
            continue;
        }
        uint32_t need;
        uint8_t lo = 0x80, hi = 0xBF;  // bounds of the second byte
        if (b >= 0xC2 && b <= 0xDF) need = 1;
        else if (b >= 0xE0 && b <= 0xEF) {
            need = 2;
            if (b == 0xE0) lo = 0xA0;       // no overlong three-byte forms
            else if (b == 0xED) hi = 0x9F;  // no surrogates
        } else if (b >= 0xF0 && b <= 0xF4) {
            need = 3;
            if (b == 0xF0) lo = 0x90;       // no overlong four-byte forms
            else if (b == 0xF4) hi = 0x8F;  // nothing above U+10FFFF
        } else return bad(i);               // a continuation byte, 0xC0, 0xC1, 0xF5..0xFF
        if (i + need >= n) return bad(i);  // truncated
        if (s[i + 1] < lo || s[i + 1] > hi) return bad(i);
        for (uint32_t k = 2; k <= need; ++k)
            if ((s[i + k] & 0xC0) != 0x80) return bad(i);
        i += need + 1;
    }
    return TK_OK;
}

extern "C" int tk_set_output_buffers(tk_core* c, uint32_t n) {
    if (!c) return fail(TK_VALUE_ERROR, "core is null");
    if (n != 1 && n != 2) return fail(TK_VALUE_ERROR, "tk_set_output_buffers: 1 or 2");
    std::lock_guard<std::mutex> lk(c->mu);
    c->out_bufs = n;
    return TK_OK;
}

extern "C" void tk_set_profiling(tk_core* c, int enabled) {
    if (c) c->profiling = enabled != 0;
}
extern "C" void tk_reset_kernel_ms(tk_core* c) {
    if (c) c->stats.clear();
}
extern "C" int tk_get_kernel_ms(tk_core* c, const char* name, double* ms_out, uint64_t* launches_out) {
    if (!c) return TK_VALUE_ERROR;
    auto it = c->stats.find(name);
    if (it == c->stats.end()) {
        if (ms_out) *ms_out = 0;
        if (launches_out) *launches_out = 0;
        return TK_KEY_ERROR;
    }
    if (ms_out) *ms_out = it->second.ms;
    if (launches_out) *launches_out = it->second.launches;
    return TK_OK;
}
extern "C" void tk_last_stats(tk_core* c, uint64_t* n_bytes, uint64_t* n_pieces, uint64_t* n_tokens, uint64_t* n_docs,
                              uint64_t* n_medium, uint64_t* n_long) {
    if (!c) return;
    if (n_bytes) *n_bytes = c->st_bytes;
    if (n_pieces) *n_pieces = c->st_pieces;
    if (n_tokens) *n_tokens = c->st_tokens;
    if (n_docs) *n_docs = c->st_docs;
    if (n_medium) *n_medium = c->st_medium;
    if (n_long) *n_long = c->st_long;
}
extern "C" uint64_t tk_stat(tk_core* c, const char* name) {
    if (!c || !name) return 0;
    const std::string k(name);
    if (k == "front_wgs_per_cu") return TKF_OCC;  // (workgroups per CU of the persistent front kernel: a compile-time constant)
    if (k == "compute_units") return c->n_cu;
    if (k == "chunks") return c->st_chunks;
    if (k == "small_launches") return c->st_small_launches;  // launches of tk_k_small and the calls they carried (several callers share a launch)
    if (k == "small_calls") return c->st_small_calls;
    if (k == "mid_calls") return c->st_mid_calls;  // documents of 2 .. 128 KiB encoded as segments in one launch
    if (k == "back_streams") return (uint64_t)c->n_back;  // streams found to run beside the front stream (0: no multi-chunk batch yet)
    if (k == "resynced") return c->st_resynced;  // batches repeated because a deferred tile gave up while the host was not waiting (stage_deferred)
    if (k == "spec_find_launches") return c->st_find_launches;  // launches of the disallowed scan (tk_k_spec_find) since the core was made: one per chunk of a checked call
    if (k == "spec_mark_launches") return c->st_mark_launches;  // launches of the pair that marks allowed special tokens (tk_k_spec_cand + tk_k_spec_resolve): one per chunk that has them
    if (k == "train_table_moves") return c->st_train_table_moves;  // of the last tk_train_bpe: launches of tk_k_train_rehash (train_tab_reserve)
    if (k == "train_blob_moves") return c->st_train_blob_moves;    // ... and copies of the words' bytes into a larger blob (train_blob_reserve)
    if (k == "split_segments") return c->st_split[TK_SPLIT_ST_SEGS];          // of the last split call: document parts per block of K positions the walk pass walked
    if (k == "split_joined") return c->st_split[TK_SPLIT_ST_JOINED];          // ... blocks in which the true chain met the speculative walk
    if (k == "split_stitch_steps") return c->st_split[TK_SPLIT_ST_STITCH];    // ... steps of the stitch pass (one wavefront per document, in order)
    if (k == "split_spec_steps") return c->st_split[TK_SPLIT_ST_SPEC];        // ... steps of the speculative walks
    if (k == "fingerprint_tile") return TK_FP_TILE;  // token positions of a tile of the fingerprint pass (tk_fingerprint_rule.h)
    if (k == "jsonl_tile") return TK_JSONL_TILE;  // bytes of a tile of the JSON Lines passes (tk_jsonl_rule.h)
    if (k == "regrown") return c->st_regrown;  // batches repeated with a larger miss data since the core was made (encode_device_locked)
    if (k == "workspace_bytes") {             // device memory of the work sets (everything but the text, the tables and the outputs)
        uint64_t t = 0;
        for (auto& w : c->ws) t += w.bytes();
        return t;
    }
    // (experiments) the deferred tiles of the last chunk of work set 0: "deferred_count", "deferred_tile_<i>" (read from the device: the caller has waited for the call)
    if (k == "deferred_count") return c->ws[0].h_counters ? c->ws[0].h_counters[TK_CNT_N + TK_CNT_DEFER] : 0;
    if (k.rfind("deferred_tile_", 0) == 0) {
        uint32_t v = 0;
        const uint64_t i = strtoull(k.c_str() + 14, nullptr, 10);
        if (c->ws[0].deferred.p && (i + 1) * 4 <= c->ws[0].deferred.cap && hipMemcpy(&v, c->ws[0].deferred.as<uint32_t>() + i, 4, hipMemcpyDeviceToHost) != hipSuccess) v = 0xFFFFFFFFu;
        return v;
    }
    if (k == "fallbacks") return c->st_fallbacks;  // chunks re-split by the generic engine since the core was made (stage_deferred)
    if (k == "host_front_us") return (uint64_t)c->host_us[0];
    if (k == "host_back_us") return (uint64_t)c->host_us[1];
    if (k == "host_back_wait_us") return (uint64_t)c->host_us[2];
    if (k == "host_finish_us") return (uint64_t)c->host_us[3];
    if (k == "host_tail_us") return (uint64_t)c->host_us[4];
    if (k == "host_total_us") return (uint64_t)c->host_us[5];
    // which device tables the vocabulary's ids left this core with (tk_build_tables, tk_create): tests assert the path they mean to take
    if (k == "pair_table_packed") return c->D.pair8 != nullptr;  // 0: 16-byte slots, and a merge kernel per length bin instead of tk_k_merge_all
    if (k == "short_table") return c->D.short_tab != nullptr;    // 0: tokens of 1..4 bytes live in the mid table
    if (k == "decode_table_ids") return c->n_dec;                // 0: ids too sparse for the device decode table
    if (k == "chunk_bytes") return c->chunk_bytes;
    if (k == "stage_bytes") return TK_STAGE_BYTES;  // a block of text on its way to the device; host-buffer batches of twice that and more are pipelined (encode_batch_impl)
#ifdef TKF_TIMING
    if (k.rfind("time_", 0) == 0) {  // (experiments: tk_fused.h, TKT)
        static unsigned long long acc[2 * 1024 * 16];
        (void)hipSetDevice(c->device);
        (void)hipDeviceSynchronize();
        if (k == "time_reset") {
            memset(acc, 0, sizeof(acc));
            (void)hipMemcpyToSymbol(HIP_SYMBOL(tk_time_acc), acc, sizeof(acc));
            return 0;
        }
        (void)hipMemcpyFromSymbol(acc, HIP_SYMBOL(tk_time_acc), sizeof(acc));
        const bool starts = k.rfind("time_s", 0) == 0;  // ("time_s<i>": the deferred-tile instance)
        const int i = atoi(k.c_str() + (starts ? 6 : 5));
        unsigned long long sum = 0;
        for (int b = 0; b < 1024 && i >= 0 && i < 16; ++b) sum += acc[(starts ? 16384 : 0) + b * 16 + i];
        return sum;
    }
#endif
    return 0;
}
