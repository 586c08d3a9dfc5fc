// The row kernel of the streaming decode (tiktoken_amd/csrc/tk_stream.h) on the CPU: the plain C++ it is made of -- tk_stream_rule.h and
// what that shares with the decode-rows, stop-string and repair passes -- compiled for the host and driven the way the kernel drives it: a
// row is a wavefront of 64 lanes, lane c takes column c, the ballots and prefix sums are loops over the lanes, and the lanes of the search
// and of the repair run in ascending, descending or shuffled order.  The row's bytes are read through a buffer of exactly the bytes the
// row holds, which refuses every other index; every emitted byte goes through a writer that wants it stored exactly once inside the
// bytes the row emits.  Test infrastructure only (tests/test_stream_sim.py builds it).
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <random>
#include <vector>

#include "../../tiktoken_amd/csrc/tk_stream_rule.h"

namespace {
struct Fault {
    int64_t code = 0;  // 1: a byte read outside the row's bytes, 3: a byte stored twice, 4: a store outside the emitted bytes, 5: a byte never stored,
                       // 6: the row outgrew its buffer or its tail
    void set(int64_t c) {
        if (!code) code = c;
    }
};
struct Buf {
    const std::vector<uint8_t>* b;
    Fault* f;
    uint32_t operator()(uint32_t i) const {
        if (i >= b->size()) {
            f->set(1);
            return 0u;
        }
        return (*b)[i];
    }
};
struct Stores {
    std::vector<uint8_t>* out;
    std::vector<uint8_t>* times;
    Fault* f;
    void byte(unsigned long long off, uint8_t v) const {
        if (off >= out->size()) return f->set(4);
        if ((*times)[off]++) f->set(3);
        (*out)[off] = v;
    }
    void word(unsigned long long off, uint64_t v) const {
        if ((off & 7u) || off + 8 > out->size()) return f->set(4);
        for (int k = 0; k < 8; ++k) byte(off + k, (uint8_t)(v >> (8 * k)));
    }
};
struct Dec {  // the id -> {x, y} table
    const uint32_t* d;
    struct E {
        uint32_t x, y;
    };
    E operator[](uint32_t t) const { return E{d[2 * t], d[2 * t + 1]}; }
};
std::vector<uint32_t> lanes_in(uint32_t order, uint64_t seed) {
    std::vector<uint32_t> v(64);
    std::iota(v.begin(), v.end(), 0u);
    if (order == 1) std::reverse(v.begin(), v.end());
    if (order == 2) std::shuffle(v.begin(), v.end(), std::mt19937_64(seed));
    return v;
}
}  // namespace

extern "C" {
uint64_t stream_slot_bytes() { return sizeof(TkStreamRow); }
int32_t stream_shape(uint64_t n_rows, uint64_t w_max, uint64_t max_tok, uint32_t mode) { return tk_stream_shape(n_rows, w_max, max_tok, mode); }

// One row through one call.  op: TK_STREAM_OP_*; chosen: the row is among those a flush or reset names.  row[W]: its columns, widened as
// the kernels widen them; b, e: its begin and end as given (checked here as the kernel checks them).  dec: n_ids pairs {x, y}.  slot: the
// row's slot, replaced by its new one.  out: room for 3 * cap + 16 bytes; res: {bytes emitted, chars emitted, kept ids}.
// Returns 0, a Fault code, 100: begin / end offend (the slot is left as it was), 200 + the column of the first kept id without an entry
// (likewise), 300 + the refusal of the stop set.
int64_t stream_row(uint32_t op, uint32_t chosen, const int64_t* row, uint32_t W, uint32_t b_in, uint32_t e_in, uint32_t flags, uint32_t n_stop, const uint32_t* stop_ids,
                   uint32_t n_skip, const uint32_t* skip_ids, const uint32_t* dec_pairs, uint32_t n_ids, const uint8_t* tok_bytes, const uint8_t* spec_bytes,
                   const uint8_t* blob, const uint32_t* stop_off, uint32_t n_stops, uint32_t stop_flags, uint32_t mode, uint32_t cap, uint32_t order, TkStreamRow* slot,
                   uint8_t* out, uint64_t* res) {
    Fault f;
    TkStopSet set;
    const int why = tk_stops_make(n_stops, blob, stop_off, stop_flags, &set);
    if (why) return 300 + why;
    TkDrows p;
    if (tk_drows_shape(1, W, W, flags, n_stop, stop_ids, n_skip, skip_ids, TK_DEC_BLOCK, &p) || W > TK_STREAM_W_MAX) return 400;
    const Dec dec{dec_pairs};
    const TkStreamRow cur = *slot;
    res[0] = res[1] = res[2] = 0;
    const bool step = op == TK_STREAM_OP_STEP, live = cur.state == TK_STREAM_LIVE && (step || (op == TK_STREAM_OP_FLUSH && chosen));
    if (op == TK_STREAM_OP_RESET && chosen) {
        *slot = TkStreamRow();
        slot->hit = TK_STOPS_NO_HIT;
        return 0;
    }
    if (!live) return 0;  // (the kernel copies the slot)

    // the row rule, a column per lane
    uint32_t b = 0, e = 0;
    const uint32_t begin[1] = {b_in}, end[1] = {e_in};
    if (step && !tk_drows_range(p, begin, true, end, true, 0, &b, &e)) return 100;
    unsigned long long stops = 0, kept = 0, bad = 0;
    uint64_t v[64];
    uint32_t x[64], len[64];
    for (uint32_t c = 0; c < 64; ++c) {
        const bool in = step && c >= b && c < e;
        v[c] = in ? (uint64_t)row[c] : 0ull;  // (nothing outside [b, e) is read)
        if (in && tk_drows_listed(p.stop, p.n_stop, v[c])) stops |= 1ull << c;
    }
    uint32_t live_end;
    tk_drows_stop_col(p, stops ? tk_ctz64(stops) : 0xFFFFFFFFu, e, &live_end);
    for (uint32_t c = 0; c < 64; ++c) {
        const bool in = step && c >= b && c < e;
        x[c] = len[c] = 0;
        const bool keep = in && c < live_end && tk_stream_keep(p, v[c], dec, n_ids, &x[c], &len[c]);
        if (keep) kept |= 1ull << c;
        if (keep && !len[c]) bad |= 1ull << c;
        if (!keep) len[c] = 0;
    }
    if (bad) return 200 + tk_ctz64(bad);
    std::vector<uint8_t> bytes(cur.tail, cur.tail + cur.tail_len);
    for (uint32_t c = 0; c < 64; ++c) {
        const uint8_t* src = ((x[c] & TK_DEC_SPEC) ? spec_bytes : tok_bytes) + (x[c] & ~TK_DEC_SPEC);
        bytes.insert(bytes.end(), src, src + len[c]);
    }
    if (bytes.size() > cap) f.set(6);
    const uint32_t L = (uint32_t)bytes.size();
    const Buf B{&bytes, &f};

    // full hits, the first prefix to hold back, what to emit
    uint32_t best = TK_STOPS_NO_HIT, e0 = L;
    if (step && set.n)
        for (uint32_t lane : lanes_in(order, 1)) {
            uint32_t mine = TK_STOPS_NO_HIT, mine0 = L;
            tk_stream_find_lane(B, L, set, lane, 64u, &mine, &mine0);
            best = std::min(best, mine), e0 = std::min(e0, mine0);
        }
    const TkStreamCut cut = tk_stream_decide(B, L, best, e0, stops != 0, !step, set, mode);
    if (cut.n_emit > L || cut.tail_at > L || L - cut.tail_at > TK_STREAM_HOLD) return 6;

    // the emitted bytes, repaired
    uint32_t n_out = 0, n_ch = 0;
    std::vector<uint8_t> text, times;
    if (mode == TK_STREAM_MODE_BYTES) {
        text.assign(bytes.begin(), bytes.begin() + cut.n_emit);
        n_out = cut.n_emit;
    } else {
        std::vector<TkU8rCounts> counts;  // of every lane of every turn
        for (uint32_t q = 0; q < cut.n_emit; q += 1024u)
            for (uint32_t lane = 0; lane < 64; ++lane) {
                TkU8rNoStream none;
                counts.push_back(tk_stream_emit_lane(B, cut.n_emit, q + 16u * lane, mode, none));
                n_out += counts.back().out, n_ch += counts.back().chars;
            }
        text.assign(n_out, 0);
        times.assign(n_out, 0);
        Stores st{&text, &times, &f};
        for (uint32_t q = 0; q < cut.n_emit; q += 1024u)
            for (uint32_t lane : lanes_in(order, 2 + q)) {
                const size_t mine = (size_t)(q / 1024u) * 64 + lane;
                if (!counts[mine].out) continue;
                unsigned long long at = 0;
                for (size_t i = 0; i < mine; ++i) at += counts[i].out;
                TkU8rStream<Stores> o(st, at);
                (void)tk_stream_emit_lane(B, cut.n_emit, q + 16u * lane, mode, o);
                o.finish();
            }
        for (uint8_t t : times)
            if (t != 1) f.set(t ? 3 : 5);
    }
    if (n_out > 3ull * cap + 16) return 6;
    if (n_out) memcpy(out, text.data(), n_out);
    res[0] = n_out, res[1] = n_ch, res[2] = (uint64_t)__builtin_popcountll(kept);

    TkStreamRow next = TkStreamRow();
    next.state = cut.state, next.hit = cut.hit, next.tail_len = L - cut.tail_at;
    next.n_kept = cur.n_kept + res[2], next.n_text = cur.n_text + n_out, next.n_chars = cur.n_chars + n_ch;
    for (uint32_t i = 0; i < next.tail_len; ++i) next.tail[i] = bytes[cut.tail_at + i];
    if (!f.code) *slot = next;
    return f.code;
}
}
