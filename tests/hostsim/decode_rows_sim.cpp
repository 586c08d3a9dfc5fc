// The decode-rows passes (tiktoken_amd/csrc/tk_decode_rows.h) on the CPU: the plain C++ they are made of -- tk_decode_rows_rule.h: a
// tile's row and columns, a row's begin and end, the stop test and its minimum, the live range, which ids a lane keeps and which of them
// have no decode entry, the stores of a lane, the per-row entry -- compiled for the host and driven the way the kernels drive it: tiles of
// `block` columns per row, lanes of eight, the stop pass with its tiles in ascending or descending order (the result may not depend on it),
// the count pass, the exclusive scan, the host's verdict, the per-row pass, the write pass.  The matrix sits behind a reader that checks every
// index: a read outside the columns [0, W) of a row of the matrix is an error, and so is a token slot written twice or never.  Test
// infrastructure only (tests/test_decode_rows_sim.py builds it: as a shared library, and with -DDECODE_ROWS_SIM_MAIN as a program of its own
// under the address and undefined-behaviour sanitizers, which reads a case file and writes the results).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../tiktoken_amd/csrc/tk_decode_rows_rule.h"
#include "sim_readers.h"

namespace {
// the id -> {offset | TK_DEC_SPEC, length} table, entries [0, n)
struct SimDec {
    struct Entry {
        uint32_t x, y;
    };
    const uint32_t* p;
    uint64_t n;
    bool* oob;
    Entry operator[](uint64_t i) const {
        if (i >= n) {
            *oob = true;
            return Entry{0u, 0u};
        }
        return Entry{p[2 * i], p[2 * i + 1]};
    }
};
// The matrix: element i is counted from (0, 0); it exists when it is a column below W of a row below R.  Eight at once where their address
// is a multiple of 16, as on the device.
struct SimMatrix {
    const uint8_t* p;  // element (0, 0)
    uint64_t R, W, ld;
    uint32_t flags;
    bool* oob;
    bool inside(uint64_t i, uint64_t n) const {
        if (!ld) return false;
        const uint64_t r = i / ld, c = i - r * ld;
        return r < R && c + n <= W;
    }
    uint64_t fetch(uint64_t i) const {
        if (flags & TK_DROWSF_I64) {
            int64_t v;
            memcpy(&v, p + i * 8, 8);
            return (uint64_t)v;
        }
        uint32_t v;
        memcpy(&v, p + i * 4, 4);
        return (flags & TK_DROWSF_I32) ? (uint64_t)(int64_t)(int32_t)v : (uint64_t)v;
    }
    uint64_t one(uint64_t i) const {
        if (!inside(i, 1)) {
            *oob = true;
            return 0;
        }
        return fetch(i);
    }
    bool eight(uint64_t i, uint64_t out[8]) const {
        if ((uintptr_t)(p + i * tk_drows_elem_size(flags)) & 15u) return false;
        if (!inside(i, 8)) {
            *oob = true;
            return false;
        }
        for (int j = 0; j < 8; ++j) out[j] = fetch(i + j);
        return true;
    }
};
// tokens as the lanes fill it: every slot below K exactly once
struct SimOut {
    uint32_t* tokens;
    uint64_t K;
    uint8_t* seen;
    bool *oob, *twice;
    void put(uint64_t i, uint32_t id) const {
        if (i >= K) {
            *oob = true;
            return;
        }
        if (seen[i]) *twice = true;
        seen[i] = 1;
        tokens[i] = id;
    }
};
}  // namespace

extern "C" {
// ids: element (0, 0).  result = {K, first offending row, row-major position of the first kept id without entry}.  Returns 0; 1 .. 8:
// tk_drows_shape's refusal; 16: a row's begin / end offend; 17: a kept id has no entry; 18: K >= 2^32; -1: an index out of bounds; -2: a
// token slot written twice or never; -3: `cap` tokens are too few.  tokens: room for cap; tok_off: R + 1; n_kept, stop_col: R.
int64_t decode_rows_sim(const void* ids, uint64_t R, uint64_t W, uint64_t ld, const uint32_t* begin, const uint32_t* end, uint32_t flags, uint32_t n_stop, const uint32_t* stop,
                        uint32_t n_skip, const uint32_t* skip, const uint32_t* dec, uint32_t n_ids, uint32_t block, uint32_t order, uint64_t* result, uint32_t* tokens,
                        uint64_t cap, uint64_t* tok_off, uint32_t* n_kept, uint32_t* stop_col) {
    TkDrows p;
    const int refused = tk_drows_shape(R, W, ld, flags, n_stop, stop, n_skip, skip, block, &p);
    if (refused) return refused;
    bool oob = false, twice = false;
    const SimMatrix m{(const uint8_t*)ids, R, W, ld, flags, &oob};
    const SimDec d{dec, n_ids, &oob};
    const SimArray<uint32_t> sb{begin, R, &oob}, se{end, R, &oob};
    const uint64_t nt = tk_drows_n_tiles(p);
    unsigned long long words[TK_DROWS_WORDS] = {~0ull, ~0ull, 0};
    std::vector<uint32_t> found(R + 1, 0xFFFFFFFFu);
    std::vector<unsigned long long> cnt(nt + 1, 0);
    auto tile_of = [&](uint64_t k) { return order ? nt - 1 - k : k; };
    // tk_k_drows_stop
    for (uint64_t k = 0; k < nt; ++k) {
        const uint64_t t = tile_of(k);
        uint64_t r, col0;
        uint32_t b, e;
        tk_drows_tile(p, t, block, &r, &col0);
        const bool ok = tk_drows_range(p, sb, begin != nullptr, se, end != nullptr, r, &b, &e);
        if (!ok && col0 == 0) tk_report_min(words + TK_DROWS_BAD_ROW, r);
        uint32_t first = 0xFFFFFFFFu;  // (the wavefront's minimum)
        for (uint32_t th = 0; th < block / 8; ++th) {
            const uint64_t c0 = col0 + th * 8u;
            if (p.n_stop && c0 < p.W) {
                const uint32_t f = tk_drows_stop_lane(p, m, r, c0, b, e);
                first = f < first ? f : first;
            }
        }
        if (first != 0xFFFFFFFFu) tk_drows_stop_min(found.data() + r, first);
    }
    // tk_k_drows_count
    for (uint64_t k = 0; k < nt; ++k) {
        const uint64_t t = tile_of(k);
        uint64_t r, col0;
        uint32_t b, e, live_end;
        tk_drows_tile(p, t, block, &r, &col0);
        tk_drows_range(p, sb, begin != nullptr, se, end != nullptr, r, &b, &e);
        tk_drows_stop_col(p, found[r], e, &live_end);
        unsigned long long tot = 0;
        if (tk_drows_tile_live(col0, block, b, live_end))
            for (uint32_t th = 0; th < block / 8; ++th) {
                const uint64_t c0 = col0 + th * 8u;
                if (c0 < p.W) tot += tk_drows_count_lane(p, m, d, n_ids, r, c0, b, live_end, words);
            }
        cnt[t] = tot;
    }
    // tk_k_drows_scan, and the host behind it
    const uint64_t K = sim_scan(cnt.data(), nt);
    words[TK_DROWS_K] = K;
    result[0] = K;
    result[1] = words[TK_DROWS_BAD_ROW];
    result[2] = words[TK_DROWS_BAD_ID];
    if (oob) return -1;
    if (words[TK_DROWS_BAD_ROW] != ~0ull) return 16;
    if (words[TK_DROWS_BAD_ID] != ~0ull) return 17;
    if (K >> 32) return 18;
    if (K > cap) return -3;
    // tk_k_drows_rows
    const SimArray<unsigned long long> tile_off{cnt.data(), nt, &oob};
    const SimArray<uint32_t> fw{found.data(), R, &oob};
    for (uint64_t r = 0; r <= R; ++r) tk_drows_row_entry(p, tile_off, fw, sb, begin != nullptr, se, end != nullptr, K, r, tok_off, n_kept, stop_col);
    // tk_k_drows_write
    std::vector<uint8_t> seen(K + 1, 0);
    const SimOut out{tokens, K, seen.data(), &oob, &twice};
    for (uint64_t k = 0; k < nt; ++k) {
        const uint64_t t = tile_of(k);
        uint64_t r, col0;
        uint32_t b, e, live_end;
        tk_drows_tile(p, t, block, &r, &col0);
        tk_drows_range(p, sb, begin != nullptr, se, end != nullptr, r, &b, &e);
        tk_drows_stop_col(p, found[r], e, &live_end);
        if (!tk_drows_tile_live(col0, block, b, live_end)) continue;
        uint64_t before = 0;  // (the workgroup's exclusive scan)
        for (uint32_t th = 0; th < block / 8; ++th) {
            const uint64_t c0 = col0 + th * 8u;
            if (c0 >= p.W) continue;
            uint64_t v[8];
            uint32_t bad;
            const uint32_t keep = tk_drows_keep_lane(p, m, d, n_ids, r, c0, b, live_end, v, &bad);
            if (keep) tk_drows_store_lane(keep, v, tile_off[t] + before, out);
            before += tk_drows_popc8(keep);
        }
    }
    for (uint64_t i = 0; i < K; ++i)
        if (!seen[i]) twice = true;
    return oob ? -1 : twice ? -2 : 0;
}
}

#ifdef DECODE_ROWS_SIM_MAIN
// Case file: per case sixteen uint64 {R, W, ld, shift, flags, n_stop, n_skip, n_ids, block, order, has_begin, has_end, 0, 0, 0, 0}, then
// stop[16], skip[16], dec[2 n_ids] (uint32), begin[R] and end[R] where they exist, and the allocation that holds the matrix: `shift`
// elements, then the (R - 1) ld + W elements from (0, 0) to the last one -- exactly those, so that the sanitizer sees a read behind them.
// Result file: per case {rc, K, bad row, bad id} (int64 / uint64) and, for rc == 0, tokens[K], tok_off[R + 1], n_kept[R], stop_col[R].
template <class T>
static bool get(FILE* f, std::vector<T>& v, uint64_t n) {
    v.assign(n, 0);
    return !n || fread(v.data(), sizeof(T), n, f) == n;
}
template <class T>
static void put(FILE* f, const std::vector<T>& v, uint64_t n) {
    if (n) fwrite(v.data(), sizeof(T), n, f);
}
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint64_t h[16];
    int n_cases = 0;
    while (fread(h, 8, 16, in) == 16) {
        const uint64_t R = h[0], W = h[1], ld = h[2], shift = h[3];
        const uint32_t flags = (uint32_t)h[4], es = tk_drows_elem_size(flags);
        std::vector<uint32_t> stop, skip, dec, begin, end;
        std::vector<uint8_t> room;
        const uint64_t n_elems = shift + (R && W ? (R - 1) * ld + W : 0);
        if (!get(in, stop, 16) || !get(in, skip, 16) || !get(in, dec, 2 * h[7]) || !get(in, begin, h[10] ? R : 0) || !get(in, end, h[11] ? R : 0) || !get(in, room, n_elems * es))
            return 3;
        std::vector<uint32_t> tokens(R * W + 1), n_kept(R + 1), stop_col(R + 1);
        std::vector<uint64_t> tok_off(R + 1);
        uint64_t res[4] = {0, 0, 0, 0};
        const uint8_t* base = room.empty() ? (const uint8_t*)tokens.data() : room.data() + shift * es;  // (no element: any pointer, it is not read)
        const int64_t rc = decode_rows_sim(base, R, W, ld, h[10] ? begin.data() : nullptr, h[11] ? end.data() : nullptr, flags, (uint32_t)h[5], stop.data(), (uint32_t)h[6],
                                           skip.data(), dec.data(), (uint32_t)h[7], (uint32_t)h[8], (uint32_t)h[9], res + 1, tokens.data(), R * W, tok_off.data(),
                                           n_kept.data(), stop_col.data());
        res[0] = (uint64_t)rc;
        fwrite(res, 8, 4, out);
        if (!rc) {
            put(out, tokens, res[1]);
            put(out, tok_off, R + 1);
            put(out, n_kept, R);
            put(out, stop_col, R);
        }
        ++n_cases;
    }
    fclose(in);
    fclose(out);
    printf("%d cases\n", n_cases);
    return 0;
}
#endif
