// The scan elements of the word statistics and of the line cleaning (tiktoken_amd/csrc/tk_words.h, tk_clean.h) on the CPU:
// tk_words_rule.h and tk_clean_rule.h compiled for the host and driven the way the kernels drive them, at any geometry -- L lanes of 16
// bytes a tile, P tiles a thread of the carry pass, W lanes a wavefront.  A lane's masks are built from the buffer as tk_wd_stage and
// tk_cl_stage build them; its element is tk_wd_lane_tail's or tk_cl_lane_tail's; the element that enters a lane is computed in the
// kernels' order: inside a tile a Hillis-Steele doubling scan over every group of W lanes and the groups joined left to right
// (tk_wd_block_exscan), the tiles' totals in stretches of P, the stretch totals by the same group scan, every stretch replayed with
// run = join(run, s) (tk_k_wd_carry), and `before` = join(what enters the tile, the exclusive value inside it).  Then the words, the
// ellipses and the lines are handed out as tk_k_wd_count and tk_k_cl_decide hand them out, to the document of doc_before(j) / doc(j).
// Every read of the text is checked against N; document phrases and the write pass are not here.
//   >= 0 (clean: the number of dropped lines); -1 .. -7 the refusals of tk_wd_shape / tk_cl_shape; -10 the geometry; -20 an event for
//   a local document that is none; -21 more dropped lines than `cap`
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../tiktoken_amd/csrc/tk_clean_rule.h"
#include "../../tiktoken_amd/csrc/tk_words_rule.h"

namespace {
const uint64_t NONE = ~0ull;

struct Buf {  // the packed text and where documents start; every read is checked
    const uint8_t* text;
    const uint64_t* doc_off;
    uint64_t N, n_docs;
    std::vector<uint8_t> starts;   // starts[p]: an entry of doc_off is p, 0 <= p <= N
    std::vector<uint32_t> n_before;  // the start positions below p, 0 <= p <= N + 1
    Buf(const uint8_t* t, const uint64_t* off, uint64_t n) : text(t), doc_off(off), N(off[n]), n_docs(n), starts(off[n] + 1, 0), n_before(off[n] + 2, 0) {
        for (uint64_t i = 0; i <= n; ++i)
            if (off[i] <= N) starts[off[i]] = 1;
        for (uint64_t p = 0; p <= N; ++p) n_before[p + 1] = n_before[p] + starts[p];
    }
    uint32_t raw(uint64_t p) const { return p < N ? text[p] : 0u; }
    uint32_t folded(uint64_t p) const { return tk_cl_fold(raw(p)); }
    bool start(uint64_t p) const { return p <= N && starts[p]; }
    uint32_t starts_in(uint64_t a, uint64_t b) const { return n_before[std::min(b, N + 1)] - n_before[std::min(a, N + 1)]; }  // in [a, b)
};

// The word rule's view of the 16 bytes at `at`, as tk_wd_stage gives it; g0: the lane's tile.  fold: the look-around reads folded text.
template <class IsLetter>
TkWdLane wd_lane(const Buf& b, uint64_t g0, uint64_t at, bool fold, IsLetter&& is_letter) {
    TkWdLane L;
    uint64_t lo = 0, hi = 0;
    for (uint32_t j = 0; j < 16; ++j) (j < 8 ? lo : hi) |= (uint64_t)b.raw(at + j) << (8 * (j & 7u));
    uint32_t B = 0;
    for (uint32_t k = 0; k < 32; ++k)
        if (at + k >= 2 && b.start(at + k - 2)) B |= 1u << k;
    const uint32_t n_left = at >= b.N ? 0u : b.N - at < 17u ? (uint32_t)(b.N - at) : 17u;
    L.pos = (uint32_t)(at - g0);
    tk_wd_lane_masks(
        lo, hi, n_left, B, b.raw(at + 16), [&](int k) -> uint32_t { return fold ? b.folded(at + (uint64_t)(int64_t)k) : b.raw(at + (uint64_t)(int64_t)k); }, is_letter, &L);
    L.rank = b.starts_in(g0, at);
    return L;
}
// The documents of a tile by local index, as tk_cl_local_docs finds them: index 0 owns the byte before the tile, index r > 0 is the
// non-empty document at the r-th start position at or behind g0
std::vector<uint64_t> local_docs(const Buf& b, uint64_t g0, uint64_t tile) {
    std::vector<uint64_t> d{g0 && b.n_docs ? tk_last_le(b.doc_off, 0, b.n_docs, g0 - 1) : NONE};
    for (uint64_t p = g0; p < g0 + tile && p <= b.N; ++p) {
        if (!b.start(p)) continue;
        const uint64_t i = b.n_docs ? tk_last_le(b.doc_off, 0, b.n_docs, p) : 0;
        d.push_back(b.n_docs && b.doc_off[i] == p && b.doc_off[i + 1] > p ? i : NONE);
    }
    return d;
}

// The exclusive scan of tk_wd_block_exscan over any number of lanes: groups of W by doubling, the groups left to right from `init`
template <class El, class Join>
std::vector<El> exscan(const std::vector<El>& in, const El& init, const El& empty, uint32_t W, Join&& join, El* total) {
    std::vector<El> ex(in.size(), empty);
    El pre = init;
    for (size_t g = 0; g < in.size(); g += W) {
        const size_t n = std::min<size_t>(W, in.size() - g);
        std::vector<El> v(in.begin() + g, in.begin() + g + n);
        for (size_t o = 1; o < W; o <<= 1) {
            const std::vector<El> u = v;  // (what __shfl_up reads: the values before the round)
            for (size_t l = o; l < n; ++l) v[l] = join(u[l - o], u[l]);
        }
        for (size_t l = 0; l < n; ++l) ex[g + l] = join(pre, l ? v[l - 1] : empty);
        pre = join(pre, v[n - 1]);
    }
    if (total) *total = pre;
    return ex;
}
// The element that enters every lane, from the lanes' own: the sum pass, the carry pass and the scan of the pass that hands out
template <class El, class Join>
std::vector<El> entering(const std::vector<El>& lanes, const El& empty, uint32_t L, uint32_t P, uint32_t W, Join&& join) {
    const size_t n_tiles = lanes.size() / L;
    std::vector<El> tiles(n_tiles, empty), before;
    for (size_t t = 0; t < n_tiles; ++t) exscan(std::vector<El>(lanes.begin() + t * L, lanes.begin() + (t + 1) * L), empty, empty, W, join, &tiles[t]);
    std::vector<El> mine((n_tiles + P - 1) / P, empty);
    for (size_t t = 0; t < n_tiles; ++t) mine[t / P] = join(mine[t / P], tiles[t]);
    const std::vector<El> runs = exscan(mine, empty, empty, W, join, (El*)nullptr);
    for (size_t s = 0; s < mine.size(); ++s) {
        El run = runs[s];
        for (size_t t = s * P; t < n_tiles && t < (s + 1) * P; ++t) {
            const El own = tiles[t];
            tiles[t] = run;
            run = join(run, own);
        }
    }
    for (size_t t = 0; t < n_tiles; ++t) {
        const std::vector<El> ex = exscan(std::vector<El>(lanes.begin() + t * L, lanes.begin() + (t + 1) * L), tiles[t], empty, W, join, (El*)nullptr);
        before.insert(before.end(), ex.begin(), ex.end());
    }
    return before;
}
bool geometry(uint32_t L, uint32_t P, uint32_t W) { return L && P && W && L <= 4096 && W <= 4096; }
}  // namespace

// out: uint64[5][n_docs] -- n_words, word_chars, n_alpha_words, stop_mask, n_ellipsis.  letters: a bit per code point below 0x110000.
extern "C" int64_t text_scan_sim_words(const uint8_t* text, const uint64_t* doc_off, uint64_t n_docs, const uint8_t* stop_bytes, const uint64_t* stop_off, uint64_t n_stop,
                                       const uint8_t* letters, uint32_t L, uint32_t P, uint32_t W, uint64_t* out) {
    if (!geometry(L, P, W)) return -10;
    const Buf b(text, doc_off, n_docs);
    TkWd p;
    if (const int rc = tk_wd_shape(b.N, n_docs, stop_bytes, stop_off, n_stop, nullptr, 0, &p)) return -rc;
    const uint64_t tile = (uint64_t)L * TK_WD_LANE, n_tiles = b.N / tile + 1;
    auto is_letter = [&](uint32_t cp) -> bool { return cp < 0x110000u && ((letters[cp >> 3] >> (cp & 7u)) & 1u); };
    std::vector<TkWdLane> lane;
    std::vector<TkWdRun> own;
    for (uint64_t i = 0; i < n_tiles * L; ++i) {
        lane.push_back(wd_lane(b, i / L * tile, i * TK_WD_LANE, false, is_letter));
        own.push_back(tk_wd_lane_tail(lane.back()));
    }
    const std::vector<TkWdRun> before = entering(own, tk_wd_empty(), L, P, W, [](const TkWdRun& l, const TkWdRun& r) { return tk_wd_join(l, r); });
    for (uint64_t i = 0; i < 5 * n_docs; ++i) out[i] = 0;
    bool lost = false;
    for (uint64_t t = 0; t < n_tiles; ++t) {
        const std::vector<uint64_t> docs = local_docs(b, t * tile, tile);
        auto put = [&](uint32_t li, uint32_t f, uint64_t v, bool is_or) {
            const uint64_t d = li < docs.size() ? docs[li] : NONE;
            if (d == NONE) return void(lost = true);
            is_or ? void(out[f * n_docs + d] |= v) : void(out[f * n_docs + d] += v);
        };
        for (uint64_t i = t * L; i < (t + 1) * L; ++i) {
            const TkWdLane& ln = lane[i];
            for (uint32_t ev = tk_wd_ends(ln, before[i]); ev; ev &= ev - 1u) {
                const uint32_t j = (uint32_t)__builtin_ctz(ev), li = ln.doc_before(j);
                const TkWdRun w = tk_wd_word(ln, before[i], j);
                put(li, 0, 1, false), put(li, 1, w.chars, false), put(li, 2, w.flags & TK_WD_F_ALPHA, false), put(li, 3, tk_wd_stop_bits(p, w), true);
            }
            for (uint32_t ev = ln.ell; ev; ev &= ev - 1u) put(ln.doc((uint32_t)__builtin_ctz(ev)), 4, 1, false);
            for (uint32_t ev = tk_wd_dot_starts(ln); ev; ev &= ev - 1u) {
                const uint32_t j = (uint32_t)__builtin_ctz(ev);
                put(ln.doc(j), 4, tk_wd_dot_triples(ln, before[i], j), false);
            }
        }
    }
    return lost ? -20 : 0;
}

// out: uint64[6][n_docs] -- n_lines, n_short, n_long, n_no_end, n_ellipsis, n_phrase.  starts: the starts of the dropped lines, sorted.
extern "C" int64_t text_scan_sim_clean(const uint8_t* text, const uint64_t* doc_off, uint64_t n_docs, uint64_t min_words, uint64_t max_word_chars, uint32_t flags,
                                       const uint8_t* terminal, uint64_t n_terminal, const uint8_t* line_bytes, const uint64_t* line_off, uint64_t n_line, uint32_t L, uint32_t P,
                                       uint32_t W, uint64_t* out, uint64_t* starts, uint64_t cap) {
    if (!geometry(L, P, W)) return -10;
    const Buf b(text, doc_off, n_docs);
    TkCl q;
    if (const int rc = tk_cl_shape(b.N, n_docs, min_words, max_word_chars, flags, terminal, n_terminal, line_bytes, line_off, n_line, nullptr, nullptr, 0, &q)) return -rc;
    const uint64_t tile = (uint64_t)L * TK_CL_LANE, n_tiles = b.N / tile + 1;
    std::vector<TkClLane> lane;
    std::vector<TkClSt> own;
    for (uint64_t i = 0; i < n_tiles * L; ++i) {
        const uint64_t at = i * TK_CL_LANE;
        TkClLane ln;
        ln.w = wd_lane(b, i / L * tile, at, true, [](uint32_t) -> bool { return false; });
        tk_cl_lane_masks((uint32_t)at, at >= b.N ? 0u : b.N - at < 17u ? (uint32_t)(b.N - at) : 17u, &ln);
        for (uint32_t j = 0; j < TK_CL_LANE && at + j < b.N; ++j) {
            const uint64_t pos = at + j, next = b.doc_off[tk_last_le(b.doc_off, 0, n_docs + 1, pos) + 1];  // (pos < N: an entry lies behind it)
            const uint32_t room = (uint32_t)std::min<uint64_t>(std::min(next, b.N) - pos, 64);
            for (uint32_t s = 0; s < q.n_line; ++s)
                if (tk_cl_occurs(q.ph[s], q.len[s], room, [&](uint32_t k) -> uint32_t { return b.folded(pos + k); })) ln.lhit |= 1u << j;
        }
        lane.push_back(ln);
        own.push_back(tk_cl_lane_tail(ln));
    }
    const std::vector<TkClSt> before = entering(own, tk_cl_empty(), L, P, W, [](const TkClSt& l, const TkClSt& r) { return tk_cl_join(l, r); });
    for (uint64_t i = 0; i < 6 * n_docs; ++i) out[i] = 0;
    std::vector<uint64_t> dropped;
    bool lost = false;
    for (uint64_t t = 0; t < n_tiles; ++t) {
        const std::vector<uint64_t> docs = local_docs(b, t * tile, tile);
        for (uint64_t i = t * L; i < (t + 1) * L; ++i) {
            const TkClLane& ln = lane[i];
            for (uint32_t ev = tk_cl_closes(ln, before[i]); ev; ev &= ev - 1u) {
                const uint32_t j = (uint32_t)__builtin_ctz(ev), li = ln.w.doc_before(j);
                const TkClSt line = tk_cl_line(ln, before[i], j);
                const uint32_t r = tk_cl_judge(q, line, [&](uint32_t pos) -> uint32_t { return b.raw(pos); });
                const uint64_t d = li < docs.size() ? docs[li] : NONE;
                if (d == NONE) {
                    lost = true;
                    continue;
                }
                const uint32_t rule[5] = {TK_CL_R_SHORT, TK_CL_R_LONG, TK_CL_R_NO_END, TK_CL_R_ELLIPSIS, TK_CL_R_PHRASE};
                out[d] += 1;
                for (uint32_t f = 0; f < 5; ++f) out[(f + 1) * n_docs + d] += (r & rule[f]) ? 1u : 0u;
                if (r) dropped.push_back(line.start);
            }
        }
    }
    if (lost) return -20;
    if (dropped.size() > cap) return -21;
    std::sort(dropped.begin(), dropped.end());
    for (size_t i = 0; i < dropped.size(); ++i) starts[i] = dropped[i];
    return (int64_t)dropped.size();
}
