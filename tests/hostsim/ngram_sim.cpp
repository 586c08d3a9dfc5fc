// The n-gram passes (tiktoken_amd/csrc/tk_ngram.h) on the CPU: tk_ngram_rule.h compiled for the host and driven tile by tile, share by
// share and lane by lane the way the kernels do -- the key, the probe behind the filter, the insert, the smear across words, the counts
// per document --, at any tile of 8 k positions (a tile below 256 is one segment of the count step).  The readers check every index,
// and the sink checks what the flushes rely on: a document that is stored plainly is stored once and never also added to.
//   0; -1, -2 the refusals of tk_ng_shape; -10 the tile; -20 an index out of range; -22 a plain store and another flush for one
//   document; -30 an add past the capacity (nothing is written)
#include <stdint.h>
#include <vector>

#include "../../tiktoken_amd/csrc/tk_ngram_rule.h"

namespace {
struct Errors { bool range = false, mixed = false; };
template <class T>
struct Checked {  // an array whose every index is checked
    T* p;
    uint64_t n;
    Errors* err;
    T operator[](uint64_t i) const { return i < n ? p[i] : (err->range = true, T(0)); }
    void put(uint64_t i, T v) const { i < n ? void(p[i] = v) : void(err->range = true); }
};
struct Set { TkNg p; uint64_t capacity, bound, count; std::vector<uint64_t> table; std::vector<uint32_t> filter; };
struct Sink {  // the flushes of tk_ngram.h's TkNgSink: the four-lane sum is the sum over the lanes that call one after the other
    uint64_t n_docs, *n_hit, *n_cov, *first;
    std::vector<uint8_t> how;  // per document: 1 stored, 2 added to
    Errors* err;
    uint32_t lane = 0;
    void counts(uint64_t d, bool whole, uint64_t nh, uint64_t nc, uint64_t f) {
        if (d >= n_docs) return void(err->range = true);
        if (lane == 0 && (whole ? how[d] != 0 : how[d] == 1)) err->mixed = true;
        if (lane == 0) how[d] = whole ? 1 : 2;
        n_hit[d] += nh, n_cov[d] += nc, first[d] = f < first[d] ? f : first[d];
    }
};
const uint32_t LANES = 8;  // lanes of a share of the key step
}  // namespace

extern "C" uint32_t ngram_sim_tile() { return TK_NG_TILE; }
extern "C" void* ngram_sim_create(uint32_t k, uint64_t seed, uint64_t capacity, int64_t* rc) {
    TkNg p;
    if ((*rc = -tk_ng_shape(k, seed, capacity, &p))) return nullptr;
    return new Set{p, capacity, 0, 0, std::vector<uint64_t>(p.S, 0), std::vector<uint32_t>(tk_ng_filter_words(p.S), 0)};
}
extern "C" void ngram_sim_destroy(void* s) { delete (Set*)s; }
extern "C" uint64_t ngram_sim_count(void* s) { return ((Set*)s)->bound = ((Set*)s)->count; }

static std::vector<uint32_t> stage(const uint32_t* tokens, uint64_t n, uint64_t g0, uint32_t tile) {  // as tk_ng_stage leaves them
    std::vector<uint32_t> ids(tile + 2 * TK_NG_HALO);
    for (uint64_t i = 0; i < ids.size(); ++i) ids[i] = g0 + i - TK_NG_HALO < n ? tokens[g0 + i - TK_NG_HALO] : 0u;
    return ids;
}

extern "C" int64_t ngram_sim_add(void* sv, const uint32_t* tokens, uint64_t n, const uint64_t* tok_off, uint64_t n_docs, uint32_t tile) {
    Set& st = *(Set*)sv;
    if (!tile || tile % 8) return -10;
    if (st.bound + n > st.capacity) return -30;
    Errors err;
    const TkNg p{st.p.k, st.p.seed, st.p.S, n, n_docs};
    const Checked<const uint64_t> off{tok_off, n_docs + 1, &err};
    Checked<uint64_t> table{st.table.data(), p.S, &err};
    for (uint64_t g0 = 0; g0 < n; g0 += tile) {
        const uint64_t g1 = g0 + tile < n ? g0 + tile : n;
        std::vector<uint32_t> staged = stage(tokens, n, g0, tile);
        const Checked<uint32_t> ids{staged.data(), staged.size(), &err};
        for (uint32_t lane = 0; lane < LANES; ++lane)
            tk_ng_seg_keys(p, off, ids, g0, g0, g1, lane, LANES, [&](uint64_t, uint64_t key) {
                if (!key) return;
                st.count += tk_ng_insert(table, p.S, key, [&](uint64_t i, uint64_t k) { return table[i] ? table[i] : (table.put(i, k), 0ull); });
                const uint64_t b = tk_ng_filter_bit(key, p.S);
                if ((b >> 5) >= st.filter.size()) return void(err.range = true);
                st.filter[b >> 5] |= 1u << (b & 31);
            });
    }
    st.bound += n;
    return err.range ? -20 : 0;
}

extern "C" int64_t ngram_sim_overlap(void* sv, const uint32_t* tokens, uint64_t n, const uint64_t* tok_off, uint64_t n_docs, uint32_t tile, uint64_t* n_hit, uint64_t* n_cov,
                                     uint64_t* n_ng, uint64_t* first, uint8_t* mask) {
    Set& st = *(Set*)sv;
    if (!tile || tile % 8) return -10;
    Errors err;
    const TkNg p{st.p.k, st.p.seed, st.p.S, n, n_docs};
    const Checked<const uint64_t> off{tok_off, n_docs + 1, &err};
    const Checked<uint64_t> table{st.table.data(), p.S, &err};
    const Checked<uint32_t> filter{st.filter.data(), st.filter.size(), &err};
    for (uint64_t d = 0; d < n_docs; ++d) n_hit[d] = n_cov[d] = 0, first[d] = TK_NG_NONE, n_ng[d] = tk_ng_starts_end(tok_off[d], tok_off[d + 1], p.k) - tok_off[d];  // the fill pass
    Sink sink{n_docs, n_hit, n_cov, first, std::vector<uint8_t>(n_docs, 0), &err};
    const uint32_t n_words = (tile + TK_NG_LEFT + 63) / 64, segs = tile % 256 ? 1 : 4, seg = tile / segs;
    for (uint64_t g0 = 0; g0 < n; g0 += tile) {
        const uint64_t g1 = g0 + tile < n ? g0 + tile : n, h0 = g0 >= p.k - 1 ? g0 - (p.k - 1) : 0;
        std::vector<uint32_t> staged = stage(tokens, n, g0, tile);
        const Checked<uint32_t> ids{staged.data(), staged.size(), &err};
        std::vector<uint64_t> keys_v(tile + TK_NG_LEFT, 0xDEADBEEFull), hit_v(n_words, 0), cov_v(n_words, 0);
        Checked<uint64_t> keys{keys_v.data(), keys_v.size(), &err};
        const uint64_t share = (g1 - h0 + 3) / 4;
        for (uint32_t w = 0; w < 4; ++w)
            for (uint32_t lane = 0; lane < LANES; ++lane) {
                const uint64_t c0 = h0 + w * share, c1 = c0 + share < g1 ? c0 + share : g1;
                if (c0 < c1) tk_ng_seg_keys(p, off, ids, g0, c0, c1, lane, LANES, [&](uint64_t g, uint64_t key) { keys.put(g - g0 + TK_NG_LEFT, key); });
            }
        for (uint64_t i = 0; i < keys_v.size(); ++i) {  // the probe step: a position's bit of its word
            const uint64_t g = g0 + i - TK_NG_LEFT, key = g - h0 < g1 - h0 ? keys[i] : 0ull;
            if (key && tk_ng_filter_has(filter, p.S, key) && tk_ng_probe(table, p.S, key)) hit_v[i >> 6] |= 1ull << (i & 63);
        }
        for (uint32_t w = 1; w < n_words; ++w) cov_v[w] = tk_ng_smear(hit_v[w - 1], hit_v[w], p.k);
        const Checked<uint64_t> hit{hit_v.data(), n_words, &err}, cov{cov_v.data(), n_words, &err};
        for (uint64_t i = 0; i < g1 - g0; ++i) mask[g0 + i] = (uint8_t)((cov[(i + TK_NG_LEFT) >> 6] >> (i & 63)) & 1);
        for (uint32_t w = 0; w < segs; ++w)
            for (uint32_t lane = 0; lane < (seg + 63) / 64; ++lane) {
                const uint64_t c0 = g0 + (uint64_t)w * seg, c1 = c0 + seg < g1 ? c0 + seg : g1;
                sink.lane = lane;
                if (c0 < c1) tk_ng_seg_count(p, off, hit, cov, g0, c0, c1, lane, sink);
            }
    }
    return err.range ? -20 : err.mixed ? -22 : 0;
}
