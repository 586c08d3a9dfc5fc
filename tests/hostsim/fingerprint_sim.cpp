// The fingerprint passes (tiktoken_amd/csrc/tk_fingerprint.h) on the CPU: tk_fingerprint_rule.h compiled for the host and driven tile by
// tile, segment by segment, slice by slice and lane by lane the way the kernels do, at any tile size that is a multiple of four.  The
// readers check every index (tok_off, the staged ids, the tile's hashes -- a hash that is read must have been written in this tile), and
// the sink checks what the kernels' flushes rely on: a document that is stored plainly is stored once and never also added to.
//   fingerprint_sim(...) -> 0; -1 .. -3 the refusals of tk_fp_shape; -10 a tile that is no multiple of 4; -20 an index out of range;
//   -21 a hash read before it was written; -22 a plain store and another flush for one document
#include <stdint.h>

#include <vector>

#include "../../tiktoken_amd/csrc/tk_fingerprint_rule.h"

namespace {
struct Errors {
    bool range = false, unwritten = false, mixed = false;
};
template <class T>
struct Checked {  // an array whose every index is checked
    const T* p;
    uint64_t n;
    Errors* err;
    T operator[](uint64_t i) const {
        if (i >= n) return err->range = true, T(0);
        return p[i];
    }
};
struct TileHash {  // the tile's hashes in LDS
    std::vector<uint64_t> v;
    std::vector<uint8_t> written;
    Errors* err;
    uint64_t sink = 0;
    uint64_t& operator[](uint64_t i) {
        if (i >= v.size()) return err->range = true, sink;
        written[i] = 1;
        return v[i];
    }
    uint64_t operator[](uint64_t i) const {
        if (i >= v.size()) return err->range = true, 0;
        if (!written[i]) err->unwritten = true;
        return v[i];
    }
};
struct Sink {  // the flushes of tk_fingerprint.h's TkFpSink: the wavefront's sum is the sum over the lanes that call one after the other
    TkFp p;
    uint32_t* out_sig;
    uint64_t *exact, *nsh;
    std::vector<uint8_t> how_sum, how_sig;  // per document (the signature: per document and permutation): 1 stored, 2 added to
    Errors* err;
    uint32_t lane = 0;
    void note(uint8_t& how, bool whole) {
        if (whole ? how != 0 : how == 1) err->mixed = true;
        how = whole ? 1 : 2;
    }
    void sums(uint64_t d, bool whole, uint64_t sum, uint64_t n) {
        if (d >= p.n_docs) return void(err->range = true);
        exact[d] += sum;
        if (lane == 0) nsh[d] += n, note(how_sum[d], whole);
    }
    void sig(uint64_t d, bool whole, uint32_t perm, uint32_t v) {
        if (d >= p.n_docs || perm >= p.P) return void(err->range = true);
        note(how_sig[d * p.P + perm], whole);
        uint32_t& s = out_sig[d * p.P + perm];
        s = v < s ? v : s;
    }
};
}  // namespace

extern "C" uint32_t fingerprint_sim_tile() { return TK_FP_TILE; }

extern "C" int64_t fingerprint_sim(const uint32_t* tokens, uint64_t n, const uint64_t* tok_off, uint64_t n_docs, uint32_t k, uint32_t P, uint32_t B, uint64_t seed, uint32_t tile,
                                   uint32_t* sig, uint64_t* band, uint64_t* exact, uint64_t* nsh) {
    TkFp p;
    const int why = tk_fp_shape(k, P, B, seed, n, n_docs, &p);
    if (why) return -why;
    if (!tile || tile % 4) return -10;
    Errors err;
    const Checked<uint64_t> off{tok_off, n_docs + 1, &err};
    // the fill pass
    for (uint64_t i = 0; i < n_docs * P; ++i) sig[i] = TK_FP_NONE;
    for (uint64_t d = 0; d < n_docs; ++d) exact[d] = nsh[d] = 0;
    Sink sink{p, sig, exact, nsh, std::vector<uint8_t>(n_docs, 0), std::vector<uint8_t>(n_docs * P, 0), &err};
    // the tile pass
    const uint32_t waves = 4, seg = tile / waves, lanes = tk_fp_slice_lanes(P), slices = 256 / lanes, len = tile / slices;
    std::vector<uint32_t> staged(tile + TK_FP_MAX_NGRAM - 1);
    for (uint64_t g0 = 0; g0 < n; g0 += tile) {
        const uint64_t g1 = g0 + tile < n ? g0 + tile : n;
        for (uint64_t i = 0; i < staged.size(); ++i) staged[i] = g0 + i < n ? tokens[g0 + i] : 0u;
        const Checked<uint32_t> ids{staged.data(), staged.size(), &err};
        TileHash hash{std::vector<uint64_t>(tile, 0xDEADBEEFDEADBEEFull), std::vector<uint8_t>(tile, 0), &err};
        for (uint32_t w = 0; w < waves; ++w) {
            const uint64_t c0 = g0 + (uint64_t)w * seg, c1 = c0 + seg < g1 ? c0 + seg : g1;
            for (uint32_t lane = 0; lane < 64 && c0 < c1; ++lane) {
                sink.lane = lane;
                tk_fp_seg_hash(p, off, ids, g0, c0, c1, lane, 64u, hash, sink);
            }
        }
        const TileHash& done = hash;
        for (uint32_t t = 0; t < 256; ++t) {
            const uint32_t perm = t % lanes;
            const uint64_t c0 = g0 + (uint64_t)(t / lanes) * len, c1 = c0 + len < g1 ? c0 + len : g1;
            if (perm < P && c0 < c1) tk_fp_slice_sig(p, off, done, g0, c0, c1, perm, sink);
        }
    }
    // the finish pass
    for (uint64_t d = 0; d < n_docs; ++d)
        for (uint32_t j = 0; j < B; ++j) tk_fp_finish(p, off, d, j, sig, band, exact);
    return err.range ? -20 : err.unwritten ? -21 : err.mixed ? -22 : 0;
}
