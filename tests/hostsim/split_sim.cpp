// The split passes (tiktoken_amd/csrc/tk_split.h) on the CPU: the plain C++ they are made of -- tk_split_rule.h: what a spec may say, the
// class of a boundary, a step of the chain, the walks of a block, the stitch of a document, fold, rank and record -- compiled for the host
// and driven the way the kernels drive it: planes by "wavefronts" of 64 positions in workgroups of `block`, a walk per block of K, the
// stitch per document, fold and count per plane word with count blocks of `cb` positions, scan, write, doc_chunk.  A step's window goes
// through the same lane / ballot / choose functions as on the device, the 64 lanes computed one after the other.  Every array is read
// through a reader that checks the index.  Test infrastructure only (tests/test_split_sim.py builds it).
#include <stdint.h>

#include <vector>

#include "../../include/tiktoken_amd.h"
#include "../../tiktoken_amd/csrc/tk_split_rule.h"
#include "sim_readers.h"

namespace {
struct SimPlanes {
    const uint64_t* p;
    uint64_t W;
    uint32_t n_planes;
    bool* oob;
    uint64_t word(uint32_t pl, uint64_t w) const {
        if (pl >= n_planes || w >= W) {
            *oob = true;
            return 0;
        }
        return p[pl * W + w];
    }
};
struct SimBits {
    const uint64_t* p;
    uint64_t W;
    bool* oob;
    bool bit(uint64_t g) const {
        if ((g >> 6) >= W) {
            *oob = true;
            return false;
        }
        return (p[g >> 6] >> (g & 63u)) & 1u;
    }
};
struct SimMark {
    uint64_t* p;
    uint64_t W;
    bool* oob;
    void operator()(uint64_t g) const {
        if ((g >> 6) >= W) *oob = true;
        else p[g >> 6] |= 1ull << (g & 63u);
    }
};
struct SimAdd {
    uint64_t* stats;
    void operator()(int which, uint64_t v) const { stats[which] += v; }
};
struct SimWave {  // the 64 lanes one after the other
    uint64_t w[64];
    template <class F>
    uint64_t gather(F&& f) {
        uint64_t ballot = 0;
        for (uint32_t lane = 0; lane < 64; ++lane) {
            w[lane] = f(lane);
            if (w[lane]) ballot |= 1ull << lane;
        }
        return ballot;
    }
    uint64_t word(uint32_t lane) const { return w[lane]; }
};
const uint32_t GUARD = 0xDEADBEEFu;
}  // namespace

extern "C" {
// Returns C, the chunks written; -1: an index out of bounds; -2: a guard word overwritten; -(16 + why): tk_split_shape's refusal;
// -(64 + tk_rows_bad_key): tok_off is refused.  The chunk arrays have room for T + 1 entries (a chunk owns a token), doc_chunk for
// n_docs + 1; byte_start / char_start hold T entries, byte_off / char_off and the offsets n_docs + 1.  stats: TK_SPLIT_STATS counters.
int64_t split_sim(const uint8_t* text_in, uint64_t n_bytes, const uint64_t* doc_off_in, const uint64_t* tok_off_in, uint64_t n_docs, uint64_t T, const uint32_t* byte_start_in,
                  const uint32_t* char_start_in, const uint64_t* byte_off_in, const uint64_t* char_off_in, const tk_split_spec* spec, uint32_t block, uint32_t cb,
                  uint32_t* doc, uint32_t* tok_begin, uint32_t* tok_end, uint32_t* byte_begin, uint32_t* byte_end, uint32_t* char_begin, uint32_t* char_end, uint8_t* cut_out,
                  uint32_t* doc_chunk, uint64_t* stats) {
    if (spec->n_levels > 4) return -(16 + 4);
    TkSplit p;
    const int why = tk_split_shape(T, n_docs, spec->max_tokens, spec->min_tokens, spec->overlap, spec->n_levels, spec->n_seps, spec->sep, spec->seg_tokens, spec->flags, &p);
    if (why) return -(16 + why);
    bool oob = false;
    const SimOffsets tok_off{tok_off_in, n_docs, &oob}, doc_off{doc_off_in, n_docs, &oob}, byte_off{byte_off_in, n_docs, &oob}, char_off{char_off_in, n_docs, &oob};
    const SimArray<uint8_t> text{text_in, n_bytes, &oob};
    const SimArray<uint32_t> byte_start{byte_start_in, T, &oob}, char_start{char_start_in, T, &oob};
    // tk_k_split_check
    unsigned long long bad = ~0ull;
    for (uint64_t d = 0; d <= n_docs; ++d) {
        uint64_t a, b;
        tk_rows_off_check(tok_off, d, n_docs, T, &a, &b, &bad);
    }
    if (oob) return -1;
    if (bad != ~0ull) return -(64 + (int64_t)bad);
    // tk_k_split_class: workgroups of `block` positions over the W * 64 positions of a plane, a ballot per wavefront of 64
    const uint32_t n_planes = p.L + 1;
    std::vector<uint64_t> planes(n_planes * p.W + 1, 0), cut(p.W + 1, 0), spec_plane(p.W + 1, 0);
    planes.back() = cut.back() = spec_plane.back() = GUARD;
    for (uint64_t b0 = 0; b0 < p.W * 64; b0 += block) {
        uint64_t d_lo = 0, d_hi = 0;
        if (b0 < T) tk_split_block_docs(p, tok_off, b0, block, &d_lo, &d_hi);
        for (uint64_t w0 = b0; w0 < b0 + block && w0 < p.W * 64; w0 += 64) {
            uint64_t ballot[5] = {0, 0, 0, 0, 0};
            for (uint64_t g = w0; g < w0 + 64; ++g) {
                const uint32_t bits = g < T ? tk_split_class_at(p, text, doc_off, tok_off, byte_start, d_lo, d_hi, g) : 0u;
                for (uint32_t pl = 0; pl < n_planes; ++pl) ballot[pl] |= (uint64_t)((bits >> pl) & 1u) << (g & 63u);
            }
            for (uint32_t pl = 0; pl < n_planes; ++pl) planes[pl * p.W + (w0 >> 6)] = ballot[pl];
        }
    }
    if (oob) return -1;
    // tk_k_split_walk: a wavefront per block of K positions
    const uint64_t n_blocks = (T + p.K - 1) / p.K;
    std::vector<uint32_t> exit_at(n_blocks + 1, TK_SPLIT_NOWHERE), join_at(n_blocks + 1, TK_SPLIT_NOWHERE);
    exit_at.back() = join_at.back() = GUARD;
    const SimPlanes P{planes.data(), p.W, n_planes, &oob};
    SimWave wave;
    SimMark mark_cut{cut.data(), p.W, &oob}, mark_spec{spec_plane.data(), p.W, &oob};
    for (int i = 0; i < TK_SPLIT_STATS; ++i) stats[i] = 0;
    SimAdd add{stats};
    for (uint64_t b = 0; b < n_blocks; ++b) tk_split_block(p, P, wave, tok_off, b, mark_cut, mark_spec, exit_at.data(), add);
    if (oob) return -1;
    // tk_k_split_stitch: a wavefront per document
    const SimBits spec_bits{spec_plane.data(), p.W, &oob};
    if (n_blocks > 1)
        for (uint64_t d = 0; d < n_docs; ++d) tk_split_stitch(p, P, wave, tok_off, spec_bits, d, mark_cut, exit_at.data(), join_at.data(), add);
    if (oob) return -1;
    // tk_k_split_count, tk_k_split_scan
    const uint32_t cb_words = cb / 64;
    const uint64_t nb = (p.W + cb_words - 1) / cb_words;
    std::vector<uint32_t> cnt(nb + 1, 0);
    cnt.back() = GUARD;
    for (uint64_t w = 0; w < p.W; ++w) {
        cut[w] = tk_split_fold(p, cut[w], spec_plane[w], w, join_at.data());
        cnt[w / cb_words] += (uint32_t)__builtin_popcountll(cut[w]);
    }
    const uint64_t C = sim_scan(cnt.data(), nb);
    if (planes.back() != GUARD || cut.back() != GUARD || spec_plane.back() != GUARD || exit_at.back() != GUARD || join_at.back() != GUARD || cnt.back() != GUARD) return -2;
    if (C > T) return -2;
    // tk_k_split_write: a thread per plane word; tk_k_split_docs
    const SimArray<uint64_t> cut_r{cut.data(), p.W, &oob};
    const SimArray<uint32_t> cnt_r{cnt.data(), nb, &oob};
    const TkSplitOut out{doc, tok_begin, tok_end, byte_begin, byte_end, char_begin, char_end, cut_out};
    for (uint64_t w = 0; w < p.W; ++w) {
        uint64_t v = cut[w];
        if (!v) continue;
        uint64_t i = tk_split_rank(cut_r, cnt_r, cb_words, w * 64);
        for (; v; v &= v - 1, ++i) {
            if (i >= C) return -1;
            tk_split_record(p, P, tok_off, byte_start, char_start, byte_off, char_off, w * 64 + (uint64_t)__builtin_ctzll(v), i, out);
        }
    }
    for (uint64_t d = 0; d <= n_docs; ++d) doc_chunk[d] = (uint32_t)tk_split_rank(cut_r, cnt_r, cb_words, tok_off[d]);
    return oob ? -1 : (int64_t)C;
}
}
