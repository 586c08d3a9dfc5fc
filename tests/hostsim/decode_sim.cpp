// The decode passes (tiktoken_amd/csrc/tk_decode.h) on the CPU: the plain C++ they are made of -- tk_decode_rule.h: the length of an id, a
// lane of the copy pass with every store it makes, the entry of the per-document pass -- compiled for the host and driven the way the
// kernels drive it: workgroups of `block` tokens, lanes of eight, the length pass with its per-workgroup sums and the first bad position,
// the exclusive scan, the copy pass.  The lanes are visited in an order a seed chooses; the copy pass stores through a writer that checks
// and counts.  Test infrastructure only (tests/test_decode_sim.py builds it; tests/hostsim/decode_sanitize.cpp includes it).
#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "../../tiktoken_amd/csrc/tk_decode_rule.h"
#include "sim_readers.h"

// the id -> {offset, length} table, entries [0, n): an index beyond sets *oob instead of being read
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

enum {
    DEC_SIM_BAD_ID = 1,        // an id without entry: result[1] = its position (the first one)
    DEC_SIM_OOB = -1,          // the table, the ids or an offsets array were indexed out of bounds
    DEC_SIM_MISALIGNED = -2,   // an 8-byte store at an offset that is no multiple of 8
    DEC_SIM_WORD_OUTSIDE = -3, // an 8-byte store that does not lie wholly inside [0, total)
    DEC_SIM_BYTE_OUTSIDE = -4, // a 1-byte store outside [0, total)
    DEC_SIM_TWICE = -5,        // an output byte stored more than once
    DEC_SIM_NEVER = -6,        // an output byte never stored
    DEC_SIM_GUARD = -7,        // the bytes before or behind the output were changed
    DEC_SIM_ROOM = -8,         // the caller's buffers are too small
};

// The stores of the simulation: into a buffer between guard bytes, every offset checked, every byte counted.  A store that offends is
// reported and not made.
struct SimStores {
    static constexpr uint64_t GUARD = 32;
    std::vector<uint8_t> buf;    // GUARD bytes, the output, GUARD bytes
    std::vector<uint8_t> count;  // stores per output byte (saturating)
    uint64_t total;
    int64_t err = 0;
    uint64_t* log;  // (may be null) the stores in the order made: offset << 1 | (1 for an 8-byte store)
    uint64_t log_cap;
    uint64_t n_log = 0;
    SimStores(uint64_t total_, uint64_t* log_, uint64_t log_cap_) : buf(total_ + 2 * GUARD, 0xA5), count(total_, 0), total(total_), log(log_), log_cap(log_cap_) {}
    void fail(int64_t e) {
        if (!err) err = e;
    }
    void note(uint64_t off, uint32_t n) {
        if (log && n_log < log_cap) log[n_log] = (off << 1) | (n == 8u ? 1u : 0u);
        ++n_log;
        uint8_t* c = count.data();
        for (uint32_t k = 0; k < n; ++k) {
            if (c[off + k]) fail(DEC_SIM_TWICE);
            if (c[off + k] < 255) ++c[off + k];
        }
    }
    void word(unsigned long long off, uint64_t v) {
        if (off & 7ull) return fail(DEC_SIM_MISALIGNED);
        if (off >= total || total - off < 8) return fail(DEC_SIM_WORD_OUTSIDE);
        note(off, 8);
        uint8_t* b = buf.data() + GUARD + off;
        for (uint32_t k = 0; k < 8; ++k) b[k] = (uint8_t)(v >> (8 * k));
    }
    void byte(unsigned long long off, uint8_t v) {
        if (off >= total) return fail(DEC_SIM_BYTE_OUTSIDE);
        note(off, 1);
        buf[GUARD + off] = v;
    }
    int64_t verdict() const {
        if (err) return err;
        for (uint64_t k = 0; k < GUARD; ++k)
            if (buf[k] != 0xA5 || buf[GUARD + total + k] != 0xA5) return DEC_SIM_GUARD;
        for (uint64_t k = 0; k < total; ++k)
            if (!count[k]) return DEC_SIM_NEVER;
        return 0;
    }
};

// the lanes of all workgroups in the order of the seed: 0 ascending, 1 descending, otherwise shuffled (a linear congruential generator)
static std::vector<uint64_t> lane_order(uint64_t n_lanes, uint64_t seed) {
    std::vector<uint64_t> o(n_lanes);
    std::iota(o.begin(), o.end(), 0);
    if (seed == 1) std::reverse(o.begin(), o.end());
    if (seed > 1) {
        uint64_t x = seed * 0x9E3779B97F4A7C15ull + 1;
        for (uint64_t k = n_lanes; k > 1; --k) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            std::swap(o[k - 1], o[(x >> 33) % k]);
        }
    }
    return o;
}

// tk_k_dec_len, tk_k_dec_scan64 and (once the host has seen no bad id) tk_k_dec_copy over n tokens.  `make_out(total)` gives the writer of
// the copy pass.  dec has dec_len entries (n_ids, unless a test hands in less); extra_blocks: workgroups behind the last token's (they
// hold no token).  result = {total bytes, first bad position or ~0}.  Returns 0, DEC_SIM_BAD_ID or DEC_SIM_OOB; what the writer finds is
// the caller's to ask for.
template <class MakeOut, class Done>
static int64_t decode_passes(const uint32_t* tokens_in, uint64_t n, const uint32_t* dec_in, uint32_t n_ids, uint64_t dec_len, const uint8_t* tok_bytes,
                             const uint8_t* spec_bytes, uint32_t block, uint64_t seed, uint32_t extra_blocks, uint64_t pos_base, uint64_t off_base,
                             unsigned long long* tok_byte_off, uint64_t* result, MakeOut&& make_out, Done&& done) {
    bool oob = false;
    const SimDec dec{dec_in, dec_len, &oob};
    const SimArray<uint32_t> tokens{tokens_in, n, &oob};
    const uint64_t nb = (n + block - 1) / block + extra_blocks, lanes_per_block = block / 8;
    const std::vector<uint64_t> order = lane_order(nb * lanes_per_block, seed);
    std::vector<uint32_t> lens(n ? n : 1, 0xDEADBEEFu);
    std::vector<unsigned long long> bsum(nb + 1, 0);
    // tk_k_dec_len: a lane's eight lengths, their sum into the workgroup's, the first bad position through a minimum
    unsigned long long bad = ~0ull;
    for (const uint64_t lane : order) {
        const uint64_t i0 = lane * 8;
        uint32_t sum = 0;
        for (int j = 0; j < 8; ++j) {
            const uint64_t i = i0 + j;
            uint32_t len = 0;
            if (i < n) {
                len = tk_dec_len_of(dec, n_ids, tokens[i]);
                if (len == 0u) bad = std::min(bad, (unsigned long long)(pos_base + i));
                lens[i] = len;
            }
            sum += len;
        }
        bsum[lane / lanes_per_block] += sum;
    }
    // tk_k_dec_scan64
    const uint64_t total = sim_scan(bsum.data(), nb);
    result[0] = total;
    result[1] = bad;
    if (oob) return DEC_SIM_OOB;
    if (bad != ~0ull) return DEC_SIM_BAD_ID;  // (the host: the copy pass is not launched)
    // tk_k_dec_copy: the workgroup's base + the exclusive scan of its lanes' sums = the lane's first byte
    auto out = make_out(total);
    std::vector<unsigned long long> lane_at(nb * lanes_per_block, 0);
    for (uint64_t b = 0; b < nb; ++b) {
        unsigned long long at = bsum[b];
        for (uint64_t t = 0; t < lanes_per_block; ++t) {
            lane_at[b * lanes_per_block + t] = at;
            for (uint64_t i = (b * lanes_per_block + t) * 8; i < std::min(n, (b * lanes_per_block + t + 1) * 8); ++i) at += lens[i];
        }
    }
    for (const uint64_t lane : order) {
        const uint64_t i0 = lane * 8;
        uint32_t len[8];
        for (int j = 0; j < 8; ++j) len[j] = i0 + j < n ? lens[i0 + j] : 0u;
        tk_dec_lane(tokens, i0, n, len, lane_at[lane], dec, tok_bytes, spec_bytes, out, tok_byte_off, off_base);
    }
    if (oob) return DEC_SIM_OOB;
    return done(out, total);
}

extern "C" {
// The three passes with the checking writer.  out: room for out_cap bytes (the total must fit); tok_byte_off (may be null): n entries;
// log (may be null): room for log_cap stores, result[2] = how many were made.  Returns 0 or one of the codes above.
int64_t decode_sim(const uint32_t* tokens, uint64_t n, const uint32_t* dec, uint32_t n_ids, uint64_t dec_len, const uint8_t* tok_bytes, const uint8_t* spec_bytes,
                   uint32_t block, uint64_t seed, uint32_t extra_blocks, uint64_t pos_base, uint64_t off_base, uint8_t* out, uint64_t out_cap,
                   unsigned long long* tok_byte_off, uint64_t* log, uint64_t log_cap, uint64_t* result) {
    if (block < 8 || block % 8) return DEC_SIM_ROOM;
    result[2] = 0;
    return decode_passes(
        tokens, n, dec, n_ids, dec_len, tok_bytes, spec_bytes, block, seed, extra_blocks, pos_base, off_base, tok_byte_off, result,
        [&](uint64_t total) { return SimStores(total, log, log_cap); },
        [&](const SimStores& w, uint64_t total) -> int64_t {
            result[2] = w.n_log;
            if (total > out_cap) return DEC_SIM_ROOM;
            std::copy(w.buf.begin() + SimStores::GUARD, w.buf.begin() + SimStores::GUARD + total, out);
            return w.verdict();
        });
}

// tk_k_dec_docoff: byte_off[d] for d <= n_docs.  tok_off holds off_len entries (n_docs + 1, unless a test hands in less), tok_byte_off n.
int64_t decode_sim_docoff(const uint64_t* tok_off_in, uint64_t off_len, uint64_t n_docs, uint64_t n, const unsigned long long* tok_byte_off_in, uint64_t total,
                          uint64_t* byte_off) {
    bool oob = false;
    if (!off_len) return DEC_SIM_OOB;
    const SimOffsets tok_off{tok_off_in, off_len - 1, &oob};
    const SimArray<unsigned long long> tok_byte_off{tok_byte_off_in, n, &oob};
    const unsigned long long tot = total;
    for (uint64_t d = 0; d <= n_docs; ++d) byte_off[d] = tk_dec_doc_off(tok_off, d, n, tok_byte_off, &tot);
    return oob ? DEC_SIM_OOB : 0;
}
}
