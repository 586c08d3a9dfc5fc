// The JSON Lines passes (tiktoken_amd/csrc/tk_jsonl.h) on the CPU: the plain C++ they are made of -- tk_jsonl_rule.h: the classes and
// masks of 64 bytes, a tile's summary, the carry's steps between the scans, select, the text pass, a line's status -- compiled for the host
// and driven the way the kernels drive it: a "wavefront" per tile of `tile` bytes (any multiple of 64: the result does not depend on it),
// its 64 lanes computed one after the other, the scans as loops, the line passes per line.  Every array lives in a heap block of exactly
// its size (jsonl_sanitize.cpp runs this file under the address sanitizer).  Test infrastructure only (tests/test_jsonl_sim.py builds it).
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/tiktoken_amd.h"
#include "../../tiktoken_amd/csrc/tk_jsonl_rule.h"

namespace {
struct SimJWave {  // the 64 lanes one after the other
    uint32_t regs[64], pres[64];
    template <class F>
    uint64_t ballot(F&& f) {
        uint64_t b = 0;
        for (uint32_t l = 0; l < 64; ++l)
            if (f(l)) b |= 1ull << l;
        return b;
    }
    template <class F>
    void each(F&& f) {
        for (uint32_t l = 0; l < 64; ++l) f(l);
    }
    template <class F>
    void once(F&& f) { f(); }
    template <class F>
    uint32_t scan(F&& f) {
        uint32_t run = 0;
        for (uint32_t l = 0; l < 64; ++l) {
            pres[l] = run;
            run += f(l);
        }
        return run;
    }
    uint32_t& reg(uint32_t l) { return regs[l]; }
    uint32_t pre(uint32_t l) const { return pres[l]; }
};
// exclusive scans in place, as tk_scan_blocks leaves them
template <class T>
uint64_t sum_scan(std::vector<T>& a) {
    uint64_t carry = 0;
    for (auto& x : a) {
        const T v = x;
        x = (T)carry;
        carry += (uint64_t)(uint32_t)v;
    }
    return carry;
}
void max_scan(std::vector<uint32_t>& a) {
    uint32_t carry = 0;
    for (auto& x : a) {
        const uint32_t v = x;
        x = carry;
        if (v > carry) carry = v;
    }
}
struct SelectOut {
    TkJsonlLines L;
    uint64_t* loff;
    uint64_t* ep;
    uint32_t n_lines;
    uint64_t W;
    bool* oob;
    bool ok(uint32_t line) const { return line < n_lines || (*oob = true, false); }
    void flag(uint32_t line, uint32_t bits) const { if (ok(line)) L.flags[line] |= bits; }
    void low(uint32_t line) const { if (ok(line)) L.low[line] += 1; }
    void vmax(uint32_t line, uint64_t v) const { if (ok(line) && v > L.vmax[line]) L.vmax[line] = v; }
    void line_off(uint32_t line, uint32_t pos) const {
        if (line > n_lines) *oob = true;
        else loff[line] = pos;
    }
    void eplane(uint32_t word, uint64_t m) const {
        if (word >= W) *oob = true;
        else ep[word] = m;
    }
};
struct TextSink {
    TkJsonlLines L;
    uint32_t* cnt;       // count pass
    const uint32_t* G;   // write pass
    const uint64_t* doc_off;
    uint8_t* text;
    uint64_t n_text;
    uint32_t tile, gt, n_lines;
    bool write;
    bool* oob;
    void bad(uint32_t line, uint32_t bits) const { if (!write) L.flags[line] |= bits; }
    void vstart(uint32_t line, uint32_t rel) const { if (!write) L.vs_rel[line] = rel; }
    void vend(uint32_t line, uint32_t pos, uint32_t rel) const { if (!write) L.ve_pos[line] = pos, L.ve_rel[line] = rel; }
    void bytes(uint32_t line, uint32_t rel, uint32_t v, uint32_t n) const {
        if (!write || L.status[line] != TK_JSONL_ST_OK || L.doc[line] == 0xFFFFFFFFu) return;
        const uint32_t vpos = (uint32_t)(L.vmax[line] >> 1) - 1u;
        const uint64_t at = doc_off[L.doc[line]] + ((gt + rel) - (G[vpos / tile] + L.vs_rel[line]));
        for (uint32_t i = 0; i < n; ++i) {
            if (at + i >= n_text) *oob = true;
            else text[at + i] = (uint8_t)(v >> (8u * i));
        }
    }
    void done(uint32_t t, uint32_t total) const { if (!write) cnt[t] = total; }
};
}  // namespace

extern "C" {
uint32_t jsonl_sim_tile(void) { return TK_JSONL_TILE; }
// Returns 0; -1: an index out of bounds; -(16 + why): tk_jsonl_shape's refusal; -3: more lines than cap_lines; 1: TK_JSONL_RAISE refuses,
// bad[0 .. 2] = line, byte offset, status.  text has room for n + 1 bytes, doc_off and line_off for cap_lines + 1 entries, line and status
// for cap_lines; counts[0 .. 2] = n_docs, n_lines, n_text.
int64_t jsonl_sim(const uint8_t* bytes_in, uint64_t n, const uint8_t* field, uint64_t flen, uint32_t mode, uint32_t tile, uint64_t cap_lines, uint8_t* text,
                  uint64_t* doc_off, uint64_t* doc_line, uint64_t* line_off, uint8_t* status, uint64_t* counts, uint64_t* bad) {
    TkJsonl j;
    const int why = tk_jsonl_shape(n, field, flen, mode, tile, &j);
    if (why) return -(16 + why);
    const std::vector<uint8_t> src(bytes_in, bytes_in + n);  // a block of exactly n bytes
    tk_jsonl_ends(&j, src.data());
    const uint32_t nt = j.n_tiles;
    const uint64_t W = (uint64_t)nt * (tile / 64u);
    bool oob = false;
    SimJWave w;
    std::vector<uint32_t> nonbs(nt), nl(nt), nonws(nt), lastq(nt), nnl(nt), nq(nt), lead(nt), qtail(nt), bits(nt), cnt(nt);
    std::vector<int32_t> d(nt), dhead0(nt), dhead1(nt), drest(nt), dtail(nt);
    const TkJsonlTiles T{nonbs.data(), nl.data(), nonws.data(), lastq.data(), nnl.data(), nq.data(), d.data(), lead.data(), qtail.data(),
                         dhead0.data(), dhead1.data(), drest.data(), dtail.data(), bits.data()};
    for (uint32_t t = 0; t < nt; ++t) tk_jsonl_tile_sum(j, w, t, T);
    // tk_k_jsonl_carry
    max_scan(nonbs), max_scan(nl), max_scan(nonws);
    const uint64_t n_lines = sum_scan(nnl);
    for (uint32_t t = 0; t < nt; ++t) tk_jsonl_carry_q(j, T, t);
    sum_scan(nq), max_scan(lastq);
    for (uint32_t t = 0; t < nt; ++t) tk_jsonl_carry_d(j, T, t);
    sum_scan(d);
    std::vector<TkJsonlCarry> entry(nt);
    for (uint32_t t = 0; t < nt; ++t) entry[t] = tk_jsonl_carry_entry(j, T, t);
    if (n_lines > cap_lines) return -3;
    // per line
    const uint32_t nl1 = (uint32_t)n_lines + 1u;
    std::vector<uint32_t> flags(nl1), low(nl1), vs_rel(nl1), ve_pos(nl1), ve_rel(nl1), len(nl1), doc(nl1);
    std::vector<uint64_t> vmax(nl1), loff(nl1), ep(W);
    std::vector<uint8_t> st(nl1);
    const TkJsonlLines L{flags.data(), low.data(), vs_rel.data(), ve_pos.data(), ve_rel.data(), len.data(), doc.data(), vmax.data(), st.data()};
    SelectOut sel{L, loff.data(), ep.data(), (uint32_t)n_lines, W, &oob};
    for (uint32_t t = 0; t < nt; ++t) tk_jsonl_tile_select(j, w, t, entry[t], sel);
    if (oob) return -1;
    TextSink sink{L, cnt.data(), nullptr, nullptr, nullptr, 0, tile, 0, (uint32_t)n_lines, false, &oob};
    for (uint32_t t = 0; t < nt; ++t) tk_jsonl_tile_text(j, w, t, entry[t], ep.data(), vmax.data(), sink);
    sum_scan(cnt);
    uint64_t n_docs = 0, n_text = 0, first_bad = ~0ull;
    for (uint32_t line = 0; line < n_lines; ++line) {
        tk_jsonl_line(j, L, cnt.data(), line);
        if (mode == TK_JSONL_M_RAISE && st[line] != TK_JSONL_ST_OK && st[line] != TK_JSONL_ST_BLANK && first_bad == ~0ull) first_bad = line;
    }
    if (first_bad != ~0ull) {
        bad[0] = first_bad, bad[1] = loff[first_bad], bad[2] = st[first_bad];
        return 1;
    }
    // tk_k_jsonl_docs
    for (uint32_t line = 0; line < n_lines; ++line) {
        const bool keep = tk_jsonl_keeps(mode, st[line]);
        doc[line] = keep ? (uint32_t)n_docs : 0xFFFFFFFFu;
        if (keep) {
            doc_off[n_docs] = n_text, doc_line[n_docs] = line;
            n_docs += 1, n_text += len[line];
        }
    }
    doc_off[n_docs] = n_text;
    if (n_text > n) return -1;
    sink.write = true, sink.G = cnt.data(), sink.doc_off = doc_off, sink.text = text, sink.n_text = n_text;
    memset(text, 0xAB, n_text);
    for (uint32_t t = 0; t < nt; ++t) {
        sink.gt = cnt[t];
        tk_jsonl_tile_text(j, w, t, entry[t], ep.data(), vmax.data(), sink);
    }
    for (uint32_t line = 0; line <= n_lines; ++line) line_off[line] = loff[line];
    for (uint32_t line = 0; line < n_lines; ++line) status[line] = st[line];
    counts[0] = n_docs, counts[1] = n_lines, counts[2] = n_text;
    return oob ? -1 : 0;
}
}
