// The back end of the encode pipeline (tiktoken_amd/csrc/tk_fused.h: tk_k_count_tiles, the scan, tk_k_place, tk_k_bigcopy) on the CPU: the
// rules the kernels take from tk_back_rule.h, compiled for the host and driven in the kernels' frame -- the count pass by half-wavefronts
// of 32 lanes in rounds of 32 * ROWS * 2 refs, a plain exclusive scan, the place pass by wavefronts in steps of 256 pieces, four per
// lane, with the list of listed pieces, its prefix sums, the documents in chunks of sixty-four and both the staged and the direct form
// of a tile.  The frame itself (what crosses lanes, the lists, loads and stores) is written again here.  starts, res and cnt8 are read
// through index-checked readers over exactly the words the host gives the device buffers.
// Test infrastructure only (tests/test_back_sim.py builds it).
#include <stdint.h>

#include <vector>

#include "../../tiktoken_amd/csrc/tk_back_rule.h"
#include "sim_readers.h"

namespace {
constexpr uint32_t NONE = 0xFFFFFFFFu;
struct Miss {  // TkMiss: table slots of 16 words {start, len, res_cnt, tok[13]}, overflow entries of 4 {start, len, res_cnt, res_tok}
    SimArray<uint32_t> tab, ovf;
    uint32_t ovf_base;
    SimArray<uint8_t> cnt8;
    uint32_t head(uint32_t i, uint32_t k) const { return i < ovf_base ? tab[16ull * i + k] : ovf[4ull * (i - ovf_base) + k]; }
};
uint32_t inclusive_scan(uint32_t (&v)[64]) {  // tk_wave_scan_u32 over the wavefront; returns lane 63's
    for (int l = 1; l < 64; ++l) v[l] += v[l - 1];
    return v[63];
}
}  // namespace

extern "C" {
uint64_t back_sim_res_words(uint64_t n) { return tk_pid_cap(n); }
uint64_t back_sim_starts_words(uint64_t n, uint64_t ntiles) { return tk_starts_words((n + 31) / 32, ntiles); }

// sizes: {res words, starts words, tab slots (= ovf_base), ovf entries, cnt8 bytes, staging words, out words, count-pass ROWS, wavefronts of the count pass}
// stats out: {total tokens, pieces, tiles placed through LDS, entries left to the big copy}
// Returns 0; -1: an access out of bounds (a reader, an LDS list, the output, tok_off).
int64_t back_sim(uint64_t n, uint64_t ntiles, const uint32_t* tile_np_in, const uint32_t* res_in, const uint32_t* tab_in, const uint32_t* ovf_in, const uint8_t* cnt8_in,
                 const uint32_t* staging_in, const uint32_t* starts_in, const uint64_t* doc_off_in, uint64_t n_docs, const uint32_t* doc_first_in, uint64_t chunk_base,
                 uint64_t tok_base, const uint64_t* sizes, uint32_t* out, uint64_t* tok_off, uint32_t* tile_nt, uint64_t* stats) {
    bool oob = false;
    const SimArray<uint32_t> tile_np{tile_np_in, ntiles, &oob}, res{res_in, sizes[0], &oob}, starts{starts_in, sizes[1], &oob}, staging{staging_in, sizes[5], &oob};
    const SimArray<uint32_t> doc_first{doc_first_in, ntiles + 1, &oob};
    const SimOffsets doc_off{doc_off_in, n_docs, &oob};
    const Miss data{{tab_in, 16 * sizes[2], &oob}, {ovf_in, 4 * sizes[3], &oob}, (uint32_t)sizes[2], {cnt8_in, sizes[4], &oob}};
    const uint64_t out_cap = sizes[6];
    const uint32_t ROWS = (uint32_t)sizes[7];
    auto put_out = [&](uint64_t i, uint32_t v) {
        if (i >= out_cap) oob = true;
        else out[i] = v;
    };

    // ---- tk_k_count_tiles<ROWS>: half a wavefront per tile, both halves walk the longer list
    const uint64_t nhalves = 2 * sizes[8], rounds = (ntiles + nhalves - 1) / nhalves;
    uint64_t pieces = 0;
    for (uint64_t wave = 0; wave < sizes[8]; ++wave)
        for (uint64_t r = 0; r < rounds; ++r) {
            uint32_t np[2], rb[2], ng[2], nm[2], extra[2][32] = {};
            bool have[2];
            for (int h = 0; h < 2; ++h) {
                const uint64_t t = 2 * wave + h + r * nhalves;
                have[h] = t < ntiles;
                np[h] = have[h] ? tile_np[t] : 0u;
                rb[h] = have[h] ? (uint32_t)t * TKF_CAP : 0u;
                pieces += np[h];
                ng[h] = np[h] ? res[rb[h] + TKF_TAIL_NGAP] : 0u;
                nm[h] = np[h] ? res[rb[h] + TKF_TAIL_NMISS] : 0u;
            }
            const uint32_t nm_max = nm[0] > nm[1] ? nm[0] : nm[1];
            for (uint32_t q0 = 0; q0 < nm_max; q0 += 32u * ROWS * 2u) {
                std::vector<uint32_t> ref(64 * ROWS * 2), cb(64 * ROWS * 2);
                bool escape = false;  // (the ballot: any lane of the wavefront)
                for (int h = 0; h < 2; ++h)
                    for (uint32_t hl = 0; hl < 32; ++hl)
                        for (uint32_t j = 0; j < ROWS * 2; ++j) {
                            const uint32_t q = q0 + j * 32u + hl, at = (h * 32 + hl) * ROWS * 2 + j;
                            ref[at] = res[rb[h] + TKF_TAIL_REFS - (q < nm[h] ? q : 0u)];
                            if (q >= nm[h]) ref[at] = TKF_NONE;
                            const bool in_tab = TK_REF_IN_TAB(ref[at], data.ovf_base);
                            cb[at] = data.cnt8[TK_REF_CNT8_AT(ref[at], in_tab)];
                            if (TK_REF_ESCAPES(ref[at], in_tab, cb[at])) escape = true;
                            else if (in_tab) extra[h][hl] += cb[at] - 1u;
                        }
                if (escape)
                    for (int h = 0; h < 2; ++h)
                        for (uint32_t hl = 0; hl < 32; ++hl)
                            for (uint32_t j = 0; j < ROWS * 2; ++j) {
                                const uint32_t at = (h * 32 + hl) * ROWS * 2 + j;
                                const bool in_tab = TK_REF_IN_TAB(ref[at], data.ovf_base), esc = TK_REF_ESCAPES(ref[at], in_tab, cb[at]);
                                const uint32_t cw = data.head(TK_REF_HEAD_AT(ref[at], esc, data.ovf_base), 2);
                                if (esc) extra[h][hl] += TKD_COUNT(cw) - 1u;
                            }
            }
            for (int h = 0; h < 2; ++h) {
                uint32_t sum = 0;
                for (uint32_t hl = 0; hl < 32; ++hl) sum += extra[h][hl];
                if (have[h]) tile_nt[2 * wave + h + r * nhalves] = TK_TILE_TOKENS(np[h], ng[h], sum);
            }
        }
    // ---- the scan: tile_nt becomes the tiles' places
    const uint64_t total = sim_scan(tile_nt, ntiles);
    const uint32_t* tile_tb = tile_nt;

    // ---- tk_k_place<1>: a wavefront per tile
    constexpr uint32_t CAP = 256u, SCAP = (uint32_t)TKP_STAGE;
    std::vector<uint32_t> stl(SCAP + 4), refl(CAP), cuml(CAP), idxl(CAP);
    std::vector<uint32_t> big;  // {staging position, output position, count}
    uint64_t n_staged = 0;
    const bool want_docs = tok_off != nullptr;
    auto put_off = [&](uint64_t d, uint64_t v) {
        if (d > n_docs) oob = true;
        else tok_off[d] = v;
    };
    for (uint64_t t = 0; t < ntiles; ++t) {
        const uint32_t np = tile_np[t], rb = (uint32_t)t * TKF_CAP, run0 = tile_tb[t];
        const uint32_t nt_tile = (t + 1 < ntiles ? tile_tb[t + 1] : NONE) - run0;
        const uint32_t dfirst = want_docs ? doc_first[t] : NONE;
        const bool has_docs = dfirst != NONE;
        const uint64_t tile_lo = t * (uint64_t)TK_TILE, tile_hi = tile_lo + TK_TILE < n ? tile_lo + TK_TILE : n;
        auto doc_piece = [&](uint32_t c, uint32_t (&kp)[64]) -> bool {  // all sixty-four start here
            uint32_t sb0[64] = {}, sb1[64] = {}, spx[64];
            for (uint32_t lane = 0; lane < TK_TILE / 64; ++lane) {
                sb0[lane] = starts[t * (TK_TILE / 32) + 2u * lane];
                sb1[lane] = starts[t * (TK_TILE / 32) + 2u * lane + 1u];
            }
            for (uint32_t lane = 0, sum = 0; lane < 64; ++lane) {
                spx[lane] = sum;
                sum += (uint32_t)__builtin_popcount(sb0[lane]) + (uint32_t)__builtin_popcount(sb1[lane]);
            }
            bool all = true;
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const uint64_t d = (uint64_t)dfirst + 64u * c + lane;
                const uint64_t pos = d < n_docs ? doc_off[d] - chunk_base : ~0ull;
                const bool in = pos >= tile_lo && pos < tile_hi;
                const uint32_t it = in ? (uint32_t)(pos - tile_lo) : 0u, g = TK_START_GROUP(it);
                const uint32_t kpl = TK_PIECE_INDEX(it, sb0[g], sb1[g], spx[g]);
                kp[lane] = in ? kpl : NONE;
                all = all && in;
            }
            return all;
        };
        uint32_t kp0[64];
        for (uint32_t& k : kp0) k = NONE;
        const bool more_docs = has_docs && doc_piece(0u, kp0);
        const bool ST = np != 0u && nt_tile <= SCAP;
        n_staged += ST;
        auto W = [&](uint32_t off, uint32_t v) {
            if (!ST) put_out((uint32_t)(run0 + off), v);
            else if (off >= SCAP + 4) oob = true;
            else stl[off] = v;
        };
        uint32_t run = 0;
        for (uint32_t k0 = 0; k0 < np; k0 += CAP) {
            uint32_t tk[64][4], fm[64], lbase[64], nlist = 0;
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const uint32_t k = k0 + lane * 4u;
                for (uint32_t j = 0; j < 4; ++j) {
                    const uint32_t w = res[rb + (k < np ? k : 0u) + j];  // (sixteen bytes, whatever is there)
                    tk[lane][j] = k + j < np ? w : TK_RES_GAP;
                }
                fm[lane] = 0;
                lbase[lane] = nlist;
                for (uint32_t j = 0; j < 4; ++j)
                    if (TK_RES_LISTED(tk[lane][j])) {
                        fm[lane] |= 1u << j;
                        if (nlist >= CAP) return -1;
                        refl[nlist] = tk[lane][j];
                        idxl[nlist] = lane * 4u + j;
                        ++nlist;
                    }
            }
            uint32_t carry = 0;
            for (uint32_t d0 = 0; d0 < nlist; d0 += 64u) {
                uint32_t incx[64], cnt[64], hx[64], hy[64], off[64], ent[64];
                bool flagged[64], stg[64];
                for (uint32_t lane = 0; lane < 64; ++lane) {
                    const uint32_t d = d0 + lane;
                    const bool have = d < nlist;
                    const uint32_t w = have ? refl[d] : TK_RES_GAP;
                    flagged[lane] = TK_RES_FLAGGED(w);
                    ent[lane] = TK_RES_ENTRY(w);
                    const uint32_t at = flagged[lane] ? ent[lane] : data.ovf_base;  // (a lane without an entry reads the first overflow entry)
                    hx[lane] = data.head(at, 2);
                    hy[lane] = data.head(at, 3);
                    cnt[lane] = flagged[lane] ? TKD_COUNT(hx[lane]) : 0u;
                    incx[lane] = have ? cnt[lane] - 1u : 0u;
                }
                uint32_t extra[64];
                for (uint32_t lane = 0; lane < 64; ++lane) extra[lane] = incx[lane];
                const uint32_t last = inclusive_scan(incx);
                for (uint32_t lane = 0; lane < 64; ++lane) {
                    const uint32_t d = d0 + lane, cum = carry + incx[lane];
                    if (d < nlist) cuml[d] = cum;
                    off[lane] = TK_PIECE_PLACE(run, d < nlist ? idxl[d] : 0u, cum, extra[lane]);
                    stg[lane] = false;
                    if (flagged[lane]) {
                        if (TK_FROM_HEAD(cnt[lane])) {
                            W(off[lane], hy[lane]);
                        } else if (TK_FROM_ENTRY(hx[lane])) {
                            for (uint32_t i = 0; i < cnt[lane] && i < (uint32_t)TKD_INLINE; ++i) W(off[lane] + i, data.tab[16ull * ent[lane] + 3u + i]);
                        } else if (TK_FROM_STAGING(cnt[lane])) {
                            stg[lane] = true;
                        }
                    }
                }
                carry += last;
                for (uint32_t lane = 0; lane < 64; ++lane)  // the staging area's pieces, one at a time
                    if (stg[lane]) {
                        if (TK_COPIED_IN_PLACE(ST, cnt[lane]))
                            for (uint32_t i = 0; i < cnt[lane]; ++i) W(off[lane] + i, staging[hy[lane] + i]);
                        else big.insert(big.end(), {hy[lane], run0 + off[lane], cnt[lane]});
                    }
            }
            if (has_docs) {
                auto emit = [&](const uint32_t (&kp)[64], uint32_t c) {
                    for (uint32_t lane = 0; lane < 64; ++lane) {
                        if (!(kp[lane] != NONE && kp[lane] >= k0 && kp[lane] < k0 + CAP)) continue;
                        const uint32_t j = kp[lane] - k0, src = (j & 255u) >> 2;
                        const uint32_t nl = lbase[src] + (uint32_t)__builtin_popcount(fm[src] & ((1u << (j & 3u)) - 1u));
                        const uint32_t ex = nl ? cuml[nl - 1u] : 0u;
                        put_off((uint64_t)dfirst + 64u * c + lane, TK_DOC_TOK_OFF(tok_base, run0, run, j, ex));
                    }
                };
                emit(kp0, 0u);
                if (more_docs)
                    for (uint32_t c = 1;; ++c) {
                        uint32_t kp[64];
                        const bool all = doc_piece(c, kp);
                        emit(kp, c);
                        if (!all) break;
                    }
            }
            for (uint32_t lane = 0; lane < 64; ++lane) {  // the single tokens: place = index + the sum over the listed pieces before
                uint32_t rk = lbase[lane], ex = rk ? cuml[rk - 1u] : 0u;
                const uint32_t o = run + lane * 4u;
                if (fm[lane] == 15u) continue;
                for (uint32_t j = 0; j < 4; ++j) {
                    if ((fm[lane] >> j) & 1u) ex = cuml[rk++];
                    else W(o + j + ex, tk[lane][j]);
                }
            }
            run += CAP + carry;  // (a step's dead words cancel out: one piece, minus one)
        }
        if (ST)
            for (uint32_t i = 0; i < nt_tile; ++i) put_out(run0 + i, stl[i]);
        if (want_docs && t + 1 == ntiles) {
            const uint32_t dl = doc_first[ntiles];
            for (uint64_t d = dl == NONE ? n_docs : (uint64_t)dl; d <= n_docs; ++d) put_off(d, tok_base + total);
        }
    }
    // ---- tk_k_bigcopy
    for (uint64_t e = 0; e + 2 < big.size(); e += 3)
        for (uint32_t i = 0; i < big[e + 2]; ++i) put_out(big[e + 1] + i, staging[big[e] + i]);
    stats[0] = total;
    stats[1] = pieces;
    stats[2] = n_staged;
    stats[3] = big.size() / 3;
    return oob ? -1 : 0;
}
}
