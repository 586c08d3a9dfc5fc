// The long-piece merges (tk_k_merge_rounds, tk_k_merge_rounds_wide, tk_k_merge_long of tiktoken_amd/csrc/tk_fused.h) on the CPU: the plain
// C++ they are made of -- tk_merge_rule.h -- compiled for the host and driven the way the kernels drive it.  A piece is shared by NWV
// wavefronts; each walks its range in rows of 512 (64 lanes x 8 parts); what the kernels do across lanes (the scan of run states, the
// sums, the ballot for the leading run) is done here by plain loops over the lanes' values.  A round runs phase by phase -- b: the ranges'
// summaries; the prefix over them (the narrow loop, or the wide form: a block of summaries per lane, two hypotheses, the owner's walk);
// c: the survivors move; d: the new pairs' ranks and the next minimum -- with a count of the phase boundaries per wavefront.  Within a
// phase wavefronts, lanes and threads run in an order a seed chooses.  P0/R0/P1/R1 are heap blocks of exactly n entries, every index
// is checked, and every survivor slot of a round has to be written exactly once.  A round that is not valid marks the piece REDO: it
// then goes through the level tree of tk_k_merge_long, one merge at a time, with the same header's level arithmetic, link update and
// refresh list.  Test infrastructure only (tests/test_merge_sim.py builds it; tests/hostsim/merge_sanitize.cpp includes it).
#include <stdint.h>

#include <algorithm>
#include <memory>
#include <numeric>
#include <vector>

#include "../../tiktoken_amd/csrc/tk_merge_rule.h"

enum {
    MS_OOB = -1,      // a buffer was indexed out of bounds
    MS_TWICE = -2,    // a slot of P1/R1 written twice in one round
    MS_NEVER = -3,    // a survivor slot never written
    MS_OUTSIDE = -4,  // a slot at or beyond the round's total written
    MS_BARRIER = -5,  // the simulation's own phase count differs between wavefronts (cannot happen as it is written)
    MS_TOTAL = -6,    // the wavefronts disagree about the round's total
    MS_TREE = -7,     // after a merge the level tree is not the tree of the ranks
    MS_ROUNDS = -8,   // more rounds than parts
};
enum { MS_VIOL_BETWEEN = 1, MS_VIOL_LASTING = 2 };

template <class T>
struct Buf {  // a heap block of exactly n entries; an index beyond it is reported, not used
    std::unique_ptr<T[]> p;
    uint64_t n;
    int64_t* err;
    T dummy = 0;
    Buf(uint64_t n_, int64_t* err_) : p(new T[n_ ? n_ : 1]), n(n_), err(err_) {}
    T& operator[](uint64_t i) {
#ifdef MERGE_SIM_RAW  // (merge_sanitize.cpp: AddressSanitizer watches the block instead)
        return p[i];
#endif
        if (i >= n) {
            if (!*err) *err = MS_OOB;
            return dummy = 0;
        }
        return p[i];
    }
};
template <class T>
struct Ref {  // what the header's functions get: copyable, indexes the block
    Buf<T>* b;
    T& operator[](uint64_t i) const { return (*b)[i]; }
};

struct SimTables {
    const uint32_t *byte_rank, *pair2;
};
struct SimPairs {  // (a, b) -> the rank of the token that is a's bytes and b's: keys a << 32 | b, ascending
    const uint64_t* keys;
    const uint32_t* vals;
    uint64_t n;
    uint32_t operator()(uint32_t a, uint32_t b) const {
        const uint64_t key = ((uint64_t)a << 32) | b;
        const uint64_t* it = std::lower_bound(keys, keys + n, key);
        return it != keys + n && *it == key ? vals[it - keys] : TK_RANK_MAX;
    }
};

// 0 .. n - 1 in the order of the seed: 0 ascending, 1 descending, otherwise shuffled
static std::vector<uint32_t> order_of(uint32_t n, uint64_t seed) {
    std::vector<uint32_t> o(n);
    std::iota(o.begin(), o.end(), 0);
    if (seed == 1) std::reverse(o.begin(), o.end());
    if (seed > 1) {
        uint64_t x = seed * 0x9E3779B97F4A7C15ull + n;
        for (uint32_t k = n; k > 1; --k) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            std::swap(o[k - 1], o[(x >> 33) % k]);
        }
    }
    return o;
}

struct MergeCase {
    const uint8_t* text;
    uint32_t n;
    SimTables T;
    SimPairs probe;
    uint32_t nwv;  // wavefronts that share the piece
    bool wide;     // the prefix over the summaries in the wide form
    uint64_t seed;
};
// result: [0] tokens, [1] rounds, [2] MS_VIOL_* of the round that was not valid, [3] barriers every wavefront passed, [4] merges of the
// level tree, [5..7] of them with 1 / 2 / 3 blocks to refresh at level 1, [8] at the first part, [9] with the last part, [10] levels
enum { MS_RESULTS = 11 };

// ---------------------------------------------------------------- tk_k_merge_long: one wavefront, one merge at a time
static int64_t long_piece(const MergeCase& C, uint32_t* out, uint64_t* result) {
    int64_t err = 0;
    const uint32_t n = C.n;
    struct {
        int nl;
        uint32_t cnt[TK_MAX_LEVELS + 1], off[TK_MAX_LEVELS + 1];
    } L;
    L.nl = tk_long_levels(n, L.cnt, L.off);
    uint64_t lv_n = 0;
    for (int l = 1; l <= L.nl; ++l) lv_n += L.cnt[l];
    Buf<uint32_t> b_id(n, &err), b_rk(n, &err), b_nx(n, &err), b_pv(n, &err);
    Buf<uint64_t> b_lv(lv_n, &err);
    const Ref<uint32_t> id{&b_id}, rk{&b_rk}, nx{&b_nx}, pv{&b_pv};
    const Ref<uint64_t> lv{&b_lv};
    for (const uint32_t k : order_of(n, C.seed)) {
        uint32_t a, r;
        tk_piece_part(C.T, C.text, 0, k, n, a, r);
        id[k] = a, rk[k] = r, nx[k] = k + 1, pv[k] = k - 1;
    }
    auto block_min = [&](int l, uint32_t b) {
        uint64_t key = ~0ull;
        for (uint32_t lane = 0; lane < 64; ++lane) key = std::min(key, tk_long_key(L.cnt, L.off, l, b * 64 + lane, rk, lv));
        return key;
    };
    for (int l = 1; l <= L.nl; ++l)
        for (uint32_t b = 0; b < L.cnt[l]; ++b) lv[L.off[l] + b] = block_min(l, b);
    result[10] = (uint64_t)L.nl;
    for (;;) {
        uint64_t top = ~0ull;
        for (uint32_t lane = 0; lane < 64 && lane < L.cnt[L.nl]; ++lane) top = std::min(top, (uint64_t)lv[L.off[L.nl] + lane]);
        const uint32_t m = (uint32_t)(top >> 32);
        if (m == TK_RANK_MAX || err) break;
        const uint32_t i = (uint32_t)top, j = nx[i], nn = nx[j], pp = pv[i];
        const uint32_t r_i = nn < n ? C.probe(m, id[nn]) : TK_RANK_MAX;  // (lane 0)
        const uint32_t r_p = pp != TK_LONG_NONE ? C.probe(id[pp], m) : TK_RANK_MAX;  // (lane 1)
        tk_long_link(id, rk, nx, pv, n, m, i, j, nn, r_i);
        if (pp != TK_LONG_NONE) rk[pp] = r_p;
        for (int l = 1; l <= L.nl; ++l) {
            const TkLongBlocks B = tk_long_blocks(l, i, j, pp);
            for (int t = 0; t < 3; ++t)
                if (B.on[t]) lv[L.off[l] + B.b[t]] = block_min(l, B.b[t]);
            if (l == 1) ++result[4 + B.on[0] + B.on[1] + B.on[2]];
        }
        ++result[4];
        result[8] += i == 0;
        result[9] += nn >= n;
        if (n <= 8192)  // the whole tree, from the ranks: nothing stale
            for (int l = 1; l <= L.nl; ++l)
                for (uint32_t b = 0; b < L.cnt[l]; ++b)
                    if (lv[L.off[l] + b] != block_min(l, b)) return MS_TREE;
    }
    uint32_t t = 0;
    for (uint32_t k = 0; k < n; ++k)
        if (id[k] != TK_RANK_MAX) out[t++] = id[k];
    result[0] = t;
    return err;
}

// ---------------------------------------------------------------- tk_rounds_piece
// returns 0 and result[2] == 0: the tokens are in out; result[2] != 0: the piece is marked REDO
static int64_t rounds_piece(const MergeCase& C, uint32_t* out, uint64_t* result) {
    constexpr uint32_t EPL = TK_MERGE_EPL, ROW = 64 * EPL;
    int64_t err = 0;
    const uint32_t n = C.n, NWV = C.nwv, gthreads = NWV * 64;
    Buf<uint32_t> bufs[4] = {{n, &err}, {n, &err}, {n, &err}, {n, &err}};
    Buf<uint32_t>*P0 = &bufs[0], *R0 = &bufs[1], *P1 = &bufs[2], *R1 = &bufs[3];
    std::vector<uint64_t> bar(NWV, 0);
    // bar[w]: the phase boundaries wavefront w has passed -- where the kernel has sync() or all_min.  It documents the phase structure
    // (result[3]); every wavefront is counted without condition, so it says nothing about the kernel's own control flow
    auto barrier = [&]() {
        for (uint32_t w = 0; w < NWV; ++w) ++bar[w];
    };
    uint32_t m = TK_RANK_MAX;
    for (const uint32_t t : order_of(std::min(gthreads, n), C.seed))
        for (uint32_t k = t; k < n; k += gthreads) {
            uint32_t a, r;
            tk_piece_part(C.T, C.text, 0, k, n, a, r);
            (*P0)[k] = a, (*R0)[k] = r;
            m = std::min(m, r);
        }
    barrier();
    uint32_t cnt = n, viol = 0;
    uint64_t rounds = 0;
    while (m != TK_RANK_MAX && !err) {
        if (++rounds > n) return MS_ROUNDS;
        const uint32_t per = ((cnt + NWV - 1) / NWV + ROW - 1u) / ROW * ROW;
        struct Row {
            uint32_t rk[64][EPL], n_in[64], fm[64];
            TkRunState inc[64];  // the inclusive scan of the lanes' states
            TkRunState before(uint32_t lane) const { return lane ? inc[lane - 1] : TkRunState{1u, 0u}; }
        };
        auto range = [&](uint32_t w, uint32_t& wlo, uint32_t& whi) {
            wlo = (uint64_t)w * per < cnt ? w * per : cnt;
            whi = wlo + per < cnt ? wlo + per : cnt;
        };
        auto load_row = [&](uint32_t r0, uint32_t whi, Row& row, const std::vector<uint32_t>& lanes) {
            TkRunState st[64];
            for (const uint32_t lane : lanes) {
                const uint32_t i0 = r0 + EPL * lane;
                const uint32_t n_in = row.n_in[lane] = i0 < whi ? (whi - i0 < EPL ? whi - i0 : EPL) : 0u;
                for (uint32_t q = 0; q < EPL; ++q) row.rk[lane][q] = q < n_in ? (*R0)[i0 + q] : 0u;
                st[lane] = tk_merge_lane_state(row.rk[lane], m, n_in, row.fm[lane]);
            }
            for (uint32_t lane = 0; lane < 64; ++lane) row.inc[lane] = lane ? tk_run_combine(row.inc[lane - 1], st[lane]) : st[0];
        };
        const std::vector<uint32_t> waves = order_of(NWV, C.seed), lanes = order_of(64, C.seed + (C.seed > 1));
        // b. the summary of every wavefront's range
        std::vector<TkRangeSum> sc(NWV);
        for (const uint32_t w : waves) {
            uint32_t wlo, whi, keep0 = 0, lead = 0;
            range(w, wlo, whi);
            TkRunState acc{1u, 0u};
            bool open = true;
            for (uint32_t r0 = wlo; r0 < whi; r0 += ROW) {
                Row row;
                load_row(r0, whi, row, lanes);
                for (const uint32_t lane : lanes) keep0 += tk_merge_lane_rule(tk_run_combine(acc, row.before(lane)).par, row.fm[lane], row.n_in[lane]).count;
                if (open) {
                    uint32_t l0 = 0;
                    while (l0 < 64 && row.fm[l0] == (1u << EPL) - 1u) ++l0;
                    if (l0 < 64) {
                        lead += l0 * EPL + (uint32_t)__builtin_ctz(~row.fm[l0]);
                        open = false;
                    } else
                        lead += ROW;
                }
                acc = tk_run_combine(acc, row.inc[63]);
            }
            sc[w] = tk_range_summary(acc, keep0, lead, whi - wlo);
            ++bar[w];
        }
        // the prefix over the summaries, as wavefront w computes it
        struct Place {
            TkRunState before;
            uint32_t at, total;
        };
        auto place = [&](uint32_t w) {
            Place p{{1u, 0u}, 0, 0};
            if (C.wide) {
                const uint32_t blk = (NWV + 63u) / 64u;
                TkRunState mine[64], ex[64];
                uint32_t k0[64], k1[64], kl[64], kinc[64];
                for (const uint32_t lane : lanes) {
                    mine[lane] = TkRunState{1u, 0u};
                    k0[lane] = k1[lane] = 0;
                    for (uint32_t j = 0; j < blk; ++j) {
                        const uint32_t q = lane * blk + j;
                        if (q < NWV) {
                            TkRunState odd_in = tk_run_combine(TkRunState{1u, 1u}, mine[lane]);
                            k1[lane] += tk_range_enter(odd_in, sc[q]);
                            k0[lane] += tk_range_enter(mine[lane], sc[q]);
                        }
                    }
                }
                TkRunState run{1u, 0u};
                uint32_t sum = 0;
                for (uint32_t lane = 0; lane < 64; ++lane) {
                    ex[lane] = run;
                    run = tk_run_combine(run, mine[lane]);
                    kl[lane] = ex[lane].par ? k1[lane] : k0[lane];
                    kinc[lane] = sum += kl[lane];
                }
                p.total = kinc[63];
                const uint32_t owner = w / blk;
                p.before = ex[owner];
                p.at = kinc[owner] - kl[owner];
                for (uint32_t q = owner * blk; q < w; ++q) p.at += tk_range_enter(p.before, sc[q]);
            } else {
                TkRunState st{1u, 0u};
                for (uint32_t q = 0; q < NWV; ++q) {
                    if (q == w) p.before = st;
                    const uint32_t k = tk_range_enter(st, sc[q]);
                    if (q < w) p.at += k;
                    p.total += k;
                }
            }
            return p;
        };
        // c. the survivors move to their places: every slot below the total once, none beyond
        std::vector<uint8_t> written(n, 0);
        const auto rank0 = [&](uint32_t k) { return (*R0)[k]; };
        const auto id0 = [&](uint32_t k) { return (*P0)[k] & ~TK_MERGE_MARK; };
        const auto put = [&](uint32_t o, uint32_t part, uint32_t r) {
            if (o < n && written[o]++ && !err) err = MS_TWICE;
            (*P1)[o] = part, (*R1)[o] = r;
        };
        uint32_t total = 0;
        bool first = true, bad = false;
        for (const uint32_t w : waves) {
            uint32_t wlo, whi;
            range(w, wlo, whi);
            // (a wavefront without parts computes the same prefix and moves nothing: the first and the last of them stand for the rest --
            // the wide geometry has a thousand, of 64 x 16 summaries each)
            if (wlo < whi || w == NWV - 1 || w * (uint64_t)per < cnt + per) {
                Place p = place(w);
                if (!first && p.total != total) return MS_TOTAL;
                total = p.total, first = false;
                TkRunState carry = p.before;
                for (uint32_t r0 = wlo; r0 < whi; r0 += ROW) {
                    Row row;
                    load_row(r0, whi, row, lanes);
                    TkLaneKeep kp[64];
                    uint32_t ex[64], sum = 0;
                    for (const uint32_t lane : lanes) kp[lane] = tk_merge_lane_rule(tk_run_combine(carry, row.before(lane)).par, row.fm[lane], row.n_in[lane]);
                    for (uint32_t lane = 0; lane < 64; ++lane) ex[lane] = sum, sum += kp[lane].count;
                    for (const uint32_t lane : lanes)
                        bad |= tk_round_move_lane(m, r0 + EPL * lane, kp[lane].mask, row.fm[lane], row.rk[lane], p.at + ex[lane], cnt, rank0, id0, put, C.probe);
                    p.at += sum;
                    carry = tk_run_combine(carry, row.inc[63]);
                }
            }
            ++bar[w];
        }
        if (err) return err;
        for (uint32_t o = 0; o < n; ++o) {
            if (o < total && !written[o]) return MS_NEVER;
            if (o >= total && written[o]) return MS_OUTSIDE;
        }
        if (bad) viol |= MS_VIOL_BETWEEN;
        // d. the ranks of the pairs a merge has touched, the lowest rank of the next round
        uint32_t mn = TK_RANK_MAX;
        bad = false;
        for (const uint32_t t : order_of(std::min(gthreads, total), C.seed))
            for (uint32_t j = t; j < total; j += gthreads)
                mn = std::min(mn, tk_round_rank(
                                      m, j, total, [&](uint32_t k) { return (*P1)[k]; }, [&](uint32_t k) { return (*R1)[k]; },
                                      [&](uint32_t k, uint32_t v) { (*R1)[k] = v; }, C.probe, bad));
        if (bad) viol |= MS_VIOL_LASTING;
        barrier();
        m = mn;
        for (uint32_t w = 1; w < NWV; ++w)
            if (bar[w] != bar[0]) return MS_BARRIER;
        if (viol) break;
        std::swap(P0, P1), std::swap(R0, R1);
        cnt = total;
    }
    if (!viol)
        for (uint32_t k = 0; k < cnt; ++k) out[k] = (*P0)[k] & ~TK_MERGE_MARK;
    barrier();
    result[0] = cnt, result[1] = rounds, result[2] = viol, result[3] = bar[0];
    return err;
}

// the piece as the host sends it: in rounds, and if they mark it REDO (or the test says so: force_long) one merge at a time
static int64_t merge_piece(const MergeCase& C, bool force_long, uint32_t* out, uint64_t* result) {
    std::fill(result, result + MS_RESULTS, 0);
    int64_t rc = force_long ? 0 : rounds_piece(C, out, result);
    if (!rc && (force_long || result[2])) rc = long_piece(C, out, result);
    return rc;
}

extern "C" {
// out: room for n tokens; result: MS_RESULTS entries.  Returns 0 or one of the codes above.
int64_t merge_sim(const uint8_t* text, uint32_t n, const uint32_t* byte_rank, const uint32_t* pair2, const uint64_t* keys, const uint32_t* vals, uint64_t n_pairs,
                  uint32_t nwv, int wide, uint64_t seed, int force_long, uint32_t* out, uint64_t* result) {
    const MergeCase C{text, n, SimTables{byte_rank, pair2}, SimPairs{keys, vals, n_pairs}, nwv, wide != 0, seed};
    return merge_piece(C, force_long != 0, out, result);
}
// the level counts and offsets of a piece of n parts: cnt and off hold TK_MAX_LEVELS + 1 entries; returns the number of levels
int merge_sim_levels(uint32_t n, uint32_t* cnt, uint32_t* off) {
    return tk_long_levels(n, cnt, off);
}
}
