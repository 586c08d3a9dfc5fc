// The packed-sample-rows passes (tiktoken_amd/csrc/tk_sample_rows.h) on the CPU: the plain C++ they are made of -- tk_sample_rows_rule.h on
// top of tk_samples_rule.h: the placed lengths, the successor search, the rounds of pointer doubling, a sample's row and column, a row's
// segments, a whole lane of the write pass -- compiled for the host and driven the way the kernels drive it: one entry per sample, the
// rounds one after the other with their entries in ascending or descending order (the result may not depend on it), lanes of eight
// positions, workgroups of `block` positions, every array behind a reader that checks the index.  Test infrastructure only
// (tests/test_sample_rows_sim.py builds it: as a shared library, and with -DSAMPLE_ROWS_SIM_MAIN as a program of its own under the address
// and undefined-behaviour sanitizers, which reads a case file and writes the results).
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../tiktoken_amd/csrc/tk_sample_rows_rule.h"
#include "sim_readers.h"

namespace {
using SimRoles = TkSmpRoles<SimArray<uint32_t>, SimArray<uint32_t>, SimArray<uint8_t>>;
using SimIn = TkSmpIn<SimOffsets, SimOffsets, SimArray<uint8_t>, SimArray<uint64_t>>;
using SimRows = TkSrowIn<SimArray<uint64_t>, SimArray<uint64_t>, SimArray<uint32_t>, SimArray<uint32_t>>;
// cu_seqlens as the lanes fill it: every index below n_segs exactly once
struct SimCu {
    uint32_t* cu;
    uint64_t n;
    uint8_t* seen;
    bool *oob, *twice;
    void put(uint32_t index, uint32_t position) const {
        if (index >= n) {
            *oob = true;
            return;
        }
        if (seen[index]) *twice = true;
        seen[index] = 1;
        cu[index] = position;
    }
};
}  // namespace

extern "C" {
// Everything before the host's wait: tk_k_smp_count / _scan / _samples, tk_k_srow_plen / _sums / _succ, tk_srow_rounds launches of
// tk_k_srow_double (order: 0 entries ascending, 1 descending), tk_k_srow_rows / _place / _segs, and the host behind them.  counts = {R,
// n_segs}.  Returns 0; 1 .. 12: tk_srow_shape's / tk_srow_size's refusal; 16 + tk_rows_bad_key: tok_off is refused; 2^40 + tk_rows_bad_key:
// sample_off is; 2^41 + p: part p has no role; -1: an index out of bounds.  pstart: room for n_parts + 1; full .. sample_col: n_samples;
// c, f, row_sample, row_seg: n_samples + 1.
int64_t sample_rows_sim_place(uint64_t T, const uint64_t* tok_off, uint64_t n_parts, const uint8_t* part_role, const uint64_t* sample_off, uint64_t n, uint64_t n_roles,
                              const uint32_t* role_ids, const uint32_t* role_off, const uint8_t* role_train, uint32_t max_len, uint32_t width_multiple, uint32_t bos,
                              uint32_t eos, uint32_t pad, int32_t ignore, uint32_t flags, uint32_t order, uint64_t* pstart, uint64_t* full, uint32_t* len, uint32_t* n_trained,
                              uint64_t* c, uint64_t* f, uint32_t* sample_row, uint32_t* sample_col, uint32_t* row_sample, uint32_t* row_seg, uint64_t* counts) {
    TkSmp p;
    const int refused = tk_srow_shape(T, n_parts, n, n_roles, role_off, max_len, width_multiple, bos, eos, pad, ignore, flags, &p);
    if (refused) return refused;
    bool oob = false;
    const uint32_t n_ids = n_roles ? role_off[2 * n_roles] : 0;
    const SimArray<uint32_t> roff{role_off, n_roles ? 2 * n_roles + 1 : 0, &oob};
    const SimRoles t{roff, SimArray<uint32_t>{role_ids, n_ids, &oob}, SimArray<uint8_t>{role_train, n_roles, &oob}};
    const SimOffsets toff{tok_off, n_parts, &oob}, soff{sample_off, n, &oob};
    const SimArray<uint8_t> roles{part_role, n_parts, &oob};
    unsigned long long words[TK_SROW_WORDS] = {~0ull, ~0ull, ~0ull, 0, 0, 0, 0};
    const uint64_t m = n_parts > n ? n_parts : n;
    for (uint64_t i = 0; i <= m; ++i) tk_smp_count_entry(p, toff, soff, roles, roff, i, pstart, words);
    const uint64_t carry = sim_scan(pstart, n_parts);
    pstart[n_parts] = carry;
    words[TK_SMP_TOTAL] = carry;
    if (!tk_smp_reported(words)) {  // (as every kernel behind the count pass asks)
        const SimArray<uint64_t> ps{pstart, n_parts + 1, &oob};
        const SimIn in{toff, soff, roles, ps};
        for (uint64_t s = 0; s < n; ++s) tk_smp_sample_entry(p, soff, ps, roles, t, s, full, len, n_trained);
        for (uint64_t s = 0; s < n; ++s) tk_srow_plen_entry(p, in, t, s, full, len, n_trained, c, f);
        c[n] = sim_scan(c, n);
        f[n] = sim_scan(f, n);
        const SimArray<uint64_t> rc{c, n + 1, &oob}, rf{f, n + 1, &oob};
        std::vector<uint32_t> succ(n + 1), mark(n + 1), jump[2] = {std::vector<uint32_t>(n + 1), std::vector<uint32_t>(n + 1)};
        for (uint64_t s = 0; s <= n; ++s) tk_srow_succ_entry(rc, rf, n, max_len, s, succ.data(), mark.data());
        const uint32_t rounds = tk_srow_rounds(n);
        for (uint32_t k = 0; k < rounds; ++k) {
            const SimArray<uint32_t> jin{k ? jump[(k - 1) & 1].data() : succ.data(), n + 1, &oob};
            for (uint64_t i = 0; i <= n; ++i) tk_srow_double_entry(jin, n, order ? n - i : i, jump[k & 1].data(), mark.data());
        }
        const uint64_t R = sim_scan(mark.data(), n);
        mark[n] = (uint32_t)R;
        words[TK_SROW_R] = R;
        const SimArray<uint32_t> ex{mark.data(), n + 1, &oob}, rs{succ.data(), n + 1, &oob};
        for (uint64_t s = 0; s < n; ++s) tk_srow_place_entry(ex, rc, rs, max_len, s, sample_row, sample_col, row_sample, row_seg);
        row_sample[R] = (uint32_t)n;
        const uint64_t pads = sim_scan(row_seg, R);
        const SimArray<uint32_t> rsmp{row_sample, R + 1, &oob};
        for (uint64_t r = 0; r < R; ++r) row_seg[r] = tk_srow_row_seg(rf, rsmp, r, row_seg[r]);
        row_seg[R] = (uint32_t)(f[n] + pads);
        words[TK_SROW_NSEGS] = f[n] + pads;
    }
    if (oob) return -1;
    if (words[TK_BAD_OFF] != ~0ull) return 16 + (int64_t)words[TK_BAD_OFF];
    if (words[TK_SMP_BAD_SOFF] != ~0ull) return (1ll << 40) + (int64_t)words[TK_SMP_BAD_SOFF];
    if (words[TK_SMP_BAD_ROLE] != ~0ull) return (1ll << 41) + (int64_t)words[TK_SMP_BAD_ROLE];
    const int too_big = tk_srow_size(&p, words[TK_SMP_TOTAL], words[TK_SROW_R]);
    counts[0] = p.R;
    counts[1] = words[TK_SROW_NSEGS];
    return too_big;
}

// tk_k_srow_write after sample_rows_sim_place has accepted the call: through tk_srow_lane -- the function the kernel itself calls -- with
// the kernel's stores.  ids / labels / seg / pos: room for R * L; cu: n_segs + 1.  -1: an index out of bounds; -2: a cu_seqlens entry was
// written twice or not at all.
int64_t sample_rows_sim_write(const uint32_t* tokens, uint64_t T, const uint64_t* tok_off, uint64_t n_parts, const uint8_t* part_role, const uint64_t* sample_off, uint64_t n,
                              uint64_t n_roles, const uint32_t* role_ids, const uint32_t* role_off, const uint8_t* role_train, uint32_t max_len, uint32_t bos, uint32_t eos,
                              uint32_t pad, int32_t ignore, uint32_t flags, uint32_t block, const uint64_t* pstart, const uint64_t* c, const uint64_t* f,
                              const uint32_t* row_sample, const uint32_t* row_seg, uint64_t R, uint64_t n_segs, uint32_t* ids_out, int32_t* labels_out, uint32_t* seg_out,
                              uint32_t* pos_out, uint32_t* cu) {
    TkSmp p;
    if (tk_srow_shape(T, n_parts, n, n_roles, role_off, max_len, 0, bos, eos, pad, ignore, flags, &p)) return -3;
    p.R = R;
    bool oob = false, twice = false;
    const uint32_t n_ids = n_roles ? role_off[2 * n_roles] : 0;
    const SimRoles t{SimArray<uint32_t>{role_off, n_roles ? 2 * n_roles + 1 : 0, &oob}, SimArray<uint32_t>{role_ids, n_ids, &oob}, SimArray<uint8_t>{role_train, n_roles, &oob}};
    const SimIn in{SimOffsets{tok_off, n_parts, &oob}, SimOffsets{sample_off, n, &oob}, SimArray<uint8_t>{part_role, n_parts, &oob},
                   SimArray<uint64_t>{pstart, n_parts + 1, &oob}};
    const SimRows rw{SimArray<uint64_t>{c, n + 1, &oob}, SimArray<uint64_t>{f, n + 1, &oob}, SimArray<uint32_t>{row_sample, R + 1, &oob},
                     SimArray<uint32_t>{row_seg, R + 1, &oob}};
    const SimTokens tok{tokens, T, &oob};
    std::vector<uint8_t> seen(n_segs + 1, 0);
    const SimCu put{cu, n_segs, seen.data(), &oob, &twice};
    const uint32_t N = (uint32_t)(p.R * p.W), nb = (uint32_t)(((uint64_t)N + block - 1) / block);
    cu[n_segs] = N;
    for (uint32_t blk = 0; blk < nb; ++blk) {
        const uint32_t b0 = blk * block;
        for (uint32_t th = 0; th < block / 8; ++th) {
            if (N - b0 <= th * 8u) continue;
            const uint32_t i0 = b0 + th * 8u;
            uint32_t id[8], sg[8], ps[8];
            int32_t lab[8];
            tk_srow_lane(p, tok, in, rw, t, i0, N, id, lab, sg, ps, put);
            for (uint32_t j = 0; j < 8; ++j)
                if (N - i0 > j) {
                    ids_out[i0 + j] = id[j];
                    labels_out[i0 + j] = lab[j];
                    seg_out[i0 + j] = sg[j];
                    pos_out[i0 + j] = ps[j];
                }
        }
    }
    for (uint64_t i = 0; i < n_segs; ++i)
        if (!seen[i]) twice = true;
    return oob ? -1 : twice ? -2 : 0;
}
}

#ifdef SAMPLE_ROWS_SIM_MAIN
// Case file: per case sixteen uint64 {T, n_parts, n_samples, n_roles, n_ids, max_len, width_multiple, bos, eos, pad, ignore (two's
// complement), flags, block, order, 0, 0}, then tok_off[n_parts + 1], sample_off[n_samples + 1], role_off[2 n_roles + 1] (uint32),
// role_ids[n_ids], tokens[T], part_role[n_parts] (bytes), role_train[n_roles].  Result file: per case {rc, R, n_segs} (int64 / uint64) and,
// for rc == 0, ids, labels, seg, pos [R L] (4 bytes each), cu[n_segs + 1], row_seg[R + 1], row_sample[R + 1], len[n], full[n] uint64,
// n_trained[n], sample_row[n], sample_col[n].
template <class T>
static bool get(FILE* f, std::vector<T>& v, uint64_t n) {
    v.assign(n + 1, 0);  // (one more: data() of no elements is still a pointer)
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
        std::vector<uint64_t> tok_off, sample_off;
        std::vector<uint32_t> role_off, role_ids, tokens;
        std::vector<uint8_t> part_role, role_train;
        if (!get(in, tok_off, h[1] + 1) || !get(in, sample_off, h[2] + 1) || !get(in, role_off, 2 * h[3] + 1) || !get(in, role_ids, h[4]) || !get(in, tokens, h[0]) ||
            !get(in, part_role, h[1]) || !get(in, role_train, h[3]))
            return 3;
        tok_off.resize(h[1] + 1);  // (exactly the entries there are: the sanitizer sees an access behind them)
        sample_off.resize(h[2] + 1);
        part_role.resize(h[1]);
        tokens.resize(h[0] ? h[0] : 1);
        const uint64_t n = h[2];
        std::vector<uint64_t> pstart(h[1] + 1), full(n), c(n + 1), f(n + 1);
        std::vector<uint32_t> len(n), ntr(n), srow(n), scol(n), rsmp(n + 1), rseg(n + 1);
        uint64_t counts[2] = {0, 0};
        const uint32_t L = (uint32_t)h[5];
        int64_t rc = sample_rows_sim_place(h[0], tok_off.data(), h[1], part_role.data(), sample_off.data(), n, h[3], role_ids.data(), role_off.data(), role_train.data(), L,
                                           (uint32_t)h[6], (uint32_t)h[7], (uint32_t)h[8], (uint32_t)h[9], (int32_t)(uint32_t)h[10], (uint32_t)h[11], (uint32_t)h[13],
                                           pstart.data(), full.data(), len.data(), ntr.data(), c.data(), f.data(), srow.data(), scol.data(), rsmp.data(), rseg.data(), counts);
        const uint64_t R = rc ? 0 : counts[0], S = rc ? 0 : counts[1], N = R * L;
        std::vector<uint32_t> ids(N), seg(N), pos(N), cu(S + 1);
        std::vector<int32_t> labels(N);
        if (!rc)
            rc = sample_rows_sim_write(tokens.data(), h[0], tok_off.data(), h[1], part_role.data(), sample_off.data(), n, h[3], role_ids.data(), role_off.data(),
                                       role_train.data(), L, (uint32_t)h[7], (uint32_t)h[8], (uint32_t)h[9], (int32_t)(uint32_t)h[10], (uint32_t)h[11], (uint32_t)h[12],
                                       pstart.data(), c.data(), f.data(), rsmp.data(), rseg.data(), R, S, ids.data(), labels.data(), seg.data(), pos.data(), cu.data());
        const uint64_t res[3] = {(uint64_t)rc, R, S};
        fwrite(res, 8, 3, out);
        if (!rc) {
            put(out, ids, N);
            put(out, labels, N);
            put(out, seg, N);
            put(out, pos, N);
            put(out, cu, S + 1);
            put(out, rseg, R + 1);
            put(out, rsmp, R + 1);
            put(out, len, n);
            put(out, full, n);
            put(out, ntr, n);
            put(out, srow, n);
            put(out, scol, n);
        }
        ++n_cases;
    }
    fclose(in);
    fclose(out);
    printf("%d cases\n", n_cases);
    return 0;
}
#endif
