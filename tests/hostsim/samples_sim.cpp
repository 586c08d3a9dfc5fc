// The samples passes (tiktoken_amd/csrc/tk_samples.h) on the CPU: the plain C++ they are made of -- tk_samples_rule.h: what a call may say,
// the elements of a part, the part of a stream position, where an element comes from and whether it is trained, a sample's figures, a
// whole lane of the write pass -- compiled for the host and driven the way the kernels drive it: lanes of eight positions, workgroups of
// `block` positions, every array behind a reader that checks the index.  Test infrastructure only (tests/test_samples_sim.py builds it:
// as a shared library, and with -DSAMPLES_SIM_MAIN as a program of its own under the address and undefined-behaviour sanitizers, which
// reads a case file and writes the results).
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../tiktoken_amd/csrc/tk_samples_rule.h"
#include "sim_readers.h"

namespace {
using SimRoles = TkSmpRoles<SimArray<uint32_t>, SimArray<uint32_t>, SimArray<uint8_t>>;
using SimIn = TkSmpIn<SimOffsets, SimOffsets, SimArray<uint8_t>, SimArray<uint64_t>>;
}  // namespace

extern "C" {
// The count pass, the scan, the per-sample pass and the host between them: counts = {R, W}.  Returns 0; 1 .. 10: tk_smp_shape's /
// tk_smp_size's refusal; 16 + tk_rows_bad_key: tok_off is refused; 2^40 + tk_rows_bad_key: sample_off is; 2^41 + p: part p has no role;
// -1: an index out of bounds.  pstart: room for n_parts + 1; full / len / n_trained: n_samples.
int64_t samples_sim_count(uint64_t T, const uint64_t* tok_off, uint64_t n_parts, const uint8_t* part_role, const uint64_t* sample_off, uint64_t n_samples, uint64_t n_roles,
                          const uint32_t* role_ids, const uint32_t* role_off, const uint8_t* role_train, uint32_t max_len, uint32_t width_multiple, uint32_t bos, uint32_t eos,
                          uint32_t pad, int32_t ignore, uint32_t flags, uint64_t* pstart, uint64_t* full, uint32_t* len, uint32_t* n_trained, uint64_t* counts) {
    TkSmp p;
    const int refused = tk_smp_shape(T, n_parts, n_samples, n_roles, role_off, max_len, width_multiple, bos, eos, pad, ignore, flags, &p);
    if (refused) return refused;
    bool oob = false;
    const uint32_t n_ids = n_roles ? role_off[2 * n_roles] : 0;
    const SimArray<uint32_t> roff{role_off, n_roles ? 2 * n_roles + 1 : 0, &oob};
    const SimRoles t{roff, SimArray<uint32_t>{role_ids, n_ids, &oob}, SimArray<uint8_t>{role_train, n_roles, &oob}};
    const SimOffsets toff{tok_off, n_parts, &oob}, soff{sample_off, n_samples, &oob};
    const SimArray<uint8_t> roles{part_role, n_parts, &oob};
    // tk_k_smp_count
    unsigned long long words[TK_SMP_WORDS] = {~0ull, ~0ull, ~0ull, 0, 0};
    const uint64_t n = n_parts > n_samples ? n_parts : n_samples;
    for (uint64_t i = 0; i <= n; ++i) tk_smp_count_entry(p, toff, soff, roles, roff, i, pstart, words);
    // tk_k_smp_scan
    const uint64_t carry = sim_scan(pstart, n_parts);
    pstart[n_parts] = carry;
    words[TK_SMP_TOTAL] = carry;
    // tk_k_smp_samples
    if (!tk_smp_reported(words)) {
        const SimArray<uint64_t> ps{pstart, n_parts + 1, &oob};
        for (uint64_t s = 0; s < n_samples; ++s) {
            const uint32_t l = tk_smp_sample_entry(p, soff, ps, roles, t, s, full, len, n_trained);
            if (l > words[TK_SMP_LONGEST]) words[TK_SMP_LONGEST] = l;
        }
    }
    if (oob) return -1;
    // the host
    if (words[TK_BAD_OFF] != ~0ull) return 16 + (int64_t)words[TK_BAD_OFF];
    if (words[TK_SMP_BAD_SOFF] != ~0ull) return (1ll << 40) + (int64_t)words[TK_SMP_BAD_SOFF];
    if (words[TK_SMP_BAD_ROLE] != ~0ull) return (1ll << 41) + (int64_t)words[TK_SMP_BAD_ROLE];
    const int too_big = tk_smp_size(&p, words[TK_SMP_TOTAL], (uint32_t)words[TK_SMP_LONGEST]);
    counts[0] = p.R;
    counts[1] = p.W;
    return too_big;
}

// tk_k_smp_write after samples_sim_count has accepted the call and left pstart: through tk_smp_lane -- the function the kernel itself
// calls -- with the kernel's stores.  ids / labels / mask: room for R * W.  -1 if an index lies out of bounds.
int64_t samples_sim(const uint32_t* tokens, uint64_t T, const uint64_t* tok_off, uint64_t n_parts, const uint8_t* part_role, const uint64_t* sample_off, uint64_t n_samples,
                    uint64_t n_roles, const uint32_t* role_ids, const uint32_t* role_off, const uint8_t* role_train, uint32_t max_len, uint32_t width_multiple, uint32_t bos,
                    uint32_t eos, uint32_t pad, int32_t ignore, uint32_t flags, uint32_t block, const uint64_t* pstart, uint32_t W, uint32_t* ids_out, int32_t* labels_out,
                    uint8_t* mask_out) {
    TkSmp p;
    if (tk_smp_shape(T, n_parts, n_samples, n_roles, role_off, max_len, width_multiple, bos, eos, pad, ignore, flags, &p)) return -3;
    p.W = W;  // (what samples_sim_count settled)
    bool oob = false;
    const uint32_t n_ids = n_roles ? role_off[2 * n_roles] : 0;
    const SimRoles t{SimArray<uint32_t>{role_off, n_roles ? 2 * n_roles + 1 : 0, &oob}, SimArray<uint32_t>{role_ids, n_ids, &oob}, SimArray<uint8_t>{role_train, n_roles, &oob}};
    const SimIn in{SimOffsets{tok_off, n_parts, &oob}, SimOffsets{sample_off, n_samples, &oob}, SimArray<uint8_t>{part_role, n_parts, &oob},
                   SimArray<uint64_t>{pstart, n_parts + 1, &oob}};
    const SimTokens tok{tokens, T, &oob};
    const uint32_t N = (uint32_t)(p.R * p.W), nb = (uint32_t)(((uint64_t)N + block - 1) / block);
    for (uint32_t blk = 0; blk < nb; ++blk) {
        const uint32_t b0 = blk * block;
        for (uint32_t th = 0; th < block / 8; ++th) {
            if (N - b0 <= th * 8u) continue;
            const uint32_t i0 = b0 + th * 8u;
            uint32_t id[8];
            int32_t lab[8];
            uint64_t mask;
            tk_smp_lane(p, tok, in, t, i0, N, id, lab, &mask);
            for (uint32_t j = 0; j < 8; ++j)
                if (N - i0 > j) {
                    ids_out[i0 + j] = id[j];
                    labels_out[i0 + j] = lab[j];
                    mask_out[i0 + j] = (uint8_t)(mask >> (8 * j));
                }
        }
    }
    return oob ? -1 : 0;
}
}

#ifdef SAMPLES_SIM_MAIN
// Case file: per case sixteen uint64 {T, n_parts, n_samples, n_roles, n_ids, max_len, width_multiple, bos, eos, pad, ignore (two's
// complement), flags, block, 0, 0, 0}, then tok_off[n_parts + 1], sample_off[n_samples + 1], role_off[2 n_roles + 1] (uint32),
// role_ids[n_ids], tokens[T], part_role[n_parts] (bytes), role_train[n_roles].  Result file: per case {rc, R, W} (int64 / uint64) and, for
// rc == 0, ids[R W] uint32, labels[R W] int32, mask[R W] bytes, len[R] uint32, full[R] uint64, n_trained[R] uint32.
template <class T>
static bool get(FILE* f, std::vector<T>& v, uint64_t n) {
    v.assign(n + 1, 0);  // (one more: data() of no elements is still a pointer)
    return !n || fread(v.data(), sizeof(T), n, f) == n;
}
template <class T>
static void put(FILE* f, const std::vector<T>& v) {
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
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
        std::vector<uint64_t> pstart(h[1] + 1), full(h[2]);
        std::vector<uint32_t> len(h[2]), ntr(h[2]);
        uint64_t counts[2] = {0, 0};
        const uint32_t spec[5] = {(uint32_t)h[5], (uint32_t)h[6], (uint32_t)h[7], (uint32_t)h[8], (uint32_t)h[9]};
        int64_t rc = samples_sim_count(h[0], tok_off.data(), h[1], part_role.data(), sample_off.data(), h[2], h[3], role_ids.data(), role_off.data(), role_train.data(), spec[0],
                                       spec[1], spec[2], spec[3], spec[4], (int32_t)(uint32_t)h[10], (uint32_t)h[11], pstart.data(), full.data(), len.data(), ntr.data(), counts);
        const uint64_t N = rc ? 0 : counts[0] * counts[1];
        std::vector<uint32_t> ids(N);
        std::vector<int32_t> labels(N);
        std::vector<uint8_t> mask(N);
        if (!rc)
            rc = samples_sim(tokens.data(), h[0], tok_off.data(), h[1], part_role.data(), sample_off.data(), h[2], h[3], role_ids.data(), role_off.data(), role_train.data(),
                             spec[0], spec[1], spec[2], spec[3], spec[4], (int32_t)(uint32_t)h[10], (uint32_t)h[11], (uint32_t)h[12], pstart.data(), (uint32_t)counts[1],
                             ids.data(), labels.data(), mask.data());
        const uint64_t res[3] = {(uint64_t)rc, counts[0], counts[1]};
        fwrite(res, 8, 3, out);
        if (!rc) {
            put(out, ids);
            put(out, labels);
            put(out, mask);
            put(out, len);
            put(out, full);
            put(out, ntr);
        }
        ++n_cases;
    }
    fclose(in);
    fclose(out);
    printf("%d cases\n", n_cases);
    return 0;
}
#endif
