// The long-piece merges under AddressSanitizer / UBSan, as a program of its own (tests/test_merge_sim.py builds and runs it; nothing of it
// is loaded into Python): the driver of merge_sim.cpp with unchecked buffers -- P0/R0/P1/R1, the one-at-a-time form's id/rk/nx/pv and its
// level tree are heap blocks of exactly the entries the host gives them, the text one of exactly n bytes -- so that an index beyond one
// ends the run here.
// Reads a case file: u64 {n_pairs, n_cases}, byte_rank (256 u32), pair2 (65536 u32), the pair keys (u64, ascending) and their ranks
// (u32), then per case u64 {n, wavefronts, wide, seed, force_long, n_tokens}, the text, the expected tokens (u32).  Prints "ok <cases>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define MERGE_SIM_RAW
#include "merge_sim.cpp"

template <class T>
static T* exact(FILE* f, uint64_t count) {  // a heap block of exactly count elements, read from the file
    T* p = (T*)malloc(count ? count * sizeof(T) : 1);
    if (count && fread(p, sizeof(T), count, f) != count) {
        fprintf(stderr, "case file is short\n");
        exit(2);
    }
    return p;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t* h = exact<uint64_t>(f, 2);
    const uint64_t n_pairs = h[0], n_cases = h[1];
    uint32_t* byte_rank = exact<uint32_t>(f, 256);
    uint32_t* pair2 = exact<uint32_t>(f, 65536);
    uint64_t* keys = exact<uint64_t>(f, n_pairs);
    uint32_t* vals = exact<uint32_t>(f, n_pairs);
    for (uint64_t c = 0; c < n_cases; ++c) {
        uint64_t* ch = exact<uint64_t>(f, 6);
        const uint32_t n = (uint32_t)ch[0];
        uint8_t* text = exact<uint8_t>(f, n);
        uint32_t* want = exact<uint32_t>(f, ch[5]);
        uint32_t* out = (uint32_t*)malloc(n * sizeof(uint32_t));
        uint64_t result[MS_RESULTS];
        const MergeCase C{text, n, SimTables{byte_rank, pair2}, SimPairs{keys, vals, n_pairs}, (uint32_t)ch[1], ch[2] != 0, ch[3]};
        const int64_t rc = merge_piece(C, ch[4] != 0, out, result);
        if (rc || result[0] != ch[5] || memcmp(out, want, ch[5] * sizeof(uint32_t)) != 0) {
            fprintf(stderr, "case %llu: %lld\n", (unsigned long long)c, (long long)rc);
            return 1;
        }
        free(ch), free(text), free(want), free(out);
    }
    free(h), free(byte_rank), free(pair2), free(keys), free(vals);
    fclose(f);
    printf("ok %llu\n", (unsigned long long)n_cases);
    return 0;
}
