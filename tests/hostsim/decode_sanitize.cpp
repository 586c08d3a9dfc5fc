// The decode passes under AddressSanitizer / UBSan, as a program of its own (tests/test_decode_sim.py builds and runs it; nothing of it is
// loaded into Python): the driver of decode_sim.cpp with the kernel's own writer (TkDecStores: raw stores), every buffer a heap
// allocation of exactly the size the host gives it -- each blob its bytes plus the 16 bytes the table builder leaves behind them, the
// output total + 16 bytes (tk_api.hip) -- so that a source word read or a byte stored beyond them ends the run here.
// Reads a case file: u64 {n_ids, tok_blob bytes, spec_blob bytes, n_cases}, dec (n_ids x 2 u32), the blobs (with their padding), then per
// case u64 {n, block, seed, total}, the ids (u32), the expected bytes.  Prints "ok <cases> <bytes>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "decode_sim.cpp"

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
    uint64_t* h = exact<uint64_t>(f, 4);
    const uint64_t n_ids = h[0], n_cases = h[3];
    uint32_t* dec = exact<uint32_t>(f, n_ids * 2);
    uint8_t* tok_bytes = exact<uint8_t>(f, h[1]);
    uint8_t* spec_bytes = exact<uint8_t>(f, h[2]);
    uint64_t bytes = 0;
    for (uint64_t c = 0; c < n_cases; ++c) {
        uint64_t* ch = exact<uint64_t>(f, 4);
        const uint64_t n = ch[0], total = ch[3];
        uint32_t* ids = exact<uint32_t>(f, n);
        uint8_t* want = exact<uint8_t>(f, total);
        uint8_t* out = (uint8_t*)malloc(total + 16);
        unsigned long long* tbo = (unsigned long long*)malloc(n ? n * 8 : 1);
        uint64_t result[3] = {0, 0, 0};
        const int64_t rc = decode_passes(
            ids, n, dec, (uint32_t)n_ids, n_ids, tok_bytes, spec_bytes, (uint32_t)ch[1], ch[2], 0, 0, 0, tbo, result, [&](uint64_t) { return TkDecStores{out}; },
            [&](const TkDecStores&, uint64_t got) -> int64_t { return got == total && (!total || memcmp(out, want, total) == 0) ? 0 : 100; });
        if (rc) {
            fprintf(stderr, "case %llu: %lld\n", (unsigned long long)c, (long long)rc);
            return 1;
        }
        bytes += total;
        free(ch), free(ids), free(want), free(out), free(tbo);
    }
    free(h), free(dec), free(tok_bytes), free(spec_bytes);
    fclose(f);
    printf("ok %llu %llu\n", (unsigned long long)n_cases, (unsigned long long)bytes);
    return 0;
}
