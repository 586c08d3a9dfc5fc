// The UTF-8 repair passes under AddressSanitizer / UBSan, as a program of its own (tests/test_utf8_repair_sim.py builds and runs it; nothing
// of it is loaded into Python): the driver of utf8_repair_sim.cpp, every buffer a heap allocation of exactly its contract size -- the
// input n + 16 bytes, the offsets n_docs + 1 words, the bitmap one word past bit n + 16 and the output n_text + 16 bytes (both made by the
// driver) -- so that a read or a store beyond them ends the run here.
// Reads a case file: u64 n_cases, then per case u64 {n, n_docs, mode, wg_lanes, order, n_text, replaced}, the bytes (n + 16), the offsets,
// the expected text and its three offset arrays.  Prints "ok <cases> <bytes>".
#include <stdio.h>

#include "utf8_repair_sim.cpp"

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
    uint64_t* h = exact<uint64_t>(f, 1);
    const uint64_t n_cases = h[0];
    uint64_t total = 0;
    for (uint64_t c = 0; c < n_cases; ++c) {
        uint64_t* ch = exact<uint64_t>(f, 7);
        const uint64_t n = ch[0], n_docs = ch[1], n_text = ch[5];
        uint8_t* bytes = exact<uint8_t>(f, n + 16);
        uint64_t* off = exact<uint64_t>(f, n_docs + 1);
        uint8_t* want = exact<uint8_t>(f, n_text);
        uint64_t* want_off = exact<uint64_t>(f, 3 * (n_docs + 1));
        uint8_t* text = (uint8_t*)malloc(3 * n + 16);
        uint64_t* got_off = (uint64_t*)malloc(3 * (n_docs + 1) * 8);
        uint64_t totals[5];
        const int64_t rc = u8r_run(bytes, n, off, n_docs, (uint32_t)ch[2], (uint32_t)ch[3], (uint32_t)ch[4], text, got_off, got_off + n_docs + 1, got_off + 2 * (n_docs + 1), totals);
        if (rc || totals[0] != n_text || totals[2] != ch[6] || (n_text && memcmp(text, want, n_text)) || memcmp(got_off, want_off, 3 * (n_docs + 1) * 8)) {
            fprintf(stderr, "case %llu: %lld\n", (unsigned long long)c, (long long)rc);
            return 1;
        }
        total += n;
        free(ch), free(bytes), free(off), free(want), free(want_off), free(text), free(got_off);
    }
    free(h);
    fclose(f);
    printf("ok %llu %llu\n", (unsigned long long)n_cases, (unsigned long long)total);
    return 0;
}
