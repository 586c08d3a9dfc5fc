// The stop-string passes under AddressSanitizer / UBSan, as a program of its own (tests/test_stop_text_sim.py builds and runs it; nothing
// of it is loaded into Python): the driver of stop_text_sim.cpp, every buffer a heap allocation of exactly its contract size -- the input
// n + 16 bytes (it ends exactly 16 bytes behind the text), the offsets n_docs + 1 words, the stop blob and its offsets, the staged tile
// and the output n_text + 16 bytes (both made by the driver) -- so that a read or a store beyond them ends the run here.
// Reads a case file: u64 n_cases, then per case u64 {n, n_docs, n_stops, stop_bytes, flags, wg_lanes, order, n_text, n_hit}, the bytes
// (n + 16), the offsets, the stop blob, its offsets (u32), the expected text, text_off and hit (u32).  Prints "ok <cases> <bytes>".
#include <stdio.h>

#include "stop_text_sim.cpp"

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
        uint64_t* ch = exact<uint64_t>(f, 9);
        const uint64_t n = ch[0], n_docs = ch[1], n_stops = ch[2], stop_bytes = ch[3], n_text = ch[7];
        uint8_t* bytes = exact<uint8_t>(f, n + 16);
        uint64_t* off = exact<uint64_t>(f, n_docs + 1);
        uint8_t* blob = exact<uint8_t>(f, stop_bytes);
        uint32_t* stop_off = exact<uint32_t>(f, n_stops + 1);
        uint8_t* want = exact<uint8_t>(f, n_text);
        uint64_t* want_off = exact<uint64_t>(f, n_docs + 1);
        uint32_t* want_hit = exact<uint32_t>(f, n_docs);
        uint8_t* text = (uint8_t*)malloc(n + 16);
        uint64_t* got_off = (uint64_t*)malloc((n_docs + 1) * 8);
        uint32_t* got_hit = (uint32_t*)malloc(n_docs ? n_docs * 4 : 1);
        uint64_t totals[3];
        const int64_t rc = stops_run(bytes, n, off, n_docs, blob, stop_off, (uint32_t)n_stops, (uint32_t)ch[4], (uint32_t)ch[5], (uint32_t)ch[6], text, got_off, got_hit, totals);
        if (rc || totals[0] != n_text || totals[1] != ch[8] || (n_text && memcmp(text, want, n_text)) || memcmp(got_off, want_off, (n_docs + 1) * 8) ||
            (n_docs && memcmp(got_hit, want_hit, n_docs * 4))) {
            fprintf(stderr, "case %llu: %lld\n", (unsigned long long)c, (long long)rc);
            return 1;
        }
        total += n;
        free(ch), free(bytes), free(off), free(blob), free(stop_off), free(want), free(want_off), free(want_hit), free(text), free(got_off), free(got_hit);
    }
    free(h);
    fclose(f);
    printf("ok %llu %llu\n", (unsigned long long)n_cases, (unsigned long long)total);
    return 0;
}
