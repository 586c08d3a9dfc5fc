// The JSON Lines driver (jsonl_sim.cpp) as a program of its own, for -fsanitize=address,undefined: seeded random buffers made of JSON
// fragments -- quotes, backslash runs, brackets, \u escapes whole and cut, surrogates, raw multi-byte chars whole and cut, newlines, a BOM --
// in heap blocks of exactly their size, every mode, at tiles of 64, 128 and TK_JSONL_TILE bytes: the runs must be clean, agree with each
// other array for array and keep the pass's invariants (offsets ascend, the text is no longer than the buffer).  Host code only.
#include <stdio.h>

#include <random>
#include <string>

#include "jsonl_sim.cpp"

namespace {
const char* const PARTS[] = {"{", "}", "[", "]", "\"", "\\", "\\\\", ":", ",", " ", "\t", "\r", "\n", "\n", "\"text\"", "\"text\":\"", "{\"text\":\"", "\"}\n", "text",
                             "\\u00e9", "\\ud83d", "\\ude00", "\\ud83d\\ude00", "\\u12", "\\n", "\\q", "\xc3\xa9", "\xe2\x82\xac", "\xf0\x9f\x98\x80", "\xe2\x82", "\x80", "\x01",
                             "null", "12", "abc", "{\"id\":1,\"text\":\"hello\"}\n", "{\"text\" : \"a\\tb\"}\r\n"};
struct Result {
    int64_t rc;
    std::vector<uint8_t> text, status;
    std::vector<uint64_t> doc_off, line, line_off;
    uint64_t counts[3], bad[3];
    bool operator==(const Result& o) const {
        if (rc != o.rc) return false;
        if (rc == 1) return bad[0] == o.bad[0] && bad[1] == o.bad[1] && bad[2] == o.bad[2];
        return text == o.text && status == o.status && doc_off == o.doc_off && line == o.line && line_off == o.line_off;
    }
};
Result run(const std::string& buf, uint32_t mode, uint32_t tile) {
    uint64_t cap = 1;
    for (char ch : buf) cap += ch == '\n';
    Result r;
    r.text.assign(buf.size() + 1, 0);
    r.status.assign(cap, 0), r.line.assign(cap, 0), r.doc_off.assign(cap + 1, 0), r.line_off.assign(cap + 1, 0);
    r.counts[0] = r.counts[1] = r.counts[2] = r.bad[0] = r.bad[1] = r.bad[2] = 0;
    const std::vector<uint8_t> src(buf.begin(), buf.end());
    const uint8_t field[4] = {'t', 'e', 'x', 't'};
    r.rc = jsonl_sim(src.data(), src.size(), field, 4, mode, tile, cap, r.text.data(), r.doc_off.data(), r.line.data(), r.line_off.data(), r.status.data(), r.counts, r.bad);
    if (r.rc == 0) {
        r.text.resize(r.counts[2]), r.status.resize(r.counts[1]), r.line.resize(r.counts[0]), r.doc_off.resize(r.counts[0] + 1), r.line_off.resize(r.counts[1] + 1);
    }
    return r;
}
}  // namespace

int main() {
    std::mt19937 rng(0x75A1);
    const size_t n_parts = sizeof PARTS / sizeof PARTS[0];
    for (int it = 0; it < 400; ++it) {
        std::string buf = it % 7 == 0 ? "\xef\xbb\xbf" : "";
        const int parts = (int)(rng() % (it % 20 == 0 ? 3000 : 120));
        for (int k = 0; k < parts; ++k) buf += PARTS[rng() % n_parts];
        for (uint32_t mode = 0; mode < 3; ++mode) {
            const Result a = run(buf, mode, 64);
            if (a.rc != 0 && a.rc != 1) return printf("rc %lld at %d\n", (long long)a.rc, it), 1;
            if (!(a == run(buf, mode, 128)) || !(a == run(buf, mode, TK_JSONL_TILE))) return printf("the tile size changes the result at %d mode %u\n", it, mode), 1;
            if (a.rc == 1) continue;
            if (a.counts[2] > buf.size() || a.doc_off.back() != a.counts[2] || a.line_off.back() != buf.size()) return printf("totals at %d\n", it), 1;
            for (size_t d = 0; d + 1 < a.doc_off.size(); ++d)
                if (a.doc_off[d] > a.doc_off[d + 1] || (d + 1 < a.line.size() && a.line[d] >= a.line[d + 1])) return printf("order at %d\n", it), 1;
        }
    }
    printf("jsonl_sanitize ok\n");
    return 0;
}
