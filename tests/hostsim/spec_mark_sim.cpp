// The two passes that mark allowed special tokens (tk_k_spec_cand, tk_k_spec_resolve; tk_kernels.h) on the CPU: the per-thread body of the
// first -- tk_spec_hits16 and tk_special_at of tk_special.h -- for every lane of sixteen bytes, then tk_spec_resolve_one for every
// candidate, a word of the candidate bitmap at a time as the kernel's threads take them.  Lanes and words run in ascending order or in a
// seeded shuffled one.  The buffers have exactly the sizes the library gives them (stage_front, tk_api.hip): the candidate and
// document-start bitmaps nwords + 4 words, the two special-token bitmaps and the break bitmap nwords + 2, the text readable 64 bytes past
// its end and no further -- so that the address sanitizer sees every read or write that the device's buffers would not cover.
// Built as a shared library for tests/test_spec_mark_sim.py and, with -DSPEC_MARK_SIM_MAIN, as a program of its own that runs a file
// of cases (the same test, under the sanitizers).  Test infrastructure only.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <utility>
#include <vector>

#include "../../tiktoken_amd/csrc/tk_special.h"
#include "../../tiktoken_amd/csrc/tk_tables.h"

namespace {
struct Sim {
    TkHostTables H;
    TkTables T;
    std::vector<uint32_t> head;
    uint32_t max_len = 0;
};
struct OrBit {
    void operator()(uint32_t* bm, uint64_t word, uint32_t mask) const { bm[word] |= mask; }
};
// 0 .. count - 1, shuffled by `seed` (0: ascending)
std::vector<uint64_t> order_of(uint64_t count, uint64_t seed) {
    std::vector<uint64_t> o(count);
    for (uint64_t i = 0; i < count; ++i) o[i] = i;
    uint64_t x = seed * 0x9E3779B97F4A7C15ull + 1;
    for (uint64_t i = count; seed && i > 1; --i) {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        std::swap(o[i - 1], o[x % i]);
    }
    return o;
}
}  // namespace

extern "C" {
void* sms_create(const uint8_t* ranks_blob, const uint64_t* ranks_off, const uint32_t* ranks_ids, uint64_t n_ranks, const uint8_t* spec_blob,
                 const uint64_t* spec_off, const uint32_t* spec_ids, uint64_t n_spec, const char* pat_str, char* err, uint64_t errcap) {
    Sim* s = new Sim();
    const std::string e = tk_build_tables(ranks_blob, ranks_off, ranks_ids, n_ranks, spec_blob, spec_off, spec_ids, n_spec, pat_str, &s->H);
    if (!e.empty()) {
        strncpy(err, e.c_str(), errcap - 1);
        err[errcap - 1] = 0;
        delete s;
        return nullptr;
    }
    memset(&s->T, 0, sizeof s->T);
    s->T.spec_bytes = s->H.spec_bytes.data();
    s->T.spec_off = s->H.spec_off.data();
    s->T.spec_id = s->H.spec_id.data();
    tk_spec_tables(s->H, s->head, s->T);
    s->T.spec_head = s->head.data();
    for (size_t k = 0; k + 1 < s->H.spec_off.size(); ++k)  // (as tk_create: over every registered special token, allowed or not)
        if (s->H.spec_off[k + 1] - s->H.spec_off[k] > s->max_len) s->max_len = s->H.spec_off[k + 1] - s->H.spec_off[k];
    return s;
}
void sms_destroy(void* p) { delete (Sim*)p; }
// 0xFF: the 256-bit set decides the first byte, else the number of distinct first bytes (the four-byte form)
uint32_t sms_first_bytes(void* p) { return ((Sim*)p)->T.n_spec_fb; }
uint32_t sms_max_len(void* p) { return ((Sim*)p)->max_len; }

// One chunk: text[0, n) with documents doc_off[0 .. n_docs] (absolute offsets, `base` is subtracted, as tk_k_mark_docs does), the
// special tokens with an id among allowed_ids allowed.  order_seed: 0 = lanes and words ascending, else shuffled.  out: the three
// bitmaps spec_start, spec_in and brk one behind the other, nwords + 2 words each (the two words of slack included: they stay zero).
void sms_mark(void* p, const uint8_t* text_in, uint64_t n, const uint64_t* doc_off, uint64_t n_docs, uint64_t base, const uint32_t* allowed_ids,
              uint64_t n_allowed, uint64_t order_seed, uint32_t* out) {
    const Sim* s = (const Sim*)p;
    const TkTables& T = s->T;
    const uint64_t nwords = (n + 31) / 32;
    std::vector<uint64_t> store((n + 64) / 8, 0);  // (8-byte words as the device's buffer: tk_load8 reads whole ones; readable to n + 64 rounded down)
    uint8_t* text = (uint8_t*)store.data();
    if (n) memcpy(text, text_in, n);
    std::vector<uint32_t> docb(nwords + 4, 0u), cand(nwords + 4, 0u), ss(nwords + 2, 0u), si(nwords + 2, 0u), brk(nwords + 2, 0u);
    for (uint64_t d = 0; d < n_docs; ++d) {  // tk_k_mark_docs
        const uint64_t pos = doc_off[d] - base;
        if (pos < n) {
            brk[pos >> 5] |= 1u << (pos & 31);
            docb[pos >> 5] |= 1u << (pos & 31);
        }
    }
    std::vector<uint8_t> allowed(s->H.spec_id.size(), 0);
    for (size_t k = 0; k < s->H.spec_id.size(); ++k)
        for (uint64_t j = 0; j < n_allowed; ++j)
            if (s->H.spec_id[k] == allowed_ids[j]) allowed[k] = 1;
    const OrBit or_bit;
    for (const uint64_t lane : order_of((n + 15) / 16, order_seed)) {  // tk_k_spec_cand
        const uint64_t p0 = lane * 16;
        uint32_t w[4], nx4;
        memcpy(w, text + p0, 16);
        memcpy(&nx4, text + p0 + 16, 4);
        uint32_t hits = tk_spec_hits16(T, w, nx4 & 0xFFu);
        while (hits) {
            const uint64_t pos = p0 + tk_ctz32(hits);
            hits &= hits - 1;
            uint32_t idx;
            if (pos < n && tk_special_at(T, text, pos, n, allowed.data(), docb.data(), &idx)) or_bit(cand.data(), pos >> 5, 1u << (pos & 31));
        }
    }
    for (const uint64_t wi : order_of(nwords, order_seed ? order_seed + 1 : 0))  // tk_k_spec_resolve
        for (uint32_t cw = cand[wi]; cw; cw &= cw - 1)
            tk_spec_resolve_one(T, text, n, allowed.data(), docb.data(), cand.data(), s->max_len, wi * 32 + tk_ctz32(cw), ss.data(), si.data(), brk.data(), or_bit);
    memcpy(out, ss.data(), (nwords + 2) * 4);
    memcpy(out + nwords + 2, si.data(), (nwords + 2) * 4);
    memcpy(out + 2 * (nwords + 2), brk.data(), (nwords + 2) * 4);
}
}

#ifdef SPEC_MARK_SIM_MAIN
// spec_mark_sim <cases> <results>.  The file of cases: u64 length and bytes of the pat_str, then the cases.  A case: u64 n_spec, per special token {u32 id, u32 len, bytes}; u64 n_allowed, u32 ids; u64 n, n_docs,
// base, order_seed; u64 doc_off[n_docs + 1]; the text.  A result: u32 first bytes, u32 max_len, u64 nwords, then sms_mark's `out`.
namespace {
bool rd(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }
}  // namespace
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* outf = fopen(argv[2], "wb");
    if (!in || !outf) return 2;
    std::vector<uint8_t> ranks_blob(256);
    std::vector<uint64_t> ranks_off(257);
    std::vector<uint32_t> ranks_ids(256);
    for (uint32_t b = 0; b < 256; ++b) {  // (a vocabulary of the 256 single bytes: the passes never look at it)
        ranks_blob[b] = (uint8_t)b;
        ranks_off[b] = b;
        ranks_ids[b] = b;
    }
    ranks_off[256] = 256;
    uint64_t cases = 0, n_spec, pat_len;
    if (!rd(in, &pat_len, 8) || pat_len > 4096) return 3;
    std::string pat(pat_len, ' ');
    if (!rd(in, &pat[0], pat_len)) return 3;
    while (fread(&n_spec, 8, 1, in) == 1) {
        std::vector<uint8_t> sb;
        std::vector<uint64_t> so(1, 0);
        std::vector<uint32_t> sid;
        for (uint64_t k = 0; k < n_spec; ++k) {
            uint32_t il[2];
            if (!rd(in, il, 8)) return 3;
            sid.push_back(il[0]);
            sb.resize(sb.size() + il[1]);
            if (!rd(in, sb.data() + so.back(), il[1])) return 3;
            so.push_back(sb.size());
        }
        sb.push_back(0);
        uint64_t n_allowed, hd[4];
        if (!rd(in, &n_allowed, 8)) return 3;
        std::vector<uint32_t> allowed(n_allowed + 1);
        if (!rd(in, allowed.data(), 4 * n_allowed) || !rd(in, hd, 32)) return 3;
        const uint64_t n = hd[0], n_docs = hd[1], nwords = (n + 31) / 32;
        std::vector<uint64_t> doc_off(n_docs + 1);
        std::vector<uint8_t> text(n + 1);
        if (!rd(in, doc_off.data(), 8 * (n_docs + 1)) || !rd(in, text.data(), n)) return 3;
        char err[256];
        void* s = sms_create(ranks_blob.data(), ranks_off.data(), ranks_ids.data(), 256, sb.data(), so.data(), sid.data(), n_spec,
                             pat.c_str(), err, sizeof err);
        if (!s) {
            fprintf(stderr, "case %llu: %s\n", (unsigned long long)cases, err);
            return 4;
        }
        std::vector<uint32_t> res(3 * (nwords + 2));
        sms_mark(s, text.data(), n, doc_off.data(), n_docs, hd[2], allowed.data(), n_allowed, hd[3], res.data());
        const uint32_t fm[2] = {sms_first_bytes(s), sms_max_len(s)};
        fwrite(fm, 4, 2, outf);
        fwrite(&nwords, 8, 1, outf);
        fwrite(res.data(), 4, res.size(), outf);
        sms_destroy(s);
        ++cases;
    }
    fclose(in);
    if (fclose(outf)) return 5;
    printf("%llu cases\n", (unsigned long long)cases);
    return 0;
}
#endif
