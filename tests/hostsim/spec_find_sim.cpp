// The scan for a disallowed special token (tk_k_spec_find, tk_kernels.h) on the CPU: the kernel's per-thread body -- tk_spec_hits16 and
// tk_spec_find16 of tk_special.h, with tk_special_at below them -- compiled for the host and driven lane by lane over a packed batch,
// with the kernel's own bookkeeping around it (a current minimum that is read first, lanes in any order).  The buffers are laid out
// as the library lays them out: the text readable 64 bytes past its end, the document-start bitmap two words past the last position's.
// Test infrastructure only (tests/test_spec_find_sim.py builds it).
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../tiktoken_amd/csrc/tk_special.h"
#include "../../tiktoken_amd/csrc/tk_tables.h"

namespace {
struct Sim {
    TkHostTables H;
    TkTables T;
    std::vector<uint32_t> head;
};
}  // namespace

extern "C" {
void* sfs_create(const uint8_t* ranks_blob, const uint64_t* ranks_off, const uint32_t* ranks_ids, uint64_t n_ranks, const uint8_t* spec_blob,
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
    return s;
}
void sfs_destroy(void* p) { delete (Sim*)p; }
// 0xFF: the 256-bit set decides the first byte, else the number of distinct first bytes (the four-byte form)
uint32_t sfs_first_bytes(void* p) { return ((Sim*)p)->T.n_spec_fb; }

// One chunk: text[0, n) with documents doc_off[0 .. n_docs] (absolute offsets, `base` is subtracted, as tk_k_mark_docs does), the
// special tokens with an id among dis_ids disallowed.  Lanes run in the order lane_order gives (null: ascending).  Returns what the
// kernel leaves in its word: base + the leftmost match, or all ones; id_len_out[0..1]: id and length of the longest disallowed
// token at that position.
uint64_t sfs_find(void* p, const uint8_t* text_in, uint64_t n, const uint64_t* doc_off, uint64_t n_docs, uint64_t base, const uint32_t* dis_ids,
                  uint64_t n_dis, const uint64_t* lane_order, uint32_t* id_len_out) {
    const Sim* s = (const Sim*)p;
    const TkTables& T = s->T;
    std::vector<uint64_t> store((n + 64 + 16 + 7) / 8 + 2, 0);  // (aligned like the device's buffers: tk_load8 reads whole 8-byte words)
    uint8_t* text = (uint8_t*)store.data();
    if (n) memcpy(text, text_in, n);
    const uint64_t nwords = (n + 31) / 32;
    std::vector<uint32_t> docb(nwords + 4, 0u);
    for (uint64_t d = 0; d < n_docs; ++d) {
        const uint64_t pos = doc_off[d] - base;
        if (pos < n) docb[pos >> 5] |= 1u << (pos & 31);
    }
    std::vector<uint8_t> dis(s->H.spec_id.size() + 16, 0);
    for (size_t k = 0; k < s->H.spec_id.size(); ++k)
        for (uint64_t j = 0; j < n_dis; ++j)
            if (s->H.spec_id[k] == dis_ids[j]) dis[k] = 1;
    uint64_t first = ~0ull;
    const uint64_t lanes = (n + 15) / 16;
    for (uint64_t i = 0; i < lanes; ++i) {
        const uint64_t p0 = (lane_order ? lane_order[i] : i) * 16;
        uint32_t w[4];
        memcpy(w, text + p0, 16);
        const uint32_t nxt = text[p0 + 16];
        const uint32_t hits = tk_spec_hits16(T, w, nxt);
        if (!hits) continue;
        const uint64_t cur = first;
        if (cur <= base + p0) continue;
        const uint64_t pos = tk_spec_find16(T, text, p0, n, hits, dis.data(), docb.data(), cur - base);
        if (pos != ~0ull && base + pos < first) first = base + pos;
    }
    if (first != ~0ull && id_len_out) {
        uint32_t idx = 0;
        id_len_out[1] = tk_special_at(T, text, first - base, n, dis.data(), docb.data(), &idx);
        id_len_out[0] = s->H.spec_id[idx];
    }
    return first;
}
}
