// The masking rule (tk_pii_rule.h) on the CPU, one document at a time and candidate by candidate as the kernels decide: triggers from
// tk_pii_lane_masks over lanes of 16 bytes, an e-mail per '@', then an address per digit whose first byte no e-mail covers.  Every read
// is checked against the document.  Returns the bytes of the masked document (written to out while they fit cap), -1 after a read
// outside the document; counts: e-mails, addresses.
#include <stdint.h>

#include <vector>

#include "../../tiktoken_amd/csrc/tk_pii_rule.h"

extern "C" int64_t pii_sim_mask(const uint8_t* doc, uint64_t n, const uint8_t* email, uint64_t n_email, const uint8_t* ip, uint64_t n_ip, uint32_t public_only, uint8_t* out,
                                uint64_t cap, uint64_t* counts) {
    TkPii p;
    if (tk_pii_shape(n, 1, email, n_email, ip, n_ip, public_only, &p)) return -2;
    bool oob = false;
    auto rd = [&](int64_t i) -> uint32_t {
        if (i < 0 || (uint64_t)i >= n) {
            oob = true;
            return 0;
        }
        return doc[i];
    };
    std::vector<uint8_t> kind(n + 1, 0);  // 1, 2: an e-mail, an address starts here; 4: the byte lies in a match
    std::vector<uint32_t> at(n / 16 + 1), dig(n / 16 + 1), wdot(n / 16 + 1);
    for (uint64_t c = 0; c * 16 < n; ++c) {
        uint64_t lo = 0, hi = 0;
        for (uint64_t j = 0; j < 16 && c * 16 + j < n; ++j) (j < 8 ? lo : hi) |= (uint64_t)doc[c * 16 + j] << (8 * (j & 7));
        tk_pii_lane_masks(lo, hi, &at[c], &dig[c], &wdot[c]);
    }
    for (uint64_t i = 0; i < n; ++i) {
        int64_t s, e;
        if (((at[i / 16] >> (i % 16)) & 1u) != (doc[i] == '@')) return -3;
        if (((at[i / 16] >> (i % 16)) & 1u) && tk_pii_email(rd, 0, (int64_t)n, (int64_t)i, &s, &e)) {
            kind[s] |= 1, ++counts[0];
            for (int64_t k = s; k < e; ++k) kind[k] |= 4;
        }
    }
    for (uint64_t i = 0; i < n; ++i) {
        const bool before = i && ((wdot[(i - 1) / 16] >> ((i - 1) % 16)) & 1u);
        if (!((dig[i / 16] >> (i % 16)) & 1u) || before || (kind[i] & 4)) continue;
        uint32_t a = 0, b = 0;
        const uint32_t len = tk_pii_ip(rd, 0, (int64_t)n, (int64_t)i, &a, &b);
        if (!len || (p.public_only && tk_pii_ip_private(a, b))) continue;
        kind[i] |= 2, ++counts[1];
        for (uint32_t k = 0; k < len; ++k) kind[i + k] |= 4;
    }
    uint64_t o = 0;
    auto put = [&](uint8_t b) {
        if (o < cap) out[o] = b;
        ++o;
    };
    for (uint64_t i = 0; i < n; ++i) {
        if (kind[i] & 1)
            for (uint32_t k = 0; k < p.len_email; ++k) put((uint8_t)(p.ph[0][k >> 2] >> (8 * (k & 3))));
        if (kind[i] & 2)
            for (uint32_t k = 0; k < p.len_ip; ++k) put((uint8_t)(p.ph[1][k >> 2] >> (8 * (k & 3))));
        if (!(kind[i] & 4)) put(doc[i]);
    }
    return oob ? -1 : (int64_t)o;
}
