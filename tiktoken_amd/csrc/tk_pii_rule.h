// The rule of the personal-data masking pass (tk_pii.h) in plain C++: which bytes of a document are an e-mail address or an IPv4
// address, decided from the bytes around a trigger byte alone.  The rule is stated in include/tiktoken_amd.h as a regular expression;
// here it is a function of an '@' (the e-mail that ends its local part there) and a function of a digit (the IPv4 address that
// starts there), over a byte reader and the document's bounds [lo, hi).  Neither reads outside the document, nor further than
// TK_PII_BACK bytes before an '@', TK_PII_AHEAD behind it, one byte before a digit or TK_PII_IP_AHEAD behind it: the kernels stage
// exactly that around a tile, the CPU simulation of the tests runs the same functions over a whole document.
// Positions are signed: a window's positions before the text are negative in the kernels.
#pragma once
#include <stdint.h>

#include "tk_rows_rule.h"  // TK_HD, tk_last_le

#define TK_PII_TILE 4096u     // bytes of text per workgroup
#define TK_PII_THREADS 256u   // its lanes
#define TK_PII_LANE 16u       // bytes per lane: one 16-byte load
#define TK_PII_WAVE 1024u     // bytes per wavefront
#define TK_PII_MAX_LOCAL 64   // bytes before the '@'
#define TK_PII_MAX_DOMAIN 253 // bytes of [A-Za-z0-9.-] behind it
#define TK_PII_BACK 66        // 64 local bytes, the byte that ends a run of 65, the byte before the run
#define TK_PII_AHEAD 255      // 253 domain bytes, the byte that makes a run of 254, the byte behind the run
#define TK_PII_IP_AHEAD 17    // 15 bytes of address, the byte behind them, a digit behind a dot
#define TK_PII_HALO 336u      // TK_PII_BACK + TK_PII_AHEAD + an address that starts 14 bytes before the tile, rounded up to lanes
#define TK_PII_MAX_PLACEHOLDER 32u
#define TK_PII_MAX_BYTES 0xFFFF0000ull
static_assert(TK_PII_HALO % TK_PII_LANE == 0 && TK_PII_HALO >= TK_PII_BACK + TK_PII_AHEAD + 14, "whole lanes; an e-mail over an address that reaches the tile is decided in the window");

struct TkPii {
    uint64_t n_bytes, n_docs;
    uint32_t n_tiles, len_email, len_ip, public_only;
    uint32_t ph[2][TK_PII_MAX_PLACEHOLDER / 4];  // the placeholders' bytes, little-endian: e-mail, address
};

TK_HD bool tk_pii_digit(uint32_t b) { return b - '0' < 10u; }
TK_HD bool tk_pii_alpha(uint32_t b) { return (b | 0x20u) - 'a' < 26u; }
TK_HD bool tk_pii_word(uint32_t b) { return tk_pii_digit(b) || tk_pii_alpha(b) || b == '_'; }                         // [A-Za-z0-9_]
TK_HD bool tk_pii_domain(uint32_t b) { return tk_pii_digit(b) || tk_pii_alpha(b) || b == '.' || b == '-'; }           // [A-Za-z0-9.-]
TK_HD bool tk_pii_local(uint32_t b) { return tk_pii_domain(b) || b == '_' || b == '%' || b == '+'; }                  // [A-Za-z0-9._%+-]

// The e-mail match whose '@' is at p, lo <= p < hi: [*s, *e), or false.
//  Start: the run of local bytes that ends at the '@' is maximal, 1 .. 64 long and not preceded by '@'.
//  End: D, the run of domain bytes behind the '@', is at most 253 long; its labels are what lies between dots; the match ends behind
//   label j, the largest j >= 2 among the non-empty labels before the first empty one that is letters only and at least two long --
//   and, where it ends D, is not followed by '_' (the only byte of [A-Za-z0-9_-] that can follow D).
template <class Rd>
TK_HD bool tk_pii_email(Rd&& rd, int64_t lo, int64_t hi, int64_t p, int64_t* s, int64_t* e) {
    int64_t a = p;
    while (a > lo && p - a <= TK_PII_MAX_LOCAL && tk_pii_local(rd(a - 1))) --a;
    if (a == p || p - a > TK_PII_MAX_LOCAL || (a > lo && rd(a - 1) == '@')) return false;
    int64_t dend = p + 1;
    while (dend < hi && dend - (p + 1) <= TK_PII_MAX_DOMAIN && tk_pii_domain(rd(dend))) ++dend;
    if (dend - (p + 1) > TK_PII_MAX_DOMAIN) return false;
    int64_t best = -1;
    uint32_t j = 0;
    for (int64_t from = p + 1; from < dend;) {
        int64_t to = from;
        bool letters = true;
        for (; to < dend && rd(to) != '.'; ++to) letters = letters && tk_pii_alpha(rd(to));
        if (to == from) break;  // an empty label
        ++j;
        if (j >= 2u && letters && to - from >= 2 && !(to == dend && dend < hi && rd(dend) == '_')) best = to;
        from = to + 1;
    }
    if (best < 0) return false;
    *s = a, *e = best;
    return true;
}

// The bytes of the IPv4 match that starts at q, lo <= q < hi, 0 for none; *a, *b: its first two numbers.
//  Before q: the document's start, or a byte outside [A-Za-z0-9_.].  Four numbers with a dot between: a number is a maximal run of 1 to
//  3 digits, at most 255, that starts with '0' only when it is "0".  Behind: no byte of [A-Za-z0-9_], and no dot with a digit behind it.
template <class Rd>
TK_HD uint32_t tk_pii_ip(Rd&& rd, int64_t lo, int64_t hi, int64_t q, uint32_t* a, uint32_t* b) {
    if (q > lo && (tk_pii_word(rd(q - 1)) || rd(q - 1) == '.')) return 0;
    int64_t i = q;
    for (uint32_t k = 0; k < 4u; ++k) {
        if (k) {
            if (i >= hi || rd(i) != '.') return 0;
            ++i;
        }
        const int64_t from = i;
        uint32_t v = 0;
        for (; i < hi && i - from < 4 && tk_pii_digit(rd(i)); ++i) v = v * 10u + (rd(i) - '0');
        if (i == from || i - from > 3 || v > 255u || (i - from > 1 && rd(from) == '0')) return 0;
        if (k == 0) *a = v;
        if (k == 1) *b = v;
    }
    if (i < hi && (tk_pii_word(rd(i)) || (rd(i) == '.' && i + 1 < hi && tk_pii_digit(rd(i + 1))))) return 0;
    return (uint32_t)(i - q);
}
// a.b.c.d is not a public address: this network, private use, loopback, shared address space, link local, multicast and reserved
TK_HD bool tk_pii_ip_private(uint32_t a, uint32_t b) {
    return a == 0u || a == 10u || a == 127u || a >= 224u || (a == 100u && b - 64u < 64u) || (a == 169u && b == 254u) || (a == 172u && b - 16u < 16u) || (a == 192u && b == 168u);
}

// 0x80 in every byte of v that equals c / whose low seven bits are at least c (c < 0x80), and bit j of the result for 0x80 in byte j
TK_HD uint64_t tk_pii_eq8(uint64_t v, uint32_t c) {
    const uint64_t x = v ^ (0x0101010101010101ull * c), m = 0x7F7F7F7F7F7F7F7Full;
    return ~(((x & m) + m) | x | m);
}
TK_HD uint64_t tk_pii_ge8(uint64_t v, uint32_t c) { return ((v & 0x7F7F7F7F7F7F7F7Full) + 0x0101010101010101ull * (0x80u - c)) & 0x8080808080808080ull; }
TK_HD uint32_t tk_pii_bits8(uint64_t m) { return (uint32_t)(((m >> 7) * 0x0102040810204080ull) >> 56); }
// Of the 16 bytes (lo, hi) of a lane: bit j of *at: byte j is '@'; of *dig: a digit; of *wdot: a byte of [A-Za-z0-9_.]
TK_HD void tk_pii_lane_masks(uint64_t lo, uint64_t hi, uint32_t* at, uint32_t* dig, uint32_t* wdot) {
    auto half = [](uint64_t v, uint32_t* a, uint32_t* d, uint32_t* w) {
        const uint64_t ascii = ~v & 0x8080808080808080ull, f = v | 0x2020202020202020ull;
        const uint64_t digit = tk_pii_ge8(v, '0') & ~tk_pii_ge8(v, '9' + 1) & ascii, alpha = tk_pii_ge8(f, 'a') & ~tk_pii_ge8(f, 'z' + 1) & ascii;
        *a = tk_pii_bits8(tk_pii_eq8(v, '@')), *d = tk_pii_bits8(digit), *w = tk_pii_bits8(digit | alpha | tk_pii_eq8(v, '_') | tk_pii_eq8(v, '.'));
    };
    uint32_t a0, d0, w0, a1, d1, w1;
    half(lo, &a0, &d0, &w0), half(hi, &a1, &d1, &w1);
    *at = a0 | (a1 << 8), *dig = d0 | (d1 << 8), *wdot = w0 | (w1 << 8);
}

// A placeholder is 0 .. 32 bytes of well-formed UTF-8 without '\n'.  0, or why not: 2 too long, 3 a newline, 4 ill-formed.
TK_HD int tk_pii_placeholder_ok(const uint8_t* s, uint64_t n) {
    if (n > TK_PII_MAX_PLACEHOLDER) return 2;
    for (uint64_t i = 0; i < n;) {
        const uint32_t b = s[i];
        if (b == '\n') return 3;
        const uint32_t len = b < 0x80u ? 1u : b - 0xC2u < 0x1Eu ? 2u : (b & 0xF0u) == 0xE0u ? 3u : b - 0xF0u < 5u ? 4u : 0u;
        if (!len || i + len > n) return 4;
        for (uint32_t k = 1; k < len; ++k)
            if ((s[i + k] & 0xC0u) != 0x80u) return 4;
        if ((b == 0xE0u && s[i + 1] < 0xA0u) || (b == 0xEDu && s[i + 1] > 0x9Fu) || (b == 0xF0u && s[i + 1] < 0x90u) || (b == 0xF4u && s[i + 1] > 0x8Fu)) return 4;
        i += len;
    }
    return 0;
}
// The arguments of a call into *p.  0, or why not: 1 n_bytes, 2 .. 4 a placeholder (tk_pii_placeholder_ok)
TK_HD int tk_pii_shape(uint64_t n_bytes, uint64_t n_docs, const uint8_t* email, uint64_t n_email, const uint8_t* ip, uint64_t n_ip, uint32_t public_only, TkPii* p) {
    if (n_bytes > TK_PII_MAX_BYTES) return 1;
    if (int rc = tk_pii_placeholder_ok(email, n_email)) return rc;
    if (int rc = tk_pii_placeholder_ok(ip, n_ip)) return rc;
    p->n_bytes = n_bytes, p->n_docs = n_docs, p->n_tiles = (uint32_t)(n_bytes / TK_PII_TILE + 1);  // (position N lies in a tile)
    p->len_email = (uint32_t)n_email, p->len_ip = (uint32_t)n_ip, p->public_only = public_only ? 1u : 0u;
    for (uint32_t w = 0; w < TK_PII_MAX_PLACEHOLDER / 4; ++w) p->ph[0][w] = p->ph[1][w] = 0;
    for (uint32_t i = 0; i < n_email; ++i) p->ph[0][i >> 2] |= (uint32_t)email[i] << (8u * (i & 3u));
    for (uint32_t i = 0; i < n_ip; ++i) p->ph[1][i >> 2] |= (uint32_t)ip[i] << (8u * (i & 3u));
    return 0;
}
