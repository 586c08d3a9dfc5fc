// The scan value of the normalising line sets (tk_lines.h: TkLnNorm) on the CPU.  A line is cut at given places; every piece becomes
// values of at most 16 bytes the way TkLnNorm::View::tail makes a lane's, and the values are folded with tk_lnn_join left to right and
// as a balanced tree (-1 when the two differ).  line_norm_sim_plain: the plain hash of a byte string, for the reference's normal form.
#include <stdint.h>

#include <vector>

#include "../../tiktoken_amd/csrc/tk_line_set_rule.h"

namespace {
TkLnNSeg chunk(const TkLn& p, const uint8_t* s, uint32_t n) {  // n <= 16
    uint64_t lo = 0, hi = 0;
    for (uint32_t j = 0; j < n; ++j) (j < 8 ? lo : hi) |= (uint64_t)s[j] << (8 * (j & 7u));
    TkLnNSeg v = tk_lnn_empty();
    tk_lnn_append(p, tk_lnn_lane(lo, hi, p.norm), 0, n, v);
    for (uint32_t i = 0; i < v.e.len; ++i) v.e.w1 = tk_ln_mulmod(v.e.w1, p.B1), v.e.w2 = tk_ln_mulmod(v.e.w2, p.B2);
    return v;
}
TkLnNSeg tree(const TkLn& p, const std::vector<TkLnNSeg>& v, size_t a, size_t b) {  // [a, b), a < b
    if (b - a == 1) return v[a];
    const size_t m = a + (b - a) / 2;
    return tk_lnn_join(p, tree(p, v, a, m), tree(p, v, m, b));
}
bool same(const TkLnNSeg& x, const TkLnNSeg& y) {
    return x.e.h1 == y.e.h1 && x.e.w1 == y.e.w1 && x.e.h2 == y.e.h2 && x.e.w2 == y.e.w2 && x.e.bytes == y.e.bytes && x.e.len == y.e.len && x.cut == y.cut;
}
}  // namespace

// out: h1, h2, the body's length, the raw bytes, the key
extern "C" int64_t line_norm_sim_fold(const uint8_t* line, uint64_t n, const uint64_t* cuts, uint64_t n_cuts, uint64_t seed, uint32_t norm, uint64_t* out) {
    TkLn p;
    if (tk_ln_shape(n, 1, seed, &p)) return -2;
    p.norm = norm;
    std::vector<TkLnNSeg> v{tk_lnn_empty()};
    uint64_t a = 0;
    for (uint64_t c = 0; c <= n_cuts; ++c) {
        const uint64_t b = c < n_cuts ? cuts[c] : n;
        if (a == b) v.push_back(tk_lnn_empty());  // (an empty piece: the identity)
        for (; a < b; a += 16) v.push_back(chunk(p, line + a, (uint32_t)(b - a < 16 ? b - a : 16)));
        a = b;
    }
    TkLnNSeg left = tk_lnn_empty();
    for (const TkLnNSeg& x : v) left = tk_lnn_join(p, left, x);
    const TkLnNSeg t = tree(p, v, 0, v.size());
    out[0] = t.e.h1, out[1] = t.e.h2, out[2] = t.e.len, out[3] = t.e.bytes, out[4] = tk_ls_key(seed, t.e);
    return same(left, t) ? 0 : -1;
}
extern "C" int64_t line_norm_sim_plain(const uint8_t* line, uint64_t n, uint64_t seed, uint64_t* out) {
    TkLn p;
    if (tk_ln_shape(n, 1, seed, &p)) return -2;
    TkLnEl e = tk_ln_empty();
    for (uint64_t i = 0; i < n; ++i) tk_ln_push(p, e, line[i]);
    out[0] = e.h1, out[1] = e.h2, out[2] = e.bytes, out[3] = n, out[4] = tk_ls_key(seed, e);
    return 0;
}
