// JSON Lines on the device (tk_jsonl.h): the rule, as plain C++ shared by the kernels and the CPU simulation (tests/test_jsonl_sim.py).
// It is quoted in include/tiktoken_amd.h and restated, as a byte scanner, in tests/jsonl_ref.py.
//
// THE RULE.  A buffer of n bytes is cut into lines at every raw 0x0A; a last line without a newline counts; a buffer that ends with a
// newline has no empty line behind it.  A UTF-8 BOM at byte 0 of the buffer is skipped: its three bytes count as whitespace.  Whitespace is
// space, \t and \r, so a \r before the newline is trailing whitespace.  JSON forbids a raw newline inside a string, so string state never
// crosses a line: LINES ARE INDEPENDENT, and that is what makes the pass parallel.
// Within a line, byte by byte:
//  * A byte is ESCAPED if an odd run of backslashes ends right before it (inside and outside strings alike; a run does not cross a line).
//  * An unescaped " toggles the IN-STRING state; the state is off at the line's start.
//  * Outside strings { and [ raise the DEPTH, } and ] lower it; the depth is 0 at the line's start.
//  * A KEY is a string that opens at depth 1 and whose closing quote is followed, after any of space \t \r, by ':'.
//  * The FIELD (1 .. 64 bytes, none of them ", \ or below 0x20) matches a key whose raw bytes between the quotes equal it.  A key spelled
//    with escapes ("text") does not match: keys are compared as bytes, not as strings.
//  * Of several matching keys the last one wins, as with json.loads.
//  * The VALUE: after the colon and any of space \t \r, if the next byte is " the value is the string that opens there; anything else
//    (null, a number, an object, an array, the line's end) gives NOT_STRING.
//  * UNESCAPE of the value's bytes: \" \\ \/ \b \f \n \r \t become one byte each; \uXXXX (hex digits in either case) becomes the UTF-8 of
//    the code point; a high surrogate escape directly followed by a low surrogate escape becomes one 4-byte char; a surrogate escape without
//    its partner becomes U+FFFD (EF BF BD), which is what Encoding.encode makes of the str json.loads returns for it; every other byte is
//    copied.  Every escape shrinks, so the text of a buffer never exceeds n bytes.
//  * STATUS of a line (uint8): TK_JSONL_BLANK: only whitespace (never a record).  TK_JSONL_BAD: the first non-whitespace byte is not '{'; a
//    string is open at the line's end; the depth is not 0 at the line's end, or drops below 1 before the last structural byte (stated as:
//    the structural bytes outside strings behind which the depth is <= 0 are exactly one); a raw byte < 0x20 inside any string; inside the
//    SELECTED VALUE a backslash followed by anything outside the list above, or \u without four hex digits; inside the selected value
//    ill-formed UTF-8, by the strictness of the device check of decode (tk_utf8_repair_rule.h: no overlong forms, no surrogates, nothing
//    above U+10FFFF).  TK_JSONL_MISSING: no matching key at depth 1.  TK_JSONL_NOT_STRING.  TK_JSONL_OK.  BAD takes precedence over
//    MISSING, NOT_STRING and OK.
//  * THE PASS IS NOT A JSON VALIDATOR.  Numbers, literals, commas and escapes in strings other than the selected value are not checked.
// Consequence: for every line json.loads accepts as an object, status and text equal what json.loads(line).get(field) gives, with the
// surrogate repair above (keys spelled with escapes aside).
// The UTF-8 check looks at the value's raw bytes: an escape's output is well formed by itself and starts with a byte that continues
// nothing, so the written text is well formed exactly when the raw bytes >= 0x80 between the escapes are.
//
// HOW IT IS COMPUTED.  The buffer is read in tiles of `tile` bytes (TK_JSONL_TILE on the device; any multiple of 64 gives the same
// result), a wavefront per tile, 64 bytes per step: the classes of the 64 bytes as ballot masks, the escaped mask from the backslash
// runs, in-string by the parity of the unescaped quotes since the line's start, depth by their counted brackets.
//  1 summary (tk_jsonl_tile_sum): a tile does not know the state it is entered in.  Only two things depend on it: whether the byte behind
//    the tile's leading backslashes is escaped, and the in-string state up to the tile's first newline.  So the summary holds the counts
//    of both hypotheses for the head, and entry-independent counts for the rest.
//  2 carry (tk_jsonl_carry_*): exclusive sums and maxima over the tiles (tk_scan.h) give every tile its entry state: backslash parity from
//    the last byte that is no backslash, the line's start from the last newline, in-string and depth as differences of running counts
//    between the tile's start and the line's start.  A line of many MiB costs these scans, not a walk.
//  3 select (tk_jsonl_tile_select): with the entry state every byte's state is exact.  Per line: flags, the count of low structural bytes,
//    the last matching key's value (a maximum), the line's offset.  The escaped mask is kept as a bit plane.
//  4 text (tk_jsonl_tile_text, run twice): the unescaped length of every byte of a selected value, per tile and, at the value's two
//    quotes, per line; after a sum over the tiles every byte knows where it goes.  An escape is owned by its backslash, a surrogate pair
//    by the backslash of its high half; the other bytes of an escape write nothing.  Bytes of other tiles and the escaped plane are read
//    where an escape, a pair, a key or a char straddles a tile's edge.
#pragma once
#include <stdint.h>

#include "tk_utf8_repair_rule.h"  // tk_u8r_lead_len, tk_u8r_cont, tk_u8r_first_ok: the strictness of decode's check; TK_HD, tk_popc64

#define TK_JSONL_TILE 4096u
#define TK_JSONL_FIELD_MAX 64u
#define TK_JSONL_MAX_BYTES 0xFFFF0000ull  // positions are 32-bit on the device

#define TK_JSONL_ST_OK 0u
#define TK_JSONL_ST_BLANK 1u
#define TK_JSONL_ST_MISSING 2u
#define TK_JSONL_ST_NOT_STRING 3u
#define TK_JSONL_ST_BAD 4u

#define TK_JSONL_M_RAISE 0u
#define TK_JSONL_M_SKIP 1u
#define TK_JSONL_M_EMPTY 2u

// classes of a byte (one ballot each)
#define TK_JC_BS 1u
#define TK_JC_Q 2u
#define TK_JC_NL 4u
#define TK_JC_OP 8u
#define TK_JC_CL 16u
#define TK_JC_WS 32u
#define TK_JC_CTL 64u
#define TK_JC_VALID 128u
// flags of a line
#define TK_JF_NONBLANK 1u
#define TK_JF_FIRST 2u    // the first non-whitespace byte is not '{'
#define TK_JF_OPEN 4u     // a string is open at the line's end
#define TK_JF_DEPTH 8u    // the depth is not 0 at the line's end
#define TK_JF_CTL 16u     // a raw byte < 0x20 inside a string
#define TK_JF_ESC 32u     // selected value: a bad escape
#define TK_JF_UTF8 64u    // selected value: ill-formed UTF-8
#define TK_JF_BAD (TK_JF_FIRST | TK_JF_OPEN | TK_JF_DEPTH | TK_JF_CTL | TK_JF_ESC | TK_JF_UTF8)

// report words of a call
#define TK_JSONL_W_LINES 0
#define TK_JSONL_W_DOCS 1
#define TK_JSONL_W_TEXT 2
#define TK_JSONL_W_BADLINE 3  // the first line TK_JSONL_RAISE refuses (all ones: none)
#define TK_JSONL_WORDS 4
#define TK_JSONL_LB 256u  // lines per block of the line passes

struct TkJsonl {
    const uint8_t* p;
    uint32_t n, bom, eof_nl;  // bom: 3 if the buffer starts with EF BB BF; eof_nl: the last line has no newline: one is imagined at n
    uint32_t tile, n_tiles, mode, flen;
    uint8_t field[TK_JSONL_FIELD_MAX];
};
// 0, or why a call is refused: 1 field length, 2 field byte, 3 flags, 4 too many bytes, 5 tile
TK_HD int tk_jsonl_shape(uint64_t n, const uint8_t* field, uint64_t flen, uint32_t flags, uint32_t tile, TkJsonl* j) {
    if (flen < 1 || flen > TK_JSONL_FIELD_MAX) return 1;
    for (uint64_t i = 0; i < flen; ++i)
        if (field[i] == '"' || field[i] == '\\' || field[i] < 0x20u) return 2;
    if (flags > TK_JSONL_M_EMPTY) return 3;
    if (n > TK_JSONL_MAX_BYTES) return 4;
    if (!tile || tile % 64u) return 5;
    j->n = (uint32_t)n;
    j->tile = tile;
    j->n_tiles = (uint32_t)((n + 1 + tile - 1) / tile);  // (positions 0 .. n: the imagined newline has a lane)
    j->mode = flags;
    j->flen = (uint32_t)flen;
    for (uint32_t i = 0; i < TK_JSONL_FIELD_MAX; ++i) j->field[i] = i < flen ? field[i] : 0;
    return 0;
}
// ... what of it the buffer's first and last bytes decide (the entries copy those four bytes to the host first)
TK_HD void tk_jsonl_ends(TkJsonl* j, const uint8_t* p) {
    j->p = p;
    j->bom = j->n >= 3 && p[0] == 0xEFu && p[1] == 0xBBu && p[2] == 0xBFu ? 3u : 0u;
    j->eof_nl = j->n && p[j->n - 1] != '\n' ? 1u : 0u;
}
TK_HD uint32_t tk_jsonl_at(const TkJsonl& j, uint64_t pos) { return pos < j.n ? j.p[pos] : 0u; }
TK_HD uint32_t tk_jsonl_class(const TkJsonl& j, uint32_t pos) {
    if (pos >= j.n) return pos == j.n && j.eof_nl ? (TK_JC_NL | TK_JC_VALID) : TK_JC_WS;
    if (pos < j.bom) return TK_JC_WS | TK_JC_VALID;
    const uint32_t c = j.p[pos];
    uint32_t k = TK_JC_VALID;
    if (c == '\\') k |= TK_JC_BS;
    else if (c == '"') k |= TK_JC_Q;
    else if (c == '\n') k |= TK_JC_NL;
    else if (c == '{' || c == '[') k |= TK_JC_OP;
    else if (c == '}' || c == ']') k |= TK_JC_CL;
    else if (c == ' ' || c == '\t' || c == '\r') k |= TK_JC_WS;
    if (c < 0x20u && c != '\n') k |= TK_JC_CTL;
    return k;
}

struct TkJsonlMasks {
    uint64_t bs, q, nl, op, cl, ws, ctl, valid;
};
// the bits below lane i (i = 64: all)
TK_HD uint64_t tk_jsonl_lo(uint32_t i) { return i >= 64u ? ~0ull : (1ull << i) - 1ull; }
TK_HD uint32_t tk_jsonl_msb(uint64_t v) { return 63u - tk_clz64(v); }
// the bits below lane i that lie behind the last newline below it; *fresh: there is one
TK_HD uint64_t tk_jsonl_seg(uint64_t nl, uint32_t i, bool* fresh) {
    const uint64_t lo = tk_jsonl_lo(i), nlb = nl & lo;
    *fresh = nlb != 0;
    return nlb ? lo & ~((2ull << tk_jsonl_msb(nlb)) - 1ull) : lo;
}
// parity of the backslash run that ends right before lane i (carry: the parity of the run that ends right before the word)
TK_HD uint32_t tk_jsonl_run_parity(uint64_t bs, uint32_t i, uint32_t carry) {
    const uint64_t x = ~bs & tk_jsonl_lo(i);
    return x ? (i - 1u - tk_jsonl_msb(x)) & 1u : (i + carry) & 1u;
}
// the state a tile (and inside it every word) is entered in
struct TkJsonlCarry {
    uint32_t e, s, nonws, line, opener;  // backslash parity; in-string; the line has a non-whitespace byte; line index; 1 + the last unescaped quote
    int32_t depth;
};
TK_HD uint32_t tk_jsonl_lane_s(uint64_t nl, uint64_t uq, uint32_t i, uint32_t s_in) {
    bool fresh;
    const uint64_t seg = tk_jsonl_seg(nl, i, &fresh);
    return (tk_popc64(uq & seg) & 1u) ^ (fresh ? 0u : s_in);
}
TK_HD int32_t tk_jsonl_lane_depth(uint64_t nl, uint64_t so, uint64_t sc, uint32_t i, int32_t d_in) {
    bool fresh;
    const uint64_t seg = tk_jsonl_seg(nl, i, &fresh);
    return (fresh ? 0 : d_in) + (int32_t)tk_popc64(so & seg) - (int32_t)tk_popc64(sc & seg);
}
TK_HD uint32_t tk_jsonl_lane_opener(uint64_t nl, uint64_t uq, uint32_t i, uint32_t base, uint32_t op_in) {
    bool fresh;
    const uint64_t q = uq & tk_jsonl_seg(nl, i, &fresh);
    return q ? base + tk_jsonl_msb(q) + 1u : fresh ? 0u : op_in;
}

// The 64 bytes from `base` on as masks.  Wave: ballot(f), each(f), reg(lane) -- the wavefront on the device, a loop over 64 lanes on the host.
template <class Wave>
TK_HD void tk_jsonl_masks(const TkJsonl& j, Wave& w, uint32_t base, TkJsonlMasks* m) {
    w.each([&](uint32_t l) { w.reg(l) = tk_jsonl_class(j, base + l); });
    m->bs = w.ballot([&](uint32_t l) { return (w.reg(l) & TK_JC_BS) != 0; });
    m->q = w.ballot([&](uint32_t l) { return (w.reg(l) & TK_JC_Q) != 0; });
    m->nl = w.ballot([&](uint32_t l) { return (w.reg(l) & TK_JC_NL) != 0; });
    m->op = w.ballot([&](uint32_t l) { return (w.reg(l) & TK_JC_OP) != 0; });
    m->cl = w.ballot([&](uint32_t l) { return (w.reg(l) & TK_JC_CL) != 0; });
    m->ws = w.ballot([&](uint32_t l) { return (w.reg(l) & TK_JC_WS) != 0; });
    m->ctl = w.ballot([&](uint32_t l) { return (w.reg(l) & TK_JC_CTL) != 0; });
    m->valid = w.ballot([&](uint32_t l) { return (w.reg(l) & TK_JC_VALID) != 0; });
}

// ---- 1: the summary of a tile.  Arrays of n_tiles entries each; the first seven are scanned in place by the carry.
struct TkJsonlTiles {
    uint32_t *nonbs, *nl, *nonws, *lastq;  // 1 + the position of the tile's last byte that is no backslash / newline / non-whitespace byte / unescaped quote (0: none)
    uint32_t *nnl, *nq;                    // newlines, unescaped quotes
    int32_t* d;                            // depth delta (set by the carry: it depends on the hypothesis)
    uint32_t *lead, *qtail;                // leading backslashes, bit 31: the byte behind them is a quote; unescaped quotes behind the last newline
    int32_t *dhead0, *dhead1, *drest, *dtail;  // delta up to the first newline entered outside / inside a string; behind it; behind the last newline
    uint32_t* bits;                        // set by the carry: 1 e, 2 the quote behind the leading backslashes is unescaped, 4 s, 8 hypothesis
};
template <class Wave>
TK_HD void tk_jsonl_tile_sum(const TkJsonl& j, Wave& w, uint32_t t, const TkJsonlTiles& T) {
    uint32_t e = 0, s = 0, lead = 0, isq = 0, nonbs = 0, nl = 0, nonws = 0, lastq = 0, nnl = 0, nq = 0, qtail = 0;
    int32_t dhead0 = 0, dhead1 = 0, drest = 0, dtail = 0;
    bool leading = true, head = true;
    for (uint32_t k = 0; k < j.tile / 64u; ++k) {
        const uint32_t base = t * j.tile + k * 64u;
        TkJsonlMasks m;
        tk_jsonl_masks(j, w, base, &m);
        const uint64_t E = w.ballot([&](uint32_t l) { return tk_jsonl_run_parity(m.bs, l, e) != 0; });
        e = tk_jsonl_run_parity(m.bs, 64u, e);
        uint64_t uq = m.q & ~E;
        if (leading) {
            if (~m.bs) {
                const uint32_t L = tk_ctz64(~m.bs);
                lead += L;
                leading = false;
                if ((m.q >> L) & 1u) {
                    isq = 1;
                    uq &= ~(1ull << L);
                }
            } else {
                lead += 64u;
            }
        }
        const uint64_t Sb = w.ballot([&](uint32_t l) { return tk_jsonl_lane_s(m.nl, uq, l, s) != 0; });
        s = tk_jsonl_lane_s(m.nl, uq, 64u, s);
        const uint64_t so = m.op & ~Sb, sc = m.cl & ~Sb;
        const uint64_t hm = !head ? 0ull : m.nl ? tk_jsonl_lo(tk_ctz64(m.nl)) : ~0ull, rm = ~hm;
        dhead0 += (int32_t)tk_popc64(so & hm) - (int32_t)tk_popc64(sc & hm);
        dhead1 += (int32_t)tk_popc64(m.op & Sb & hm) - (int32_t)tk_popc64(m.cl & Sb & hm);
        drest += (int32_t)tk_popc64(so & rm) - (int32_t)tk_popc64(sc & rm);
        if (m.nl) {
            const uint64_t after = ~((2ull << tk_jsonl_msb(m.nl)) - 1ull);
            dtail = (int32_t)tk_popc64(so & after) - (int32_t)tk_popc64(sc & after);
            qtail = tk_popc64(uq & after);
            nl = base + tk_jsonl_msb(m.nl) + 1u;
            head = false;
        } else {
            dtail += (int32_t)tk_popc64(so & rm) - (int32_t)tk_popc64(sc & rm);
            qtail += tk_popc64(uq);
        }
        nq += tk_popc64(uq);
        nnl += tk_popc64(m.nl);
        if (~m.bs) nonbs = base + tk_jsonl_msb(~m.bs) + 1u;
        const uint64_t nw = m.valid & ~m.ws & ~m.nl;
        if (nw) nonws = base + tk_jsonl_msb(nw) + 1u;
        if (uq) lastq = base + tk_jsonl_msb(uq) + 1u;
    }
    w.once([&] {
        T.nonbs[t] = nonbs, T.nl[t] = nl, T.nonws[t] = nonws, T.lastq[t] = lastq, T.nnl[t] = nnl, T.nq[t] = nq, T.d[t] = 0;
        T.lead[t] = lead | (isq << 31), T.qtail[t] = qtail, T.dhead0[t] = dhead0, T.dhead1[t] = dhead1, T.drest[t] = drest, T.dtail[t] = dtail, T.bits[t] = 0;
    });
}

// ---- 2: the carry.  Between the scans (exclusive, in place), per tile:
// behind the scans of nonbs, nl, nonws, nnl: is the byte behind the leading backslashes escaped?  A quote there counts if it is not.
TK_HD void tk_jsonl_carry_q(const TkJsonl& j, const TkJsonlTiles& T, uint32_t t) {
    const uint32_t e = (t * j.tile - T.nonbs[t]) & 1u, lead = T.lead[t] & 0x7FFFFFFFu;
    const uint32_t flip = (T.lead[t] >> 31) && ((e + lead) & 1u) == 0u ? 1u : 0u;
    T.bits[t] = e | (flip << 1);
    if (flip) {
        T.nq[t] += 1u;
        const uint32_t at = t * j.tile + lead + 1u;
        if (at > T.lastq[t]) T.lastq[t] = at;
    }
}
// behind the scans of nq and lastq: in-string at the tile's start, the hypothesis of its head, its depth delta
TK_HD void tk_jsonl_carry_d(const TkJsonl& j, const TkJsonlTiles& T, uint32_t t) {
    const uint32_t ls = T.nl[t];  // the line's start
    uint32_t at_ls = 0;
    if (ls) {
        const uint32_t u = (ls - 1u) / j.tile;
        at_ls = T.nq[u + 1u] - T.qtail[u];
    }
    const uint32_t s = (T.nq[t] - at_ls) & 1u, h = s ^ ((T.bits[t] >> 1) & 1u);
    T.bits[t] |= (s << 2) | (h << 3);
    T.d[t] = (h ? T.dhead1[t] : T.dhead0[t]) + T.drest[t];
}
// behind the scan of d: the entry state
TK_HD TkJsonlCarry tk_jsonl_carry_entry(const TkJsonl& j, const TkJsonlTiles& T, uint32_t t) {
    const uint32_t ls = T.nl[t];
    int32_t at_ls = 0;
    if (ls) {
        const uint32_t u = (ls - 1u) / j.tile;
        at_ls = T.d[u + 1u] - T.dtail[u];
    }
    TkJsonlCarry c;
    c.e = T.bits[t] & 1u;
    c.s = (T.bits[t] >> 2) & 1u;
    c.nonws = T.nonws[t] > ls ? 1u : 0u;
    c.line = T.nnl[t];
    c.opener = T.lastq[t];
    c.depth = T.d[t] - at_ls;
    return c;
}

// ---- 3: select
// the key that opens at `pos` (an unescaped quote at depth 1): 0, or 2 (1 + the position of its value's first byte) + (it is a quote)
TK_HD uint64_t tk_jsonl_key(const TkJsonl& j, uint32_t pos) {
    uint64_t q = (uint64_t)pos + 1u;
    for (uint32_t i = 0; i < j.flen; ++i, ++q)
        if (tk_jsonl_at(j, q) != j.field[i]) return 0;
    if (tk_jsonl_at(j, q) != '"') return 0;
    ++q;
    for (uint32_t c = tk_jsonl_at(j, q); c == ' ' || c == '\t' || c == '\r'; c = tk_jsonl_at(j, ++q)) {}
    if (tk_jsonl_at(j, q) != ':') return 0;
    ++q;
    for (uint32_t c = tk_jsonl_at(j, q); c == ' ' || c == '\t' || c == '\r'; c = tk_jsonl_at(j, ++q)) {}
    return 2ull * (q + 1u) + (tk_jsonl_at(j, q) == '"' ? 1u : 0u);
}
// Out: flag(line, bits), low(line), vmax(line, v), line_off(line, pos), eplane(word, mask)
template <class Wave, class Out>
TK_HD void tk_jsonl_tile_select(const TkJsonl& j, Wave& w, uint32_t t, TkJsonlCarry c, Out& out) {
    for (uint32_t k = 0; k < j.tile / 64u; ++k) {
        const uint32_t base = t * j.tile + k * 64u;
        TkJsonlMasks m;
        tk_jsonl_masks(j, w, base, &m);
        const uint64_t E = w.ballot([&](uint32_t l) { return tk_jsonl_run_parity(m.bs, l, c.e) != 0; });
        w.once([&] { out.eplane(base / 64u, E); });
        const uint64_t uq = m.q & ~E;
        const uint64_t Sb = w.ballot([&](uint32_t l) { return tk_jsonl_lane_s(m.nl, uq, l, c.s) != 0; });
        const uint64_t so = m.op & ~Sb, sc = m.cl & ~Sb, nw = m.valid & ~m.ws & ~m.nl;
        w.each([&](uint32_t l) {
            const uint64_t bit = 1ull << l;
            if (!(m.valid & bit)) return;
            bool fresh;
            const uint64_t seg = tk_jsonl_seg(m.nl, l, &fresh);
            const uint32_t sb = (uint32_t)((Sb >> l) & 1u), pos = base + l, line = c.line + tk_popc64(m.nl & tk_jsonl_lo(l));
            const int32_t db = tk_jsonl_lane_depth(m.nl, so, sc, l, c.depth);
            if (m.nl & bit) {
                uint32_t f = 0;
                if (sb) f |= TK_JF_OPEN;
                if (db != 0) f |= TK_JF_DEPTH;
                if (f) out.flag(line, f);
                out.line_off(line + 1u, pos + 1u < j.n ? pos + 1u : j.n);
                return;
            }
            if ((m.ctl & bit) && sb) out.flag(line, TK_JF_CTL);
            if ((nw & bit) && !(nw & seg) && (fresh || !c.nonws)) out.flag(line, TK_JF_NONBLANK | (tk_jsonl_at(j, pos) == '{' && pos >= j.bom ? 0u : TK_JF_FIRST));
            if ((so | sc) & bit) {
                if (db + ((so & bit) ? 1 : -1) <= 0) out.low(line);
            }
            if ((uq & bit) && !sb && db == 1) {
                const uint64_t v = tk_jsonl_key(j, pos);
                if (v) out.vmax(line, v);
            }
        });
        const TkJsonlCarry in = c;
        c.e = tk_jsonl_run_parity(m.bs, 64u, in.e);
        c.s = tk_jsonl_lane_s(m.nl, uq, 64u, in.s);
        c.depth = tk_jsonl_lane_depth(m.nl, so, sc, 64u, in.depth);
        c.line = in.line + tk_popc64(m.nl);
        c.opener = tk_jsonl_lane_opener(m.nl, uq, 64u, base, in.opener);
        bool fresh;
        const uint64_t seg = tk_jsonl_seg(m.nl, 64u, &fresh);
        c.nonws = (nw & seg) || (!fresh && in.nonws) ? 1u : 0u;
    }
}

// ---- 4: text
TK_HD int32_t tk_jsonl_hex4(const TkJsonl& j, uint64_t pos) {
    uint32_t v = 0;
    for (uint32_t i = 0; i < 4u; ++i) {
        const uint32_t c = tk_jsonl_at(j, pos + i);
        uint32_t d;
        if (c >= '0' && c <= '9') d = c - '0';
        else if (c >= 'a' && c <= 'f') d = c - 'a' + 10u;
        else if (c >= 'A' && c <= 'F') d = c - 'A' + 10u;
        else return -1;
        v = v * 16u + d;
    }
    return (int32_t)v;
}
TK_HD bool tk_jsonl_esc_bit(const uint64_t* ep, uint64_t pos) { return (ep[pos >> 6] >> (pos & 63u)) & 1u; }
// a raw byte c >= 0x80 at pos: is it part of an ill-formed sequence?  A lead checks what follows it, a continuation byte that a lead reaches it.
TK_HD bool tk_jsonl_utf8_bad(const TkJsonl& j, uint32_t pos, uint32_t c) {
    if (tk_u8r_cont(c)) {
        for (uint32_t k = 1; k <= 3u && k <= pos; ++k) {
            const uint32_t b = tk_jsonl_at(j, pos - k);
            if (!tk_u8r_cont(b)) return !(tk_u8r_lead_len(b) > k);
        }
        return true;
    }
    const uint32_t len = tk_u8r_lead_len(c);
    if (!len) return true;
    for (uint32_t i = 1; i < len; ++i) {
        const uint32_t b = tk_jsonl_at(j, (uint64_t)pos + i);
        if (!tk_u8r_cont(b) || (i == 1u && !tk_u8r_first_ok(c, b))) return true;
    }
    return false;
}
TK_HD uint32_t tk_jsonl_utf8(uint32_t cp, uint32_t* out) {
    if (cp < 0x80u) return *out = cp, 1u;
    if (cp < 0x800u) return *out = (0xC0u | (cp >> 6)) | ((0x80u | (cp & 63u)) << 8), 2u;
    if (cp < 0x10000u) return *out = (0xE0u | (cp >> 12)) | ((0x80u | ((cp >> 6) & 63u)) << 8) | ((0x80u | (cp & 63u)) << 16), 3u;
    return *out = (0xF0u | (cp >> 18)) | ((0x80u | ((cp >> 12) & 63u)) << 8) | ((0x80u | ((cp >> 6) & 63u)) << 16) | ((0x80u | (cp & 63u)) << 24), 4u;
}
// What the byte at pos of the value that opens at vpos writes: the count, the bytes in *out (the first in the low byte); *bad: TK_JF_ESC, TK_JF_UTF8.
TK_HD uint32_t tk_jsonl_unescape(const TkJsonl& j, const uint64_t* ep, uint32_t pos, uint32_t vpos, uint32_t* out, uint32_t* bad) {
    const uint32_t c = tk_jsonl_at(j, pos);
    if (tk_jsonl_esc_bit(ep, pos)) return 0;  // the byte behind an escape's backslash
    if (c != '\\') {
        for (uint32_t k = 2; k <= 5u; ++k)  // a hex digit of \uXXXX
            if (pos >= vpos + 1u + k && tk_jsonl_at(j, pos - k) == '\\' && !tk_jsonl_esc_bit(ep, pos - k) && tk_jsonl_at(j, pos - k + 1u) == 'u') return 0;
        if (c >= 0x80u && tk_jsonl_utf8_bad(j, pos, c)) *bad |= TK_JF_UTF8;
        *out = c;
        return 1;
    }
    const uint32_t n = tk_jsonl_at(j, (uint64_t)pos + 1u);
    switch (n) {
        case '"': case '\\': case '/': *out = n; return 1;
        case 'b': *out = 8; return 1;
        case 'f': *out = 12; return 1;
        case 'n': *out = 10; return 1;
        case 'r': *out = 13; return 1;
        case 't': *out = 9; return 1;
        case 'u': break;
        default: *bad |= TK_JF_ESC; return 0;
    }
    int32_t cp = tk_jsonl_hex4(j, (uint64_t)pos + 2u);
    if (cp < 0) {
        *bad |= TK_JF_ESC;
        return 0;
    }
    if (cp >= 0xD800 && cp < 0xDC00) {
        const int32_t lo = tk_jsonl_at(j, (uint64_t)pos + 6u) == '\\' && tk_jsonl_at(j, (uint64_t)pos + 7u) == 'u' ? tk_jsonl_hex4(j, (uint64_t)pos + 8u) : -1;
        cp = lo >= 0xDC00 && lo < 0xE000 ? 0x10000 + ((cp - 0xD800) << 10) + (lo - 0xDC00) : 0xFFFD;
    } else if (cp >= 0xDC00 && cp < 0xE000) {
        if (pos >= vpos + 7u && tk_jsonl_at(j, pos - 6u) == '\\' && !tk_jsonl_esc_bit(ep, pos - 6u) && tk_jsonl_at(j, pos - 5u) == 'u') {
            const int32_t hi = tk_jsonl_hex4(j, pos - 4u);
            if (hi >= 0xD800 && hi < 0xDC00) return 0;  // the pair is the high half's
        }
        cp = 0xFFFD;
    }
    return tk_jsonl_utf8((uint32_t)cp, out);
}
// Sink: bad(line, bits), vstart(line, rel), vend(line, pos, rel), bytes(line, rel, v, n), done(t, total); rel counts the tile's output so far.
// vmax: what select left per line.
template <class Wave, class Sink>
TK_HD void tk_jsonl_tile_text(const TkJsonl& j, Wave& w, uint32_t t, TkJsonlCarry c, const uint64_t* ep, const uint64_t* vmax, Sink& sink) {
    uint32_t run = 0;
    for (uint32_t k = 0; k < j.tile / 64u; ++k) {
        const uint32_t base = t * j.tile + k * 64u;
        TkJsonlMasks m;
        tk_jsonl_masks(j, w, base, &m);
        const uint64_t uq = m.q & ~ep[base / 64u];
        const uint64_t Sb = w.ballot([&](uint32_t l) { return tk_jsonl_lane_s(m.nl, uq, l, c.s) != 0; });
        // reg: bit 0 the lane's byte belongs to the selected value; bit 1 it is its opening quote, bit 2 its closing quote
        w.each([&](uint32_t l) {
            const uint64_t bit = 1ull << l;
            uint32_t r = 0;
            if ((m.valid & bit) && !(m.nl & bit)) {
                const uint64_t v = vmax[c.line + tk_popc64(m.nl & tk_jsonl_lo(l))];
                if (v & 1u) {
                    const uint32_t vq = (uint32_t)(v >> 1);  // 1 + the opening quote
                    const bool sb = (Sb >> l) & 1u;
                    if (base + l + 1u == vq) r = 2;
                    else if (sb && tk_jsonl_lane_opener(m.nl, uq, l, base, c.opener) == vq) r = (uq & bit) ? 4u : 1u;
                }
            }
            w.reg(l) = r;
        });
        const uint32_t total = w.scan([&](uint32_t l) {
            if (!(w.reg(l) & 1u)) return 0u;
            uint32_t v = 0, bad = 0;
            const uint64_t vm = vmax[c.line + tk_popc64(m.nl & tk_jsonl_lo(l))];
            return tk_jsonl_unescape(j, ep, base + l, (uint32_t)(vm >> 1) - 1u, &v, &bad);
        });
        w.each([&](uint32_t l) {
            const uint32_t r = w.reg(l);
            if (!r) return;
            const uint32_t line = c.line + tk_popc64(m.nl & tk_jsonl_lo(l)), rel = run + w.pre(l);
            if (r == 2u) sink.vstart(line, rel);
            else if (r == 4u) sink.vend(line, base + l, rel);
            else {
                uint32_t v = 0, bad = 0;
                const uint32_t nb = tk_jsonl_unescape(j, ep, base + l, (uint32_t)(vmax[line] >> 1) - 1u, &v, &bad);
                if (bad) sink.bad(line, bad);
                if (nb) sink.bytes(line, rel, v, nb);
            }
        });
        run += total;
        const TkJsonlCarry in = c;
        c.s = tk_jsonl_lane_s(m.nl, uq, 64u, in.s);
        c.line = in.line + tk_popc64(m.nl);
        c.opener = tk_jsonl_lane_opener(m.nl, uq, 64u, base, in.opener);
    }
    w.once([&] { sink.done(t, run); });
}

// ---- per line
TK_HD uint32_t tk_jsonl_status(uint32_t flags, uint32_t low, uint64_t vmax) {
    if (!(flags & TK_JF_NONBLANK)) return TK_JSONL_ST_BLANK;
    if ((flags & TK_JF_BAD) || low != 1u) return TK_JSONL_ST_BAD;
    if (!vmax) return TK_JSONL_ST_MISSING;
    return (vmax & 1u) ? TK_JSONL_ST_OK : TK_JSONL_ST_NOT_STRING;
}
// is the line a document under the mode?  (TK_JSONL_M_RAISE keeps what SKIP keeps; the call is refused if anything else is not blank)
TK_HD bool tk_jsonl_keeps(uint32_t mode, uint32_t status) { return mode == TK_JSONL_M_EMPTY ? status != TK_JSONL_ST_BLANK : status == TK_JSONL_ST_OK; }
struct TkJsonlLines {
    uint32_t *flags, *low, *vs_rel, *ve_pos, *ve_rel, *len, *doc;  // per line; len: the text's bytes; doc: its document, all ones: none
    uint64_t* vmax;
    uint8_t* status;
};
// status and length of a line; G: the exclusive sums of the tiles' output counts
TK_HD void tk_jsonl_line(const TkJsonl& j, const TkJsonlLines& L, const uint32_t* G, uint32_t line) {
    const uint64_t v = L.vmax[line];
    const uint32_t st = tk_jsonl_status(L.flags[line], L.low[line], v);
    uint32_t len = 0;
    if (st == TK_JSONL_ST_OK) {
        const uint32_t vpos = (uint32_t)(v >> 1) - 1u;
        len = (G[L.ve_pos[line] / j.tile] + L.ve_rel[line]) - (G[vpos / j.tile] + L.vs_rel[line]);
    }
    L.status[line] = (uint8_t)st;
    L.len[line] = len;
}
