"""The reference of the line cleaning (tk_clean.h): per document re.finditer over the pieces, str.split (for ill-formed text the
white-space regex of the word rule), bytes.lower and `in` -- and the named batches of the GPU tests, a literal dict built from the tile
T, the lane width and the wavefront span.  Nothing from the code under test."""
import re
from collections import namedtuple

import numpy as np

from words_ref import WS, pack

FIELDS = ("n_lines", "n_kept", "n_short", "n_long", "n_no_end", "n_ellipsis", "n_phrase", "doc_hit")
Ref = namedtuple("Ref", ("text", "doc_off", *FIELDS, "counts"))
LINE_PHRASES = (b"javascript", b"terms of use", b"privacy policy", b"cookie policy", b"uses cookies", b"use of cookies", b"use cookies")
DOC_PHRASES = (b"lorem ipsum", b"{")
C4 = dict(min_words=5, max_word_chars=1000, terminal=b".!?\"", drop_ellipsis=True, line_phrases=LINE_PHRASES, doc_phrases=DOC_PHRASES)
OFF = dict(min_words=0, max_word_chars=0, terminal=b"", drop_ellipsis=False, line_phrases=(), doc_phrases=())  # every rule off, one at a time


def doc_clean(t: bytes, r):
    """(the document's kept bytes, the eight counts in the order of FIELDS)"""
    hit = sum(1 << i for i, p in enumerate(r["doc_phrases"]) if p.lower() in t.lower())
    kept, n = [], dict.fromkeys(FIELDS[:-1], 0)
    for piece in (m.group() for m in re.finditer(rb"[^\n]+\n?|\n", t)):
        if piece == b"\n":
            kept.append(piece)
            continue
        line = piece.rstrip(b"\n")
        try:
            words = [w.encode() for w in line.decode().split()]
        except UnicodeDecodeError:
            words = [w for w in WS.split(line) if w]
        end = line.rstrip(b" \t\r")
        rules = (r["min_words"] > 0 and len(words) < r["min_words"],
                 r["max_word_chars"] > 0 and max([sum((c & 0xC0) != 0x80 for c in w) for w in words], default=0) > r["max_word_chars"],
                 len(r["terminal"]) > 0 and (not end or end[-1] not in r["terminal"]),
                 r["drop_ellipsis"] and (end.endswith(b"...") or end.endswith("…".encode())),
                 any(p.lower() in line.lower() for p in r["line_phrases"]))
        n["n_lines"] += 1
        for f, holds in zip(FIELDS[2:7], rules):
            n[f] += bool(holds)
        if not any(rules):
            n["n_kept"] += 1
            kept.append(piece)
    if hit:
        kept, n["n_kept"] = [], 0
    return b"".join(kept), (*n.values(), hit)


def clean(docs, **rules) -> Ref:
    r = {**C4, **rules}
    rows = [doc_clean(bytes(t), r) for t in docs]
    text, off = pack([k for k, _ in rows])
    per_doc = [np.array([c[i] for _, c in rows], np.uint64) for i in range(len(FIELDS))]
    return Ref(text, off, *per_doc, np.array([len(text), int(per_doc[0].sum() - per_doc[1].sum())], np.uint64))


def batches(T: int, lane: int, wave: int):
    """{name: (documents as bytes, the rules that differ from C4's)}; together under 1 MiB"""
    sent = lambda n, last=b".": (b"aa bb cc dd ee " * (n // 15 + 1))[:n - 1] + last  # noqa: E731  (a kept line of n bytes without its '\n')
    e_acute, p32 = "\xe9".encode(), b"0123456789abcdefghijKLMNOPQRSTUV"
    c, upto = b"\x96", lambda n: b"aa bb cc " + b"y" * (n - 10) + b" "  # noqa: E731  (a continuation byte: a word without a char; four words in n bytes)
    # six words a line, one of them continuation bytes alone: cut by the tile edge at T, before 2T, behind 3T; then, from a lane edge on,
    # in lines of two lanes, before, at and behind the lane edge; at a line's end before and behind a lane edge.  Then five words: dropped.
    cont = (upto(T - 2) + c * 4 + b" dd\n" + upto(T - 7) + c + b" dd\n" + upto(T - 4) + c + b" dd\n" + b"\n" * (2 * lane - 5)
            + b"".join((b"y" * k + b" " + c + b" bb cc dd ee").ljust(2 * lane - 1) + b"\n" for k in range(lane - 5, lane + 1))
            + b"aa bb cc dd ee".ljust(lane - 1) + c + b"\n" + b"aa bb cc dd ee".ljust(lane) + c + b"\n" + c + b" bb cc dd ee\n" + c * 3 + b"\n")
    one_each = [b"too few words.\n" + sent(40) + b"\n" + b"y" * 1001 + b" bb cc dd ee.\nthis line has no end\nand this one trails off...\nand so does this one \xe2\x80\xa6 \n"
                b"We use Cookies on this site.\n" + sent(33) + b"\n", b"the {brace} line is fine here.\n"]
    out = {
        "no document": ([], {}),
        "no byte": ([b"", b""], {}),
        "only newlines": ([b"\n", b"\n\n\n", b"", b"\n" * (T + 3)], {}),
        "blanks and empty": ([sent(T - 6, b"!") + b"end...  \r\n" + sent(T - 12) + b" aa end.  \n" + sent(9), b" \t \r\n", b"", b"  ", sent(20) + b" \t\r\n"], {}),
        "nothing dropped": ([sent(50) + b"\n\n" + sent(T) + b"\n", sent(17, b"?"), b"\n" + sent(3 * lane, b"\"") + b"\n"], {}),
        "everything dropped": ([b"no end here at all\n" * 300, b"a b c.\nshort.\n", sent(40) + b"\nlorem IPSUM\n\n"], {}),
        "a line over three tiles": ([sent(2 * T + 100) + b"\n" + sent(2 * T + 100, b",") + b"\n" + b"aa bb cc " + b"y" * (2 * T) + b" dd ee.\n", b"z" * (2 * T + 5) + b"."], {}),
        "a word across a tile edge": ([b"w " * ((T - 10) // 2) + b"y" * 20 + b" end.\n" + sent(T - 26, b" ") + b"y" * 21 + b" end.\n"], dict(max_word_chars=20)),
        "the longest word allowed": ([b"w " * (T // 2 - 250) + e_acute * 1000 + b" a b c d.\n", b"w " * (T // 2 - 250) + e_acute * 1001 + b" a b c d.\n",
                                      b"a b c d " + b"y" * 999 + b".", b"a b c d " + b"y" * 1000 + b"."], {}),
        "phrases at the edges": ([sent(lane - 4, b" ") + b"JavaScript aa bb cc dd.\n" + sent(T - 43, b" ") + b"pRiVaCy PoLiCy aa bb cc.\n" + sent(30) + b"\n",
                                  b"aa bb cc dd ee java", b"script aa bb cc dd.", b"aa bb cc dd ee lorem ", b"ipsum aa bb cc dd.", b"aa bb cc dd uses cookies"], {}),
        "a phrase of 32 bytes": ([sent(T - 11, b" ") + p32.swapcase() + b" bb cc dd ee.\n" + sent(20) + b"\n" + p32[:31] + b" aa bb cc dd ee."], dict(line_phrases=(p32,))),
        "a document phrase with a newline": ([sent(20) + b"\nThe End.\nnext aa bb cc dd.\n", sent(20) + b"\nthe end.\n", b"next aa bb cc dd.\n"], dict(doc_phrases=(b"end.\nNEXT", b"{"))),
        "document phrases first and last": ([b"\n\nLorem Ipsum dolor sit amet.\n\n", sent(T + 9) + b"\n\n" + sent(20), b"\n" + sent(30) + b"\n{\n\n"], {}),
        "many short documents": ([(b"{ b c.\n", b"a b c.\n", b"a b.\n", b"a b c", b"\n")[i % 5] for i in range(3 * T // 8)], dict(min_words=3)),
        "one of each": (one_each, {}),
        "words of continuation bytes": ([cont, c + b" bb cc dd ee ff", b"aa bb cc dd ee " + c, c, c + b" bb cc dd ee\n"], dict(min_words=6, max_word_chars=0, terminal=b"")),
        "ill-formed text": ([b"caf\xc3 \xe2\x80 aa bb cc.\n\xf0\x9f\x98 x \xbf\xbf y.\n\x80\x80 \xbf a \xc3\xa9\xa9 b c end\xe2\x80\naa bb cc dd end\xe2\x80\xa6\n\xff aa\xe2\x80\xa8bb cc dd.\n",
                             b"aa bb cc dd ee\xe2\x80", b"\xa8ff gg hh ii jj.", b"\xc3" * 1001 + b" \xa9 aa bb cc.\n" + b"\xa9" * 1001 + b" aa bb cc dd."], {}),
    }
    for name, edge in (("lane", lane), ("wave", wave), ("tile", T)):
        for k in (-1, 0, 1):  # the '\n' at edge + k, a short line behind it
            out[f"newline at {name} edge {k:+d}"] = ([sent(edge + k) + b"\nshort.\n" + sent(40) + b"\n" + sent(edge + k, b",") + b"\n" + sent(25)], {})
    for last in (b".", b","):  # N a multiple of the tile and the last line open: the empty tile behind the text closes it
        out[f"an open line to the tile's end {last.decode()}"] = ([sent(40) + b"\n" + sent(T - 41, last)], {})
    for rule, value in OFF.items():
        out[f"one of each without {rule}"] = (one_each, {rule: value})
    return out
