"""The reference of the word statistics (tk_words.h): str.split, str.isalpha, bytes.count and split(b"\\n") per document -- for ill-formed
text the white-space regex of the rule and a decode that replaces -- and the named batches of the GPU tests, built from the tile T, the
lane width and the wavefront span.  Nothing from the code under test."""
import re
from collections import namedtuple

import numpy as np

Ref = namedtuple("Ref", "n_words word_chars n_alpha_words stop_mask n_hash n_ellipsis n_lines n_punct_lines")
GOPHER = (b"the", b"be", b"to", b"of", b"and", b"that", b"have", b"with")
TERMINAL = b".!?\"'"
WS = re.compile(rb"[\x09-\x0d\x1c-\x20]|\xc2[\x85\xa0]|\xe1\x9a\x80|\xe2\x80[\x80-\x8a\xa8\xa9\xaf]|\xe2\x81\x9f|\xe3\x80\x80")


def doc_stats(t: bytes, stop, terminal):
    try:
        words = [w.encode() for w in t.decode().split()]
    except UnicodeDecodeError:
        words = [w for w in WS.split(t) if w]
    lines = [s for s in t.split(b"\n") if s]
    return (len(words), sum((c & 0xC0) != 0x80 for w in words for c in w), sum(any(c.isalpha() for c in w.decode("utf-8", "replace")) for w in words),
            sum(1 << i for i, s in enumerate(stop) if s in words), t.count(b"#"), t.count(b"...") + t.count("…".encode()), len(lines),
            sum(s[-1] in terminal for s in lines))


def stats(docs, stop=GOPHER, terminal=TERMINAL) -> Ref:
    rows = [doc_stats(bytes(t), stop, terminal) for t in docs]
    return Ref(*[np.array([r[i] for r in rows], np.uint64) for i in range(len(Ref._fields))])


def pack(docs):
    off = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.uint64)
    return np.frombuffer(b"".join(bytes(d) for d in docs), np.uint8), off


def batches(T: int, lane: int, wave: int):
    """{name: (documents as bytes, stop words, terminal bytes)}; together under 1 MiB"""
    rng = np.random.default_rng(T)
    word = lambda n: bytes(rng.integers(97, 123, max(n, 0), dtype=np.uint8))  # noqa: E731  (n letters)
    digits = lambda n: bytes(rng.integers(48, 58, max(n, 0), dtype=np.uint8))  # noqa: E731
    u = lambda s: s.encode()  # noqa: E731
    pad = lambda piece, edge: piece + b" " + word(-(len(piece) + 1) % edge)  # noqa: E731  (the next piece starts on the grid again)
    spaces = "\u3000\u2003\xa0\x85\u2028\u2029\u202f\u205f\u1680\u200a"
    out = {
        "no document": [],
        "empty and white space": [b"", b" \t\n", b"", u(spaces), b"x", b"", b"\x1c\x1d\x1e\x1f\x0b\x0c\r", u("a" + "b".join(spaces) + "c")],
        "words and symbols": [u("The cat... sat# on #the mat\u2026. 42 \u0663\u0663 \xe9\u4e2d\u03a9 \U0001f600 \u2026\u2026 .. . ...... ....... a.b"),
                              b"to be, or not to be: that is of and with have the", b"12 34 !! ?? #### # #", u("\u4e2d \u6587 \u2014 \u0663")],
        # ill-formed text: the values are written out by hand in test_gpu_words.py
        "ill-formed": [b"a\xc3 b", b"x\xa0y", b"ab \xe2\x80", b"q\xc2", b"\x85r", b"\xe3\x80", b"\x80 z", b"\xf0\x9f\x98 k\xe2\x80\xa6\xa6"],
        # patterns cut by a document boundary: none counts
        "cut patterns": [b"ab\xe2\x80", b"\xa8cd", b"e..", b".f", b"g\xe2\x80", b"\xa6h", b"i\xe3", b"\x80\x80j", b"th", b"e end", b"k\xc3", b"\xa9l"],
        "many one-word documents": [word(1 + i % 3) for i in range(3 * T // 2)] + [b"", b" ", b"the the", b""] * 20,
        "lines": [b"One. Two!\nthree?\n\nfour\n\"five\"\nsix'", b"ends.\n", b"\r\nwin.\r\nlast.\r", b"\n\n", b"no newline."],
        "custom terminal": ([b"a;\nb:\nc.\nd;", b";", b"x\n;"], GOPHER, b";:"),
    }
    stop32 = [b"s%02d" % i for i in range(32)]
    out["stop words"] = ([b"them other The theatre the", b"abcdefghi abcdefgh0", b"abcdefgh", b"s31 s02 s30", b"s31", word(T - 9) + b" the " + word(20) + b" s07"],
                         [b"the", b"abcdefgh"] + stop32[2:], TERMINAL)
    for k in (-1, 0, 1):  # '.' at T + k - 1 with its '\n' behind it; a document that ends on '?' at 2T - 1; one that ends on '!' at 3T + k - 1
        out[f"terminal byte at tile edge {k:+d}"] = [word(T + k - 1) + b".\n" + word(T - k - 2) + b"?", word(T + k - 1) + b"!", b"y'", b"\n" + word(T - k - 5) + b":\n" + word(T - 1) + b"\""]
    chars = "\xe9\u4e2d\u03a9\u0663\U0001f600\u2026\U00010400\U00020000"  # letters of 2 and 3 bytes, a digit, a symbol of 4 bytes, the ellipsis, letters of 4
    # a word end, a document end, a dot run, white space and chars of two to four bytes ending at, one before and one after every kind of edge
    for name, edge in (("lane", lane), ("wave", wave), ("tile", T)):
        for k in (-1, 0, 1):
            e = edge + k
            out[f"word and document end at {name} edge {k:+d}"] = [word(e - 4) + b" the", b"of " + word(e - 3), word(5) + b" " + word(e - 9) + b" be", word(7)]
            out[f"dots at {name} edge {k:+d}"] = [b"".join(pad(word(e - r) + b"." * r, edge) for r in (3, 4, 5, 6, 7))]
            out[f"white space at {name} edge {k:+d}"] = [b"".join(pad(word(e - len(u(c))) + u(c) + b"w", edge) for c in "\xa0\u2028\u3000")]
            out[f"chars at {name} edge {k:+d}"] = [b"".join(pad(digits(e - len(u(c))) + u(c), edge) for c in chars), digits(e - 4) + u("\U0001f600"), digits(e - 2) + u("\xe9")]
    for k in (2, 3):  # chars, white space and the stop word with the tile edge inside them
        out[f"straddling tile edge +{k}"] = [b"".join(pad(digits(T + k - len(u(c))) + u(c), T) for c in "\u4e2d\U0001f600\u2026") +
                                             b"".join(pad(word(T + k - 3) + u(c) + b"w", T) for c in "\u3000\u2028") + pad(word(T + k - 6) + b" the", T) + pad(word(T - k) + b" the ", T)]
    long = digits(2 * T + 100)
    out["a word over three tiles"] = [word(9) + b" " + long[:T + 50] + b"q" + long[T + 51:] + b" " + word(3), long + b" of", long[:T] + u("\u0663") + long[T:], b"." * (2 * T + 2),
                                      b"a" + b"." * (2 * T + 3) + b"#"]
    return {k: v if isinstance(v, tuple) else (v, GOPHER, TERMINAL) for k, v in out.items()}
