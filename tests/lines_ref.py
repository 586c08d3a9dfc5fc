"""The reference of the line statistics (tk_lines.h): re.split, Counter, startswith / endswith and a count of non-continuation bytes per
document -- and the named batches of the GPU tests, built from the tile T, the lane width and the wavefront span.  Nothing from the code
under test."""
import re
from collections import Counter, namedtuple

import numpy as np

Ref = namedtuple("Ref", "n_chars n_lines n_dup_lines dup_line_chars n_paragraphs n_dup_paragraphs dup_paragraph_chars n_bullet_lines n_ellipsis_lines")


def chars(b: bytes) -> int:
    return sum((c & 0xC0) != 0x80 for c in b)


def dups(parts):
    count = Counter(parts)
    return len(parts), len(parts) - len(count), sum(chars(s) * (c - 1) for s, c in count.items())


def doc_stats(t: bytes):
    core = t.strip(b"\n")
    lines = re.split(rb"\n+", core) if core else []
    paragraphs = re.split(rb"\n{2,}", core) if core else []
    return (chars(t), *dups(lines), *dups(paragraphs), sum(s.startswith((b"-", b"*", "•".encode(), "●".encode())) for s in lines),
            sum(s.endswith((b"...", "…".encode())) for s in lines))


def stats(docs) -> Ref:
    rows = [doc_stats(bytes(t)) for t in docs]
    return Ref(*[np.array([r[i] for r in rows], np.uint64) for i in range(len(Ref._fields))])


def pack(docs):
    off = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.uint64)
    return np.frombuffer(b"".join(bytes(d) for d in docs), np.uint8), off


def batches(T: int, lane: int, wave: int):
    """{name: [documents as bytes]}; all but "long lines" together under 1 MiB"""
    rng = np.random.default_rng(T)
    word = lambda n: bytes(rng.integers(97, 123, n, dtype=np.uint8))  # noqa: E731  (n letters)
    out = {
        "no document": [],
        "empty and newlines": [b"", b"\n", b"", b"\n\n\n\n", b"", b"x", b""],
        "no newline, leading, trailing": [b"one line only", b"\n\nab\ncd", b"ab\ncd\n\n", b"\nab\n"],
        "a-nnn-b": [b"a\n\n\nb", b"a\nb\n\na\nb", b"a\nb\n\na\n\nb", b"ab\nc\n\na\nbc", b"a\n\nb\n\na\n\n\nb\na\n"],
        "equal length, prefix": [b"abcd\nabce\nabcd", b"abc\nabcd\nabc\nab\nabcd", b"\r\na\r\na\na\r"],
        "same line in two documents": [b"same line\nother", b"same line\nmore"],
        "bullets and ellipses": ["-\n...\n*\n•\n● x\n…\nwait...\nso…\n -\n.. .\n..\n.\n•".encode(), b"-", b"...", b"..", "…".encode(),
                                 b"\xe2\x80", b"\xe2\n\x80\xa2", b"- a\n- a\n- b..."],
        "20000 distinct": [b"\n".join(bytes([48 + i % 40, 48 + i // 40 % 40, 48 + i // 1600]) for i in range(20000))],
        "20000 equal": [b"abc\n" * 20000],
        "many one-line documents": [word(1 + i % 3) for i in range(3 * T // 2)] + [b"q\nq"] * 40,
        "one document over many tiles": [b"\n".join([word(37), word(T // 3)] * 9) + b"\n\n" + word(5)],
    }
    # a line (and a paragraph) ending exactly at, one before and one after an edge of a lane, a wavefront and a tile; the same for a document
    for name, edge in (("lane", lane), ("wave", wave), ("tile", T)):
        for k in (-1, 0, 1):
            out[f"line ends at {name} edge {k:+d}"] = [word(edge + k) + b"\n" + word(9) + b"\n\n" + word(edge + k - 11) + b"\n" + word(9)]
            out[f"document ends at {name} edge {k:+d}"] = [word(edge + k), word(7) + b"\n" + word(7), word(edge - 15), b"\n" + word(3) + b"\n"]
    # newline pairs and single newlines against a tile edge: the paragraph rule reads one byte beyond the tile on each side
    for k in (-2, -1, 0, 1):
        out[f"two newlines at tile edge {k:+d}"] = [word(T + k) + b"\n\n" + word(5) + b"\n" + word(T - 8 - k) + b"\n" + word(6)]
        w = word(T + k)  # three paragraphs: the second is the first with its inner newline one byte earlier, the third is the first again
        out[f"inner newline at tile edge {k:+d}"] = [w + b"\nxy\n\n" + w[:-1] + b"\n" + w[-1:] + b"xy\n\n" + w + b"\nxy"]
    # two-, three- and four-byte chars across lane and tile edges, in duplicated lines
    multi = "é€\U0001f600".encode()
    for k in range(1, 10):
        out[f"multibyte at tile edge -{k}"] = [word(T - k) + multi + b"\n" + multi * 3 + b"\n" + word(lane - k) + multi * 3 + b"\n" + multi * 3]
    for k in (1, 2):  # a bullet and an ellipsis char split by a tile edge; the bullet's line ends in the next tile
        out[f"bullet and ellipsis at tile edge -{k}"] = [word(T - k - 1) + b"\n" + "• x\n".encode() + word(T - 6) + "…".encode()]
    # one line over three tiles; an equal one that lies differently against the grid; one that differs by a byte in the middle tile
    long = word(2 * T + 100)
    other = bytearray(long)
    other[T + 50] ^= 1
    out["long lines"] = [word(T // 2 + 3) + b"\n" + long + b"\n" + word(lane + 1) + b"\n" + long + b"\n" + bytes(other) + b"\n\n" + long]
    return out
