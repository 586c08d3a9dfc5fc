"""The reference of the normalising line sets (tk_line_set.h, a `normalize` mask): the normal form of a line in Python, and
line_set_ref.dedup with the set keyed on it.  Nothing from the code under test."""
import re
import string

import numpy as np

CASE, DIGITS, SPACE, PUNCT, ALL = 1, 2, 4, 8, 15
LOWER = bytes.maketrans(string.ascii_uppercase.encode(), string.ascii_lowercase.encode())
ZEROS = bytes.maketrans(b"0123456789", b"0" * 10)


def normal_form(line: bytes, normalize: int) -> bytes:
    if normalize & PUNCT:
        line = line.translate(None, string.punctuation.encode())
    if normalize & CASE:
        line = line.translate(LOWER)
    if normalize & DIGITS:
        line = line.translate(ZEROS)
    if normalize & SPACE:
        line = b" ".join(line.split())  # (bytes.split: 0x09 .. 0x0D and 0x20; a line holds no 0x0A)
    return line


def dedup(seen: set, docs, add=True, min_bytes=1, normalize=0):
    """(kept documents, n_lines, n_dropped); `seen`, a set of normal forms, grows when `add`"""
    out, n_lines, n_dropped = [], [], []
    for doc in docs:
        kept, lines, dropped = [], 0, 0
        for piece in re.findall(rb"[^\n]+\n?|\n", bytes(doc)):
            line = piece.rstrip(b"\n")
            lines += bool(line)
            key = normal_form(line, normalize)
            if line and len(key) >= min_bytes:
                if key in seen:
                    dropped += 1
                    continue
                if add:
                    seen.add(key)
            kept.append(piece)
        out.append(b"".join(kept)), n_lines.append(lines), n_dropped.append(dropped)
    return out, np.array(n_lines, np.uint64), np.array(n_dropped, np.uint64)
