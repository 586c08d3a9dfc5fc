"""The reference of the line sets (tk_line_set.h): re.finditer over each document and a Python set of bytes, documents in order.
Nothing from the code under test."""
import re

import numpy as np


def dedup(seen: set, docs, add=True, min_bytes=1):
    """(kept documents, n_lines, n_dropped); `seen` grows when `add`"""
    out, n_lines, n_dropped = [], [], []
    for doc in docs:
        kept, lines, dropped = [], 0, 0
        for piece in re.findall(rb"[^\n]+\n?|\n", bytes(doc)):
            line = piece.rstrip(b"\n")
            lines += bool(line)
            if line and len(line) >= min_bytes:
                if line in seen:
                    dropped += 1
                    continue
                if add:
                    seen.add(line)
            kept.append(piece)
        out.append(b"".join(kept)), n_lines.append(lines), n_dropped.append(dropped)
    return out, np.array(n_lines, np.uint64), np.array(n_dropped, np.uint64)
