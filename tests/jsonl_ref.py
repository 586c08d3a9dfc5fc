"""The JSON Lines rule (include/tiktoken_amd.h, tiktoken_amd/csrc/tk_jsonl_rule.h) restated in Python as a byte scanner: one loop over the
bytes of every line, written from the rule's description and not on top of `json`.  What the CPU simulation and the GPU are compared with."""
from typing import NamedTuple

import numpy as np

OK, BLANK, MISSING, NOT_STRING, BAD = range(5)
RAISE, SKIP, EMPTY = range(3)
MODES = {"raise": RAISE, "skip": SKIP, "empty": EMPTY}
WS = b" \t\r"
SIMPLE = {ord('"'): 0x22, ord("\\"): 0x5C, ord("/"): 0x2F, ord("b"): 8, ord("f"): 12, ord("n"): 10, ord("r"): 13, ord("t"): 9}


def lines_of(buf: bytes):
    """(start, end) of every line, the newline excluded; a buffer that ends with a newline has no empty line behind it"""
    out, a = [], 0
    while a < len(buf):
        b = buf.find(b"\n", a)
        if b < 0:
            b = len(buf)
        out.append((a, b))
        a = b + 1
    return out


def _hex4(b: bytes, i: int) -> int:
    h = b[i:i + 4]
    if len(h) < 4 or any(c not in b"0123456789abcdefABCDEF" for c in h):
        return -1
    return int(h, 16)


def unescape(v: bytes):
    """the bytes between a value's quotes -> its text, or None: a bad escape or ill-formed UTF-8"""
    out, i = bytearray(), 0
    while i < len(v):
        c = v[i]
        if c != 0x5C:
            out.append(c)
            i += 1
            continue
        n = v[i + 1] if i + 1 < len(v) else -1
        if n in SIMPLE:
            out.append(SIMPLE[n])
            i += 2
            continue
        if n != ord("u"):
            return None
        cp = _hex4(v, i + 2)
        if cp < 0:
            return None
        i += 6
        if 0xD800 <= cp < 0xDC00:
            lo = _hex4(v, i + 2) if v[i:i + 2] == b"\\u" else -1
            if 0xDC00 <= lo < 0xE000:
                cp = 0x10000 + ((cp - 0xD800) << 10) + (lo - 0xDC00)
                i += 6
            else:
                cp = 0xFFFD
        elif 0xDC00 <= cp < 0xE000:
            cp = 0xFFFD
        out += chr(cp).encode("utf-8")
    # raw bytes and escapes' outputs never join into a char, so checking the whole is checking the raw stretches
    try:
        bytes(out).decode("utf-8")
    except UnicodeDecodeError:
        return None
    return bytes(out)


def scan_line(line: bytes, field: bytes, bom: int = 0):
    """(status, text) of one line (without its newline); bom: leading bytes that count as whitespace"""
    run = depth = low = 0
    instr = False
    first = None
    bad = False
    best = None  # (is a string, position of the value's first byte)
    for i, c in enumerate(line):
        escaped = run & 1
        run = run + 1 if c == 0x5C else 0
        if first is None and i >= bom and c not in WS:
            first = c
        if c == 0x22 and not escaped:
            if not instr and depth == 1:  # a string opens at depth 1: a key?
                q = i + 1 + len(field)
                if line[i + 1:q] == field and line[q:q + 1] == b'"':
                    q += 1
                    while q < len(line) and line[q] in WS:
                        q += 1
                    if line[q:q + 1] == b":":
                        q += 1
                        while q < len(line) and line[q] in WS:
                            q += 1
                        best = (line[q:q + 1] == b'"', q)
            instr = not instr
        elif instr:
            if c < 0x20:
                bad = True
        elif c in b"{[":
            depth += 1
            low += depth <= 0
        elif c in b"}]":
            depth -= 1
            low += depth <= 0
    if first is None:
        return BLANK, None
    if bad or first != 0x7B or instr or depth != 0 or low != 1:
        return BAD, None
    if best is None:
        return MISSING, None
    if not best[0]:
        return NOT_STRING, None
    # the value: from behind its opening quote to the next unescaped quote
    a = best[1] + 1
    b, run = a, 0
    while not (line[b] == 0x22 and not run & 1):  # (no string is open at the line's end: there is one)
        run = run + 1 if line[b] == 0x5C else 0
        b += 1
    text = unescape(line[a:b])
    return (BAD, None) if text is None else (OK, text)


class Extract(NamedTuple):
    text: np.ndarray
    doc_off: np.ndarray
    line: np.ndarray
    line_off: np.ndarray
    status: np.ndarray
    bad: "tuple | None"  # RAISE: (line, pos, status) of the first line refused; nothing else is given then

    def texts(self):
        return [self.text[int(a):int(b)].tobytes() for a, b in zip(self.doc_off[:-1], self.doc_off[1:])]


def extract(buf: bytes, field: bytes = b"text", mode: int = RAISE) -> Extract:
    buf = bytes(buf)
    spans = lines_of(buf)
    bom = 3 if buf[:3] == b"\xef\xbb\xbf" else 0
    status, docs, line = [], [], []
    for k, (a, b) in enumerate(spans):
        st, text = scan_line(buf[a:b], field, bom if k == 0 else 0)
        status.append(st)
        if mode == RAISE and st not in (OK, BLANK):
            return Extract(None, None, None, None, None, (k, a, st))
        if st == OK or (mode == EMPTY and st != BLANK):
            docs.append(text if st == OK else b"")
            line.append(k)
    doc_off = np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64)
    return Extract(np.frombuffer(b"".join(docs), np.uint8), doc_off, np.array(line, np.uint64), np.array([a for a, _ in spans] + [len(buf)], np.uint64),
                   np.array(status, np.uint8), None)
