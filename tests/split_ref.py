"""The text-chunk rule (include/tiktoken_amd.h, tk_split_device) as a plain loop per document over `bytes`, written from the rule's text and
not from the kernels.  A document is its bytes and the byte lengths of its tokens; separators are levels of (tail, head) pairs."""
from typing import NamedTuple

import numpy as np

HARD, FORCED, END = 0xFD, 0xFE, 0xFF
DEFAULT = [[(b"\n\n", b"")], [(b"\n", b"")], [(b".", b" "), (b"?", b" "), (b"!", b" ")], [(b"", b" ")]]


class Chunks(NamedTuple):
    doc: np.ndarray
    tok_begin: np.ndarray
    tok_end: np.ndarray
    byte_begin: np.ndarray
    byte_end: np.ndarray
    char_begin: np.ndarray
    char_end: np.ndarray
    cut: np.ndarray
    doc_chunk: np.ndarray


def is_cont(b: int) -> bool:
    return 0x80 <= b <= 0xBF


def spans(text: bytes, lens):
    """byte_start and char_start of every token of one document, with the document's totals behind them (the span rule: the chars before
    a token are the bytes outside 0x80..0xBF before it, less one when its first byte is a continuation byte, never below 0)"""
    byte_start, char_start, p, chars = [], [], 0, 0
    for n in lens:
        byte_start.append(p)
        char_start.append(max(chars - 1, 0) if is_cont(text[p]) else chars)
        chars += sum(1 for b in text[p:p + n] if not is_cont(b))
        p += n
    assert p == len(text), "the tokens do not add up to the text"
    return byte_start + [p], char_start + [chars]


def boundary(text: bytes, p: int, levels):
    """(legal, level or None) of the boundary at byte p, 0 < p < len(text)"""
    if is_cont(text[p]):
        return False, None
    for lv, seps in enumerate(levels):
        for tail, head in seps:
            if len(tail) <= p and text[p - len(tail):p] == tail and text[p:p + len(head)] == head and len(head) <= len(text) - p:
                return True, lv
    return True, None


def chain(text: bytes, lens, N: int, M: int, O: int, levels):
    """[(s, e, cut)] of one document"""
    n = len(lens)
    if n == 0:
        return []
    bs, _ = spans(text, lens)
    cls = [None] + [boundary(text, bs[i], levels) for i in range(1, n)]
    out, s = [], 0
    while True:
        if n - s <= N:
            out.append((s, n, END))
            return out
        best = None  # (level, e): the lowest level, of it the largest e
        last_legal = None
        for e in range(s + M, s + N + 1):
            legal, lv = cls[e]
            if not legal:
                continue
            last_legal = e
            if lv is not None and (best is None or lv <= best[0]):
                best = (lv, e)
        if best is not None:
            e, cut = best[1], best[0]
        elif last_legal is not None:
            e, cut = last_legal, HARD
        else:
            e, cut = s + N, FORCED
        out.append((s, e, cut))
        nxt = e
        for q in range(e - O, e + 1):
            if cls[q][0]:
                nxt = q
                break
        assert nxt > s
        s = nxt


def norm_levels(separators):
    """levels of (tail, head) byte pairs; a bare str / bytes means (x, b"")"""
    def part(x):
        return x.encode("utf-8") if isinstance(x, str) else bytes(x)
    out = []
    for seps in separators:
        lv = []
        for sp in seps:
            lv.append((part(sp), b"") if isinstance(sp, (str, bytes)) else (part(sp[0]), part(sp[1])))
        out.append(lv)
    return out


def split_rule(docs, doc_lens, N: int, M: int, O: int = 0, separators=DEFAULT) -> Chunks:
    """docs: the documents' bytes; doc_lens: per document the byte lengths of its tokens"""
    levels = norm_levels(separators)
    cols = [[] for _ in range(8)]
    doc_chunk = [0]
    for d, (text, lens) in enumerate(zip(docs, doc_lens)):
        lens = [int(x) for x in lens]
        if lens:
            bs, cs = spans(text, lens)
            for s, e, cut in chain(text, lens, N, M, O, levels):
                for col, v in zip(cols, (d, s, e, bs[s], bs[e], cs[s], cs[e], cut)):
                    col.append(v)
        else:
            assert len(text) == 0
        doc_chunk.append(len(cols[0]))
    arrs = [np.array(c, np.uint32) for c in cols[:7]] + [np.array(cols[7], np.uint8)]
    return Chunks(*arrs, np.array(doc_chunk, np.uint32))


def same(got, want, what=""):
    for name in Chunks._fields:
        g, w = np.asarray(getattr(got, name)), getattr(want, name)
        assert g.shape == w.shape, (name, g.shape, w.shape, what)
        if not np.array_equal(g, w):
            i = int(np.flatnonzero(g != w)[0])
            raise AssertionError((name, i, g[max(i - 2, 0):i + 3].tolist(), w[max(i - 2, 0):i + 3].tolist(), what))


def token_lens(enc, tokens, tok_off):
    """per document the byte lengths of its tokens, from the encoding's own decoder"""
    cache = {}
    out = []
    for d in range(len(tok_off) - 1):
        row = []
        for t in tokens[int(tok_off[d]):int(tok_off[d + 1])]:
            t = int(t)
            if t not in cache:
                cache[t] = len(enc.decode_single_token_bytes(t))
            row.append(cache[t])
        out.append(row)
    return out
