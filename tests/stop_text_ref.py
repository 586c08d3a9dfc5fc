"""The stop-string rule of include/tiktoken_amd.h (tk_stop_text_device) as plain Python, written from the header's text: a document is cut
at the least position where one of the stop strings lies entirely inside it, and among the strings that lie there the one listed first
hits.  Shared by the CPU simulation's and the GPU's tests, together with the inputs both use."""
import random

import numpy as np

from utf8_repair_ref import WIDE_FORCED, WIDE_N, WIDE_PREFIXES, draw, pooled_docs, spread  # noqa: F401  (the pooled batches' sizes and tools)
from utf8_repair_ref import pack  # noqa: F401  (bytes with 16 readable bytes of 0xA5 behind them, n, byte_off)

NO_HIT = 0xFFFFFFFF
KEEP = 1  # TK_STOPS_KEEP
BEHIND = 0xA5  # the byte `pack` leaves in the 16 readable bytes behind the text


def cut_doc(doc: bytes, stops, keep: bool):
    """(kept length, hit) of one document"""
    found = [(doc.find(s), k) for k, s in enumerate(stops)]
    found = [f for f in found if f[0] >= 0]
    if not found:
        return len(doc), NO_HIT
    p, k = min(found)
    return p + (len(stops[k]) if keep else 0), k


def cut_batch(docs, stops, keep: bool):
    """(text, text_off as a list of n + 1, hit as a list of n, documents with a hit)"""
    text, off, hit = bytearray(), [0], []
    for d in docs:
        kept, k = cut_doc(d, stops, keep)
        text += d[:kept]
        off.append(len(text))
        hit.append(k)
    return bytes(text), off, hit, sum(1 for k in hit if k != NO_HIT)


def n_tok_ref(token_lens, kept: int) -> int:
    """the tokens of a row, of these lengths, whose first byte lies before byte `kept` of the row"""
    at, n = 0, 0
    for length in token_lens:
        if at < kept:
            n += 1
        at += length
    return n


def stop_of(n: int, first: int = 0x53) -> bytes:
    """a stop string of n bytes that no filler holds: it starts with `first`, the rest counts up from 0xB0"""
    return bytes([first] + [0xB0 + j % 64 for j in range(1, n)])


LENGTHS = (1, 2, 15, 16, 17, 63, 64)


def cases(lane: int, wave: int, block: int):
    """The smallest shapes at which each part of the passes can go wrong, for workgroups of `block` bytes: a list of (name, docs, stops)."""
    out = []
    s4 = stop_of(4)
    for o in range(16):  # a match starting at each of a lane's 16 offsets
        out.append((f"lane offset {o}", [b"x" * (2 * lane + o) + s4 + b"yy"], [s4]))
    for edge, what in ((lane, "lane"), (wave, "wave"), (block, "block")):
        for n in (2, 17, 64):
            s = stop_of(n)
            for start in sorted({edge - 1, edge - n + 1, edge - n // 2, edge - n, edge}):
                if start >= 0:
                    out.append((f"{what} edge, {n} bytes from {start}", [b"x" * start + s + b"tail"], [s]))
    for n in LENGTHS:
        s = stop_of(n)
        out.append((f"length {n}", [b"abcde" + s + b"z", b"x" * (block - 3) + s, b"none"], [s]))
        out.append((f"length {n} ends its document", [b"x" * 10 + s, b"next"], [s]))
        if n > 1:
            out.append((f"length {n}, a byte short, the next document has it", [b"x" * 10 + s[:-1], s[-1:] + b"zz"], [s]))
    for missing in (1, 2, 15):  # the missing bytes sit in the readable bytes behind the text
        s = b"ST" + bytes([BEHIND]) * missing
        out.append((f"{missing} bytes short at the text's end", [b"ok", b"x" * 10 + b"ST"], [s]))
        out.append((f"{missing} bytes short at the text's end, at a block's end", [b"x" * (block - 2) + b"ST"], [s]))
    out.append(("a boundary inside a lane, a match on each side", [b"ab" + s4, s4 + b"cd", b"e" + s4], [s4]))
    out.append(("a boundary inside a match", [b"abc" + s4[:2], s4[2:] + b"cd" + s4], [s4]))
    for k in (1, 2, 70):
        e = [b""] * k
        out.append((f"runs of {k} empty documents", e + [b"xx" + s4 + b"y"] + e + [b"q" * 40 + s4] + e + [s4] + e + [b"none"] + e, [s4]))
        out.append((f"only {k} empty documents", e, [s4]))
    out.append(("no documents", [], [s4]))
    out.append(("an empty stop set", [b"abc" + s4, b"", b"def"], []))
    out.append(("no documents, no strings", [], []))
    out.append(("ab before abc", [b"xxabcxx", b"abc", b"xab"], [b"ab", b"abc"]))
    out.append(("abc before ab", [b"xxabcxx", b"abc", b"xab"], [b"abc", b"ab"]))
    a, b = stop_of(5, 0x41), stop_of(7, 0x42)
    out.append(("position before list order", [b"xx" + b + b"yy" + a, a + b, b + a, b"x" * (block - 2) + b + a], [a, b]))
    one_first = [b"q" + bytes([0xC0 + i]) * (i % 5 + 1) for i in range(16)]
    out.append(("sixteen strings with one first byte", [b"qq" + one_first[13] + b"x", b"q" * 30, b"zq" + one_first[15] + one_first[0], one_first[4][:-1] + b"q"], one_first))
    many_first = [bytes([0x61 + i]) + b"#" * (i % 3) for i in range(16)]
    out.append(("sixteen strings with sixteen first bytes", [b"ZZZ" + many_first[9] + b"Z", b"Z" * 50, b"Zp#Zc##", b"YYp"], many_first))
    out.append(("one-byte stops 00 80 FF", [b"ab\x00cd", b"\x7f\x81\x80", b"\xfe\xff", b"plain", b"\xff\x00\x80"], [b"\x00", b"\x80", b"\xff"]))
    s9 = stop_of(9)
    long_doc = b"x" * (3 * block + 100)
    last = long_doc[: 3 * block + 40] + s9 + b"end"
    out.append(("a document over three blocks, a hit in the last", [b"ab", last, b"cd"], [s9]))
    every = bytearray(long_doc)
    for at in (block - 500, 2 * block - 4, 3 * block + 7):
        every[at:at + 9] = s9
    out.append(("a document over three blocks, hits in all", [b"ab", bytes(every), s9], [s9]))
    out.append(("64 KiB of a, stop aa", [b"a" * 40000, b"a" * 20000, b"a", b"a" * 5535], [b"aa"]))
    out.append(("no hit anywhere", [b"The quick brown fox. " * 300, b"", "中文😀é".encode() * 50], [b"\n\n", b"Question:", b"</s>", b"###"]))
    return out


def random_cases(seed: int, count: int):
    """documents over a small alphabet, so that stop strings drawn from it match often, overlap and tie"""
    rng = random.Random(seed)
    out = []
    for i in range(count):
        alphabet = bytes(rng.sample(range(256), rng.choice([2, 3, 5])))
        stops = []
        for _ in range(rng.choice([1, 2, 4, 16])):
            stops.append(bytes(rng.choice(alphabet) for _ in range(rng.choice([1, 2, 3, 5, 17, 64]))))
        docs = [bytes(rng.choice(alphabet) for _ in range(rng.choice([0, 1, 7, 40, 300, 5000]))) for _ in range(rng.choice([1, 3, 12]))]
        out.append((f"random {i}", docs, stops))
    return out


# ---------------------------------------------------------------- pooled batches (utf8_repair_ref.py: WIDE_N documents from a small pool)
WIDE_STOPS = [b"<END>", b"##", b"<EN"]  # where <END> lies, <EN lies too: the list's order decides there
NO_STOPS = [b"\n\n", b"<ENX", b"#!"]  # strings that lie nowhere in the pool's documents; two of them start like ones that do
WIDE_POOL = [
    # no hit: empty, plain, and the halves of stop strings -- a proper prefix at the end, the rest at the start: neighbours form a match
    # across their boundary, which is none
    b"", b"", b"a", b"plain text", b"twelve bytes", "中文".encode(), b"xy<E", b"ND>zz", b"ab#", b"#cd", b"q<", b"EN", b"D>", b"<E#N>",
    # a hit at byte 0, in the middle, at the end; the document that is the stop string
    b"<END>tail", b"ab<END>cd", b"abc<END>", b"##", b"x##y", "中##".encode(), b"0123456789##",
    # two strings at different places (the position decides), one string alone where the other is cut short
    b"a##b<END>", b"<END>##", b"<EN##", b"x<ENx", b"#<EN", b"z<END",
]


def wide_batch():
    """(pool, idx): WIDE_N documents; those of WIDE_FORCED have a hit behind their first byte and before their last, with either `keep`"""
    mid = [i for i, p in enumerate(WIDE_POOL) if 1 <= cut_doc(p, WIDE_STOPS, False)[0] and cut_doc(p, WIDE_STOPS, True)[0] < len(p)]
    return WIDE_POOL, draw(len(WIDE_POOL), mid, 0x570D)


def pooled_cut(pool, idx, stops, keep: bool):
    """`cut_batch` of the documents pool[idx], the rule run once per pool entry: (text uint8[...], text_off uint64[n + 1], hit uint32[n])"""
    per = [cut_doc(p, stops, keep) for p in pool]
    text, text_off = spread([p[:kept] for p, (kept, _) in zip(pool, per)], idx)
    return text, text_off, np.array([k for _, k in per], np.uint32)[idx]


def crosses(a: bytes, b: bytes, stops) -> bool:
    """a stop string lies in a + b across the boundary between the two"""
    return any((a + b)[p:p + len(s)] == s for s in stops for p in range(max(len(a) - len(s) + 1, 0), len(a)) if p + len(s) > len(a))


def stop_arrays(stops):
    """(blob uint8, off uint32[n + 1]) as tk_stops takes them"""
    blob = np.frombuffer(b"".join(stops) + b"\0", np.uint8)
    off = np.zeros(len(stops) + 1, np.uint32)
    if stops:
        off[1:] = np.cumsum([len(s) for s in stops])
    return blob, off
