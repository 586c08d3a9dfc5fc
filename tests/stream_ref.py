"""The streaming-decode rule of include/tiktoken_amd.h (tk_stream_create) as plain Python, written from the header's text and composed from
the three rules it names: the row rule (decode_rows_ref.rows_rule), the stop search (stop_text_ref.cut_doc) and the repair
(utf8_repair_ref.repair).  `Stream` is the step rule; `one_shot` is what tk_decode_rows_until makes of all the live columns a row was fed,
for the concatenation property.  Shared by the CPU simulation's and the GPU's tests."""
from __future__ import annotations

from typing import Callable

import numpy as np

import decode_rows_ref as D
import stop_text_ref as S
import utf8_repair_ref as U

LIVE, STOP_ID, STOP_TEXT, FLUSHED = 0, 1, 2, 3
REPLACE, IGNORE, BYTES = U.REPLACE, U.IGNORE, 2
HOLD = 66
NO_HIT = S.NO_HIT


def hold_from(B: bytes, stops) -> int:
    """e0: the least p such that B[p:] is a non-empty proper prefix of a stop string, or len(B)"""
    for p in range(max(len(B) - 63, 0), len(B)):
        if any(len(s) > len(B) - p and s.startswith(B[p:]) for s in stops):
            return p
    return len(B)


def unit_starts(B: bytes):
    """(the unit starts of B, e1): the units of the repair rule from offset 0; a lead that has accepted every byte up to the end of B, fewer
    than it declared, is unfinished: e1 = its offset, or len(B)"""
    starts, i, e1 = [], 0, len(B)
    while i < len(B):
        starts.append(i)
        b, took = B[i], 1
        L = U.declared(b)
        if L:
            while took < L and i + took < len(B):
                lo, hi = U.NARROW.get(b, (0x80, 0xBF)) if took == 1 else (0x80, 0xBF)
                if not lo <= B[i + took] <= hi:
                    break
                took += 1
            if took < L and i + took == len(B):
                e1 = i
        i += took
    starts.append(len(B))
    return starts, e1


def emit_end(B: bytes, stops, mode: int) -> int:
    e0 = hold_from(B, stops)
    if mode == BYTES:
        return e0
    starts, e1 = unit_starts(B)
    return max(s for s in starts if s <= min(e0, e1))


def repaired(piece: bytes, mode: int):
    """(text, chars) of an emitted piece, a whole document to the repair"""
    if mode == BYTES:
        return piece, 0
    text, chars, _ = U.repair(piece, mode)
    return text, chars


class Stream:
    """token_bytes(t): the bytes of id t, 0 <= t < 2^32, or None when it has no decode entry; special(t): it is a special token"""

    def __init__(self, n_rows: int, stops=(), *, token_bytes: Callable[[int], "bytes | None"], special: Callable[[int], bool] = lambda t: False, w_max: int = 1,
                 stop=(), skip=(), skip_special: bool = False, keep_stop: bool = False, keep_stop_text: bool = False, mode: int = REPLACE):
        if not 1 <= w_max <= 64:
            raise D.Refused("w_max")
        self.R, self.w_max, self.stops, self.mode, self.keep_text = n_rows, w_max, [bytes(s) for s in stops], mode, keep_stop_text
        self.token_bytes, self.special = token_bytes, special
        self.rule = dict(stop=list(stop), skip=list(skip), skip_special=skip_special, keep_stop=keep_stop)
        self.state, self.hit, self.tail = [LIVE] * n_rows, [NO_HIT] * n_rows, [b""] * n_rows
        self.n_kept, self.n_text, self.n_chars = [0] * n_rows, [0] * n_rows, [0] * n_rows
        self.fed = [[] for _ in range(n_rows)]  # the live columns every row was fed since its reset
        self.emitted = [b""] * n_rows  # ... and everything it emitted

    def _emit(self, r: int, piece: bytes) -> bytes:
        text, chars = repaired(piece, self.mode)
        self.n_text[r] += len(text)
        self.n_chars[r] += chars
        self.emitted[r] += text
        return text

    def step(self, ids: np.ndarray, begin=None, end=None) -> "list[bytes]":
        """what every row emits; D.Refused / D.InvalidToken (row and column of the step's matrix) leave the stream as it was"""
        R, W = ids.shape
        if R != self.R or W > self.w_max:
            raise D.Refused("shape")
        live = [r for r in range(R) if self.state[r] == LIVE]
        b = np.zeros(R, np.int64) if begin is None else np.asarray(begin, np.int64)
        e = np.full(R, W, np.int64) if end is None else np.asarray(end, np.int64)
        try:
            rows = D.rows_rule(ids[live] if live else ids[:0], b[live], e[live], valid=lambda t: self.token_bytes(t) is not None, special=self.special, **self.rule)
        except D.Refused as x:
            raise D.Refused(str(x), None if x.row is None else live[x.row]) from None
        except D.InvalidToken as x:
            raise D.InvalidToken(x.value, live[x.row], x.col) from None
        out = [b""] * R
        for i, r in enumerate(live):
            kept = rows.tokens[int(rows.tok_off[i]):int(rows.tok_off[i + 1])].tolist()
            found_stop = int(rows.stop_col[i]) < int(e[r])
            self.fed[r] += ids[r, int(b[r]):int(e[r])].tolist()
            self.n_kept[r] += len(kept)
            B = self.tail[r] + b"".join(self.token_bytes(t) for t in kept)
            cut, k = S.cut_doc(B, self.stops, self.keep_text)
            if k != NO_HIT:
                out[r], self.state[r], self.hit[r], self.tail[r] = self._emit(r, B[:cut]), STOP_TEXT, k, b""
            elif found_stop:
                out[r], self.state[r], self.tail[r] = self._emit(r, B), STOP_ID, b""
            else:
                at = emit_end(B, self.stops, self.mode)
                out[r], self.tail[r] = self._emit(r, B[:at]), B[at:]
                assert len(self.tail[r]) <= HOLD
        return out

    def _rows(self, rows):
        rows = range(self.R) if rows is None else [int(r) for r in rows]
        if any(not 0 <= r < self.R for r in rows):
            raise D.Refused("row")
        return rows

    def flush(self, rows=None) -> "list[bytes]":
        out = [b""] * self.R
        for r in set(self._rows(rows)):
            if self.state[r] == LIVE:
                out[r], self.state[r], self.tail[r] = self._emit(r, self.tail[r]), FLUSHED, b""
        return out

    def reset(self, rows=None) -> None:
        for r in self._rows(rows):
            self.state[r], self.hit[r], self.tail[r], self.fed[r], self.emitted[r] = LIVE, NO_HIT, b"", [], b""
            self.n_kept[r] = self.n_text[r] = self.n_chars[r] = 0

    def one_shot(self, r: int):
        """(text, hit) that tk_decode_rows_until returns for the row made of all the live columns row r was fed"""
        ids = np.array([self.fed[r]], np.int64).reshape(1, len(self.fed[r]))
        rows = D.rows_rule(ids, valid=lambda t: self.token_bytes(t) is not None, special=self.special, **self.rule)
        doc = b"".join(self.token_bytes(t) for t in rows.tokens.tolist())
        cut, k = S.cut_doc(doc, self.stops, self.keep_text)
        return repaired(doc[:cut], self.mode)[0], k


def chop(row_ids, widths):
    """row_ids cut into pieces of the given widths (the last one as long as what is left)"""
    out, at = [], 0
    for w in widths:
        if at >= len(row_ids):
            break
        out.append(row_ids[at:at + w])
        at += w
    return out


# ---------------------------------------------------------------- a small vocabulary: id == byte below 256, a few longer tokens, ids without a token, two specials
TOKENS = {256: b"\n\n", 257: b".\n\n", 258: b"Question:", 259: b" the", 260: "é".encode(), 261: "😀".encode(), 262: b"ab", 263: b"abc", 264: "中文".encode(), 265: b"x" * 40}
SPECIALS = {300: b"<|eot|>", 301: b"<|pad|>"}
HOLE, N_IDS, PAD = 280, 302, 100000


def token_bytes(t):
    if 0 <= t < 256:
        return bytes([t])
    return TOKENS.get(t, SPECIALS.get(t))


def stop_cases():
    """name -> (stop strings, the ids of one row, fed one per step): stop strings that arrive across steps"""
    long_stop = S.stop_of(64)
    return {
        "two ids in two steps": (["\n\n"], list(b"ab\n") + list(b"\ncd")),
        "one id": (["\n\n"], list(b"ab") + [256] + list(b"cd")),
        "the tail of a token": (["\n\n"], list(b"ab") + [257] + list(b"cd")),
        "64 bytes, a byte per step": ([long_stop], list(b"xy") + list(long_stop) + list(b"z")),
        "a prefix that breaks": (["\n\nQuestion:"], list(b"a\n\nQuest") + list(b"! more")),
        "ab and abc": (["ab", "abc"], list(b"xxabcxx")),
        "abc and ab": (["abc", "ab"], list(b"xxabcxx")),
        "the hit beats a lower, longer candidate": (["bc", "abcdef"], list(b"xabcdefy")),
        "a stop string inside a char's bytes": ([b"\x9f\x98"], list("a😀b".encode())),
    }
