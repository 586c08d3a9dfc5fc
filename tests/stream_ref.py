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
STOP64 = S.stop_of(64, first=0x80)  # a stop string of the greatest length that starts with a continuation byte: a lead in front of it takes it
TOKENS = {256: b"\n\n", 257: b".\n\n", 258: b"Question:", 259: b" the", 260: "é".encode(), 261: "😀".encode(), 262: b"ab", 263: b"abc", 264: "中文".encode(), 265: b"x" * 40,
          266: b"\x80" * 40, 267: b"\xf0\x9f\x98", 268: STOP64[:30]}
X40, BAD40, LEAD3, HALF_STOP = 265, 266, 267, 268
ROW_LDS = 16000  # TK_STREAM_ROW_LDS: a row's buffer, HOLD + w_max * (the longest token), is at most this
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


# ---------------------------------------------------------------- steps as wide as the row's wavefront
EDGES = (0, 31, 32, 33, 63, 64)  # begin and end on both sides of the wavefront's halves


def full_width_steps():
    """(the stream's arguments, steps): nine rows, no two alike, fed steps of 64, 63, 33, 32 and 64 columns -- begin and end per row at
    every one of EDGES, stop ids at columns 31, 32 and 63 (and outside a row's range, where they do not count), skipped ids and a skipped
    special all over both halves, a stop string across columns 31 / 32; HOLE where a row has ended: such ids are not judged."""
    rng = np.random.default_rng(0xF011)
    alphabet = [32, 46, 97, 98, 99, 100, 101, 0xC3, 0xA9, 0xE4, 0x98, 0xF0, 259, 260, 261, 262, 263, 264, X40, 7, 7, PAD, PAD, 301]

    def ids(W, dead=()):
        m = rng.choice(alphabet, size=(9, W)).astype(np.int64)
        m[list(dead)] = HOLE
        return m

    s1 = ids(64)
    s1[0, 63] = s1[6, 40] = s1[1, 5] = 300  # (row 6 ends at 31, row 1 begins at 31: only row 0's counts)
    s2 = ids(63, dead=[0])
    s2[1, 31] = s2[2, 32] = 300
    s3 = ids(33, dead=[0, 1, 2])
    s3[8, 31] = s3[8, 32] = 10
    s4 = ids(32, dead=[0, 1, 2, 8])
    s5 = ids(64, dead=[0, 1, 2, 8])
    s5[3, 32], s5[4, 63], s5[5, 31] = 300, 300, 300
    steps = [(s1, [0, 31, 32, 33, 63, 64, 0, 0, 0], [64, 64, 64, 64, 64, 64, 31, 32, 33]), (s2, [0, 0, 0, 31, 32, 33, 62, 63, 0], [63] * 9),
             (s3, None, [0, 0, 0, 0, 31, 32, 33, 33, 33]), (s4, [0, 0, 0, 31, 32, 0, 0, 0, 0], None), (s5, None, None)]
    return dict(stops=[b"\n\n"], stop=[300], skip=[PAD, 7], skip_special=True, w_max=64), steps


def coverage(ref: Stream, steps):
    """what the steps reach, by the rule alone (ref: a fresh Stream, fed here): the begins and ends of rows that were live, the columns of
    the stop ids that ended a row, the halves of the wavefront in which a skipped id was passed over, the states at the end"""
    begins, ends, stop_cols, skipped = set(), set(), set(), set()
    for ids, begin, end in steps:
        ids = np.asarray(ids, np.int64)
        W = ids.shape[1]
        for r in range(ref.R):
            if ref.state[r] != LIVE:
                continue
            b, e = (0 if begin is None else int(begin[r])), (W if end is None else int(end[r]))
            begins.add(b), ends.add(e)
            row = ids[r].tolist()
            s = next((c for c in range(b, e) if row[c] in ref.rule["stop"]), e)
            if s < e:
                stop_cols.add(s)
            skipped |= {c >= 32 for c in range(b, s) if row[c] in ref.rule["skip"] or (ref.rule["skip_special"] and ref.special(row[c]))}
        ref.step(ids, begin, end)
    return dict(begins=begins, ends=ends, stop_cols=stop_cols, skipped=skipped, state=list(ref.state))


# ---------------------------------------------------------------- more than 1024 bytes emitted by one row in one call
def straddles(piece: bytes, at: int) -> bool:
    """a well-formed char of several bytes lies on both sides of byte offset `at` of `piece`"""
    starts, _ = unit_starts(piece)
    return any(a < at < b for a, b in zip(starts[:-1], starts[1:]))


def long_emit_steps():
    """(stop strings, steps) for five rows.  Step 2 is 64 columns of mostly the 40-byte tokens: over 2048 bytes a row, three turns of the
    emit loop -- ASCII with short tokens between the long ones (so that a turn written to the wrong place shows), the same behind a held
    byte, 2560 bytes of 0x80, and two rows of chars of 2, 3 and 4 bytes of which one lies across byte 1024 and one across byte 2048.  Step 3:
    rows 0 and 1 end by a stop id behind 1024 bytes whose last is an unfinished lead, and behind 1025 with the lead's first continuation;
    the others take an unfinished lead into their tails, which the flush emits."""
    x, cjk, e2, smile = X40, 264, 260, 261
    ascii_row = [x] * 64
    for c, t in ((5, 258), (26, 259), (27, 46), (40, 263), (52, 262), (63, 97)):
        ascii_row[c] = t

    def chars(lead):  # the chars across 1024 and 2048 for a lead of 1 or 2 bytes
        return [lead] + [x] * 25 + [cjk, cjk, smile, e2, cjk] + [x] * 25 + [cjk, cjk, e2, cjk, smile] + [e2, cjk, x]

    s1 = np.array([[0], [10], [0], [0], [0]], np.int64)
    s2 = np.array([ascii_row, [x] * 64, [BAD40] * 64, chars(97), chars(262)], np.int64)
    assert s2.shape == (5, 64)
    head = [x] * 25 + [258, 259, 259, 259, 262, 0xF0]  # 1024 bytes, the last a lead
    s3 = np.full((5, 64), HOLE, np.int64)
    s3[0, :32], s3[1, :33] = head + [300], head + [0x9F, 300]
    s3[2, 0], s3[3, :2] = 0xF0, [10, 0xE4]
    s3[4] = [e2, smile] * 32
    s3[4, 63] = 0xF0
    return [b"\n\n"], [(s1, None, [0, 1, 0, 0, 0]), (s2, None, None), (s3, None, [32, 33, 1, 2, 64])]


# ---------------------------------------------------------------- tails at the most a row holds back
def hold_cases():
    """name -> (ids fed one per step unless they are a tuple: a step of several, the longest tail the row holds unless it holds bytes
    only, it ends by the stop string): STOP64 behind an unfinished lead whose next byte it may be.  F0 takes 90 .. BF only, so it is a unit
    of its own in front of STOP64's 80 and the row holds the 63 bytes alone; F1 takes it, which gives the 64."""
    out = {}
    for lead, held in ((b"\xf0", 63), (b"\xf1", 64), (b"\xf0\x9f", 65), (b"\xf0\x9f\x98", 66)):
        for last, hit in ((STOP64[63], True), (0x41, False)):
            out[f"{lead.hex()} then a byte per step, {'hit' if hit else 'broken'}"] = (list(b"ab") + list(lead) + list(STOP64[:63]) + [last, 0x42], held, hit)
    for last, hit in ((STOP64[63], True), (0x41, False)):
        what = "hit" if hit else "broken"
        out[f"a lead and 30 bytes in one step, {what}"] = ([98, (LEAD3, HALF_STOP)] + list(STOP64[30:63]) + [last, 0x42], 66, hit)
        out[f"30 bytes in one token behind f09f, {what}"] = ([0xF0, 0x9F, HALF_STOP, tuple(STOP64[30:62])] + [STOP64[62], last, 0x42], 65, hit)
    return out


def hold_steps(ids):
    return [(np.array([list(t) if isinstance(t, tuple) else [t]], np.int64), None, None) for t in ids]
