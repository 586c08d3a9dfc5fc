"""Decoding id matrices: the rule of tk_decode_rows_device as plain Python loops, written from its description in include/tiktoken_amd.h,
not from the kernels.  The CPU simulation (test_decode_rows_sim.py) and the GPU tests (test_gpu_decode_rows.py) are compared with it."""
from __future__ import annotations

from typing import Callable, Iterable, NamedTuple

import numpy as np

KEEP_STOP, SKIP_SPECIAL, I32, I64 = 1, 2, 4, 8
DTYPES = (np.uint32, np.int32, np.int64)
FLAG_OF = {np.dtype(np.uint32): 0, np.dtype(np.int32): I32, np.dtype(np.int64): I64}


class Rows(NamedTuple):
    tokens: np.ndarray  # uint32[K]
    tok_off: np.ndarray  # uint64[R + 1]
    n_kept: np.ndarray  # uint32[R]
    stop_col: np.ndarray  # uint32[R]


class Refused(ValueError):
    """TK_VALUE_ERROR; .row is the first row whose begin / end offend, or None for a refusal of the spec or the figures"""

    def __init__(self, why: str, row: int | None = None):
        super().__init__(why)
        self.row = row


class InvalidToken(KeyError):
    """TK_KEY_ERROR: the first kept element, in row-major order, without a decode entry"""

    def __init__(self, value: int, row: int, col: int):
        super().__init__(f"Invalid token for decoding: {value} (row {row}, column {col})")
        self.value, self.row, self.col = value, row, col


def rows_rule(ids: np.ndarray, begin=None, end=None, stop: Iterable[int] = (), skip: Iterable[int] = (), *, skip_special: bool = False, keep_stop: bool = False,
              valid: Callable[[int], bool] = lambda t: True, special: Callable[[int], bool] = lambda t: False) -> Rows:
    """ids: a 2-D array of one of DTYPES (any strides: only its elements count).  valid(t) / special(t): id t, 0 <= t < 2^32, has a decode
    entry / is a special token."""
    stop, skip = list(stop), list(skip)
    if len(stop) > 16 or len(skip) > 16:
        raise Refused("more than 16 ids in a list")
    R, W = ids.shape
    if R >= 2**32 - 1 or W >= 2**32:
        raise Refused("too many rows or columns")
    b = [0] * R if begin is None else [int(x) for x in begin]
    e = [W] * R if end is None else [int(x) for x in end]
    for r in range(R):  # before anything else is looked at
        if b[r] > e[r] or e[r] > W:
            raise Refused("begin <= end <= W", r)
    tokens, tok_off, n_kept, stop_col = [], [0], [], []
    for r in range(R):
        row = ids[r].tolist()  # (Python ints: the loops below are the rule, this is only quicker than indexing the array)
        s = e[r]
        for c in range(b[r], e[r]):
            if row[c] in stop:  # (a negative element, or one of 2^32 and more, is in no list: the lists hold uint32)
                s = c
                break
        live_end = s + 1 if keep_stop and s < e[r] else s
        for c in range(b[r], live_end):
            t = row[c]
            if t in skip:
                continue
            in_range = 0 <= t < 2**32
            if skip_special and in_range and valid(t) and special(t):
                continue
            if not in_range or not valid(t):
                raise InvalidToken(t, r, c)
            tokens.append(t)
        stop_col.append(s)
        n_kept.append(len(tokens) - tok_off[-1])
        tok_off.append(len(tokens))
    if len(tokens) >= 2**32:
        raise Refused("K >= 2^32")
    return Rows(np.array(tokens, np.uint32), np.array(tok_off, np.uint64), np.array(n_kept, np.uint32), np.array(stop_col, np.uint32))


def same(got: Rows, want: Rows, ctx=None) -> None:
    for name, g, w in zip(Rows._fields, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (name, ctx, g[:20], w[:20])


def held(values: np.ndarray, dtype, ld_extra: int = 0, shift: int = 0) -> np.ndarray:
    """`values` [R, W] as a matrix of `dtype` that is a column slice of a wider one: rows ld = W + ld_extra elements apart, element (0, 0)
    `shift` elements behind the start of the allocation, garbage around the slice.  Returns the 2-D view."""
    R, W = values.shape
    ld = W + ld_extra
    room = np.full(shift + (R * ld if R else 0) + 8, -7 if np.dtype(dtype).kind == "i" else 0xFFFFFFF9, dtype)
    view = np.lib.stride_tricks.as_strided(room[shift:], shape=(R, W), strides=(ld * room.itemsize, room.itemsize), writeable=True)
    view[...] = values.astype(dtype)
    return view


def generation_matrix(rng, R: int, W: int, vocab: int, stops=(), pad: int = 0, p_stop: float = 0.7, specials=()):
    """A matrix shaped like a generation loop's result: ids below `vocab` (now and then one of `specials`), in most rows one stop id at a
    random column with `pad` behind it.  int64 values; begin per row."""
    m = rng.integers(0, vocab, size=(R, W)).astype(np.int64)
    if len(specials) and W:
        hit = rng.random((R, W)) < 0.05
        m[hit] = rng.choice(np.array(specials, np.int64), size=int(hit.sum()))
    begin = rng.integers(0, max(W // 3, 1), size=R).astype(np.uint32) if W else np.zeros(R, np.uint32)
    if len(stops) and W:
        for r in range(R):
            if rng.random() < p_stop:
                c = int(rng.integers(0, W))
                m[r, c] = stops[int(rng.integers(0, len(stops)))]
                m[r, c + 1:] = pad
    return m, begin
