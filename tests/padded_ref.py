"""The rule of the padded model inputs (include/tiktoken_amd.h, tk_pad_batch_device) restated in numpy from its description -- not from the
kernels: what tests/test_padded_sim.py and tests/test_gpu_padded.py compare the CPU simulation and the device with."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from rows_ref import SPECIALS, pack_docs  # noqa: F401  (the same four bos / eos combinations, the same packing)

NONE = 0xFFFFFFFF


class Padded(NamedTuple):
    ids: np.ndarray  # uint32[R, W]
    mask: np.ndarray  # uint8[R, W]
    len: np.ndarray  # uint32[R]
    row_doc: np.ndarray
    row_tok: np.ndarray
    doc_row: np.ndarray  # uint32[n_docs + 1]


class Refused(ValueError):
    pass


def padded_rule(tokens, tok_off, max_len: int, *, stride: int = 0, width_multiple: int = 0, bos=None, eos=None, pad: int = 0, windows: bool = False,
                keep_tail: bool = False, left: bool = False) -> Padded:
    tokens = np.asarray(tokens, dtype=np.uint32)
    off = [int(x) for x in tok_off]
    n_docs = len(off) - 1
    k = (bos is not None) + (eos is not None)
    c = max_len - k
    if max_len == 0 or c <= 0:
        raise Refused("max_len")
    if stride >= c:
        raise Refused("stride >= c")
    if stride and not windows:
        raise Refused("stride without windows")
    if keep_tail and windows:
        raise Refused("keep_tail with windows")
    if off[0] != 0 or off[-1] != len(tokens) or any(a > b for a, b in zip(off, off[1:])):
        raise Refused("tok_off")
    row_doc, row_tok, row_end, doc_row = [], [], [], []
    for d in range(n_docs):  # the body ranges [a, b) of every document's rows
        n = off[d + 1] - off[d]
        doc_row.append(len(row_doc))
        if windows and n > c:
            step = c - stride
            w = 1 + -(-(n - c) // step)
            ranges = [(j * step, min(j * step + c, n)) for j in range(w)]
            assert ranges[-1][1] == n and (w < 2 or ranges[-2][1] < n)  # the last window, and only it, reaches the document's end
        elif keep_tail:
            ranges = [(max(n - c, 0), n)]
        else:
            ranges = [(0, min(n, c))]
        for a, b in ranges:
            row_doc.append(d)
            row_tok.append(a)
            row_end.append(b)
    doc_row.append(len(row_doc))
    R = len(row_doc)
    i64 = np.int64
    row_doc, row_tok, row_end = np.array(row_doc, i64), np.array(row_tok, i64), np.array(row_end, i64)
    body = row_end - row_tok
    lens = body + k
    longest = int(lens.max()) if R else 0
    W = max_len if width_multiple == 0 else min(max_len, -(-longest // width_multiple) * width_multiple)
    if n_docs >= 2**32 - 1 or len(tokens) >= 2**32 or R >= 2**32 or R * W >= 2**32:
        raise Refused("32-bit")
    # element e of a row sits in column e (padding behind) or in column W - len + e (padding in front): [bos] body [eos]
    col = np.arange(W, dtype=i64)[None, :]
    e = col - (W - lens[:, None]) if left else col + 0 * lens[:, None]
    mask = (e >= 0) & (e < lens[:, None])
    t = e - (bos is not None)  # index into the row's body
    is_body = mask & (t >= 0) & (t < body[:, None])
    src = np.asarray(off, i64)[row_doc][:, None] + row_tok[:, None] + t
    ids = np.full((R, W), pad, dtype=np.uint32)
    ids[is_body] = tokens[src[is_body]]
    if bos is not None:
        ids[mask & (e == 0)] = bos
    if eos is not None:
        ids[mask & (e == lens[:, None] - 1)] = eos
    u32 = np.uint32
    return Padded(ids, mask.astype(np.uint8), lens.astype(u32), row_doc.astype(u32), row_tok.astype(u32), np.array(doc_row, u32))


def same(got: Padded, want: Padded, ctx):
    for name in Padded._fields:
        g, w = getattr(got, name), getattr(want, name)
        assert g.shape == w.shape and np.array_equal(g, w), (name, ctx, np.argwhere(g != w)[:5].tolist() if g.shape == w.shape else (g.shape, w.shape))


def cases(block: int, rng):
    """The case list of both test files around workgroups of `block` positions: (name, docs, [max_len ...]).  Ids are random below 50000.
    The callers cross every max_len with bos / eos, the padding side, head / tail / windows, strides and width multiples."""
    def doc(n):
        return rng.integers(0, 50000, size=n).tolist()

    B = block
    return [
        ("empty batch", [], [1, 7]),
        ("only empty documents", [[], [], []], [1, 4, 9]),
        ("one token", [doc(1)], [1, 3, 8]),
        ("runs of 40 and 70 empty documents", [doc(5)] + [[]] * 40 + [doc(20)] + [[]] * 70 + [doc(3)], [3, 7, 8, 64]),
        ("empty documents first and last", [[]] * 3 + [doc(9)] + [[]] + [doc(2 * B + 3)] + [[]] * 2, [7, 9, B]),
        ("one document over many windows", [doc(5 * B + 11)], [3, 7, 64, B, B + 1]),
        ("row boundaries at block - 1, block, block + 1", [doc(B - 1), doc(1), doc(1), doc(B - 2), doc(1), doc(1), doc(B // 2 + 3)], [7, 8, B - 1, B, B + 1]),
        ("short documents", [doc(n) for n in (1, 2, 3, 1, 1, 8, 7, 9, 16, 15, 17, 0, 0, 1)] * 6, [2, 5, 8, 9, 64]),
    ]


def settings(max_len: int, k: int, longest_doc: int = 0):
    """What a max_len is crossed with: dicts of stride / windows / keep_tail / left / width_multiple.  stride in {0, 1, c - 1} -- c - 1 makes
    a row per token, and is left out where the longest document would give more than 2^21 positions that way (around_capacity crosses it
    with max_len 2048 and 2049 on documents of a few rows)."""
    c = max_len - k
    if c <= 0:
        return []
    strides = sorted({0, 1, c - 1} if max(longest_doc - c, 0) * max_len <= 1 << 21 else {0, 1})
    out = []
    for left in (False, True):
        for wm in (0, 1, 8, 64):
            out.append(dict(left=left, width_multiple=wm))
            out.append(dict(left=left, width_multiple=wm, keep_tail=True))
            for stride in strides:
                if stride < c:
                    out.append(dict(left=left, width_multiple=wm, windows=True, stride=stride))
    return out


def around_capacity(max_len: int, k: int, stride: int, rng):
    """Documents of c - 1, c, c + 1, c + step - 1, c + step, c + step + 1 tokens (and an empty one between)"""
    c = max_len - k
    step = c - stride
    sizes = [c - 1, c, c + 1, 0, c + step - 1, c + step, c + step + 1]
    return [rng.integers(0, 50000, size=max(n, 0)).tolist() for n in sizes]
