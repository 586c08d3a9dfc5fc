"""The rule of the training rows (include/tiktoken_amd.h, tk_pack_rows_device) restated in numpy from its description -- not from the kernels:
what tests/test_rows_sim.py and tests/test_gpu_rows.py compare the CPU simulation and the device with."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

NONE = 0xFFFFFFFF


class Rows(NamedTuple):
    ids: np.ndarray  # uint32[M]
    doc: np.ndarray
    pos: np.ndarray
    cu_seqlens: np.ndarray
    row_seg: np.ndarray
    n_rows: int
    n_segs: int
    n_stream: int
    n_tail: int


def rows_rule(tokens, tok_off, seq_len: int, bos=None, eos=None, pad: int = 0, drop_last: bool = False) -> Rows:
    tokens = np.asarray(tokens, dtype=np.uint32)
    off = [int(x) for x in tok_off]
    n_docs, L = len(off) - 1, int(seq_len)
    k = (bos is not None) + (eos is not None)
    stream, doc_of, out_off = [], [], []
    for d in range(n_docs):  # the stream: [bos] document [eos], document after document
        out_off.append(len(stream))
        assert out_off[d] == off[d] + d * k
        elems = ([bos] if bos is not None else []) + tokens[off[d]:off[d + 1]].tolist() + ([eos] if eos is not None else [])
        stream += elems
        doc_of += [d] * len(elems)  # (with k == 0 an empty document contributes nothing and owns no position)
    S = len(stream)
    assert S == len(tokens) + n_docs * k
    R = S // L if drop_last else -(-S // L)
    M = S if drop_last else R * L
    n_tail = S - R * L if drop_last else 0
    ids = np.array(stream + [pad] * (M - S), dtype=np.uint32)
    doc = np.array(doc_of + [NONE] * (M - S), dtype=np.uint32)
    j = np.arange(M, dtype=np.int64)
    start = np.full(M, S, dtype=np.int64)
    if S:
        start[:S] = np.asarray(out_off, dtype=np.int64)[np.asarray(doc_of, dtype=np.int64)]
    pos = j - np.maximum(start, (j // L) * L)
    assert M == 0 or int(pos.min()) >= 0
    seg_starts = np.flatnonzero(pos == 0)
    cu = np.concatenate([seg_starts, [M]]).astype(np.uint32)
    row_seg = np.array([int((seg_starts < r * L).sum()) for r in range(R + 1)], dtype=np.uint32)
    return Rows(ids, doc, pos.astype(np.uint32), cu, row_seg, R, len(seg_starts), S, n_tail)


def pack_docs(docs):
    """(tokens uint32[T], tok_off uint64[n + 1]) of a list of token lists"""
    tok_off = np.zeros(len(docs) + 1, np.uint64)
    if docs:
        tok_off[1:] = np.cumsum([len(d) for d in docs])
    flat = np.array([t for d in docs for t in d], np.uint32)
    return flat, tok_off


def cases(block: int, rng):
    """The case list of both test files around workgroups of `block` positions: (name, docs, [seq_len ...]).  Ids are random below 50000."""
    def doc(n):
        return rng.integers(0, 50000, size=n).tolist()

    B = block
    out = [
        ("empty batch", [], [1, 7]),
        ("only empty documents", [[], [], []], [1, 4]),
        ("one token", [doc(1)], [1, 3]),
        ("runs of 40 and 70 empty documents", [doc(5)] + [[]] * 40 + [doc(20)] + [[]] * 70, [1, 7, 64]),
        ("empty documents first", [[]] * 3 + [doc(9)] + [[]] + [doc(2 * B + 3)], [7, B]),
        ("one document over many rows", [doc(5 * B + 11)], [1, 7, 64, B, 2 * B]),
        ("boundaries at block - 1, block, block + 1", [doc(B - 1), doc(1), doc(1), doc(B - 2), doc(1), doc(1), doc(B // 2 + 3)], [1, 7, 64, B, 2 * B]),
        ("boundaries around a block, empty documents between", [doc(B - 1), [], doc(1), [], [], doc(1), doc(B + 5)], [7, B]),
        ("document starts on, before and after row starts", [doc(64), doc(63), doc(66), doc(127), doc(1), doc(64), doc(64)], [64, 32]),
        ("short documents", [doc(n) for n in (1, 2, 3, 1, 1, 8, 7, 9, 16, 15, 17, 0, 0, 1)] * 6, [1, 5, 8, 64]),
    ]
    return out


SPECIALS = [(None, None), (50256, None), (None, 50256), (50257, 50256)]  # (bos, eos): none, bos only, eos only, both
