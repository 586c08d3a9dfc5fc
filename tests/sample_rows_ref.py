"""The rule of the packed sample rows (include/tiktoken_amd.h, tk_pack_samples_device) restated as plain Python loops over lists, from its
description -- not from the kernels: the packing loop an SFT data collator writes.  The per-sample streams (bos, before ids, body, after
ids, eos, what is trained, the cut) come from samples_ref.samples_rule.  What tests/test_sample_rows_sim.py and
tests/test_gpu_sample_rows.py compare the CPU simulation and the device with."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

import samples_ref as sr

NONE = 0xFFFFFFFF
IGNORE = sr.IGNORE
Refused = sr.Refused


class SampleRows(NamedTuple):
    ids: np.ndarray  # uint32[R, L]
    labels: np.ndarray  # int32[R, L]
    seg: np.ndarray  # uint32[R, L]
    pos: np.ndarray  # uint32[R, L]
    cu_seqlens: np.ndarray  # uint32[n_segs + 1]
    row_seg: np.ndarray  # uint32[R + 1]
    row_sample: np.ndarray  # uint32[R + 1]
    len: np.ndarray  # uint32[n]
    full_len: np.ndarray  # uint64[n]
    n_trained: np.ndarray  # uint32[n]
    sample_row: np.ndarray  # uint32[n]
    sample_col: np.ndarray  # uint32[n]


def rows_rule(tokens, tok_off, part_role, sample_off, roles, max_len: int, *, width_multiple: int = 0, bos=None, eos=None, pad: int = 0, ignore: int = IGNORE,
              keep_tail: bool = False, left: bool = False, skip_long: bool = False, ignore_first: bool = False) -> SampleRows:
    # (its refusals too; width_multiple=1: rows as wide as the longest sample, so that its R * W refusal, which is not this rule's, stays out)
    one = sr.samples_rule(tokens, tok_off, part_role, sample_off, roles, max_len, width_multiple=1, bos=bos, eos=eos, pad=pad, ignore=ignore, keep_tail=keep_tail)
    if width_multiple != 0:
        raise Refused("width_multiple")
    if left:
        raise Refused("left")
    n, L = len(one.len), max_len
    streams = []  # per sample: (ids, labels) of what is placed, [] for a sample that is not
    for s in range(n):
        k = int(one.len[s])
        if skip_long and int(one.full_len[s]) > L:
            k = 0
        ids = [int(x) for x in one.ids[s, :k]]
        lab = [int(x) for x in one.labels[s, :k]]
        if ignore_first and k:
            lab[0] = ignore
        streams.append((ids, lab))
    # next-fit in input order
    sample_row, sample_col = [NONE] * n, [0] * n
    row, fill, any_ = 0, 0, False
    for s in range(n):
        p = len(streams[s][0])
        if p == 0:
            continue
        if fill + p > L:
            row += 1
            fill = 0
        sample_row[s], sample_col[s] = row, fill
        fill += p
        any_ = True
    R = row + 1 if any_ else 0
    if R * L >= 2**32:
        raise Refused("32-bit")
    ids = [[pad] * L for _ in range(R)]
    labels = [[ignore] * L for _ in range(R)]
    seg = [[NONE] * L for _ in range(R)]
    pos = [[0] * L for _ in range(R)]
    fills = [0] * R
    row_sample = [n] * (R + 1)
    for s in range(n - 1, -1, -1):
        if sample_row[s] != NONE:
            row_sample[sample_row[s]] = s
    for s in range(n):
        r, c0 = sample_row[s], sample_col[s]
        if r == NONE:
            continue
        for i, (v, lab) in enumerate(zip(*streams[s])):
            ids[r][c0 + i], labels[r][c0 + i], seg[r][c0 + i], pos[r][c0 + i] = v, lab, s, i
        fills[r] = c0 + len(streams[s][0])
    for r in range(R):
        for c in range(fills[r], L):
            pos[r][c] = c - fills[r]
    cu, row_seg = [], []
    for r in range(R):
        row_seg.append(len(cu))
        cu += [r * L + c for c in range(L) if pos[r][c] == 0]
    row_seg.append(len(cu))
    cu.append(R * L)
    n_trained = [sum(1 for x in streams[s][1] if x != ignore) for s in range(n)] if not _ambiguous(ignore, streams) else None
    if n_trained is None:  # (an id equal to ignore_index cannot be told from an untrained element by its label: count by the rule instead)
        n_trained = []
        for s in range(n):
            k = len(streams[s][0])
            t = int(one.n_trained[s]) if k else 0
            if k and ignore_first and int(one.labels[s, 0]) != ignore:
                t -= 1
            n_trained.append(t)
    return SampleRows(np.array(ids, np.uint32).reshape(R, L), np.array(labels, np.int64).astype(np.int32).reshape(R, L), np.array(seg, np.uint32).reshape(R, L),
                      np.array(pos, np.uint32).reshape(R, L), np.array(cu, np.uint32), np.array(row_seg, np.uint32), np.array(row_sample, np.uint32), one.len.copy(),
                      one.full_len.copy(), np.array(n_trained, np.uint32).reshape(n), np.array(sample_row, np.uint32).reshape(n), np.array(sample_col, np.uint32).reshape(n))


def _ambiguous(ignore, streams):
    return any(v == ignore for ids, _ in streams for v in ids)


def same(got: SampleRows, want: SampleRows, ctx):
    for name in SampleRows._fields:
        g, w = getattr(got, name), getattr(want, name)
        assert g.dtype == w.dtype, (name, ctx, g.dtype, w.dtype)
        assert g.shape == w.shape and np.array_equal(g, w), (name, ctx, np.argwhere(g != w)[:5].tolist() if g.shape == w.shape else (g.shape, w.shape))


def invariants(got: SampleRows, L: int, ignore: int = IGNORE):
    """What holds for every result, whatever the batch: pos == 0 exactly at cu_seqlens[:-1]; rows that are full have no padding segment;
    row_seg counts the starts below every row; n_trained is the count of a sample's labels (ids that equal ignore_index aside)."""
    R = got.ids.shape[0]
    flat = got.pos.reshape(-1)
    assert np.array_equal(np.flatnonzero(flat == 0), got.cu_seqlens[:-1]) and int(got.cu_seqlens[-1]) == R * L
    assert np.array_equal(got.row_seg, np.searchsorted(got.cu_seqlens[:-1], np.arange(R + 1) * L))
    placed = got.sample_row != NONE
    fill = np.zeros(R, np.int64)
    np.add.at(fill, got.sample_row[placed].astype(np.int64), np.where(placed, got.len, 0)[placed].astype(np.int64))
    assert np.array_equal((got.seg != NONE).sum(1), fill) and (fill > 0).all() and (fill <= L).all()
    per_row = np.diff(got.row_seg.astype(np.int64))
    in_row = np.bincount(got.sample_row[placed].astype(np.int64), minlength=R)
    assert np.array_equal(per_row, in_row + (fill < L))
    counted = np.zeros(len(got.len), np.int64)
    kept = (got.labels != ignore) & (got.seg != NONE)
    np.add.at(counted, got.seg[kept].astype(np.int64), 1)
    assert np.array_equal(counted, got.n_trained), (counted[:8], got.n_trained[:8])
    assert not (got.labels[got.seg == NONE] != ignore).any()


def cases(rng):
    """The case list of both test files: (name, samples, L, [keywords of rows_rule ...]); a sample is a list of (role, body) over
    samples_ref.CHAT.  Role 3 has no ids and trains, so without bos / eos a sample [(3, body)] has exactly len(body) elements."""
    def body(k):
        return rng.integers(0, 50000, size=k).tolist()

    def plain(k):  # a sample of exactly k elements under (bos, eos) = (None, None)
        return [(3, body(k))]

    def conv(*sizes):
        return [(int(rng.integers(0, len(sr.CHAT))), body(k)) for k in sizes]

    bare = [dict()]
    flags = [dict(), dict(skip_long=True), dict(ignore_first=True), dict(keep_tail=True, skip_long=True, ignore_first=True)]
    specials = [dict(bos=b, eos=e) for b, e in sr.SPECIALS]
    out = [(f"a chain of {R} rows", [plain(5) for _ in range(R)], 8, bare) for R in (0, 1, 2, 3, 4, 5, 8, 9, 16, 17)]
    out += [(f"a chain of {R} rows across workgroups and scan blocks", [plain(5) for _ in range(R)], 8, bare) for R in (2049, 4097)]
    for n in (1023, 1024, 1025, 2049):
        out.append((f"{n} samples of mixed lengths", [conv(*rng.integers(0, 6, size=int(rng.integers(0, 3))).tolist()) for _ in range(n)], 12,
                    [dict(bos=1), dict(eos=2, skip_long=True, ignore_first=True)]))
    for R, L in ((23, 89), (256, 8), (1, 2048), (3, 683), (3, 1367)):  # R * L = 2047, 2048, 2048, 2049, 4101
        out.append((f"{R} rows of {L}: {R * L} positions", [plain(L - 1 - (i % 2)) for i in range(R)], L, bare))
    out.append(("3 rows of 683 filled by conversations", [conv(*rng.integers(0, 40, size=4).tolist()) for _ in range(40)], 683,
                [dict(bos=1, eos=2), dict(eos=2, keep_tail=True, ignore_first=True)]))
    out.append(("a fill that ends at L stays, one past opens a row", [plain(3), plain(5), plain(4), plain(5), plain(8), plain(7), plain(1), plain(1)], 8, bare))
    out.append(("plen == L alone in a row", [plain(2), plain(8), plain(11), plain(3), plain(8)], 8, flags))
    out.append(("every sample one element", [plain(1) for _ in range(50)], 8, bare + [dict(ignore_first=True)]))
    for run in (0, 1, 3000):
        out.append((f"runs of {run} unplaced samples at the start, in the middle and at the end",
                    [[]] * run + [plain(3), plain(4)] + [[]] * run + [plain(2), plain(7)] + [[]] * run + [plain(1)] + [[]] * run, 8, bare))
    out.append(("unplaced samples inside a row and at a row's edge, left out by skip_long",
                [plain(3), plain(9), plain(2), plain(20), plain(20), plain(3), plain(6), plain(9), plain(2)], 8, [dict(skip_long=True), dict()]))
    out.append(("only empty samples", [[], [], []], 8, bare))
    out.append(("no samples", [], 8, bare))
    for L in (7, 8, 9, 64):
        out.append((f"lengths around L = {L}", [plain(L - 1), plain(L), plain(L + 1), plain(L - 1), plain(L + 1), plain(L)], L, flags))
    # ignore_first: the first kept element is a bos; a before id; a trained body token (no bos, no before ids, the tail kept); a one-element sample
    first = [[(2, body(4))], [(3, body(6))], [(3, body(1))], [(0, body(2)), (2, body(30))], [(3, [])], [(5, body(3))]]
    out.append(("ignore_first", first, 16, [dict(bos=1, ignore_first=True), dict(ignore_first=True), dict(ignore_first=True, keep_tail=True),
                                            dict(eos=2, ignore_first=True, keep_tail=True), dict(bos=1, eos=2, ignore_first=True, skip_long=True)]))
    out.append(("conversations under every bos / eos", [conv(*rng.integers(0, 30, size=int(rng.integers(0, 7))).tolist()) for _ in range(60)], 64,
                specials + [dict(bos=1, eos=2, keep_tail=True, skip_long=True, ignore_first=True)]))
    out.append(("rows narrower than a lane", [conv(*rng.integers(0, 4, size=2).tolist()) for _ in range(30)], 3, specials[1:3] + [dict(ignore_first=True)]))
    return out
