"""The row passes (tk_rows.h) on the CPU: tests/hostsim/rows_sim.cpp compiles the plain C++ they are made of (tiktoken_amd/csrc/tk_rows_rule.h)
for the host and drives it the way the kernels do -- lanes of eight positions, workgroups of 8, 16 and 2048; the write pass runs through
tk_rows_lane, the function the kernel itself calls.  Compared with the numpy restatement of the rule in tests/rows_ref.py, which is written
from the rule's description (include/tiktoken_amd.h), not from the kernels."""
import bisect
import ctypes

import numpy as np
import pytest

import helpers as h
import rows_ref as rr

_lib = None
BLOCKS = (8, 16, 2048)


def lib():
    global _lib
    if _lib is None:
        L = h.build_sim("librows_sim.so", ("rows_sim.cpp", "sim_readers.h", "tk_rows_rule.h", "tk_common.h"), ("-Wall", "-Werror",))
        vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
        L.rows_sim.restype = ctypes.c_int64
        L.rows_sim.argtypes = [vp, u64, vp, u64, u32, u32, u32, u32, ctypes.c_int, u32, vp, vp, vp, vp, vp, vp]
        L.rows_sim_last_le.restype = ctypes.c_int64
        L.rows_sim_last_le.argtypes = [vp, u64, u64, u64, u64]
        L.rows_sim_row_width.restype = u32
        L.rows_sim_row_width.argtypes = [u32, u32, u32]
        _lib = L
    return _lib


def run_sim(tokens, tok_off, L, bos, eos, pad, drop_last, block):
    """(rc, Rows or None) of the simulation; the arrays sit between guard words that must survive."""
    tokens = np.ascontiguousarray(tokens, np.uint32)
    tok_off = np.ascontiguousarray(tok_off, np.uint64)
    T, n_docs = len(tokens), len(tok_off) - 1
    k = (bos is not None) + (eos is not None)
    S = T + n_docs * k
    R = S // L if drop_last else -(-S // L)
    M = S if drop_last else R * L
    G = 0xDEADBEEF
    ids, doc, pos = (np.full(M + 1, G, np.uint32) for _ in range(3))
    cu, row_seg = np.full(n_docs + R + 5, G, np.uint32), np.full(R + 2, G, np.uint32)
    counts = np.zeros(5, np.uint64)
    src = tokens if T else np.zeros(1, np.uint32)
    none = rr.NONE
    rc = lib().rows_sim(src.ctypes.data, T, tok_off.ctypes.data, n_docs, L, none if bos is None else bos, none if eos is None else eos, pad, int(drop_last), block,
                        ids.ctypes.data, doc.ctypes.data, pos.ctypes.data, cu.ctypes.data, row_seg.ctypes.data, counts.ctypes.data)
    if rc:
        return rc, None
    n_rows, n_segs, n_stream, n_tail, m = (int(x) for x in counts)
    assert m == M and ids[M] == G and doc[M] == G and pos[M] == G and cu[-1] == G and row_seg[-1] == G
    return 0, rr.Rows(ids[:M], doc[:M], pos[:M], cu[: n_segs + 1], row_seg[: n_rows + 1], n_rows, n_segs, n_stream, n_tail)


def same(got: rr.Rows, want: rr.Rows, ctx):
    assert (got.n_rows, got.n_segs, got.n_stream, got.n_tail) == (want.n_rows, want.n_segs, want.n_stream, want.n_tail), ctx
    for name in ("ids", "doc", "pos", "cu_seqlens", "row_seg"):
        g, w = getattr(got, name), getattr(want, name)
        assert g.shape == w.shape and np.array_equal(g, w), (name, ctx, np.flatnonzero(g != w)[:5] if g.shape == w.shape else (g.shape, w.shape))


def check(docs, seq_lens, blocks=BLOCKS, specials=rr.SPECIALS, pad=7):
    tokens, tok_off = rr.pack_docs(docs)
    for bos, eos in specials:
        S = len(tokens) + len(docs) * ((bos is not None) + (eos is not None))
        # ... and a row longer than the stream, the stream as one row, the stream an exact multiple of the row
        Ls = sorted(set(seq_lens) | {S + 3, max(S, 1)} | ({S // 3} if S >= 3 and S % 3 == 0 else set()) | ({S // 2} if S >= 2 and S % 2 == 0 else set()))
        for L in Ls:
            for drop_last in (False, True):
                want = rr.rows_rule(tokens, tok_off, L, bos, eos, pad, drop_last)
                for block in blocks:
                    rc, got = run_sim(tokens, tok_off, L, bos, eos, pad, drop_last, block)
                    assert rc == 0, (rc, L, bos, eos, drop_last, block)
                    same(got, want, (L, bos, eos, drop_last, block, [len(d) for d in docs][:12]))


def test_restatement_on_a_case_worked_by_hand():
    """The numpy restatement itself, on a batch small enough to write the answer down.  A guard on tests/rows_ref.py only: it touches
    neither the simulation nor the library, so it passes with or without the row passes and says nothing about them."""
    tokens, tok_off = rr.pack_docs([[10, 11, 12], [], [20], [30, 31]])
    r = rr.rows_rule(tokens, tok_off, 4, eos=99, pad=0)  # stream: 10 11 12 99 | 99 | 20 99 | 30 31 99
    assert r.ids.tolist() == [10, 11, 12, 99, 99, 20, 99, 30, 31, 99, 0, 0]
    assert r.doc.tolist() == [0, 0, 0, 0, 1, 2, 2, 3, 3, 3, rr.NONE, rr.NONE]
    assert r.pos.tolist() == [0, 1, 2, 3, 0, 0, 1, 0, 0, 1, 0, 1]
    assert r.cu_seqlens.tolist() == [0, 4, 5, 7, 8, 10, 12] and r.row_seg.tolist() == [0, 1, 4, 6]
    assert (r.n_rows, r.n_segs, r.n_stream, r.n_tail) == (3, 6, 10, 0)
    r = rr.rows_rule(tokens, tok_off, 4, drop_last=True)  # stream: 10 11 12 | 20 | 30 31; the empty document owns no position
    assert r.ids.tolist() == [10, 11, 12, 20, 30, 31] and r.doc.tolist() == [0, 0, 0, 2, 3, 3] and r.pos.tolist() == [0, 1, 2, 0, 0, 1]
    assert r.cu_seqlens.tolist() == [0, 3, 4, 6] and r.row_seg.tolist() == [0, 2] and (r.n_rows, r.n_tail) == (1, 2)
    r = rr.rows_rule(np.zeros(0, np.uint32), [0], 5)
    assert r.cu_seqlens.tolist() == [0] and r.row_seg.tolist() == [0] and r.n_rows == 0


@pytest.mark.parametrize("block", BLOCKS)
def test_case_list(block):
    rng = np.random.default_rng(block)
    for name, docs, seq_lens in rr.cases(block, rng):
        check(docs, seq_lens, blocks=(block,))


def test_document_starts_around_row_starts_and_lanes():
    rng = np.random.default_rng(3)
    stream = rng.integers(0, 50000, size=200).tolist()
    for cut in list(range(0, 34)) + [63, 64, 65, 127, 128, 129]:
        check([stream[:cut], stream[cut:]], [8, 16, 64], blocks=(8, 16))
        check([stream[:cut], [], [], stream[cut:cut + 1], stream[cut + 1:]], [16, 64], blocks=(16,))


def test_boundaries_around_a_workgroup_of_2048():
    rng = np.random.default_rng(4)
    stream = rng.integers(0, 50000, size=2 * 2048 + 40).tolist()
    for cut in (2046, 2047, 2048, 2049, 2050, 4095, 4096, 4097):
        check([stream[:cut], stream[cut:]], [7, 2048, 4096], blocks=(2048,))
        check([stream[:cut], [], stream[cut:cut + 3], [], [], stream[cut + 3:]], [64, 2048], blocks=(2048,), specials=rr.SPECIALS[::3])


def test_random_sweep():
    rng = np.random.default_rng(0x7035)
    for _ in range(120):
        docs = []
        for _ in range(int(rng.choice([1, 2, 5, 40, 120]))):
            u = rng.random()
            n = 0 if u < 0.25 else 1 if u < 0.35 else int(rng.choice([2, 7, 8, 9, 30, 200, 60, 2500 if rng.random() < 0.1 else 17]))
            docs.append(rng.integers(0, 60000, size=n).tolist())
        check(docs, [int(rng.choice([1, 2, 3, 8, 13, 64, 100, 2048]))], blocks=(8, 16, 2048), specials=[rr.SPECIALS[int(rng.integers(0, 4))]])


def placed(tokens, shift):
    """The tokens in memory of their own, the first one `shift` elements behind a multiple of 16 bytes."""
    buf = np.zeros(len(tokens) + 8, np.uint32)
    at = (-(buf.ctypes.data // 4)) % 4 + shift
    buf[at: at + len(tokens)] = tokens
    out = buf[at: at + len(tokens)]
    assert out.ctypes.data % 16 == 4 * shift
    return out


@pytest.mark.parametrize("T", [7, 8, 9, 2048 + 5])
def test_sixteen_byte_token_loads(T):
    """Without bos and eos the stream is the token array, and a lane whose eight ids all exist fetches them as two 16-byte words where
    the array's address allows it.  Both placements -- the array at a multiple of 16 bytes, where every such lane does, and one element
    behind, where none does -- give the rule's rows, and no lane reads past n_tokens (rc -1 would say so): the last lane of T = 9 and of
    2048 + 5 has fewer than eight ids left."""
    rng = np.random.default_rng(T)
    cuts = sorted(int(c) for c in rng.integers(0, T + 1, size=3))
    tokens, tok_off = rr.pack_docs([d.tolist() for d in np.split(rng.integers(0, 60000, size=T), cuts)])
    for L in (5, 8, T):
        for drop_last in (False, True):
            want = rr.rows_rule(tokens, tok_off, L, None, None, 7, drop_last)
            for block in BLOCKS:
                for shift in (0, 1):
                    rc, got = run_sim(placed(tokens, shift), tok_off, L, None, None, 7, drop_last, block)
                    assert rc == 0, (rc, L, drop_last, block, shift)
                    same(got, want, (T, L, drop_last, block, shift))


def test_refusals():
    tokens, tok_off = rr.pack_docs([[1, 2, 3], [4], [5, 6]])
    assert run_sim(tokens, tok_off, 4, None, None, 0, False, 16)[0] == 0
    # seq_len == 0 (the outputs' sizes are not defined: the call is made with the arrays of seq_len 1)
    assert lib().rows_sim(tokens.ctypes.data, 6, tok_off.ctypes.data, 3, 0, rr.NONE, rr.NONE, 0, 0, 16, None, None, None, None, None, None) == 1
    # 32-bit outputs: positions, document indices (refused from the figures alone: nothing is read)
    assert lib().rows_sim(None, (1 << 32) - 2, None, 3, 4, rr.NONE, 5, 0, 0, 16, None, None, None, None, None, None) == 2
    assert lib().rows_sim(None, (1 << 32) - 3, None, 1, 8, rr.NONE, rr.NONE, 0, 0, 16, None, None, None, None, None, None) == 2  # (R * L reaches 2^32)
    assert lib().rows_sim(None, 5, None, (1 << 32) - 1, 4, rr.NONE, rr.NONE, 0, 0, 16, None, None, None, None, None, None) == 3
    # tok_off that does not describe the batch: the first offending document, and no access out of bounds on the way (rc -1 would say so)
    for bad, doc, why in (([1, 3, 4, 6], 0, 1), ([0, 4, 3, 6], 1, 2), ([0, 3, 4, 5], 2, 3), ([0, 3, 4, 7], 2, 3), ([0, 1 << 40, 4, 6], 1, 2), ([0, 3, 1 << 63, 6], 2, 2),
                          ([0, 9, 9, 6], 2, 2), ([2, 1, 0, 9], 0, 1)):
        for bos, eos in rr.SPECIALS:
            for block in (8, 2048):
                rc, _ = run_sim(tokens, np.array(bad, np.uint64), 4, bos, eos, 0, False, block)
                assert rc == 16 + (doc << 2 | why), (bad, rc)
    assert run_sim(np.zeros(0, np.uint32), np.array([3], np.uint64), 4, None, 1, 0, False, 8)[0] == 16 + 1  # no documents, tok_off = [3]


def test_the_shared_search_on_its_own():
    """tk_last_le, the one search of the row, padded and samples passes: the last index in [lo, hi) whose key is <= x, lo if there is none
    -- bisect_right(keys, x, lo, hi) - 1, clamped to lo.  The keys are handed in as an array of exactly `hi` entries behind a reader that
    checks the index: -1 would say the search looked outside its window."""
    def check(keys, lo, hi, xs):
        held = np.array(keys[:hi] if hi else [0], np.uint64)
        for x in xs:
            want = max(bisect.bisect_right(keys, x, lo, hi) - 1, lo)
            assert lib().rows_sim_last_le(held.ctypes.data, hi, lo, hi, x) == want, (keys, lo, hi, x)

    def around(keys):
        return sorted({x for k in keys for x in (k - 1, k, k + 1) if x >= 0} | {0, 1 << 40})

    for lo in (0, 3):  # windows of 0, 1 and 2 entries; x below keys[lo], at every key, at and above the last
        front = [1, 1, 2][:lo]
        for window in ([], [5], [5, 9], [5, 5]):
            keys = front + window
            check(keys, lo, len(keys), around(keys + [5]))
    for run in (2, 5):  # runs of equal keys at the front, in the middle and at the end of the window
        for lo in (0, 2):
            front = [0, 3][:lo]
            for keys in ([7] * run + [9, 12, 20], [4, 6] + [7] * run + [9, 12], [4, 5, 6] + [7] * run):
                check(front + keys, lo, lo + len(keys), around(keys))
    rng = np.random.default_rng(0x1E)
    keys = np.cumsum(rng.choice([0, 0, 1, 3, 50], size=300)).tolist()
    check(keys, 0, 300, around(keys))
    check(keys, 17, 290, around(keys))


def test_the_width_rule_on_its_own():
    """tk_row_width against the expression of padded_ref.py / samples_ref.py"""
    for max_len in (1, 16, 100):
        for wm in (0, 1, 8):
            for longest in sorted({0, 1, max_len - 1, max_len, 8 * (max_len // 8) + 1 if max_len > 8 else max_len}):  # (the last: its round-up exceeds max_len)
                want = max_len if wm == 0 else min(max_len, -(-longest // wm) * wm)
                assert lib().rows_sim_row_width(max_len, wm, longest) == want, (max_len, wm, longest)
    assert lib().rows_sim_row_width(100, 8, 97) == 100 and lib().rows_sim_row_width(16, 8, 9) == 16 and lib().rows_sim_row_width(100, 8, 9) == 16
    assert lib().rows_sim_row_width(0xFFFFFFFF, 0x80000000, 0x80000001) == 0xFFFFFFFF  # (the round-up is 2^32: computed in 64 bits)
