"""The decode-rows passes (tk_decode_rows.h) on the CPU: tests/hostsim/decode_rows_sim.cpp compiles the plain C++ they are made of
(tiktoken_amd/csrc/tk_decode_rows_rule.h) for the host and drives it the way the kernels do -- tiles of 16 and of 2048 columns per row,
lanes of eight, the tiles of every pass in ascending and in descending order, the matrix behind a reader that refuses every index outside
the columns of its rows, the token array behind a writer that counts the stores per slot.  Compared with the restatement of the rule as
Python loops in tests/decode_rows_ref.py, which is written from the rule's description (include/tiktoken_amd.h), not from the kernels.
The same driver also runs as a program of its own under the address and undefined-behaviour sanitizers (host code only: nothing of it is
loaded into Python)."""
import ctypes
import struct
import subprocess

import numpy as np
import pytest

import decode_rows_ref as dr
import helpers as h

_lib = None
BLOCKS = (16, 2048)
SRCS = ("decode_rows_sim.cpp", "sim_readers.h", "tk_decode_rows_rule.h", "tk_decode_rule.h", "tk_rows_rule.h", "tk_device.h", "tk_common.h")
G32, G64 = 0xDEADBEEF, 0xDEADBEEFDEADBEEF
SPEC = 0x80000000
N_IDS = 1000  # the toy vocabulary: ids 0 .. 999 without 500 .. 509, and 900 .. 999 are special tokens
HOLES = range(500, 510)
STOP, STOP2, PAD = 950, 77, 1234  # a special stop, an ordinary one, a pad id outside the vocabulary


def valid(t):
    return 0 <= t < N_IDS and t not in HOLES


def special(t):
    return 900 <= t < N_IDS


def toy_dec():
    dec = np.zeros((N_IDS, 2), np.uint32)
    for t in range(N_IDS):
        if valid(t):
            dec[t] = ((SPEC if special(t) else 0) | (3 * t), 1 + t % 5)
    return dec


DEC = toy_dec()


def lib():
    global _lib
    if _lib is None:
        L = h.build_sim("libdecode_rows_sim.so", SRCS, ("-Wall", "-Werror"))
        vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
        L.decode_rows_sim.restype = ctypes.c_int64
        L.decode_rows_sim.argtypes = [vp, u64, u64, u64, vp, vp, u32, u32, vp, u32, vp, vp, u32, u32, u32, vp, vp, u64, vp, vp, vp]
        _lib = L
    return _lib


def flags_of(m, skip_special=False, keep_stop=False):
    return dr.FLAG_OF[m.dtype] | (dr.SKIP_SPECIAL if skip_special else 0) | (dr.KEEP_STOP if keep_stop else 0)


def lists(stop, skip):
    s, k = np.zeros(max(len(stop), 16), np.uint32), np.zeros(max(len(skip), 16), np.uint32)
    s[: len(stop)] = list(stop)
    k[: len(skip)] = list(skip)
    return s, k


def run_sim(m, begin=None, end=None, stop=(), skip=(), block=16, order=0, **kw):
    """(rc, Rows or None, result words) of the simulation on the 2-D array m, as it lies in memory; every output sits in front of a guard"""
    R, W = m.shape
    assert m.strides[1] == m.itemsize or W <= 1
    ld = m.strides[0] // m.itemsize if R > 1 else W
    s, k = lists(stop, skip)
    b = None if begin is None else np.ascontiguousarray(begin, np.uint32)
    e = None if end is None else np.ascontiguousarray(end, np.uint32)
    cap = R * W
    tokens, tok_off = np.full(cap + 1, G32, np.uint32), np.full(R + 2, G64, np.uint64)
    n_kept, stop_col, res = np.full(R + 1, G32, np.uint32), np.full(R + 1, G32, np.uint32), np.zeros(3, np.uint64)
    rc = lib().decode_rows_sim(m.ctypes.data, R, W, ld, None if b is None else b.ctypes.data, None if e is None else e.ctypes.data, flags_of(m, **kw), len(stop),
                               s.ctypes.data, len(skip), k.ctypes.data, DEC.ctypes.data, N_IDS, block, order, res.ctypes.data, tokens.ctypes.data, cap,
                               tok_off.ctypes.data, n_kept.ctypes.data, stop_col.ctypes.data)
    if rc:
        return rc, None, res
    K = int(res[0])
    assert (tokens[K:] == G32).all() and tok_off[-1] == G64 and n_kept[-1] == G32 and stop_col[-1] == G32
    return 0, dr.Rows(tokens[:K], tok_off[: R + 1], n_kept[:R], stop_col[:R]), res


def check(m, begin=None, end=None, stop=(), skip=(), blocks=BLOCKS, ctx=None, **kw):
    try:
        want = dr.rows_rule(m, begin, end, stop, skip, valid=valid, special=special, **kw)
    except dr.InvalidToken as bad:
        for block in blocks:
            for order in (0, 1):
                rc, _, res = run_sim(m, begin, end, stop, skip, block, order, **kw)
                assert rc == 17 and int(res[2]) == bad.row * m.shape[1] + bad.col, (ctx, rc, res, bad)
        return None
    except dr.Refused as bad:
        for block in blocks:
            for order in (0, 1):
                rc, _, res = run_sim(m, begin, end, stop, skip, block, order, **kw)
                assert rc == 16 and int(res[1]) == bad.row, (ctx, rc, res, bad.row)
        return None
    for block in blocks:
        for order in (0, 1):
            rc, got, _ = run_sim(m, begin, end, stop, skip, block, order, **kw)
            assert rc == 0, (rc, ctx, block, order)
            dr.same(got, want, (ctx, block, order, kw))
    return want


def matrix(rng, R, W, dtype, ld_extra=0, shift=0, lo=0, hi=N_IDS):
    return dr.held(rng.integers(lo, hi, size=(R, W)), dtype, ld_extra, shift)


def test_a_case_worked_by_hand():
    """Three rows of ten: row 0 stops at column 6 (950, a special token); row 1 has no stop, a special token 901 and two pads; row 2 begins
    at 4 behind a stop at column 1 that is never looked at, and ends at 9."""
    m = np.array([[5, 6, 1234, 7, 901, 8, 950, 1234, 1234, 1234], [1, 2, 3, 901, 4, 1234, 1234, 6, 7, 8], [9, 950, 9, 9, 10, 11, 12, 13, 14, 15]], np.int64)
    for block in BLOCKS:
        rc, got, _ = run_sim(m, [0, 0, 4], [10, 10, 9], [STOP], [PAD], block)
        assert rc == 0 and got.tokens.tolist() == [5, 6, 7, 901, 8, 1, 2, 3, 901, 4, 6, 7, 8, 10, 11, 12, 13, 14]
        assert got.tok_off.tolist() == [0, 5, 13, 18] and got.n_kept.tolist() == [5, 8, 5] and got.stop_col.tolist() == [6, 10, 9]
        rc, got, _ = run_sim(m, [0, 0, 4], [10, 10, 9], [STOP], [PAD], block, skip_special=True, keep_stop=True)  # the kept stop is special: skipped after all
        assert rc == 0 and got.tokens.tolist() == [5, 6, 7, 8, 1, 2, 3, 4, 6, 7, 8, 10, 11, 12, 13, 14] and got.stop_col.tolist() == [6, 10, 9]
        rc, got, _ = run_sim(m, None, None, [STOP], [PAD], block, keep_stop=True)
        assert rc == 0 and got.tokens.tolist() == [5, 6, 7, 901, 8, 950, 1, 2, 3, 901, 4, 6, 7, 8, 9, 950] and got.stop_col.tolist() == [6, 10, 1]
    check(m, [0, 0, 4], [10, 10, 9], [STOP], [PAD])


@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_shapes_around_the_tile(dtype):
    """W in {0, 1, 7, 8, 9, T - 1, T, T + 1, 2T + 1} for T = 16 (and the same figures inside one tile of 2048), R in {0, 1, 3}, rows that are
    ld == W and ld == W + 3 apart, the matrix at every element offset from a 16-byte boundary"""
    rng = np.random.default_rng(16)
    for W in (0, 1, 7, 8, 9, 15, 16, 17, 33):
        for R in (0, 1, 3):
            for ld_extra, shift in ((0, 0), (3, 1), (0, 2), (3, 3)):
                vals = rng.integers(0, 490, size=(R, W))
                if W:
                    vals[rng.random((R, W)) < 0.1] = STOP2
                    vals[rng.random((R, W)) < 0.1] = PAD
                m = dr.held(vals, dtype, ld_extra, shift)
                for kw in (dict(), dict(keep_stop=True), dict(skip_special=True)):
                    check(m, None, None, [STOP2], [PAD], ctx=(W, R, ld_extra, shift), **kw)
                b = rng.integers(0, W + 1, size=R)
                e = np.minimum(b + rng.integers(0, W + 1, size=R), W)
                check(m, b, e, [STOP2, STOP], [PAD, 3], ctx=(W, R, "range"), keep_stop=True)


@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_shapes_around_the_device_tile(dtype):
    rng = np.random.default_rng(2048)
    for W in (2047, 2048, 2049, 4097):
        vals = rng.integers(0, 490, size=(3, W))
        vals[0, [W // 3, W - 1]] = STOP2  # two stops in one row
        vals[2, W - 1] = STOP2  # a stop at end - 1
        vals[rng.random((3, W)) < 0.2] = PAD
        m = dr.held(vals, dtype, 3, 1)
        check(m, None, None, [STOP2], [PAD], ctx=W)
        check(m, [5, 0, W - 1], [W, 0, W], [STOP2], [PAD], ctx=(W, "range"), keep_stop=True)


def test_stop_positions():
    """A stop at begin, at end - 1, at columns T - 1 and T, before begin (ignored), at end (ignored); two stops in different tiles"""
    T = 16
    base = np.arange(100, 100 + 3 * T + 1)
    for begin, end, stops_at in ((4, 40, [4]), (4, 40, [39]), (0, 49, [T - 1]), (0, 49, [T]), (4, 40, [2]), (4, 40, [40]), (0, 49, [T + 3, 2 * T + 5]), (0, 49, [2 * T + 5, 3]),
                                 (4, 40, [2, 45]), (7, 7, [7])):
        row = base.copy()
        row[stops_at] = STOP2
        m = np.stack([row, base, row]).astype(np.int64)
        for kw in (dict(), dict(keep_stop=True)):
            want = check(m, [begin] * 3, [end] * 3, [STOP2], ctx=(begin, end, stops_at), **kw)
            inside = [c for c in stops_at if begin <= c < end]
            assert want.stop_col.tolist() == [min(inside, default=end), end, min(inside, default=end)]


def test_a_stop_id_that_is_also_a_skip_id():
    m = np.array([[1, 2, STOP2, 3, 4]] * 2, np.int32)
    assert check(m, stop=[STOP2], skip=[STOP2]).tokens.tolist() == [1, 2] * 2
    assert check(m, stop=[STOP2], skip=[STOP2], keep_stop=True).tokens.tolist() == [1, 2] * 2  # kept by the stop rule, then skipped
    assert check(m, stop=[STOP2], keep_stop=True).tokens.tolist() == [1, 2, STOP2] * 2
    assert check(m, skip=[STOP2]).tokens.tolist() == [1, 2, 3, 4] * 2


def test_empty_rows_and_nothing_kept():
    rng = np.random.default_rng(3)
    m = matrix(rng, 5, 40, np.int64, hi=490)
    want = check(m, [3, 40, 0, 17, 9], [3, 40, 0, 17, 9])  # begin == end in every row
    assert len(want.tokens) == 0 and want.tok_off.tolist() == [0] * 6 and want.stop_col.tolist() == [3, 40, 0, 17, 9]
    pads = np.full((4, 37), PAD, np.uint32)
    assert len(check(pads, skip=[PAD]).tokens) == 0  # every id skipped: K == 0
    specials = np.full((4, 37), 930, np.int32)
    assert len(check(specials, skip_special=True).tokens) == 0
    assert len(check(specials).tokens) == 4 * 37


def test_sixteen_ids_in_each_list():
    rng = np.random.default_rng(5)
    m = matrix(rng, 7, 61, np.uint32, ld_extra=3, shift=1, hi=64)
    check(m, stop=list(range(40, 56)), skip=list(range(0, 32, 2)), keep_stop=True)
    check(m, stop=[63], skip=[62])


def test_invalid_ids():
    """Behind the stop, in the skip list, before begin and at or behind end they are accepted; in the live range the first one in row-major
    order is named -- a later row's, an earlier column's"""
    rng = np.random.default_rng(7)
    vals = rng.integers(0, 490, size=(4, 50))
    vals[:, 30] = STOP2
    vals[:, 31:] = 505  # a hole of the table, behind the stop
    vals[:, 0] = 2000  # beyond the table, before begin
    m = vals.astype(np.int64)
    want = check(m, [1] * 4, None, [STOP2], [PAD])
    assert want.n_kept.tolist() == [29] * 4
    m[1, 3] = PAD  # outside the vocabulary, in skip_ids
    assert check(m, [1] * 4, None, [STOP2], [PAD]).n_kept.tolist() == [29, 28, 29, 29]
    m[3, 2] = 505
    m[2, 20] = 2000
    m[2, 7] = 507
    for block in BLOCKS:
        for order in (0, 1):
            rc, _, res = run_sim(m, [1] * 4, None, [STOP2], [PAD], block, order)
            assert rc == 17 and int(res[2]) == 2 * 50 + 7
    check(m, [1] * 4, None, [STOP2], [PAD])
    assert check(m, [1, 1, 21, 3], None, [STOP2], [PAD]).n_kept.tolist() == [29, 28, 9, 27]  # all three before begin now
    with pytest.raises(dr.InvalidToken):
        dr.rows_rule(m, [1, 1, 21, 2], None, [STOP2], [PAD], valid=valid, special=special)
    check(m, [1, 1, 21, 2], None, [STOP2], [PAD])


def test_values_that_are_no_uint32():
    """A negative int32 / int64 and an int64 of 2^32 and more: in no list (their low words are in both), never with an entry"""
    for dtype, bad in ((np.int32, -1), (np.int64, -1), (np.int64, (1 << 32) + 5), (np.int64, -(1 << 32) + 5), (np.int64, 1 << 63 - 1), (np.int32, -(1 << 31))):
        m = np.full((2, 20), 6, dtype)  # (no value below has the low word 6)
        m[1, 9] = bad
        low = int(np.array(bad, np.int64).view(np.uint64)) & 0xFFFFFFFF
        for block in BLOCKS:
            rc, _, res = run_sim(m, stop=[low], skip=[low], block=block)
            assert rc == 17 and int(res[2]) == 29, (dtype, bad, rc)
        assert check(m, None, [20, 9]).n_kept.tolist() == [20, 9]  # outside the live range it is not judged
        m[1, 3] = 7
        assert check(m, stop=[7]).stop_col.tolist() == [20, 3]  # ... nor behind a stop
    m = np.full((2, 20), 5, np.uint32)
    m[0, 4] = 0xFFFFFFFF  # an id like any other for uint32: skipped when listed, without entry when not
    assert check(m, skip=[0xFFFFFFFF]).n_kept.tolist() == [19, 20]
    assert run_sim(m)[0] == 17


def test_begin_and_end_that_offend():
    rng = np.random.default_rng(9)
    m = matrix(rng, 6, 40, np.int32, hi=490)
    for begin, end, row in (([0, 0, 5, 0, 0, 0], [40, 40, 4, 40, 40, 40], 2), (None, [40, 41, 40, 40, 40, 99], 1), ([41] * 6, None, 0),
                            ([0, 0, 0, 0, 0, 0xFFFFFFFF], [40, 40, 40, 40, 40, 0xFFFFFFFF], 5)):
        for block in BLOCKS:
            for order in (0, 1):
                rc, _, res = run_sim(m, begin, end, [STOP2], [PAD], block, order)
                assert rc == 16 and int(res[1]) == row
        check(m, begin, end, [STOP2], [PAD])
    empty = np.zeros((3, 0), np.int64)
    assert run_sim(empty, [0, 1, 0], None)[0] == 16  # W == 0: the rows still have a tile that checks them
    assert check(empty, [0, 0, 0], [0, 0, 0]).tok_off.tolist() == [0, 0, 0, 0]


def test_refusals_of_the_spec():
    m = np.zeros((2, 8), np.uint32)
    L, n = lib(), None
    s, k = lists(range(17), range(17))
    res = np.zeros(3, np.uint64)
    call = lambda R, W, ld, flags, ns, nk: L.decode_rows_sim(m.ctypes.data, R, W, ld, n, n, flags, ns, s.ctypes.data, nk, k.ctypes.data, DEC.ctypes.data, N_IDS, 16, 0,  # noqa: E731
                                                             res.ctypes.data, n, 0, n, n, n)
    assert call(2, 8, 8, 0, 17, 0) == 1 and call(2, 8, 8, 0, 16, 17) == 2
    assert call(2, 8, 8, dr.I32 | dr.I64, 0, 0) == 3
    assert call(2, 8, 7, 0, 0, 0) == 4
    assert call((1 << 32) - 1, 8, 8, 0, 0, 0) == 5 and call(2, 1 << 32, 1 << 32, 0, 0, 0) == 6
    assert call(2, 8, 8, 16, 0, 0) == 7
    assert call(1 << 31, 8, 1 << 30, 0, 0, 0) == 8


def test_random_sweep():
    rng = np.random.default_rng(0xD0C)
    for i in range(200):
        R, W = int(rng.choice([1, 2, 5, 30])), int(rng.choice([1, 5, 8, 16, 17, 40, 100]))
        dtype = dr.DTYPES[i % 3]
        vals = rng.integers(0, 1000, size=(R, W))
        vals[(vals >= 500) & (vals < 510)] = PAD  # the holes: skipped below, or outside the live range
        m = dr.held(vals, dtype, int(rng.integers(0, 5)), int(rng.integers(0, 4)))
        b = rng.integers(0, W + 1, size=R)
        e = np.minimum(b + rng.integers(0, W + 1, size=R), W)
        stop = rng.integers(0, 1000, size=int(rng.integers(0, 17))).tolist()
        skip = [PAD] + rng.integers(0, 1000, size=int(rng.integers(0, 16))).tolist()
        check(m, b if i % 4 else None, e if i % 5 else None, stop, skip, blocks=(16,), ctx=i, skip_special=bool(i & 1), keep_stop=bool(i & 2))


def todo_for_the_sanitizers():
    rng = np.random.default_rng(77)
    out = []
    for i, (R, W) in enumerate(((0, 0), (3, 0), (0, 9), (1, 1), (3, 7), (3, 8), (2, 9), (3, 15), (3, 16), (3, 17), (2, 33), (2, 2047), (2, 2048), (2, 2049), (1, 4097))):
        dtype = dr.DTYPES[i % 3]
        vals = rng.integers(0, 490, size=(R, W))
        if W:
            vals[rng.random((R, W)) < 0.05] = STOP2
            vals[rng.random((R, W)) < 0.1] = PAD
            vals[rng.random((R, W)) < 0.1] = 950
        m = dr.held(vals, dtype, (0, 3)[i % 2], i % 4)
        b = rng.integers(0, W + 1, size=R)
        e = np.minimum(b + rng.integers(0, W + 1, size=R), W)
        out.append((m, i % 4, b if i % 3 else None, e if i % 2 else None, [STOP2], [PAD], BLOCKS[i % 2], i % 2, dict(skip_special=bool(i & 1), keep_stop=bool(i & 2))))
    m = dr.held(rng.integers(0, 490, size=(4, 30)), np.int64, 3, 1)
    m[2, 11] = -5
    out.append((m, 1, None, None, [], [], 16, 0, dict()))  # refused: an id without entry
    out.append((m, 1, [0, 31, 0, 0], None, [], [], 16, 1, dict()))  # refused: begin > W
    return out


def test_case_list_under_sanitizers(tmp_path):
    """The driver as a program of its own, built with -fsanitize=address,undefined, on matrices that end with their last element: it must
    run clean and give the results of the restatement."""
    exe = h.build_once("decode_rows_sim_san", SRCS, ["-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DDECODE_ROWS_SIM_MAIN"])
    todo = todo_for_the_sanitizers()
    src, dst = tmp_path / "cases.bin", tmp_path / "results.bin"
    with open(src, "wb") as f:
        for m, shift, b, e, stop, skip, block, order, kw in todo:
            R, W = m.shape
            ld = m.strides[0] // m.itemsize if R > 1 else W
            s, k = lists(stop, skip)
            f.write(struct.pack("<16Q", R, W, ld, shift, flags_of(m, **kw), len(stop), len(skip), N_IDS, block, order, b is not None, e is not None, 0, 0, 0, 0))
            f.write(s.tobytes() + k.tobytes() + DEC.tobytes())
            f.write(b"" if b is None else np.asarray(b, np.uint32).tobytes())
            f.write(b"" if e is None else np.asarray(e, np.uint32).tobytes())
            n_elems = shift + ((R - 1) * ld + W if R and W else 0)
            start = m.ctypes.data - shift * m.itemsize
            f.write(ctypes.string_at(start, n_elems * m.itemsize))
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    assert r.stdout.strip() == f"{len(todo)} cases"
    raw = open(dst, "rb").read()
    at = 0
    for m, shift, b, e, stop, skip, block, order, kw in todo:
        rc, K, bad_row, bad_id = struct.unpack_from("<qQQQ", raw, at)
        at += 32
        R = m.shape[0]
        try:
            want = dr.rows_rule(m, b, e, stop, skip, valid=valid, special=special, **kw)
        except dr.InvalidToken as bad:
            assert rc == 17 and bad_id == bad.row * m.shape[1] + bad.col
            continue
        except dr.Refused as bad:
            assert rc == 16 and bad_row == bad.row
            continue
        assert rc == 0 and K == len(want.tokens)
        got = []
        for dtype, count in ((np.uint32, K), (np.uint64, R + 1), (np.uint32, R), (np.uint32, R)):
            got.append(np.frombuffer(raw, dtype, count, at))
            at += count * np.dtype(dtype).itemsize
        dr.same(dr.Rows(*got), want, (m.shape, block, order, kw))
    assert at == len(raw)
