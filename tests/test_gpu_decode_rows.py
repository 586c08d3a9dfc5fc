"""Decoding id matrices on the GPU (tk_decode_rows.h): tk_decode_rows_device and tk_decode_rows through CoreBPE and Encoding, against the
restatement of the rule as Python loops in tests/decode_rows_ref.py (written from the rule's description in include/tiktoken_amd.h, not
from the kernels) and, for the bytes, against the existing tk_decode_batch on the restatement's ids."""
import ctypes
import functools

import numpy as np
import pytest

import decode_rows_ref as dr
import helpers as h
import tiktoken_amd as tiktoken

pytestmark = pytest.mark.gpu
T = 2048  # TK_DEC_BLOCK: columns per tile
NAME = "cl100k_shaped"  # five special tokens, and ids without a token between them (100261 .. 100275)
EOT, FIM, EOP = 100257, 100258, 100276
HOLE, BEYOND, PAD = 100270, 150000, 120000  # no token; beyond the table; a pad id outside the vocabulary
TORCH_OF = {np.dtype(np.uint32): "int32", np.dtype(np.int32): "int32", np.dtype(np.int64): "int64"}


@functools.lru_cache(maxsize=None)
def enc():
    return tiktoken.get_encoding(NAME)


@functools.lru_cache(maxsize=None)
def vocab():
    e = enc()
    return frozenset(e._mergeable_ranks.values()) | frozenset(e._special_tokens.values()), frozenset(e._special_tokens.values())


def rule(m, begin=None, end=None, stop=(), skip=(), **kw):
    ids, specials = vocab()
    return dr.rows_rule(m, begin, end, stop, skip, valid=ids.__contains__, special=specials.__contains__, **kw)


def to_device(a):
    import torch

    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(getattr(np, TORCH_OF[a.dtype])).copy()).cuda() if a.size else torch.zeros(4, dtype=getattr(torch, TORCH_OF[a.dtype]), device="cuda")
    torch.cuda.synchronize()
    return t


def dev(ptr, n, typestr, dtype):
    import torch

    if not n:
        return np.zeros(0, dtype)
    return torch.as_tensor(h._DevArray(ptr, n, typestr), device="cuda").cpu().numpy().view(dtype)


def read_back(r, R):
    """(Rows, bytes, byte_off) of a DecodedRowsDevice"""
    rows = dr.Rows(h.dev_u32(r.tokens, r.n_tokens), h.dev_u64(r.tok_off, R + 1), h.dev_u32(r.n_kept, R), h.dev_u32(r.stop_col, R))
    return rows, dev(r.data, r.n_bytes, "|u1", np.uint8), h.dev_u64(r.byte_off, R + 1)


def rows_device(m, begin=None, end=None, stop=(), skip=(), **kw):
    """decode_rows_device on the memory the view m lies in (copied to the device as it lies: shift, row stride and the garbage between the rows)"""
    core = enc()._core_bpe
    R, W = m.shape
    ld = m.strides[0] // m.itemsize if R > 1 and W else W
    n = (R - 1) * ld + W if R and W else 0  # from element (0, 0) to the last one: the buffer ends where the matrix does
    shift = (m.ctypes.data % 16) // m.itemsize if n else 0  # ... and (0, 0) keeps its place behind a 16-byte boundary
    span = np.frombuffer(ctypes.string_at(m.ctypes.data, n * m.itemsize), m.dtype) if n else np.zeros(0, m.dtype)
    held = to_device(np.concatenate([np.zeros(shift, m.dtype), span]))
    d_b = None if begin is None else to_device(np.asarray(begin, np.uint32))
    d_e = None if end is None else to_device(np.asarray(end, np.uint32))
    r = core.decode_rows_device(held.data_ptr() + shift * m.itemsize, R, W, ld, dtype=m.dtype, d_begin=d_b.data_ptr() if d_b is not None else 0,
                                d_end=d_e.data_ptr() if d_e is not None else 0, stop=stop, skip=skip, **kw)
    return r, read_back(r, R)


def check_bytes(want, data, byte_off, ctx=None):
    """the bytes are what the existing decode entry makes of the restatement's ids"""
    ref, ref_off = enc()._core_bpe.decode_batch_packed(want.tokens, want.tok_off)
    assert bytes(data) == ref and np.array_equal(byte_off, ref_off), ctx


def check(m, begin=None, end=None, stop=(), skip=(), want=None, ctx=None, **kw):
    want = rule(m, begin, end, stop, skip, **kw) if want is None else want
    _, (got, data, byte_off) = rows_device(m, begin, end, stop, skip, **kw)
    dr.same(got, want, ctx)
    check_bytes(want, data, byte_off, ctx)
    return want


# ---------------------------------------------------------------- shapes
@functools.lru_cache(maxsize=None)
def shape_case(R, W):
    """values that fit all three dtypes, begin, end, and the restatement's result -- computed once, shared by the dtypes and the layouts"""
    rng = np.random.default_rng(R * 10007 + W)
    vals, begin = dr.generation_matrix(rng, R, W, 100000, stops=(EOT, 13), pad=PAD, specials=(FIM, EOP))
    end = np.minimum(begin + rng.integers(0, W + 1, size=R), W).astype(np.uint32)
    if R:
        end[0] = W
    kw = dict(stop=(EOT, 13), skip=(PAD, 7))
    return vals, begin, end, rule(vals, begin, end, **kw), rule(vals, None, None, skip_special=True, keep_stop=True, **kw), kw


@pytest.mark.parametrize("dtype", dr.DTYPES)
@pytest.mark.parametrize("R", (0, 1, 3, 300))
def test_shapes_around_the_tile(dtype, R):
    """W in {0, 1, 7, 8, 9, T - 1, T, T + 1, 2T + 1}, rows ld == W and ld == W + 3 apart, the latter from an odd element on: row bases at
    every alignment, lanes that load 16 bytes at a time and lanes that cannot"""
    for W in (0, 1, 7, 8, 9, T - 1, T, T + 1, 2 * T + 1):
        vals, begin, end, want, want_all, kw = shape_case(R, W)
        for ld_extra, shift in ((0, 0), (3, 1)):
            m = dr.held(vals, dtype, ld_extra, shift)
            check(m, begin, end, want=want, ctx=(W, ld_extra), **kw)
            check(m, want=want_all, ctx=(W, ld_extra, "all"), skip_special=True, keep_stop=True, **kw)


# ---------------------------------------------------------------- the cases of the rule
@pytest.mark.parametrize("keep_stop", (False, True))
def test_stop_positions(keep_stop):
    """A stop at begin, at end - 1, at columns T - 1 and T, before begin and at end (both ignored); two stops in one row, in different tiles"""
    W = 2 * T + 1
    base = np.arange(1000, 1000 + W)
    cases = ((4, W - 3, [4]), (4, W - 3, [W - 4]), (0, W, [T - 1]), (0, W, [T]), (4, W - 3, [2]), (4, W - 3, [W - 3]), (0, W, [T - 5, T + 9]), (0, W, [T + 9, 2 * T]),
             (4, W - 3, [1, T + 1]), (9, 9, [9]))
    m = np.stack([base] * len(cases)).astype(np.int64)
    for r, (_, _, at) in enumerate(cases):
        m[r, at] = EOT
    begin, end = [c[0] for c in cases], [c[1] for c in cases]
    want = check(m, begin, end, stop=[EOT], keep_stop=keep_stop)
    assert want.stop_col.tolist() == [min([c for c in at if b <= c < e], default=e) for b, e, at in cases]


def test_a_stop_id_that_is_also_a_skip_id():
    m = np.array([[1, 2, EOT, 3, 4]] * 2, np.int32)
    assert check(m, stop=[EOT], skip=[EOT]).tokens.tolist() == [1, 2] * 2
    assert check(m, stop=[EOT], skip=[EOT], keep_stop=True).tokens.tolist() == [1, 2] * 2  # kept by the stop rule, then skipped
    assert check(m, stop=[EOT], keep_stop=True).tokens.tolist() == [1, 2, EOT] * 2
    assert check(m, stop=[EOT], keep_stop=True, skip_special=True).tokens.tolist() == [1, 2] * 2


def test_rows_with_begin_equal_to_end_and_nothing_kept():
    rng = np.random.default_rng(3)
    m = rng.integers(0, 100000, size=(5, 40)).astype(np.int64)
    want = check(m, [3, 40, 0, 17, 9], [3, 40, 0, 17, 9])
    assert len(want.tokens) == 0 and want.tok_off.tolist() == [0] * 6
    assert len(check(np.full((4, T + 5), PAD, np.uint32), skip=[PAD]).tokens) == 0  # every id skipped: K == 0
    assert len(check(np.full((4, 37), FIM, np.int32), skip_special=True).tokens) == 0


def test_skip_special():
    rng = np.random.default_rng(4)
    vals, begin = dr.generation_matrix(rng, 20, 300, 100000, stops=(EOT,), pad=EOT, specials=tuple(h.SPECIALS[NAME].values()))
    m = dr.held(vals, np.int64, 3, 1)
    want = check(m, begin, None, stop=[EOT], skip_special=True)
    assert not set(want.tokens.tolist()) & set(h.SPECIALS[NAME].values())
    assert set(check(m, begin, None, stop=[EOT]).tokens.tolist()) & set(h.SPECIALS[NAME].values())


def test_invalid_ids_and_the_previous_result():
    """Behind the stop and in skip_ids an id without a token is accepted; in the live range the first one in row-major order is named -- a
    later row's earlier column loses to an earlier row's later column -- and the result of the call before stays whole"""
    rng = np.random.default_rng(7)
    vals = rng.integers(0, 100000, size=(4, T + 50))
    vals[:, T + 10] = EOT
    vals[:, T + 11:] = HOLE  # behind the stop
    vals[:, 0] = BEYOND  # before begin
    vals[1, 3] = PAD  # in skip_ids
    m = vals.astype(np.int64)
    begin = [1] * 4
    r0, (got0, data0, off0) = rows_device(m, begin, None, [EOT], [PAD])
    dr.same(got0, rule(m, begin, None, [EOT], [PAD]))
    m[3, 2] = HOLE
    m[2, T + 3] = BEYOND
    m[2, 9] = HOLE
    with pytest.raises(KeyError, match=rf"Invalid token for decoding: {HOLE} \(row 2, column 9\)"):
        rows_device(m, begin, None, [EOT], [PAD])
    with pytest.raises(dr.InvalidToken, match="row 2, column 9"):
        rule(m, begin, None, [EOT], [PAD])
    again, data1, off1 = read_back(r0, 4)  # the buffers of the accepted call, read again
    dr.same(again, got0)
    assert np.array_equal(data1, data0) and np.array_equal(off1, off0)
    with pytest.raises(KeyError, match=rf"Invalid token for decoding: {BEYOND} \(row 2, column {T + 3}\)"):
        rows_device(m, [1, 1, 10, 3], None, [EOT], [PAD])
    check(m, [1, 1, T + 4, 3], None, [EOT], [PAD])


def test_values_that_are_no_uint32():
    for dtype, bad in ((np.int64, -1), (np.int64, (1 << 32) + 5), (np.int32, -100)):
        m = np.full((3, 20), 6, dtype)
        m[1, 9] = bad
        low = int(np.array(bad, np.int64).view(np.uint64)) & 0xFFFFFFFF
        with pytest.raises(KeyError, match=rf"Invalid token for decoding: {bad} \(row 1, column 9\)"):
            rows_device(m, stop=[low], skip=[low])  # (its low word is in both lists: the element is in neither)
        assert check(m, None, [20, 9, 20]).n_kept.tolist() == [20, 9, 20]  # outside the live range it is not judged
        m[1, 3] = 7
        assert check(m, stop=[7]).stop_col.tolist() == [20, 3, 20]


def test_begin_and_end_that_offend():
    rng = np.random.default_rng(9)
    m = rng.integers(0, 100000, size=(6, 40)).astype(np.int32)
    r0, (got0, _, _) = rows_device(m)
    for begin, end, row in (([0, 0, 5, 0, 0, 0], [40, 40, 4, 40, 40, 40], 2), (None, [40, 41, 40, 40, 40, 99], 1), ([41] * 6, None, 0)):
        with pytest.raises(ValueError, match=rf"row {row} does not"):
            rows_device(m, begin, end, [EOT])
        with pytest.raises(dr.Refused) as bad:
            rule(m, begin, end, [EOT])
        assert bad.value.row == row
    dr.same(read_back(r0, 6)[0], got0)  # the previous result is whole
    with pytest.raises(ValueError, match="row 1 does not"):
        rows_device(np.zeros((3, 0), np.int64), [0, 1, 0], None)


def test_refusals_of_the_spec():
    core = enc()._core_bpe
    m = np.zeros((2, 8), np.int64)
    with pytest.raises(ValueError, match="more than 16 stop ids"):
        core.decode_rows_packed(m, stop=range(17))
    with pytest.raises(ValueError, match="more than 16 skip ids"):
        core.decode_rows_packed(m, skip=range(17))
    with pytest.raises(ValueError):
        core.decode_rows_packed(m.astype(np.uint16))
    with pytest.raises(ValueError, match="column stride"):
        core.decode_rows_packed(m[:, ::2])
    d = to_device(m)
    with pytest.raises(ValueError, match="ld must be at least the width"):
        core.decode_rows_device(d.data_ptr(), 2, 8, 7)


# ---------------------------------------------------------------- the entries
@pytest.mark.parametrize("dtype", dr.DTYPES)
def test_device_entry_and_host_entry_agree(dtype):
    vals, begin, end, want, _, kw = shape_case(300, T + 1)
    m = dr.held(vals, dtype, 3, 1)
    _, (got, data, byte_off) = rows_device(m, begin, end, **kw)
    host = enc()._core_bpe.decode_rows_packed(m, begin=begin, end=end, **kw)
    dr.same(dr.Rows(host.tokens, host.tok_off, host.n_kept, host.stop_col), got)
    dr.same(got, want)
    assert np.array_equal(host.data, data) and np.array_equal(host.byte_off, byte_off)
    empty = enc()._core_bpe.decode_rows_packed(np.zeros((0, 5), dtype))
    assert len(empty.tokens) == 0 and empty.tok_off.tolist() == [0] and empty.byte_off.tolist() == [0] and len(empty.data) == 0


def trimmed(row, begin, end, stop, skip, specials=()):
    """what a caller's host loop does to one row"""
    row = row[begin:end]
    for i, t in enumerate(row):
        if t in stop:
            row = row[:i]
            break
    return [t for t in row if t not in skip and t not in specials]


def test_encoding_decode_rows_equals_the_host_loop():
    import torch

    e = enc()
    texts = ["hello world", "", "The quick brown fox's 12345 jumps\n\n  over\tthe lazy dog. 中文テキスト 😀", "x" * 300, "DON'T STOP  \r\n believing ..."] * 3
    rows = [e.encode_ordinary(t) for t in texts]
    W, prompt = max(map(len, rows)) + 6, 3
    m = np.full((len(rows), W), PAD, np.int64)
    for r, ids in enumerate(rows):
        m[r, :prompt] = e.encode_ordinary("Q:")[0]
        m[r, prompt: prompt + len(ids)] = ids
        m[r, prompt + len(ids)] = EOT
        if len(ids) > 2:
            m[r, prompt + 1] = FIM  # a special token in the text
    specials = set(e._special_tokens.values())
    want = [e.decode(trimmed(row, prompt, W, {EOT}, {PAD}, specials)) for row in m.tolist()]
    assert e.decode_rows(m[:, prompt:], stop=["<|endoftext|>"], skip=[PAD], skip_special=True) == want
    assert e.decode_rows(m, begin=[prompt] * len(rows), stop=EOT, skip=[PAD], skip_special=True) == want
    assert e.decode_rows(torch.from_numpy(m).cuda()[:, prompt:], stop=[EOT], skip=[PAD], skip_special=True) == want  # a strided slice, by pointer
    assert e.decode_rows(torch.from_numpy(m.astype(np.int32)).cuda(), begin=np.full(len(rows), prompt), stop=[EOT], skip=[PAD], skip_special=True) == want
    raw = [e.decode_bytes(trimmed(row, prompt, W, {EOT}, {PAD})) for row in m.tolist()]
    assert e.decode_rows_bytes(m[:, prompt:], stop=[EOT], skip=[PAD]) == raw
    plain = e.decode_rows(np.array([rows[2]], np.uint32))  # the defaults: nothing stops a row, nothing is skipped
    assert plain == [texts[2]] == e.decode_batch([rows[2]])
    packed = e.decode_rows_packed(m[:, prompt:], stop=[EOT], skip=[PAD], keep_stop=True)
    assert packed.n_kept.tolist() == [len(trimmed(row, prompt, W, {EOT}, {PAD})) + 1 for row in m.tolist()]
    assert (packed.stop_col < W - prompt).all()
