"""The row kernel of the streaming decode (tk_stream.h) on the CPU: tests/hostsim/stream_sim.cpp compiles the plain C++ it is made of
(tiktoken_amd/csrc/tk_stream_rule.h and the three rule headers it builds on) for the host and drives it the way the kernel does -- a
wavefront of 64 lanes per row, a column per lane, the lanes of the search and of the repair in ascending, descending and shuffled order,
a row buffer that refuses every index outside the bytes the row holds, a writer that wants every emitted byte stored exactly once.
Compared step by step with the rule of include/tiktoken_amd.h restated in Python (tests/stream_ref.py), and the concatenation of what a
row emitted with the one-shot reference over all the columns it was fed."""
import ctypes
import struct

import numpy as np
import pytest

import decode_rows_ref as D
import helpers as h
import stream_ref as R

SPEC = 0x80000000
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = h.build_sim("libstream_sim.so", ("stream_sim.cpp", "tk_stream_rule.h", "tk_decode_rows_rule.h", "tk_stop_text_rule.h", "tk_utf8_repair_rule.h", "tk_decode_rule.h",
                                             "tk_rows_rule.h", "tk_device.h", "tk_common.h"), ("-Wall", "-Werror"))
        vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
        L.stream_slot_bytes.restype = u64
        L.stream_shape.restype = ctypes.c_int32
        L.stream_shape.argtypes = [u64, u64, u64, u32]
        L.stream_row.restype = ctypes.c_int64
        L.stream_row.argtypes = [u32, u32, vp, u32, u32, u32, u32, u32, vp, u32, vp, vp, u32, vp, vp, vp, vp, u32, u32, u32, u32, u32, vp, vp, vp]
        _lib = L
    return _lib


# ---------------------------------------------------------------- a small vocabulary: id == byte below 256, a few longer tokens, holes, two specials
from stream_ref import HOLE, N_IDS, PAD, SPECIALS, TOKENS, token_bytes  # noqa: E402


class Table:
    def __init__(self):
        blob, spec, pairs = bytearray(), bytearray(), np.zeros((N_IDS, 2), np.uint32)
        for t in range(N_IDS):
            b = token_bytes(t)
            if b is None:
                continue
            dst = spec if t in SPECIALS else blob
            pairs[t] = (len(dst) | (SPEC if t in SPECIALS else 0), len(b))
            dst += b
        self.pairs, self.blob, self.spec = pairs, np.frombuffer(bytes(blob) + b"\0" * 16, np.uint8), np.frombuffer(bytes(spec) + b"\0" * 16, np.uint8)


TABLE = Table()
SLOT = struct.Struct("<IIIIQQQ72s")
MAX_TOK = 40


class SimStream:
    """R slots driven through stream_row, a row at a time; a refused call leaves every slot as it was"""

    def __init__(self, n_rows, stops=(), *, w_max=1, stop=(), skip=(), skip_special=False, keep_stop=False, keep_stop_text=False, mode=R.REPLACE, order=0):
        assert lib().stream_slot_bytes() == SLOT.size and lib().stream_shape(n_rows, w_max, MAX_TOK, mode) == 0
        self.R, self.mode, self.order, self.cap = n_rows, mode, order, 66 + w_max * MAX_TOK
        self.flags = (D.KEEP_STOP if keep_stop else 0) | (D.SKIP_SPECIAL if skip_special else 0)
        self.stop, self.skip = np.array(list(stop) + [0], np.uint32), np.array(list(skip) + [0], np.uint32)
        self.n_stop, self.n_skip = len(stop), len(skip)
        self.stops = [bytes(s) for s in stops]
        self.blob, self.off = R.S.stop_arrays(self.stops)
        self.stop_flags = 1 if keep_stop_text else 0
        self.slots = [SLOT.pack(0, R.NO_HIT, 0, 0, 0, 0, 0, b"")] * n_rows

    def _call(self, op, ids, begin, end, chosen):
        W = ids.shape[1] if ids is not None else 0
        new, out, bad_row, bad_id = [], [], None, None
        for r in range(self.R):
            slot = ctypes.create_string_buffer(self.slots[r], SLOT.size)
            text = np.zeros(3 * self.cap + 16, np.uint8)
            res = np.zeros(3, np.uint64)
            row = np.ascontiguousarray(ids[r], np.int64) if W else np.zeros(1, np.int64)
            b, e = (0 if begin is None else int(begin[r])), (W if end is None else int(end[r]))
            rc = lib().stream_row(op, 1 if chosen is None or r in chosen else 0, row.ctypes.data, W, b, e, self.flags, self.n_stop, self.stop.ctypes.data, self.n_skip,
                                  self.skip.ctypes.data, TABLE.pairs.ctypes.data, N_IDS, TABLE.blob.ctypes.data, TABLE.spec.ctypes.data, self.blob.ctypes.data,
                                  self.off.ctypes.data, len(self.stops), self.stop_flags, self.mode, self.cap, self.order, slot, text.ctypes.data, res.ctypes.data)
            if rc == 100:
                bad_row = r if bad_row is None else bad_row
            elif 200 <= rc < 300:
                bad_id = (r, rc - 200) if bad_id is None else bad_id
            else:
                assert rc == 0, (rc, r)
            new.append(slot.raw)
            out.append(bytes(text[: int(res[0])]))
        if bad_row is not None:
            raise D.Refused("begin <= end <= W", bad_row)
        if bad_id is not None:
            raise D.InvalidToken(int(ids[bad_id]), *bad_id)
        self.slots = new
        return out

    def step(self, ids, begin=None, end=None):
        return self._call(0, ids, begin, end, None)

    def flush(self, rows=None):
        return self._call(1, None, None, None, None if rows is None else set(rows))

    def reset(self, rows=None):
        self._call(2, None, None, None, None if rows is None else set(rows))

    def view(self):
        f = [SLOT.unpack(s) for s in self.slots]
        return dict(state=[x[0] for x in f], hit=[x[1] for x in f], tail=[x[7][: x[2]] for x in f], n_kept=[x[4] for x in f], n_text=[x[5] for x in f], n_chars=[x[6] for x in f])


def ref_view(s):
    return dict(state=s.state, hit=s.hit, tail=s.tail, n_kept=s.n_kept, n_text=s.n_text, n_chars=s.n_chars)


def pair(n_rows, stops=(), order=0, **kw):
    return SimStream(n_rows, stops, order=order, **kw), R.Stream(n_rows, stops, token_bytes=token_bytes, special=lambda t: t in SPECIALS, **kw)


def feed(sim, ref, steps, ctx=None):
    """every step through both; (the pieces each row emitted, per step)"""
    for k, (ids, begin, end) in enumerate(steps):
        ids = np.asarray(ids, np.int64)
        got, want = sim.step(ids, begin, end), ref.step(ids, begin, end)
        assert got == want, (ctx, k, got, want)
        assert sim.view() == ref_view(ref), (ctx, k)


def finish(sim, ref, ctx=None):
    assert sim.flush() == ref.flush(), ctx
    assert sim.view() == ref_view(ref), ctx
    for r in range(ref.R):
        text, hit = ref.one_shot(r)
        assert ref.emitted[r] == text and ref.hit[r] == hit, (ctx, r, ref.emitted[r], text)  # the concatenation property, of the rule itself


def one_per_step(ids):
    return [(np.array([[t]]), None, None) for t in ids]


MODES = (R.REPLACE, R.IGNORE, R.BYTES)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order", (0, 1, 2))
def test_a_char_spelled_by_byte_tokens(mode, order):
    smile = list("😀".encode())
    sim, ref = pair(1, mode=mode, order=order)
    for k, t in enumerate(smile):
        out = sim.step(np.array([[t]], np.int64))
        assert ref.step(np.array([[t]], np.int64)) == out
        assert out == ([b""] if k < 3 and mode != R.BYTES else ["😀".encode()] if mode != R.BYTES else [bytes([t])])
    sim, ref = pair(1, mode=mode, order=order)  # broken by an ASCII byte after two bytes
    feed(sim, ref, one_per_step(smile[:2] + [0x41]))
    assert ref.emitted[0] == {R.REPLACE: R.U.FFFD + b"A", R.IGNORE: b"A", R.BYTES: bytes(smile[:2]) + b"A"}[mode]
    sim, ref = pair(1, mode=mode, order=order)  # left unfinished at the flush
    feed(sim, ref, one_per_step(smile[:3]))
    finish(sim, ref)
    assert ref.emitted[0] == {R.REPLACE: R.U.FFFD, R.IGNORE: b"", R.BYTES: bytes(smile[:3])}[mode] and ref.state == [R.FLUSHED]


@pytest.mark.parametrize("keep", (False, True))
@pytest.mark.parametrize("order", (0, 2))
def test_stop_strings_across_steps(keep, order):
    for name, (stops, ids) in R.stop_cases().items():
        stops = [s.encode() if isinstance(s, str) else s for s in stops]
        for mode in MODES:
            sim, ref = pair(1, stops, keep_stop_text=keep, mode=mode, order=order)
            feed(sim, ref, one_per_step(ids), name)
            finish(sim, ref, name)
            if name == "the hit beats a lower, longer candidate":
                assert ref.hit == [0] and ref.emitted[0] == (b"xabc" if keep else b"xa")
            if name == "a prefix that breaks":
                assert ref.state == [R.FLUSHED] and ref.emitted[0] == b"a\n\nQuest! more"


def test_stop_ids_skips_and_ended_rows():
    for keep_stop in (False, True):
        for mode in MODES:
            kw = dict(stop=[300], skip=[PAD, 7], keep_stop=keep_stop, mode=mode, w_max=3)
            sim, ref = pair(3, [b"\n\n"], **kw)
            steps = [
                ([[300, PAD, PAD], [97, 10, 7], [0xE4, 0xB8, 98]], None, None),  # a stop id in column 0; a stop string across a skipped id ...
                ([[HOLE, HOLE, HOLE], [10, 99, 100], [99, 100, 300]], None, None),  # ... completes; an ended row's ids are not judged; a stop id in the last column
                ([[HOLE, -1, 2**40], [HOLE, HOLE, HOLE], [PAD, HOLE, -5]], None, None),  # every row has ended: silent
            ]
            feed(sim, ref, steps, (keep_stop, mode))
            assert ref.state == [R.STOP_ID, R.STOP_TEXT, R.STOP_ID]
            finish(sim, ref)
    sim, ref = pair(2, [], skip_special=True, w_max=2)
    feed(sim, ref, [([[104, 301], [300, 105]], None, None)])
    assert ref.emitted == [b"h", b"i"]


def test_begin_and_end_per_row():
    sim, ref = pair(3, [b"\n\n"], w_max=3)
    feed(sim, ref, [([[HOLE, HOLE, HOLE], [97, HOLE, HOLE], [98, 10, 10]], None, [0, 1, 3]), ([[99, 10, 100], [10, 10, 7], [1, 2, 3]], [1, 0, 3], [2, 2, 3])])
    assert ref.fed == [[10], [97, 10, 10], [98, 10, 10]]
    finish(sim, ref)


def test_reset_and_partial_flush():
    sim, ref = pair(3, [b"\n\nQuestion:"])
    feed(sim, ref, [([[0xF0], [10], [104]], None, None), ([[0x9F], [10], [105]], None, None)])
    assert ref.tail == [b"\xf0\x9f", b"\n\n", b""]
    sim.reset([0, 1]), ref.reset([0, 1])
    assert sim.view() == ref_view(ref) and ref.tail == [b"", b"", b""]
    feed(sim, ref, [([[0x98], [81], [33]], None, None)])  # nothing of the old requests leaks into the new ones
    assert ref.emitted == [R.U.FFFD, b"Q", b"hi!"]
    assert sim.flush([2]) == ref.flush([2]) and ref.state == [R.LIVE, R.LIVE, R.FLUSHED]
    feed(sim, ref, [([[65], [66], [67]], None, None)])
    finish(sim, ref)


def test_refusals_leave_the_slots_whole():
    sim, ref = pair(2, [b"\n\n"], w_max=2)
    feed(sim, ref, [([[97, 10], [0xC3, 0xA9]], None, None)])
    before = sim.view()
    for ids, begin, end, exc in (([[98, HOLE], [99, 100]], None, None, D.InvalidToken), ([[98, 99], [99, 100]], [2, 0], [1, 2], D.Refused),
                                 ([[98, 99], [99, 100]], None, [2, 3], D.Refused)):
        with pytest.raises(exc) as got:
            sim.step(np.array(ids, np.int64), begin, end)
        with pytest.raises(exc) as want:
            ref.step(np.array(ids, np.int64), begin, end)
        assert str(got.value) == str(want.value) and sim.view() == before == ref_view(ref)
    feed(sim, ref, [([[98, 10], [99, 100]], None, None)])
    finish(sim, ref)


def test_figures_a_stream_refuses():
    shape = lib().stream_shape
    assert shape(4096, 4, 128, 0) == 0 and shape(0, 1, 1, 2) == 0 and shape(1, 64, 248, 0) == 0
    assert shape(1, 0, 10, 0) == 1 and shape(1, 65, 10, 0) == 1 and shape(65537, 1, 10, 0) == 2 and shape(1, 64, 249, 0) == 3 and shape(1, 1, 16000, 1) == 3
    assert shape(65536, 64, 248, 0) == 0 and shape(1, 1, 10, 3) == 5


@pytest.mark.parametrize("mode", MODES)
def test_random_streams(mode):
    """rows over a small alphabet of tokens in which the stop strings occur often, chopped into steps of 1 .. 4 columns, every lane order"""
    rng = np.random.default_rng(0x57E4 + mode)
    alphabet = [10, 10, 46, 97, 98, 99, 0xC3, 0xA9, 0xF0, 0x9F, 0x98, 0x80, 0xE4, 256, 257, 258, 260, 261, 262, 263, 264, 7, PAD, 301]
    for trial in range(60):
        n_rows = int(rng.integers(1, 6))
        stops = [[b"\n\n", b"Question:", b"abc", b"ab", "é😀".encode(), b"\x98", b".\n\nab"][i] for i in rng.choice(7, size=int(rng.integers(0, 5)), replace=False)]
        kw = dict(stop=[300] if trial % 2 else [], skip=[PAD, 7], skip_special=bool(trial % 3 == 0), keep_stop=bool(trial % 5 == 0), keep_stop_text=bool(trial % 2), mode=mode, w_max=4)
        sim, ref = pair(n_rows, stops, order=trial % 3, **kw)
        for _ in range(int(rng.integers(1, 30))):
            W = int(rng.integers(0, 5))
            ids = rng.choice(alphabet, size=(n_rows, W)).astype(np.int64)
            if W and rng.random() < 0.1:
                ids[int(rng.integers(0, n_rows)), int(rng.integers(0, W))] = 300
            end = rng.integers(0, W + 1, size=n_rows) if rng.random() < 0.3 else None
            begin = np.minimum(rng.integers(0, W + 1, size=n_rows), end if end is not None else W) if rng.random() < 0.3 else None
            feed(sim, ref, [(ids, begin, end)], trial)
            if rng.random() < 0.05:
                rows = rng.choice(n_rows, size=int(rng.integers(1, n_rows + 1)), replace=False).tolist()
                sim.reset(rows), ref.reset(rows)
        finish(sim, ref, trial)


# ---------------------------------------------------------------- steps as wide as the wavefront, rows that emit in several turns, tails at the limit
ORDERS = (0, 1, 2)


@pytest.mark.parametrize("keep_stop", (False, True))
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("mode", MODES)
def test_full_width_steps(mode, order, keep_stop):
    kw, steps = R.full_width_steps()
    stops = kw.pop("stops")
    assert sorted(len(s[0][0]) for s in steps) == [32, 33, 63, 64, 64]
    seen = R.coverage(R.Stream(9, stops, token_bytes=token_bytes, special=lambda t: t in SPECIALS, keep_stop=keep_stop, mode=mode, **kw), steps)
    assert seen["begins"] >= set(R.EDGES) and seen["ends"] >= set(R.EDGES) and seen["stop_cols"] >= {31, 32, 63} and seen["skipped"] == {False, True}, seen
    assert seen["state"].count(R.STOP_ID) == 6 and seen["state"][8] == R.STOP_TEXT, seen
    sim, ref = pair(9, stops, order=order, keep_stop=keep_stop, mode=mode, **kw)
    feed(sim, ref, steps, (mode, order, keep_stop))
    assert len(set(ref.emitted)) == 9  # (no two rows alike)
    finish(sim, ref)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("mode", MODES)
def test_more_than_1024_bytes_emitted_in_one_call(mode, order):
    stops, steps = R.long_emit_steps()
    sim, ref = pair(5, stops, order=order, stop=[300], mode=mode, w_max=64)
    feed(sim, ref, steps[:1])
    assert ref.tail == [b"", b"\n", b"", b"", b""]
    raw = [ref.tail[r] + b"".join(token_bytes(t) for t in steps[1][0][r].tolist()) for r in range(5)]
    assert all(len(b) > 2048 for b in raw) and len(raw[1]) == 2561 and raw[2] == b"\x80" * 2560
    assert all(R.straddles(raw[r], 1024) and R.straddles(raw[r], 2048) for r in (3, 4)) and raw[3][1022:1025] == "文".encode() and raw[4][2046:2050] == "😀".encode()
    got, want = sim.step(steps[1][0]), ref.step(steps[1][0])
    assert want == [{R.REPLACE: R.U.FFFD * 2560, R.IGNORE: b"", R.BYTES: raw[2]}[mode] if r == 2 else raw[r] for r in range(5)]  # (the rule, before the simulation is asked)
    assert got == want and sim.view() == ref_view(ref)
    assert ref.tail == [b""] * 5
    got, want = sim.step(*steps[2]), ref.step(*steps[2])
    lead = {R.REPLACE: R.U.FFFD, R.IGNORE: b"", R.BYTES: b"\xf0"}[mode]
    assert len(want[0]) == 1023 + len(lead) and want[0].endswith(b"ab" + lead) and want[1] == want[0][:1023] + {R.REPLACE: R.U.FFFD, R.IGNORE: b"", R.BYTES: b"\xf0\x9f"}[mode]
    assert got == want and sim.view() == ref_view(ref)
    assert ref.state == [R.STOP_ID, R.STOP_ID, R.LIVE, R.LIVE, R.LIVE] and ref.tail[2:] == ([b"\xf0", b"\xe4", b"\xf0"] if mode != R.BYTES else [b""] * 3)
    finish(sim, ref)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("mode", MODES)
def test_tails_at_the_hold_limit(mode, order):
    longest = set()
    for name, (ids, held, hit) in R.hold_cases().items():
        for keep in (False, True):
            steps = R.hold_steps(ids)
            sim, ref = pair(1, [R.STOP64, b"\n\n"], order=order, keep_stop_text=keep, mode=mode, w_max=max(s[0].shape[1] for s in steps))
            most = 0
            for k, s in enumerate(steps):
                feed(sim, ref, [s], (name, k))
                most = max(most, len(ref.tail[0]))
            assert most == (held if mode != R.BYTES else 63), (name, most)  # (the case is void unless the rule's own tail gets there)
            longest.add(most)
            assert ref.state == [R.STOP_TEXT if hit else R.LIVE] and ref.hit == [0 if hit else R.NO_HIT], name
            finish(sim, ref, name)
    assert longest == ({63, 64, 65, R.HOLD} if mode != R.BYTES else {63})


WIDE_ALPHABET = [10, 10, 46, 97, 98, 99, 0xC3, 0xA9, 0xF0, 0x9F, 0x98, 0x80, 0xE4, 256, 257, 258, 260, 261, 262, 263, 264, 7, PAD, 301, R.X40, R.X40, R.BAD40, R.LEAD3, R.HALF_STOP,
                 0xB1, 0xB2]
LONG_ALPHABET = [R.X40] * 12 + [R.BAD40] * 4 + [260, 261, 264, 0xF0, 0xC3, 0xE4, 97, 46, 32, 7, PAD, 301, R.HALF_STOP, 0xB1]  # (every third trial: rows that live long and emit much)


@pytest.mark.parametrize("mode", MODES)
def test_random_wide_streams(mode):
    """as test_random_streams, in steps of 0 .. 64 columns over an alphabet with the 40-byte tokens and the pieces of the 64-byte stop string"""
    rng = np.random.default_rng(0x51DE + mode)
    turns = []
    for trial in range(40):
        n_rows = int(rng.integers(1, 6))
        stops = [[b"\n\n", b"Question:", b"abc", b"ab", "é😀".encode(), b"\x98", b".\n\nab", R.STOP64, R.STOP64[:33]][i] for i in rng.choice(9, size=int(rng.integers(0, 5)), replace=False)]
        kw = dict(stop=[300] if trial % 2 else [], skip=[PAD, 7], skip_special=bool(trial % 3 == 0), keep_stop=bool(trial % 5 == 0), keep_stop_text=bool(trial % 2), mode=mode, w_max=64)
        sim, ref = pair(n_rows, stops, order=trial % 3, **kw)
        for _ in range(int(rng.integers(1, 12))):
            W = int(rng.integers(0, 65))
            ids = rng.choice(LONG_ALPHABET if trial % 3 == 1 else WIDE_ALPHABET, size=(n_rows, W)).astype(np.int64)
            if W and rng.random() < 0.3:
                ids[int(rng.integers(0, n_rows)), int(rng.integers(0, W))] = 300
            end = rng.integers(0, W + 1, size=n_rows) if rng.random() < 0.3 else None
            begin = np.minimum(rng.integers(0, W + 1, size=n_rows), end if end is not None else W) if rng.random() < 0.3 else None
            before = list(ref.n_text)
            feed(sim, ref, [(ids, begin, end)], trial)
            turns.append(max(a - b for a, b in zip(ref.n_text, before)))
            if rng.random() < 0.1:
                rows = rng.choice(n_rows, size=int(rng.integers(1, n_rows + 1)), replace=False).tolist()
                sim.reset(rows), ref.reset(rows)
        finish(sim, ref, trial)
    if mode != R.IGNORE:
        assert sum(1 for t in turns if t > 1024) >= 3, sorted(turns)[-5:]  # (rows that emit in more than one turn are among them)
