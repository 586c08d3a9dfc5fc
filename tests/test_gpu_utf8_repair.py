"""UTF-8 repair on the GPU (tk_utf8_repair.h): tk_utf8_repair_device, tk_decode_batch_text and the two decode-rows text entries through
CoreBPE and Encoding, against CPython's bytes.decode(..., errors) per document -- text, text_off, char_off -- and, for the count of
replaced units, against the rule of include/tiktoken_amd.h restated in tests/utf8_repair_ref.py."""
import ctypes
import functools

import numpy as np
import pytest

import decode_ref as dr
import helpers as h
import tiktoken_amd as tiktoken
import utf8_repair_ref as R
from tiktoken_amd import _lib

pytestmark = pytest.mark.gpu
MODES = ("replace", "ignore")
MODE_OF = {"replace": R.REPLACE, "ignore": R.IGNORE}
LANE, WAVE, BLOCK = 16, 1024, 4096  # the kernels' geometry in bytes


@functools.lru_cache(maxsize=None)
def enc():
    ranks, specials = dr.edge_vocab()  # the 256 single bytes (id == byte), tokens of 2 .. 300 bytes, special tokens, ids without a token
    return tiktoken.Encoding("edge", pat_str=h.PAT_STR[1], mergeable_ranks=dict(ranks), special_tokens=dict(specials))


def core():
    return enc()._core_bpe


def dev_u8(ptr, n):
    import torch

    return bytes(torch.as_tensor(h._DevArray(ptr, n, "|u1"), device="cuda").cpu().numpy()) if n else b""


class OnDevice:
    """packed text on the device: 16 readable bytes behind it that are not zero"""

    def __init__(self, docs, shift=0):
        import torch

        blob, self.n, off = R.pack(docs)
        self.n_docs = len(docs)
        self.held = torch.from_numpy(np.concatenate([np.zeros(shift, np.uint8), blob])).cuda()
        self.off = torch.from_numpy(off.view(np.int64).copy()).cuda()
        torch.cuda.synchronize()
        self.ptr, self.off_ptr = self.held.data_ptr() + shift, self.off.data_ptr()

    def repair(self, errors):
        return core().utf8_repair_device(self.ptr, self.n, self.off_ptr, self.n_docs, errors)


def read(r, n_docs):
    return dev_u8(r.data, r.n_bytes), h.dev_u64(r.text_off, n_docs + 1), h.dev_u64(r.char_off, n_docs + 1), h.dev_u64(r.repl_off, n_docs + 1)


@functools.lru_cache(maxsize=None)
def expected(key, errors):
    """(text, text_off, char_off) from CPython per document, repl_off from the restatement -- once per input and mode"""
    docs = INPUTS[key]()
    strs = [d.decode("utf-8", errors) for d in docs]
    parts = [s.encode("utf-8") for s in strs]
    text_off = np.zeros(len(docs) + 1, np.uint64)
    char_off = np.zeros(len(docs) + 1, np.uint64)
    if docs:
        text_off[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
        char_off[1:] = np.cumsum([len(s) for s in strs], dtype=np.uint64)
    ref_text, ref_to, _, ro = R.repair_batch(docs, MODE_OF[errors])
    assert ref_text == b"".join(parts) and ref_to == text_off.tolist()  # (the restatement is CPython's decoder on this input)
    return b"".join(parts), text_off, char_off, np.array(ro, np.uint64)


@functools.lru_cache(maxsize=None)
def sliding_docs():
    """the sliding set in one batch: every case starts at a workgroup's first byte (an ASCII document fills up the one before)"""
    docs = []
    for case in R.sliding(LANE, WAVE, BLOCK):  # every case: the lane's, the wavefront's and the workgroup's edge; the last is a document over three workgroups
        docs += case
        docs.append(b"." * ((-sum(map(len, case))) % BLOCK))
    return docs


INPUTS = {"exhaustive": lambda: R.exhaustive(), "sliding": sliding_docs}


@functools.lru_cache(maxsize=None)
def on_device(key):
    return OnDevice(INPUTS[key]())


# ---------------------------------------------------------------- the device primitive
@pytest.mark.parametrize("errors", MODES)
@pytest.mark.parametrize("key", sorted(INPUTS))
def test_device_primitive_against_cpython(key, errors):
    d = on_device(key)
    want = expected(key, errors)
    r = d.repair(errors)
    got = read(r, d.n_docs)
    assert r.n_replaced == int(want[3][-1]) and r.n_replaced > 0 and r.data != d.ptr
    assert got[0] == want[0]
    for g, w, what in zip(got[1:], want[1:], ("text_off", "char_off", "repl_off")):
        assert np.array_equal(g, w), what


def test_fast_path_returns_the_input():
    clean = [("The quick brown fox. 中文😀é " * 300).encode(), b"", b"plain", "żółć".encode() * 2000, b""]
    d = OnDevice(clean)
    for errors in MODES:
        r = d.repair(errors)
        assert r.n_replaced == 0 and r.data == d.ptr and r.text_off == d.off_ptr and r.n_bytes == d.n
        assert h.dev_u64(r.char_off, len(clean) + 1).tolist() == [0] + np.cumsum([len(c.decode()) for c in clean]).tolist()
        assert h.dev_u64(r.repl_off, len(clean) + 1).tolist() == [0] * (len(clean) + 1)
    same_length = OnDevice([b"abc\xf0\x9f\x98"])
    r = same_length.repair("replace")
    assert r.n_replaced == 1 and r.n_bytes == 6 and r.data != same_length.ptr and r.text_off != same_length.off_ptr
    assert dev_u8(r.data, 6) == b"abc" + R.FFFD


def test_refusals_leave_the_previous_result_whole():
    import torch

    docs = [b"ab\x80", b"\xe4\xb8", b"\xad ok"]
    d = OnDevice(docs)
    first = d.repair("replace")
    before = read(first, 3)
    assert before[0] == b"".join(x.decode("utf-8", "replace").encode() for x in docs)

    def refused(**kw):
        a = dict(ptr=d.ptr, n=d.n, off=d.off_ptr, mode=0)
        a.update(kw)
        out, cnt = [ctypes.c_void_p() for _ in range(4)], [ctypes.c_uint64(), ctypes.c_uint64()]
        rc = _lib.lib().tk_utf8_repair_device(core()._h, a["ptr"], a["n"], a["off"], 3, a["mode"], None, ctypes.byref(out[0]), ctypes.byref(cnt[0]), ctypes.byref(out[1]),
                                              ctypes.byref(out[2]), ctypes.byref(out[3]), ctypes.byref(cnt[1]))
        with pytest.raises(ValueError):
            _lib.raise_for(rc)
        got = read(first, 3)
        assert got[0] == before[0] and all(np.array_equal(g, w) for g, w in zip(got[1:], before[1:]))

    def offsets(vals):
        t = torch.tensor(vals, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        return t

    short, descending = offsets([0, 3, 5, d.n - 1]), offsets([0, 5, 3, d.n])
    refused(off=short.data_ptr())  # offsets that do not end at n_bytes
    refused(n=d.n - 1)
    refused(off=descending.data_ptr())
    shifted = OnDevice(docs, shift=4)
    refused(ptr=shifted.ptr)  # a misaligned pointer
    refused(off=d.off_ptr + 4)
    refused(mode=2)  # a bad mode
    with pytest.raises(ValueError, match="decode_batch"):
        d.repair("strict")


def test_degenerate_sizes_of_the_primitive():
    for docs in ([], [b""], [b"", b"", b""]):
        d = OnDevice(docs)
        for errors in MODES:
            r = d.repair(errors)
            assert r.n_bytes == 0 and r.n_replaced == 0
            assert h.dev_u64(r.char_off, len(docs) + 1).tolist() == [0] * (len(docs) + 1)


# ---------------------------------------------------------------- host ids in, host text out
@functools.lru_cache(maxsize=None)
def id_batch():
    table = dr.edge_table()
    rng = np.random.default_rng(0x7E47)
    batch = [dr.random_batch(table, rng, n).tolist() for n in (0, 1, 40, 3000, 0, 0, 700)]
    spelled = [list(t) for t in R.exhaustive()[:: 97]] + [list(b"".join(case)) for case in R.sliding(LANE, 64, 256)[::11]]
    return batch[:3] + spelled[:200] + batch[3:] + spelled[200:] + [[]]


@pytest.mark.parametrize("errors", MODES)
def test_decode_batch_text_packed(errors):
    e = enc()
    batch = id_batch()
    flat, tok_off = e._flatten(batch)
    got = e.decode_batch_text_packed(flat, tok_off, errors=errors)
    strs = [e.decode(d, errors=errors) for d in batch]
    assert bytes(got.data) == "".join(strs).encode()
    assert got.text_off.tolist() == [0] + np.cumsum([len(s.encode()) for s in strs]).tolist()
    assert got.char_off.tolist() == [0] + np.cumsum([len(s) for s in strs]).tolist()
    raw = [e.decode_bytes(d) for d in batch]
    assert got.repl_off.tolist() == R.repair_batch(raw, MODE_OF[errors])[3]
    assert int(got.repl_off[-1]) > 100


def test_decode_batch_text_packed_errors():
    e = enc()
    hole = dr.edge_table().holes[0]
    flat, tok_off = e._flatten([[65, 66], [67, hole, 68]])
    with pytest.raises(KeyError) as ours:
        e.decode_batch_text_packed(flat, tok_off)
    with pytest.raises(KeyError) as theirs:
        e.decode_batch([[65, 66], [67, hole, 68]])
    assert str(ours.value) == str(theirs.value)
    for bad in ("strict", "backslashreplace"):
        with pytest.raises(ValueError, match="decode_batch"):
            e.decode_batch_text_packed(flat[:2], tok_off[:2], errors=bad)
    empty = e.decode_batch_text_packed(np.zeros(0, np.uint32), np.zeros(1, np.uint64))
    assert len(empty.data) == 0 and empty.text_off.tolist() == [0]


# ---------------------------------------------------------------- id matrices
R_ROWS, WIDTH, LD = 37, 200, 264
PAD_ID = 100000  # outside the vocabulary
SKIP_BYTE = 0x98  # a skipped id that is the third byte of U+1F600


@functools.lru_cache(maxsize=None)
def row_case():
    """an int64 matrix of 37 x 200 cut from a wider one: byte-level ids that spell two-, three- and four-byte chars; begin, the stop column,
    end and a skipped id each fall inside a char in some row; the pad id behind the stops is outside the vocabulary"""
    specials = sorted(dr.edge_vocab()[1].values())
    stop, other_special = specials[0], specials[1]
    rng = np.random.default_rng(0xD0C)
    chars = ["é", "中", "😀", "a", "b", " ", "ż", "文", "x"]
    wide = np.full((R_ROWS, LD), PAD_ID, np.int64)
    begin, end = np.zeros(R_ROWS, np.uint32), np.full(R_ROWS, WIDTH, np.uint32)
    for r in range(R_ROWS):
        ids = []
        while len(ids) < LD:
            ids += list(chars[int(rng.integers(len(chars)))].encode())
            if rng.random() < 0.05:
                ids.append(other_special)
        row = np.array(ids[:LD], np.int64)
        k = r % 6
        at = 20 + 3 * r
        smile = list("😀".encode())
        row[at:at + 4] = smile
        if k == 0:
            begin[r] = at + 1 + r % 3  # begin inside the char
        elif k == 1:
            row[at + 2] = stop  # the stop column inside the char
            row[at + 3:] = PAD_ID
        elif k == 2:
            end[r] = at + 1 + r % 3  # end inside it
        elif k == 3:
            pass  # its third byte is the skipped id
        elif k == 4:
            row[at + 4] = stop
            row[at + 5:] = PAD_ID  # a clean stop behind a whole char
        wide[r] = row
    return wide, begin, end, dict(stop=[stop], skip=[PAD_ID, SKIP_BYTE], skip_special=True)


@pytest.mark.parametrize("errors", MODES)
@pytest.mark.parametrize("where", ("numpy", "torch"))
def test_decode_rows_text_packed(where, errors):
    import torch

    e = enc()
    wide, begin, end, kw = row_case()
    m = wide[:, :WIDTH]
    assert m.strides[0] == LD * 8
    want_rows = e.decode_rows(m, begin=begin, end=end, errors=errors, **kw)
    want = e.decode_rows_packed(m, begin=begin, end=end, **kw)
    ids = torch.from_numpy(wide).cuda()[:, :WIDTH] if where == "torch" else m
    got = e.decode_rows_text_packed(ids, begin=begin, end=end, errors=errors, **kw)
    view, off = bytes(got.data), got.byte_off.tolist()
    assert [view[a:b].decode("utf-8", "strict") for a, b in zip(off[:-1], off[1:])] == want_rows
    assert got.char_off.tolist() == [0] + np.cumsum([len(s) for s in want_rows]).tolist()
    raw = [bytes(want.data[int(a):int(b)]) for a, b in zip(want.byte_off[:-1], want.byte_off[1:])]
    repl = R.repair_batch(raw, MODE_OF[errors])[3]
    assert got.repl_off.tolist() == repl and sum(1 for a, b in zip(repl[:-1], repl[1:]) if b > a) >= 20
    for name in ("tokens", "tok_off", "n_kept", "stop_col"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name
    assert np.array_equal(got.text_off, got.byte_off)


def test_decode_rows_text_degenerate_shapes():
    e = enc()
    for shape in ((0, 5), (4, 0), (0, 0)):
        got = e.decode_rows_text_packed(np.zeros(shape, np.int64))
        assert len(got.data) == 0 and got.byte_off.tolist() == [0] * (shape[0] + 1) and got.char_off.tolist() == [0] * (shape[0] + 1)
    got = e.decode_rows_text_packed(np.full((3, 4), PAD_ID, np.int64), skip=[PAD_ID])  # K == 0
    assert len(got.data) == 0 and len(got.tokens) == 0 and got.repl_off.tolist() == [0, 0, 0, 0]
    with pytest.raises(ValueError, match="decode_rows"):
        e.decode_rows_text_packed(np.zeros((2, 2), np.int64), errors="strict")
