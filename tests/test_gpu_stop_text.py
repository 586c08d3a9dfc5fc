"""Stop strings on the GPU (tk_stop_text.h): tk_stop_text_device and the two decode-rows entries that cut at stop strings, through CoreBPE
and Encoding, against the rule of include/tiktoken_amd.h restated in tests/stop_text_ref.py (bytes.find per string, the least (position,
index)); the text entries also against bytes.decode(errors) of the cut bytes."""
import ctypes
import functools

import numpy as np
import pytest

import decode_ref as dr
import helpers as h
import stop_text_ref as S
import tiktoken_amd as tiktoken
from tiktoken_amd import _lib

pytestmark = pytest.mark.gpu
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

        blob, self.n, off = S.pack(docs)
        self.n_docs = len(docs)
        self.held = torch.from_numpy(np.concatenate([np.zeros(shift, np.uint8), blob])).cuda()
        self.off = torch.from_numpy(off.view(np.int64).copy()).cuda()
        torch.cuda.synchronize()
        self.ptr, self.off_ptr = self.held.data_ptr() + shift, self.off.data_ptr()

    def stop(self, stops, keep=False):
        return core().stop_text_device(self.ptr, self.n, self.off_ptr, self.n_docs, stops, keep)


def read(r, n_docs):
    return dev_u8(r.data, r.n_bytes), h.dev_u64(r.text_off, n_docs + 1).tolist(), h.dev_u32(r.hit, n_docs).tolist() if n_docs else []


def check(name, docs, stops, keep):
    d = OnDevice(docs)
    r = d.stop(stops, keep)
    want_text, want_off, want_hit, want_n = S.cut_batch(docs, stops, keep)
    assert (r.n_bytes, r.n_hit) == (len(want_text), want_n), name
    text, off, hit = read(r, len(docs))
    assert hit == want_hit, name
    assert off == want_off, name
    assert text == want_text, name
    assert (r.data == d.ptr and r.text_off == d.off_ptr) == (want_n == 0), name  # no hit anywhere: the caller's own pointers, nothing written


# ---------------------------------------------------------------- the device primitive
@pytest.mark.parametrize("keep", (False, True))
def test_edge_cases(keep):
    """match positions and lengths, document ends and boundaries, which string wins, long and dense documents"""
    for name, docs, stops in S.cases(LANE, WAVE, BLOCK):
        check(name, docs, stops, keep)


@pytest.mark.parametrize("keep", (False, True))
def test_random_batches(keep):
    for name, docs, stops in S.random_cases(0x570B, 60):
        check(name, docs, stops, keep)


def test_no_hit_hands_back_the_callers_pointers():
    docs = [b"The quick brown fox. " * 3000, b"", "中文😀é".encode() * 500, b"\n#\n# Question </s"]
    d = OnDevice(docs)
    for keep in (False, True):
        r = d.stop(["\n\n", "Question:", "</s>", "###"], keep)
        assert r.n_hit == 0 and r.data == d.ptr and r.text_off == d.off_ptr and r.n_bytes == d.n
        assert h.dev_u32(r.hit, len(docs)).tolist() == [S.NO_HIT] * len(docs)


def test_str_and_bytes_stop_text():
    d = OnDevice(["a€b".encode(), b"x\xffy"])
    r = d.stop(["€", b"\xff"])
    assert read(r, 2) == (b"ax", [0, 1, 2], [0, 1])
    r = d.stop("€", True)  # one string, not a list of its chars
    assert read(r, 2) == ("a€".encode() + b"x\xffy", [0, 4, 7], [0, S.NO_HIT])


def test_refusals_leave_the_previous_result_whole():
    import torch

    docs = [b"abSTcd", b"none", b"STx"]
    d = OnDevice(docs)
    first = d.stop([b"ST"])
    before = read(first, 3)
    assert before == (b"abnone", [0, 2, 6, 6], [0, S.NO_HIT, 0])

    def refused(stops=(b"ST",), stop_off=None, **kw):
        a = dict(ptr=d.ptr, n=d.n, off=d.off_ptr, flags=0)
        a.update(kw)
        blob, so = S.stop_arrays(list(stops))
        if stop_off is not None:
            so = np.array(stop_off, np.uint32)
        c = _lib.Stops(len(so) - 1, blob.ctypes.data, so.ctypes.data)
        out, cnt = [ctypes.c_void_p() for _ in range(3)], [ctypes.c_uint64(), ctypes.c_uint64()]
        rc = _lib.lib().tk_stop_text_device(core()._h, a["ptr"], a["n"], a["off"], 3, ctypes.byref(c), a["flags"], None, ctypes.byref(out[0]), ctypes.byref(cnt[0]),
                                            ctypes.byref(out[1]), ctypes.byref(out[2]), ctypes.byref(cnt[1]))
        with pytest.raises(ValueError):
            _lib.raise_for(rc)
        assert read(first, 3) == before

    def offsets(vals):
        t = torch.tensor(vals, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        return t

    refused(stops=[bytes([65 + i]) for i in range(17)])  # 17 strings
    refused(stops=[b"ST", b"", b"x"])  # an empty string
    refused(stops=[b"S" * 65])  # 65 bytes
    refused(stop_off=[0, 2, 1])  # stop offsets that descend
    refused(stop_off=[1, 2])  # ... that do not start at 0
    refused(flags=2)  # an unknown flag
    shifted = OnDevice(docs, shift=4)
    refused(ptr=shifted.ptr)  # a misaligned pointer
    refused(off=d.off_ptr + 4)
    descending, overshoot, short = offsets([0, 10, 6, d.n]), offsets([0, 6, 10, d.n + 5]), offsets([0, 6, 10, d.n - 1])
    refused(off=descending.data_ptr())
    refused(off=overshoot.data_ptr())
    refused(off=short.data_ptr())
    refused(n=d.n - 1)
    with pytest.raises(ValueError, match="document 1"):
        core().stop_text_device(d.ptr, d.n, descending.data_ptr(), 3, [b"ST"])
    assert read(d.stop([b"S" * 64]), 3)[2] == [S.NO_HIT] * 3  # 64 bytes are legal


def test_degenerate_sizes():
    for docs in ([], [b""], [b"", b"", b""]):
        for stops in ([b"ST"], []):
            r = OnDevice(docs).stop(stops)
            assert r.n_bytes == 0 and r.n_hit == 0
            assert h.dev_u32(r.hit, len(docs)).tolist() == [S.NO_HIT] * len(docs) if docs else True


# ---------------------------------------------------------------- id matrices
PAD_ID = 100000  # outside the vocabulary
SKIPPED = 0x07  # a skipped id inside the text
WIDTH, LD = 700, 712


@functools.lru_cache(maxsize=None)
def row_case():
    """(wide int64 matrix, begin, spec arguments, stop strings, the row of each named case)"""
    table = dr.edge_table()
    t300, t3, t4 = table.id_of_len(300), table.id_of_len(3), table.id_of_len(4)
    b300 = table.by_id[t300]
    stop_id = sorted(table.special_ids)[0]
    inside, straddle = b300[100:105], table.by_id[t3][-2:] + table.by_id[t4][:2]
    stops = ["\n\n", "Question:", inside, straddle, "€"]
    rows, begin, names = [], [], {}

    def add(name, ids, b=0):
        names[name] = len(rows)
        rows.append(list(ids))
        begin.append(b)

    add("stop id before stop string", list(b"abc") + [stop_id] + list(b"d\n\nxyz"))
    add("across a skipped id", list(b"ab\n") + [SKIPPED] + list(b"\ncd"))
    add("on a token boundary", list(b"ab\n\nc"))
    add("inside a 300-byte token", list(b"ab") + [t300] + list(b"c"))
    add("straddling two tokens", list(b"a") + [t3, t4] + list(b"c"))
    add("cut at byte 0", list(b"\n\nabc"))
    add("euro behind a char cut by begin", list("é€x€y".encode()), 1)
    add("no stop string", list(b"plain text\n and more") + [t3])
    add("only skipped ids", [SKIPPED, SKIPPED])
    add("later string earlier", list(b"x Question: y\n\n z"))
    rng = np.random.default_rng(0x5707)
    units = [b"a", b"\n", b"word ", "é".encode(), "€".encode(), b"\n\n", b"Question", b":", bytes([SKIPPED])]
    for i in range(30):
        ids = list(b"".join(units[int(k)] for k in rng.integers(0, len(units), int(rng.integers(0, 60)))))
        add(f"random {i}", ids, int(rng.integers(0, 3)) if ids else 0)
    wide = np.full((len(rows), LD), PAD_ID, np.int64)
    for r, ids in enumerate(rows):
        wide[r, :len(ids)] = ids
    return wide, np.array(begin, np.uint32), dict(stop=[stop_id], skip=[PAD_ID, SKIPPED]), stops, names


@functools.lru_cache(maxsize=None)
def row_reference(keep):
    """the existing rows pass, then the Python rule on every row's bytes: (rows result, cut bytes per row, hit, n_tok)"""
    e, table = enc(), dr.edge_table()
    wide, begin, kw, stops, _ = row_case()
    want = e.decode_rows_packed(wide[:, :WIDTH], begin=begin, **kw)
    docs = [bytes(want.data[int(a):int(b)]) for a, b in zip(want.byte_off[:-1], want.byte_off[1:])]
    stops_b = [s.encode() if isinstance(s, str) else s for s in stops]
    cut, hit, n_tok = [], [], []
    for r, doc in enumerate(docs):
        kept, k = S.cut_doc(doc, stops_b, keep)
        cut.append(doc[:kept])
        hit.append(k)
        lens = [table.len_of[int(t)] for t in want.tokens[int(want.tok_off[r]):int(want.tok_off[r + 1])]]
        n_tok.append(S.n_tok_ref(lens, kept))
    return want, cut, hit, n_tok


def held(where):
    import torch

    wide = row_case()[0]
    if where == "numpy int64 slice":
        return wide[:, :WIDTH]
    if where == "numpy uint32":
        return np.ascontiguousarray(wide[:, :WIDTH]).astype(np.uint32)
    if where == "torch int32":
        return torch.from_numpy(wide[:, :WIDTH].astype(np.int32)).cuda()
    assert where == "torch int64 slice"
    return torch.from_numpy(wide).cuda()[:, :WIDTH]


WHERE = ("numpy int64 slice", "numpy uint32", "torch int32", "torch int64 slice")


@pytest.mark.parametrize("errors", ("replace", "ignore", None))
@pytest.mark.parametrize("keep", (False, True))
@pytest.mark.parametrize("where", WHERE)
def test_decode_rows_until_packed(where, keep, errors):
    e = enc()
    _, begin, kw, stops, names = row_case()
    want, cut, hit, n_tok = row_reference(keep)
    got = e.decode_rows_until_packed(held(where), stops, begin=begin, keep_stop_text=keep, errors=errors, **kw)
    view, off = bytes(got.data), got.byte_off.tolist()
    rows = [view[a:b] for a, b in zip(off[:-1], off[1:])]
    assert got.hit.tolist() == hit
    assert got.n_tok.tolist() == n_tok
    for name in ("tokens", "tok_off", "n_kept", "stop_col"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name
    if errors is None:
        assert rows == cut and got.char_off is None and got.repl_off is None
    else:
        strs = [c.decode("utf-8", errors) for c in cut]
        assert rows == [s.encode() for s in strs]
        assert got.char_off.tolist() == [0] + np.cumsum([len(s) for s in strs]).tolist()
    # the cases are what their names say
    R = names
    NO = S.NO_HIT
    assert hit[R["stop id before stop string"]] == NO and cut[R["stop id before stop string"]] == b"abc"
    assert hit[R["across a skipped id"]] == 0 and cut[R["across a skipped id"]] == (b"ab\n\n" if keep else b"ab")
    assert n_tok[R["on a token boundary"]] == (4 if keep else 2)
    assert hit[R["inside a 300-byte token"]] == 2 and n_tok[R["inside a 300-byte token"]] == 3 and len(cut[R["inside a 300-byte token"]]) == 102 + (5 if keep else 0)
    assert hit[R["straddling two tokens"]] == 3 and n_tok[R["straddling two tokens"]] == (3 if keep else 2)
    assert n_tok[R["cut at byte 0"]] == (2 if keep else 0) and cut[R["cut at byte 0"]] == (b"\n\n" if keep else b"")
    assert hit[R["no stop string"]] == NO and n_tok[R["no stop string"]] == int(want.n_kept[R["no stop string"]])
    assert hit[R["later string earlier"]] == 1
    assert sum(1 for k in hit if k != NO) >= 15 and sum(1 for k in hit if k == NO) >= 3


@pytest.mark.parametrize("keep", (False, True))
def test_euro_behind_a_char_cut_by_begin(keep):
    """'replace' text equals decode_rows(...)[r] cut at str.find; char_off agrees with len() of it"""
    e = enc()
    wide, begin, kw, _, names = row_case()
    r = names["euro behind a char cut by begin"]
    m = wide[r:r + 1, :WIDTH]
    whole = e.decode_rows(m, begin=begin[r:r + 1], errors="replace", **kw)[0]
    assert whole == "�€x€y"
    at = whole.find("€")
    want = whole[: at + (1 if keep else 0)]
    got = e.decode_rows_until_packed(m, ["€"], begin=begin[r:r + 1], keep_stop_text=keep, errors="replace", **kw)
    assert bytes(got.data).decode() == want and got.char_off.tolist() == [0, len(want)] and got.repl_off.tolist() == [0, 1]
    assert got.hit.tolist() == [0] and got.n_tok.tolist() == [4 if keep else 1]
    assert e.decode_rows_until(m, "€", begin=begin[r:r + 1], keep_stop_text=keep, **kw) == [want]
    assert e.decode_rows_until_bytes(m, "€", begin=begin[r:r + 1], keep_stop_text=keep, **kw) == [b"\xa9" + ("€".encode() if keep else b"")]


def test_lists_of_str_and_of_bytes():
    e = enc()
    wide, begin, kw, stops, _ = row_case()
    _, cut, _, _ = row_reference(False)
    m = wide[:, :WIDTH]
    assert e.decode_rows_until(m, stops, begin=begin, **kw) == [c.decode("utf-8", "replace") for c in cut]
    assert e.decode_rows_until(m, stops, begin=begin, errors="ignore", **kw) == [c.decode("utf-8", "ignore") for c in cut]
    assert e.decode_rows_until_bytes(m, stops, begin=begin, **kw) == cut
    with pytest.raises(ValueError, match="decode_rows"):
        e.decode_rows_until(m, stops, errors="strict")
    with pytest.raises(ValueError):
        e.decode_rows_until_packed(m, [b""], begin=begin, **kw)
    with pytest.raises(ValueError):
        e.decode_rows_until_packed(m, [b"x"] * 17, begin=begin, **kw)


def test_key_error_is_the_rows_pass_s():
    e = enc()
    hole = dr.edge_table().holes[0]
    m = np.array([[65, 66, 10, 10], [67, hole, 68, 69]], np.int64)
    with pytest.raises(KeyError) as theirs:
        e.decode_rows_packed(m)
    with pytest.raises(KeyError) as ours:
        e.decode_rows_until_packed(m, ["\n\n"])
    assert str(ours.value) == str(theirs.value) and "row 1, column 1" in str(ours.value)


def test_degenerate_matrices():
    e = enc()
    for shape in ((0, 5), (4, 0), (0, 0)):
        got = e.decode_rows_until_packed(np.zeros(shape, np.int64), ["\n\n"])
        assert len(got.data) == 0 and got.byte_off.tolist() == [0] * (shape[0] + 1) and got.n_tok.tolist() == [0] * shape[0]
        assert got.hit.tolist() == [S.NO_HIT] * shape[0]
    got = e.decode_rows_until_packed(np.full((3, 4), PAD_ID, np.int64), ["\n\n"], skip=[PAD_ID], errors=None)  # K == 0
    assert len(got.data) == 0 and len(got.tokens) == 0 and got.n_tok.tolist() == [0, 0, 0]
    got = e.decode_rows_until_packed(np.array([[97, 10, 10, 98]], np.int64), [])  # an empty stop set
    assert bytes(got.data) == b"a\n\nb" and got.hit.tolist() == [S.NO_HIT] and got.n_tok.tolist() == [4]
