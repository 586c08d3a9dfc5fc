"""Line sets on the GPU (tk_line_set.h): the entries through CoreBPE, Encoding and LineSet, byte for byte against tests/line_set_ref.py
-- re.finditer and a Python set --, never against another run of the code under test.  The batches are those of the line statistics'
tests, whose lines lie on every lane, wavefront, tile and document edge, and a handful that put a DROPPED line there within one call."""
import ctypes

import numpy as np
import pytest
import torch

import line_set_ref as ref
import lines_ref as lr
import tiktoken_amd as tiktoken
from tiktoken_amd._lib import last_error as lib_error

pytestmark = pytest.mark.gpu
POISON = 0x55
T, LANE, WAVE = 4096, 16, 1024  # (checked against the shipped constants below: the batches are named at collection, before a core exists)
CAPACITY = 1 << 16
FIELDS = ("text_out", "doc_off_out", "n_lines", "n_dropped", "counts")


def enc_of():
    return tiktoken.get_encoding("gpt2_shaped")


def device_dedup(enc, ls, docs, add=True, skip=(), shift=0):
    """tk_line_dedup_device on a side stream into poisoned outputs; `shift`: text and text_out start that many bytes off a 16-byte boundary.
    Returns the five outputs as numpy arrays (text_out whole, poison included)."""
    text, off = lr.pack(docs)
    dev = torch.device("cuda", enc._core_bpe.device)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        t_text = torch.from_numpy(np.concatenate([np.zeros(shift, np.uint8), text])).to(dev)[shift:]
        t_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
        n = len(off) - 1
        outs = dict(text_out=torch.full((len(text) + shift,), POISON, dtype=torch.uint8, device=dev)[shift:], doc_off_out=torch.full((n + 1,), POISON, dtype=torch.int64, device=dev),
                    n_lines=torch.full((n,), POISON, dtype=torch.int64, device=dev), n_dropped=torch.full((n,), POISON, dtype=torch.int64, device=dev),
                    counts=torch.full((2,), POISON, dtype=torch.int64, device=dev))
        enc._core_bpe.line_dedup_device(ls._native, t_text, t_off, add, **{k: (None if k in skip else v) for k, v in outs.items()})
    stream.synchronize()
    return {k: v.cpu().numpy().view(np.uint8 if k == "text_out" else np.uint64) for k, v in outs.items()}


def same_device(got, want, what, skip=()):
    docs, n_lines, n_dropped = want
    text, off = lr.pack(docs)
    exp = dict(text_out=text, doc_off_out=off, n_lines=n_lines, n_dropped=n_dropped, counts=np.array([len(text), n_dropped.sum()], np.uint64))
    for f in FIELDS:
        if f in skip:
            assert (got[f] == POISON).all(), (what, f, "written though not asked for")
        elif f == "text_out":
            assert got[f][:len(text)].tobytes() == text.tobytes() and (got[f][len(text):] == POISON).all(), (what, f)
        else:
            assert got[f].tolist() == exp[f].tolist(), (what, f)


def same_host(got, want, what):
    docs, n_lines, n_dropped = want
    text, off = lr.pack(docs)
    assert got.text.tobytes() == text.tobytes() and got.doc_off.tolist() == off.tolist(), what
    assert got.n_lines.tolist() == n_lines.tolist() and got.n_dropped.tolist() == n_dropped.tolist() and got.n_dropped_total == n_dropped.sum(), what


def test_shipped_constants():
    stat = enc_of()._core_bpe.stat
    assert (stat("lines_tile"), stat("lines_lane"), stat("lines_wave")) == (T, LANE, WAVE)


@pytest.mark.parametrize("name", list(lr.batches(T, LANE, WAVE)))
def test_two_calls_on_a_fresh_set(name):
    enc, docs, seen = enc_of(), lr.batches(T, LANE, WAVE)[name], set()
    with enc.line_set(CAPACITY, seed=3) as ls:
        same_host(ls.dedup_packed(*lr.pack(docs), add=True), ref.dedup(seen, docs), (name, "first, host"))
        assert len(ls) == len(seen)
        want = ref.dedup(seen, docs)
        assert want[2].sum() == want[1].sum()  # (the second call drops every line)
        same_device(device_dedup(enc, ls, docs), want, (name, "second, device"))
        assert len(ls) == len(seen)


def edge_batches():
    """{name: documents}: a dropped line, or its newline, at a tile edge within ONE call"""
    rng = np.random.default_rng(7)
    word = lambda n: bytes(rng.integers(97, 123, n, dtype=np.uint8))  # noqa: E731
    out, x, long = {}, b"dupl", word(2 * T + 100)
    for k in (-1, 0, 1):
        head = x + b"\n" + word(T + k - 2 * len(x) - 2) + b"\n" + x  # its last byte is position T + k - 1
        out[f"newline of a dropped line opens the next tile {k:+d}"] = [head + b"\ntail\n" + x]
        out[f"dropped line ends its document, the next starts with a newline {k:+d}"] = [head, b"\nrest\n" + x + b"\n", b"\n\n"]
        out[f"first in the last lane, repeat in the next tile {k:+d}"] = [word(T + k - 4) + b"\nab\nab\nab"]
        out[f"three-tile line repeated, empty documents between {k:+d}"] = [word(T // 2 + k), long + b"\n", b"", b"", long, b"", long + b"\n" + x, b""]
    return out


@pytest.mark.parametrize("name", list(edge_batches()))
def test_dropped_lines_at_tile_edges_unaligned(name):
    enc, docs = enc_of(), edge_batches()[name]
    with enc.line_set(CAPACITY) as ls:
        want = ref.dedup(set(), docs)
        assert want[2].sum() > 0
        same_device(device_dedup(enc, ls, docs, shift=1), want, name)


def test_filter_only():
    enc, seen = enc_of(), set()
    block = [b"cookie banner\nnavigation\n", b"licence footer"]
    docs = [b"navigation\nbody\nbody\ncookie banner", b"", b"licence footer\nbody\n\nnavigation\n"]
    ref.dedup(seen, block)
    with enc.line_set(16) as ls:
        ls.add_packed(*lr.pack(block))
        assert len(ls) == 3
        want = ref.dedup(set(seen), docs, add=False)
        assert want[0][0] == b"body\nbody\n"  # (duplicates within the batch stay)
        same_host(ls.dedup_packed(*lr.pack(docs), add=False), want, "host")
        same_device(device_dedup(enc, ls, docs, add=False), want, "device")
        assert len(ls) == 3


@pytest.mark.parametrize("min_bytes", (1, 2, 17))
def test_min_bytes(min_bytes):
    enc, seen = enc_of(), set()
    docs = [b"\n".join(bytes([97 + i]) * n for n in (1, 2, 16, 17, 18)) for i in (0, 1, 0)] + [b"a\n" * 3 + b"b" * 17]
    with enc.line_set(64, min_bytes=min_bytes) as ls:
        want = ref.dedup(seen, docs, min_bytes=min_bytes)
        same_host(ls.dedup_packed(*lr.pack(docs)), want, min_bytes)
        assert len(ls) == len(seen) == sum(n >= min_bytes for n in (1, 2, 16, 17, 18)) * 2
        same_device(device_dedup(enc, ls, docs), ref.dedup(seen, docs, min_bytes=min_bytes), (min_bytes, "again"))


def test_entries():
    enc = enc_of()
    texts = ["menu\nnaïve – body\nmenu\n", "", "menu\nother…\n\nnaïve – body"]
    docs = [t.encode() for t in texts]
    want = ref.dedup(set(), docs)
    text, off = lr.pack(docs)
    dev = torch.device("cuda", enc._core_bpe.device)
    with enc.line_set(64) as ls:
        assert ls.dedup_batch(texts) == [d.decode() for d in want[0]]
        ls.clear()
        assert ls.dedup_batch(docs) == want[0]
        for first in (text.tobytes(), bytearray(text.tobytes()), memoryview(text.tobytes()), text, torch.from_numpy(text.copy()).to(dev)):
            ls.clear()
            same_host(ls.dedup_packed(first, off), want, type(first).__name__)
        ls.clear()
        ls.add_batch(texts[:1])
        assert len(ls) == 2
        for f in ("n_lines", "n_dropped", "counts"):
            ls.clear()
            same_device(device_dedup(enc, ls, docs, skip=(f,)), want, ("without", f), skip=(f,))


def test_refusals():
    enc = enc_of()
    core, dev = enc._core_bpe, torch.device("cuda", enc._core_bpe.device)
    docs, seen = [b"ab\ncd\nab"], set()
    text = np.frombuffer(docs[0], np.uint8)
    d_text = torch.from_numpy(text.copy()).to(dev)
    poisoned = lambda n, dtype=torch.int64: torch.full((n,), POISON, dtype=dtype, device=dev)  # noqa: E731
    with pytest.raises(ValueError, match="min_bytes"):
        enc.line_set(8, min_bytes=0)
    with pytest.raises(ValueError, match="capacity"):
        enc.line_set(0)
    with enc.line_set(5) as ls:
        same_host(ls.dedup_packed(*lr.pack(docs)), ref.dedup(seen, docs), "before")

        def refused(what, t_text, off, text_out=None):
            outs = dict(text_out=poisoned(t_text.numel(), torch.uint8) if text_out is None else text_out, doc_off_out=poisoned(len(off)), n_lines=poisoned(len(off) - 1),
                        n_dropped=poisoned(len(off) - 1), counts=poisoned(2))
            before = t_text.cpu().numpy().copy()
            with pytest.raises(ValueError):
                core.line_dedup_device(ls._native, t_text, torch.tensor(off, dtype=torch.int64, device=dev), True, **outs)
            assert what in lib_error(), (what, lib_error())
            assert all((v.cpu().numpy() == (before if v is text_out else POISON)).all() for v in outs.values()) and len(ls) == len(seen), what

        for off in ([0, 5, 4], [1, 4, 8], [0, 4, 7]):  # (does not ascend; not from 0; not to N -- seen on the device)
            refused("doc_off", d_text, off)
        refused("d_text_out", d_text, [0, 8], text_out=d_text)
        four = np.frombuffer(b"1\n2\n3\n4", np.uint8)  # (the count above has lowered the bound to the two keys: 2 + 4 is one line past the capacity)
        refused("capacity", torch.from_numpy(four.copy()).to(dev), [0, 7])
        huge, out, n_out = np.array([0, 0xFFFF0001], np.uint64), ctypes.c_void_p(), ctypes.c_uint64()
        assert core._L.tk_line_dedup(core._h, ls._native.handle(), text.ctypes.data, huge.ctypes.data, 1, 1, ctypes.byref(out), ctypes.byref(n_out), huge.ctypes.data, None, None) != 0
        assert "0xFFFF0000" in lib_error() and not out.value
        other = tiktoken.CoreBPE({bytes([b]): b for b in range(256)}, {}, enc._pat_str, device=core.device)  # (a second core; any device will do)
        off = np.array([0, 8], np.uint64)
        assert core._L.tk_line_add(other._h, ls._native.handle(), text.ctypes.data, off.ctypes.data, 1) != 0 and "another core" in lib_error()
        other.close()
        again = [b"cd\nnew", b"new"]
        same_device(device_dedup(enc, ls, again), ref.dedup(seen, again), "after the refusals")
        assert len(ls) == len(seen) == 3


def test_clear_then_first_batch_again():
    enc, docs = enc_of(), lr.batches(T, LANE, WAVE)["many one-line documents"]
    want = ref.dedup(set(), docs)
    with enc.line_set(CAPACITY) as ls:
        same_host(ls.dedup_packed(*lr.pack(docs)), want, "first")
        n = len(ls)
        ls.clear()
        assert len(ls) == 0
        same_device(device_dedup(enc, ls, docs), want, "after clear")
        assert len(ls) == n
