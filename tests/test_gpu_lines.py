"""Line statistics on the GPU (tk_lines.h): the entries through CoreBPE and Encoding, value for value against tests/lines_ref.py --
re.split and a Counter --, never against another run of the code under test.  Every batch goes through the host entry and through the
device entry on a side stream into poisoned outputs."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import lines_ref as lr
import tiktoken_amd as tiktoken
from tiktoken_amd._lib import last_error as lib_error

pytestmark = pytest.mark.gpu
POISON = 0x55
T, LANE, WAVE = 4096, 16, 1024  # (checked against the shipped constants below: the batches are named at collection, before a core exists)


def enc_of():
    return tiktoken.get_encoding("gpt2_shaped")


@functools.lru_cache(maxsize=None)
def cases():
    """{name: (text, doc_off, the reference's result)}, computed once"""
    return {name: (*lr.pack(docs), lr.stats(docs)) for name, docs in lr.batches(T, LANE, WAVE).items()}


def device_stats(enc, text, off, skip=(), seed=0):
    """tk_line_stats_device on a side stream: uploads, poison, the call and the copies back are queued there"""
    dev = torch.device("cuda", enc._core_bpe.device)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        t_text = torch.from_numpy(text.copy()).to(dev, non_blocking=True)
        t_off = torch.from_numpy(off.view(np.int64).copy()).to(dev, non_blocking=True)
        outs = [torch.full((len(off) - 1,), POISON, dtype=torch.int64, device=dev) for _ in lr.Ref._fields]
        enc._core_bpe.line_stats_device(t_text, t_off, seed=seed, **{n: o for n, o in zip(lr.Ref._fields, outs) if n not in skip})
        pinned = [torch.empty(o.shape, dtype=o.dtype, pin_memory=True) for o in outs]
        for h, o in zip(pinned, outs):
            h.copy_(o, non_blocking=True)
    stream.synchronize()
    return lr.Ref(*[h.numpy().view(np.uint64) for h in pinned])


def same(got, want, what, skip=()):
    for f in lr.Ref._fields:
        a, b = getattr(got, f), getattr(want, f)
        if f in skip:
            assert (a == POISON).all(), (what, f, "written though not asked for")
        else:
            assert a.shape == b.shape and (a == b).all(), (what, f, np.argwhere(a != b)[:8].tolist(), a[a != b][:8], b[a != b][:8])


def test_shipped_constants():
    stat = enc_of()._core_bpe.stat
    assert (stat("lines_tile"), stat("lines_lane"), stat("lines_wave")) == (T, LANE, WAVE)


@pytest.mark.parametrize("name", list(lr.batches(T, LANE, WAVE)))
def test_batch_through_host_and_device_entries(name):
    enc = enc_of()
    text, off, want = cases()[name]
    got = enc.line_stats_packed(text, off, seed=3)
    assert (got.length == np.diff(off)).all()
    same(lr.Ref(*got[1:]), want, (name, "host"))
    same(device_stats(enc, text, off, seed=5), want, (name, "device"))


def test_null_outputs():
    enc = enc_of()
    text, off, want = cases()["bullets and ellipses"]
    for f in lr.Ref._fields:
        same(device_stats(enc, text, off, skip=(f,)), want, ("without", f), skip=(f,))


def test_text_entries_and_keep_mask():
    enc = enc_of()
    texts = ["", "all\ndifferent\n\nlines and paragraphs\nhere", "again\n" * 4 + "x", "p q\n\np q\n\nr","aaaaaaaaaaaaaaaaaaaa\nb\naaaaaaaaaaaaaaaaaaaa\nc\nd\ne\nf",
             "pppppppppppppppppppp\n\nb\n\npppppppppppppppppppp\n\nc\n\nd\n\ne", "- a\n- b\n* c\n• d\n● e", "one...\ntwo…\nthree", "naïve – ok\nfine"]
    want = lr.stats([t.encode() for t in texts])
    got = enc.line_stats_batch(texts)
    same(lr.Ref(*got[1:]), want, "str")
    same(lr.Ref(*enc.line_stats_batch([t.encode() for t in texts], seed=9)[1:]), want, "bytes")
    text, off = lr.pack([t.encode() for t in texts])
    dev = torch.device("cuda", enc._core_bpe.device)
    for first in (text.tobytes(), bytearray(text.tobytes()), memoryview(text.tobytes()), text, torch.from_numpy(text.copy()).to(dev)):
        same(lr.Ref(*enc.line_stats_packed(first, off)[1:]), want, type(first).__name__)
    ratio = lambda a, b: a / np.where(b > 0, b, 1).astype(np.float64)  # noqa: E731  (a is 0 wherever b is)
    rules = [ratio(want.n_dup_lines, want.n_lines) <= .30, ratio(want.n_dup_paragraphs, want.n_paragraphs) <= .30, ratio(want.dup_line_chars, want.n_chars) <= .20,
             ratio(want.dup_paragraph_chars, want.n_chars) <= .20, ratio(want.n_bullet_lines, want.n_lines) <= .90, ratio(want.n_ellipsis_lines, want.n_lines) <= .30]
    assert all((~r).any() for r in rules) and np.logical_and.reduce(rules)[[0, 1, 8]].all()  # (every rule fails somewhere; three documents pass all)
    mask = got.keep_mask()
    assert mask.dtype == np.uint8 and mask.tolist() == np.logical_and.reduce(rules).astype(int).tolist()
    assert got.keep_mask(*[None] * 6).all() and got.keep_mask(None, None, None, None, None, .30).tolist() == rules[5].astype(int).tolist()


def test_refusals():
    core = enc_of()._core_bpe
    text = np.frombuffer(b"ab\ncd\nab", np.uint8)
    out = np.full(2, POISON, np.uint64)
    nine = [out.ctypes.data] + [ctypes.c_void_p()] * 8
    for off in ([1, 4, 8], [0, 5, 4, 8]):
        off = np.array(off, np.uint64)
        assert core._L.tk_line_stats(core._h, text.ctypes.data, off.ctypes.data, len(off) - 1, 0, *nine) != 0
        assert "doc_off" in lib_error() and (out == POISON).all()  # (the library's refusal, not Python's)
    dev = torch.device("cuda", core.device)
    d_text, d_out = torch.from_numpy(text.copy()).to(dev), torch.full((2,), POISON, dtype=torch.int64, device=dev)
    for off in ([0, 5, 4], [1, 4, 8], [0, 4, 7]):  # (does not ascend; not from 0; not to N -- seen on the device)
        with pytest.raises(ValueError):
            core.line_stats_device(d_text, torch.tensor(off, dtype=torch.int64, device=dev), n_chars=d_out)
        assert "doc_off" in lib_error() and (d_out.cpu().numpy() == POISON).all()
    huge = np.array([0, 0xFFFF0001], np.uint64)
    assert core._L.tk_line_stats(core._h, text.ctypes.data, huge.ctypes.data, 1, 0, *nine) != 0
    assert "0xFFFF0000" in lib_error() and (out == POISON).all()
