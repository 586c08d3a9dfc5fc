"""Repetition statistics on the GPU (tk_repeat.h): the entries through CoreBPE and Encoding, value for value against tests/repeat_ref.py --
a Counter of tuples --, never against another run of the code under test.  Every batch goes through the host entry and through the
device entry on a side stream into poisoned outputs."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import repeat_ref as rr
import tiktoken_amd as tiktoken
from tiktoken_amd import DisallowedSpecialError
from tiktoken_amd._lib import last_error as lib_error

pytestmark = pytest.mark.gpu
POISON = 0x55
SIZES = [(1,), (2, 13), (32,), (2, 3, 4, 5, 6, 7, 8, 9)]


def enc_of():
    return tiktoken.get_encoding("gpt2_shaped")


def edges(enc):
    return int(enc._core_bpe.stat("repeat_tile")), int(enc._core_bpe.stat("repeat_lds_tokens"))


@functools.lru_cache(maxsize=None)
def cases(T: int, C: int, sizes):
    """(name, tokens, tok_off, the reference's result), computed once"""
    return [(*b, rr.stats(b[1], b[2], sizes)) for b in rr.batches(T, C, sizes)]


def device_stats(enc, tok, off, sizes, skip=()):
    """tk_repetition_device on a side stream: uploads, poison, the call and the copies back are queued there and nothing else is waited for"""
    dev = torch.device("cuda", enc._core_bpe.device)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        t_tok = torch.from_numpy(tok.view(np.int32).copy()).to(dev, non_blocking=True)
        t_off = torch.from_numpy(off.view(np.int64).copy()).to(dev, non_blocking=True)
        outs = [torch.full((len(off) - 1, len(sizes)), POISON, dtype=torch.int64, device=dev) for _ in rr.Ref._fields]
        enc._core_bpe.repetition_device(t_tok, t_off, sizes, **{n: o for n, o in zip(rr.Ref._fields, outs) if n not in skip})
        pinned = [torch.empty(o.shape, dtype=o.dtype, pin_memory=True) for o in outs]
        for h, o in zip(pinned, outs):
            h.copy_(o, non_blocking=True)
    stream.synchronize()
    return rr.Ref(*[h.numpy().view(np.uint64) for h in pinned])


def same(got, want, what, skip=()):
    for f in rr.Ref._fields:
        a, b = getattr(got, f), getattr(want, f)
        if f in skip:
            assert (a == POISON).all(), (what, f, "written though not asked for")
        else:
            assert a.shape == b.shape and (a == b).all(), (what, f, np.argwhere(a != b)[:8].tolist())


@pytest.mark.parametrize("sizes", SIZES)
def test_every_batch_through_host_and_device_entries(sizes):
    enc = enc_of()
    for name, tok, off, want in cases(*edges(enc), sizes):
        got = enc.repetition_tokens_packed(tok, off, sizes)
        assert got.sizes == sizes and (got.length == np.diff(off)).all()
        same(got, want, (name, "host"))
        same(device_stats(enc, tok, off, sizes), want, (name, "device"))


def test_null_outputs():
    enc, sizes = enc_of(), (2, 13)
    name, tok, off, want = cases(*edges(enc), sizes)[11]
    assert name == "interleaved"
    for f in rr.Ref._fields:
        same(device_stats(enc, tok, off, sizes, skip=(f,)), want, ("without", f), skip=(f,))


def test_text_entries_and_keep_mask():
    enc = enc_of()
    texts = ["", "the cat sat on the mat and the cat sat on the mat again", "x y " * 3000, "no phrase of this one comes twice", "ha " * 40, "a <|endoftext|> b"]
    allow = {"<|endoftext|>"}
    sizes = (2, 3, 4, 5, 6, 7, 8, 9, 10)  # (nine: two calls of the library)
    for special in (False, True):
        tok, off = enc.encode_batch_packed(texts, allowed_special=allow) if special else enc.encode_ordinary_batch_packed(texts)
        want = rr.stats(tok, off, sizes)
        got = enc.repetition_batch(texts, allowed_special=allow) if special else enc.repetition_ordinary_batch(texts)
        assert got.sizes == sizes and (got.length == np.diff(off)).all()
        same(got, want, ("text", special))
    length = np.diff(off).astype(np.float64)
    assert length.max() > edges(enc)[1] and want.n_dup[1].sum() > 0
    safe = np.where(length > 0, length, 1.0)
    keep = np.ones(len(texts), bool)
    for k, limit in {2: .20, 3: .18, 4: .16}.items():
        keep &= want.top_count[:, sizes.index(k)] * k / safe <= limit
    for k, limit in {5: .15, 6: .14, 7: .13, 8: .12, 9: .11, 10: .10}.items():
        keep &= want.n_dup_covered[:, sizes.index(k)] / safe <= limit
    mask = got.keep_mask()
    assert mask.dtype == np.uint8 and mask.tolist() == keep.astype(int).tolist() and mask[0] == 1 and mask[2] == 0
    with pytest.raises(KeyError):
        enc.repetition_ordinary_batch(texts[:2], sizes=(2, 3)).keep_mask()
    with pytest.raises(DisallowedSpecialError) as e:
        enc.repetition_batch(texts)
    assert e.value.doc == 5


def test_refusals():
    enc = enc_of()
    core = enc._core_bpe
    tok, off = rr.pack([np.arange(10)])
    for sizes in ((), tuple(range(1, 10)), (0,), (2, 33)):
        with pytest.raises(ValueError):
            core.repetition_packed(tok, off, sizes)
        assert "sizes" in lib_error(), lib_error()  # (the library's refusal, not Python's)
    huge, ks, out = np.array([0, 2 ** 31], np.uint64), np.array([2], np.uint32), np.full(1, POISON, np.uint64)
    rc = core._L.tk_repetition(core._h, tok.ctypes.data, huge.ctypes.data, 1, ks.ctypes.data, 1, out.ctypes.data, *[ctypes.c_void_p()] * 4)
    assert rc != 0 and "2^31" in lib_error() and out[0] == POISON
