"""Line cleaning on the GPU (tk_clean.h): the entries through CoreBPE and Encoding, value for value and byte for byte against
tests/clean_ref.py -- re.finditer, str.split, bytes.lower, `in` --, never against another run of the code under test.  Every batch goes
through the host entry and through the device entry on a side stream into poisoned outputs."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import clean_ref as cr
import tiktoken_amd as tiktoken
from tiktoken_amd import _tiktoken
from tiktoken_amd._lib import last_error as lib_error

pytestmark = pytest.mark.gpu
POISON = 0x55
T, LANE, WAVE = 4096, 16, 1024  # (checked against the shipped constants below: the batches are named at collection, before a core exists)
NAMES = list(cr.batches(T, LANE, WAVE))


def enc_of():
    return tiktoken.get_encoding("gpt2_shaped")


@functools.lru_cache(maxsize=None)
def cases():
    """{name: (text, doc_off, rules, the reference's result)}, computed once"""
    return {name: (*cr.pack(docs), rules, cr.clean(docs, **rules)) for name, (docs, rules) in cr.batches(T, LANE, WAVE).items()}


def device_clean(enc, text, off, rules, skip=(), shift=0):
    """tk_line_clean_device on a side stream: uploads, poison, the call and the copies back are queued there; `shift`: text and text_out
    start that many bytes behind an aligned pointer.  Returns a Ref whose text is the whole buffer."""
    dev = torch.device("cuda", enc._core_bpe.device)
    stream = torch.cuda.Stream(dev)
    n = len(off) - 1
    with torch.cuda.stream(stream):
        t_text = torch.from_numpy(np.concatenate([np.zeros(shift, np.uint8), text])).to(dev, non_blocking=True)[shift:]
        t_off = torch.from_numpy(off.view(np.int64).copy()).to(dev, non_blocking=True)
        outs = dict(text_out=torch.full((shift + len(text),), POISON, dtype=torch.uint8, device=dev)[shift:], doc_off_out=torch.full((n + 1,), POISON, dtype=torch.int64, device=dev),
                    **{f: torch.full((n,), POISON, dtype=torch.int64, device=dev) for f in cr.FIELDS}, counts=torch.full((2,), POISON, dtype=torch.int64, device=dev))
        enc._core_bpe.line_clean_device(t_text, t_off, **rules, **{k: v for k, v in outs.items() if k not in skip})
        pinned = {k: torch.empty(v.shape, dtype=v.dtype, pin_memory=True) for k, v in outs.items()}
        for k, v in outs.items():
            pinned[k].copy_(v, non_blocking=True)
    stream.synchronize()
    return cr.Ref(*[pinned[k].numpy().view(np.uint8 if k == "text_out" else np.uint64) for k in ("text_out", "doc_off_out", *cr.FIELDS, "counts")])


def same(got, want, what, skip=()):
    kept = len(want.text)
    for f in cr.Ref._fields:
        a, b = getattr(got, f), getattr(want, f)
        if f in skip or (f in ("text", "doc_off") and "text_out" in skip):
            assert (a == POISON).all(), (what, f, "written though not asked for")
        elif f == "text":
            assert bytes(a[:kept]) == bytes(b) and (a[kept:] == POISON).all(), (what, f, kept)
        elif f == "counts" and "text_out" in skip:
            assert a.tolist() == [0, int(b[1])], (what, f)
        else:
            assert a.shape == b.shape and (a == b).all(), (what, f, np.argwhere(a != b)[:8].tolist(), a[a != b][:8], b[a != b][:8])


def test_shipped_constants():
    stat = enc_of()._core_bpe.stat
    assert (stat("clean_tile"), stat("clean_lane"), stat("clean_wave")) == (T, LANE, WAVE)
    assert tuple(p.encode() for p in _tiktoken.C4_LINE_PHRASES) == cr.LINE_PHRASES and tuple(p.encode() for p in _tiktoken.C4_DOC_PHRASES) == cr.DOC_PHRASES
    assert _tiktoken.C4_TERMINAL.encode() == cr.C4["terminal"]


@pytest.mark.parametrize("name", NAMES)
def test_batch_through_host_and_device_entries(name):
    enc = enc_of()
    text, off, rules, want = cases()[name]
    got = enc.clean_lines_packed(text, off, **rules)
    same(cr.Ref(*got, want.counts), want, (name, "host"))
    same(device_clean(enc, text, off, rules), want, (name, "device"))
    if name == "nothing dropped":
        assert bytes(want.text) == bytes(text) and (want.doc_off == off).all()


@pytest.mark.parametrize("shift", [1, 15])
def test_unaligned_device_pointers(shift):
    enc = enc_of()
    for name in ("one of each", "newline at tile edge +0", "phrases at the edges", "a line over three tiles"):
        text, off, rules, want = cases()[name]
        same(device_clean(enc, text, off, rules, shift=shift), want, (name, shift))


@pytest.mark.parametrize("without", ["text_out", "doc_off_out", *cr.FIELDS, "counts"])
def test_null_outputs(without):
    """one output missing at a time; without text_out the call only counts: no write pass, text_out's buffer and doc_off_out stay poisoned"""
    enc = enc_of()
    text, off, rules, want = cases()["one of each"]
    skip = ("text_out", "doc_off_out") if without == "doc_off_out" else (without,)  # (text_out needs doc_off_out)
    same(device_clean(enc, text, off, rules, skip=skip), want, ("without", without), skip=skip)


def test_text_entries_and_keep_mask():
    enc = enc_of()
    good = "The quick brown fox jumps over the lazy dog."
    texts = [good + "\n" + good, "", "Menu\nHome\n" + good + "\nRead more...\n", "We use cookies to improve your experience.\n" + good, "Lorem ipsum dolor sit amet, consectetur.\n" + good,
             good + "\nfunction f() { return 1; }", "naïve café – " + good + " \t\r\n\n" + good, "Please enable JavaScript to view this page.", good + "\nTerms of Use | Privacy Policy",
             "no full stop at the end of this one", "¿Qué tal? Muy bien, gracias — ¡hasta luego!\n\n", "x" * 1001 + " is one long word in this line."]
    want = cr.clean([t.encode() for t in texts])
    docs = [bytes(want.text[a:b]) for a, b in zip(want.doc_off[:-1].tolist(), want.doc_off[1:].tolist())]
    assert enc.clean_lines_batch(texts) == [d.decode() for d in docs] and enc.clean_lines_batch([t.encode() for t in texts]) == docs
    text, off = cr.pack([t.encode() for t in texts])
    dev = torch.device("cuda", enc._core_bpe.device)
    for first in (text.tobytes(), bytearray(text.tobytes()), memoryview(text.tobytes()), text, torch.from_numpy(text.copy()).to(dev)):
        got = enc.clean_lines_packed(first, off)
        same(cr.Ref(*got, want.counts), want, type(first).__name__)
    assert got.texts() == docs and isinstance(got, tiktoken.LineClean)
    assert got.keep_mask().dtype == np.uint8 and got.keep_mask().tolist() == (want.n_kept >= 1).astype(int).tolist() == [1, 0, 1, 1, 0, 0, 1, 0, 1, 0, 1, 0]
    assert got.keep_mask(min_lines=2).tolist() == (want.n_kept >= 2).astype(int).tolist() and got.keep_mask(0).tolist() == (want.doc_hit == 0).astype(int).tolist()


def test_refusals():
    core = enc_of()._core_bpe
    text, off = np.frombuffer(b"ab the\ncd", np.uint8), np.array([0, 4, 9], np.uint64)
    out = np.full(2, POISON, np.uint64)
    dev = torch.device("cuda", core.device)
    d_text, d_off = torch.from_numpy(text.copy()).to(dev), torch.from_numpy(off.view(np.int64).copy()).to(dev)
    d_out, d_off_out = torch.full((2,), POISON, dtype=torch.int64, device=dev), torch.full((3,), POISON, dtype=torch.int64, device=dev)
    bad = [("at most 16 in a list", dict(line_phrases=[b"p%02d" % i for i in range(17)])), ("at most 16 in a list", dict(doc_phrases=[b"p%02d" % i for i in range(17)])),
           ("1 to 32 bytes", dict(line_phrases=[b"ab", b""])), ("1 to 32 bytes", dict(doc_phrases=[b"x" * 33])), ("no newline", dict(line_phrases=[b"a\nb"])),
           ("below 0x80", dict(terminal=b".\x80")), ("at most 16 bytes", dict(terminal=bytes(range(33, 50))))]
    for why, rules in bad:
        with pytest.raises(ValueError):
            core.line_clean_device(d_text, d_off, n_lines=d_out, **rules)
        assert why in lib_error() and (d_out.cpu().numpy() == POISON).all(), why
        _keep, spec = core._clean_spec(**{**dict(min_words=5, max_word_chars=1000, terminal=b".", drop_ellipsis=True, line_phrases=(), doc_phrases=()), **rules})
        assert core._L.tk_line_clean(core._h, text.ctypes.data, off.ctypes.data, 2, ctypes.byref(spec), None, None, None, out.ctypes.data, *[None] * 8) != 0
        assert why in lib_error() and (out == POISON).all(), why
    with pytest.raises(ValueError):  # text_out == text
        core.line_clean_device(d_text, d_off, text_out=d_text, doc_off_out=d_off_out, n_lines=d_out)
    assert "must not be d_text" in lib_error() and (d_out.cpu().numpy() == POISON).all() and (d_off_out.cpu().numpy() == POISON).all() and bytes(d_text.cpu().numpy()) == bytes(text)
    d_txt_out = torch.full((9,), POISON, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError):  # text_out without doc_off_out
        core.line_clean_device(d_text, d_off, text_out=d_txt_out, n_lines=d_out)
    assert "null argument" in lib_error() and (d_out.cpu().numpy() == POISON).all() and (d_txt_out.cpu().numpy() == POISON).all()
    _keep, spec = core._clean_spec(5, 1000, b".", True, (), ())
    # N above the cap through the device entry: refused before a byte of d_text is read
    assert core._L.tk_line_clean_device(core._h, d_text.data_ptr(), 0xFFFF0001, d_off.data_ptr(), 2, ctypes.byref(spec), None, None, None, d_out.data_ptr(), *[None] * 8) != 0
    assert "0xFFFF0000" in lib_error() and (d_out.cpu().numpy() == POISON).all()
    for o in ([1, 4, 9], [0, 5, 4, 9], [0, 0xFFFF0001]):  # (not from 0; does not ascend; above the cap -- the host entry's refusals)
        o = np.array(o, np.uint64)
        assert core._L.tk_line_clean(core._h, text.ctypes.data, o.ctypes.data, len(o) - 1, ctypes.byref(spec), None, None, None, out.ctypes.data, *[None] * 8) != 0
        assert ("0xFFFF0000" if o[-1] > 9 else "doc_off") in lib_error() and (out == POISON).all()
