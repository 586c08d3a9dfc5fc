"""Masking on the GPU (tk_pii.h): the entries through CoreBPE and Encoding, byte for byte and count for count against tests/pii_ref.py
-- re.sub with the rule's expression --, never against another run of the code under test.  Every batch goes through the host entry
(aligned buffers) and through the device entry on a side stream, from and into pointers that are not aligned, into poisoned outputs."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import pii_ref as ref
import tiktoken_amd as tiktoken
from tiktoken_amd._lib import last_error as lib_error

pytestmark = pytest.mark.gpu
POISON = 0x55
T, LANE, WAVE, HALO = 4096, 16, 1024, 336
MAIL, ADDR = b"bob.x+y@mail.site.org", b"93.184.216.34"
OUTS = ("text_out", "doc_off_out", "n_email", "n_ip", "counts")


def placed(n, items):
    """n bytes of words with ' ' + match + ' ' written over them, the match from its position on"""
    text = bytearray((b"some words, no match: 12 3.4 x@ y. " * (n // 35 + 1))[:n])
    for pos, match in items:
        text[pos - 1:pos + len(match) + 1] = b" " + match + b" "
    return bytes(text)


def slid(match, edges):
    """the match once per edge: the i-th begins i - 1 bytes before its edge, so that an edge falls at every byte of it and one either side"""
    return [placed(edges[-1] + 2 * T, [(e + 1 - i, match) for i, e in enumerate(edges)])]


SHIFTS = len(MAIL) + 2
RANGES = [b"%d.%d.%d.%d" % a for a in [(0, 0, 0, 0), (0, 255, 255, 255), (1, 0, 0, 0), (9, 255, 255, 255), (10, 0, 0, 0), (10, 255, 255, 255), (11, 0, 0, 0), (126, 255, 255, 255),
          (127, 0, 0, 0), (127, 255, 255, 255), (128, 0, 0, 0), (223, 255, 255, 255), (224, 0, 0, 0), (255, 255, 255, 255), (100, 63, 255, 255), (100, 64, 0, 0), (100, 127, 255, 255),
          (100, 128, 0, 0), (169, 253, 255, 255), (169, 254, 0, 0), (169, 254, 255, 255), (169, 255, 0, 0), (172, 15, 255, 255), (172, 16, 0, 0), (172, 31, 255, 255), (172, 32, 0, 0),
          (192, 167, 255, 255), (192, 168, 0, 0), (192, 168, 255, 255), (192, 169, 0, 0)]]
LONG = [b"x" * 64 + b"@d.com", b"x" * 65 + b"@d.com", b"a@" + b"x" * 249 + b".com", b"a@" + b"x" * 250 + b".com"]
BATCHES = {  # name: (documents, spec)
    **{f"{what} over {name} edges": (slid(m, edges), {}) for what, m in (("e-mail", MAIL), ("address", ADDR))
       for name, edges in (("lane", [T + 64 * i for i in range(SHIFTS)]), ("wave", [WAVE * (i + 1) for i in range(SHIFTS)]), ("tile", [T * (i + 1) for i in range(SHIFTS)]))},
    "long runs that end at a tile edge": ([placed(2 * T, [(T - len(m), m)]) for m in LONG], {}),
    "document edges and empty documents": ([b"", b"", b"x bob", b"@site.org bob@si", b"te.org 93.184.", b"216.34 ", b"", MAIL, ADDR, b"", b""], {}),
    "an e-mail from the halo over an address": ([placed(2 * T, [(T - k, m)]) for k, m in ((1, b"1.2.3.4@example.com"), (4, b"a@b-1.2.3.4.com"), (2, b"x-1.2.3.4@example.com"),
                                                                                       (HALO - 70, b"a@" + b"x-" * 120 + b"1.2.3.4.com"))], {}),
    "the ranges that are not public": ([b" ".join(RANGES), b",".join(RANGES)], {}),
    "every range, nothing put": ([b" ".join(RANGES) + b" " + MAIL], dict(email=b"", ip=b"", public_ip_only=False)),
    "placeholders of 32 bytes": ([placed(3 * T, [(100 * i, (MAIL, ADDR)[i % 2]) for i in range(1, 120)])], dict(email=b"E" * 32, ip="…".encode() * 10 + b"..")),
    "addresses back to back": ([b"1.2.3.4 " * (2 * T // 8 + 50)], dict(ip=b"#" * 32)),
    "more than 1024 tiles": ((lambda n: [placed(n, [(50, MAIL), (1023 * T + 9, ADDR), (1024 * T + 7, MAIL), (n - 40, ADDR)])[a:b] for a, b in ((0, 5 * T + 3), (5 * T + 3, 1024 * T - 9), (1024 * T - 9, n))])(1027 * T + 100), {}),
}


def enc_of():
    return tiktoken.get_encoding("gpt2_shaped")


@functools.lru_cache(maxsize=None)
def case(name):
    """(text, doc_off, spec, the reference's result), computed once"""
    docs, spec = BATCHES[name]
    return (*ref.pack(docs), spec, ref.mask(docs, **spec))


def device_mask(enc, text, off, spec, cap, skip=()):
    """tk_pii_mask_device on a side stream: uploads, poison, the call and the copies back are queued there; text starts 3 bytes and text_out
    5 bytes behind an aligned pointer.  Returns a Ref whose text is the whole buffer of cap bytes."""
    dev = torch.device("cuda", enc._core_bpe.device)
    stream, n = torch.cuda.Stream(dev), len(off) - 1
    with torch.cuda.stream(stream):
        t_text = torch.from_numpy(np.concatenate([np.zeros(3, np.uint8), text])).to(dev, non_blocking=True)[3:]
        t_off = torch.from_numpy(off.view(np.int64).copy()).to(dev, non_blocking=True)
        sizes = dict(text_out=cap, doc_off_out=n + 1, n_email=n, n_ip=n, counts=4)
        outs = {k: torch.full((5 + c,), POISON, dtype=torch.uint8 if k == "text_out" else torch.int64, device=dev)[5:] for k, c in sizes.items()}
        enc._core_bpe.pii_mask_device(t_text, t_off, **spec, **{k: v for k, v in outs.items() if k not in skip})
        pinned = {k: torch.empty(v.shape, dtype=v.dtype, pin_memory=True) for k, v in outs.items()}
        for k, v in outs.items():
            pinned[k].copy_(v, non_blocking=True)
    stream.synchronize()
    return ref.Ref(*[pinned[k].numpy().view(np.uint8 if k == "text_out" else np.uint64) for k in OUTS])


def same(got, want, what, untouched=()):
    for f, k in zip(ref.Ref._fields, OUTS):
        a, b = getattr(got, f), getattr(want, f)
        if k in untouched:
            assert (a == POISON).all(), (what, f, "written though it must not be")
        elif f == "text":
            assert bytes(a[:len(b)]) == bytes(b) and (a[len(b):] == POISON).all(), (what, f, len(b), np.argwhere(a[:len(b)] != b)[:4].tolist())
        else:
            assert a.shape == b.shape and (a == b).all(), (what, f, np.argwhere(a != b)[:8].tolist(), a[a != b][:8], b[a != b][:8])


def test_shipped_constants():
    stat = enc_of()._core_bpe.stat
    assert (stat("pii_tile"), stat("pii_lane"), stat("pii_wave"), stat("pii_halo")) == (T, LANE, WAVE, HALO)


@pytest.mark.parametrize("name", BATCHES)
def test_batch_through_host_and_device_entries(name):
    enc = enc_of()
    text, off, spec, want = case(name)
    assert int(want.counts[1] + want.counts[2]) > 0  # (no batch is without a match)
    got = enc.mask_pii_packed(text, off, **spec)
    same(ref.Ref(*got, want.counts), want, (name, "host"))
    same(device_mask(enc, text, off, spec, len(want.text) + 64), want, (name, "device"))


def test_capacity_one_byte_short():
    text, off, spec, want = case("document edges and empty documents")
    got = device_mask(enc_of(), text, off, spec, len(want.text) - 1)
    same(got, want._replace(counts=want.counts + np.array([0, 0, 0, 1], np.uint64)), "one byte short", untouched=("text_out",))


@pytest.mark.parametrize("without", OUTS)
def test_null_outputs(without):
    """one output missing at a time; without text_out the call only counts: no write pass, text_out's buffer and doc_off_out stay poisoned"""
    text, off, spec, want = case("document edges and empty documents")
    skip = ("text_out", "doc_off_out") if without in ("text_out", "doc_off_out") else (without,)  # (text_out needs doc_off_out)
    same(device_mask(enc_of(), text, off, spec, len(want.text), skip=skip), want, ("without", without), untouched=skip)


def test_text_entries():
    enc = enc_of()
    texts = ["naïve café – écrire à " + MAIL.decode() + " …", "", "服务器 93.184.216.34。", "10.0.0.1 reste, 8.8.8.8 non", "x@y.z"]
    want = [ref.mask_doc(t.encode())[0] for t in texts]
    assert enc.mask_pii_batch(texts) == [w.decode() for w in want] and enc.mask_pii_batch([t.encode() for t in texts]) == want
    assert enc.mask_pii_batch(texts, email="<e>", ip="", public_ip_only=False) == [ref.mask_doc(t.encode(), b"<e>", b"", False)[0].decode() for t in texts]
    text, off = ref.pack([t.encode() for t in texts])
    full = ref.mask([t.encode() for t in texts])
    for first in (text.tobytes(), text, enc.clean_lines_packed(text, off, min_words=0, terminal="", drop_ellipsis=False, line_phrases=(), doc_phrases=()),
                  torch.from_numpy(text.copy()).to(torch.device("cuda", enc._core_bpe.device))):
        got = enc.mask_pii_packed(first, None if hasattr(first, "doc_off") else off)
        same(ref.Ref(*got, full.counts), full, type(first).__name__)
    assert got.texts() == want and isinstance(got, tiktoken.PiiMasked)


def test_refusals():
    core = enc_of()._core_bpe
    text, off = np.frombuffer(b"a@b.cc 1.2.3.4", np.uint8), np.array([0, 7, 14], np.uint64)
    out = np.full(2, POISON, np.uint64)
    dev = torch.device("cuda", core.device)
    d_text, d_off = torch.from_numpy(text.copy()).to(dev), torch.from_numpy(off.view(np.int64).copy()).to(dev)
    d_out, d_off_out, d_txt_out = (torch.full((c,), POISON, dtype=t, device=dev) for c, t in ((2, torch.int64), (3, torch.int64), (99, torch.uint8)))
    clean = lambda: all((t.cpu().numpy() == POISON).all() for t in (d_out, d_off_out, d_txt_out))  # noqa: E731
    for why, spec in (("at most 32 bytes", dict(email=b"x" * 33)), ("at most 32 bytes", dict(ip=b"x" * 33)), ("no newline", dict(ip=b"a\nb")), ("well-formed UTF-8", dict(email=b"\xc3")),
                      ("well-formed UTF-8", dict(ip=b"\xed\xa0\x80"))):
        with pytest.raises(ValueError):
            core.pii_mask_device(d_text, d_off, text_out=d_txt_out, doc_off_out=d_off_out, n_email=d_out, **spec)
        assert why in lib_error() and clean(), why
        _keep, s = core._pii_spec(**{**dict(email=b"e", ip=b"i", public_ip_only=True), **spec})
        assert core._L.tk_pii_mask(core._h, text.ctypes.data, off.ctypes.data, 2, ctypes.byref(s), None, None, None, out.ctypes.data, None) != 0
        assert why in lib_error() and (out == POISON).all(), why
    with pytest.raises(ValueError):  # text_out == text
        core.pii_mask_device(d_text, d_off, text_out=d_text, doc_off_out=d_off_out, n_email=d_out)
    assert "must not be d_text" in lib_error() and clean() and bytes(d_text.cpu().numpy()) == bytes(text)
    with pytest.raises(ValueError):  # text_out without doc_off_out
        core.pii_mask_device(d_text, d_off, text_out=d_txt_out, n_email=d_out)
    assert "null argument" in lib_error() and clean()
    _keep, s = core._pii_spec(b"e", b"i", True)
    # N above the cap through the device entry: refused before a byte of d_text is read
    assert core._L.tk_pii_mask_device(core._h, d_text.data_ptr(), 0xFFFF0001, d_off.data_ptr(), 2, ctypes.byref(s), None, None, 0, None, d_out.data_ptr(), None, None) != 0
    assert "0xFFFF0000" in lib_error() and clean()
    for o in ([1, 7, 14], [0, 9, 7, 14], [0, 0xFFFF0001]):  # (not from 0; does not ascend; above the cap -- the host entry's refusals)
        o = np.array(o, np.uint64)
        assert core._L.tk_pii_mask(core._h, text.ctypes.data, o.ctypes.data, len(o) - 1, ctypes.byref(s), None, None, None, out.ctypes.data, None) != 0
        assert ("0xFFFF0000" if o[-1] > 14 else "doc_off") in lib_error() and (out == POISON).all()
