"""Normalising line sets on the GPU (tk_line_set.h over TkLnNorm): `Encoding.line_set(..., normalize=mask)` through the host entry and
through tk_line_dedup_device on a side stream into poisoned outputs, byte for byte and count for count against tests/line_norm_ref.py
-- the normal form in Python and a Python set.  The batches are the smallest at which the join of the normal form can go wrong at a
tile of 4096, a lane of 16 and a wavefront of 1024 bytes."""
import pytest

import line_norm_ref as ref
import line_set_ref
import lines_ref as lr
import tiktoken_amd as tiktoken
from test_gpu_line_set import T, LANE, WAVE, device_dedup, enc_of, lib_error, same_device, same_host

pytestmark = pytest.mark.gpu
MASKS = (1, 2, 4, 8, 5, 12, 15)


def straddle(edge):
    """a white-space run of four over position `edge` of the text, its twin with one blank, and the same without any"""
    a, b = b"a" * (edge - 2), b"bcd"
    return [a + b" \t\r " + b + b"\n" + a + b" " + b + b"\n" + a + b + b"\n" + a + b"\x0b\x0c" + b]


def batches():
    """{name: (documents, min_bytes)}"""
    line = lambda a, b: b"x" * 15 + a + b"y" * (T - 1 - 17) + b + b"zz"  # noqa: E731
    edges = line(b"A7", b"Q3") + b"\n" + line(b"a7", b"q3") + b"\n" + line(b"A0", b"Q9") + b"\n" + line(b"B7", b"Q3")
    assert (edges[15:17], edges[T - 1:T + 1]) == (b"A7", b"Q3")
    out = {
        "one normal form, different raw lengths": [b"HOME | ABOUT | CONTACT\nbody\nHome  |  About | Contact \nPage 3 of 17\nPage 14 of 170\nPage 4 of 17\n"
                                                   b"\xc2\xa9 2019 Example Inc.\n\xc2\xa9 2020 Example Inc.\nRead more\nRead more \n1,024 views\n2,311 views"],
        "leading and trailing white space longer than a tile": [b" " * (T + 100) + b"lead\nlead\ntrail" + b"\t" * (T + 100) + b"\ntrail\n" + b" " * (2 * T + 5) + b"\n" + b" " * (2 * T + 5)],
        "punctuation alone in the lanes inside a word": [b"a" + b"," * 40 + b"b\nab\na , b\na b\na  b\n" + b"c" + b"." * (T + 40) + b"d\ncd"],
        "empty normal forms": [b"...\n...\n \t \n \t \n!!!\n", b"?\n \n...\n"],
        "six raw bytes, three in the normal form": [b"a,b,c!\na,b,c!\nab,cd!\nab,cd!\n  a    \n  a    \nabcd\n"],
        "case and digits at bytes 15/16 and 4095/4096": [edges],
        "bytes above 0x7F beside every class": [b"\xc3\x89 A,1\xc3\x89\n\xc3\xa9 a,1\xc3\xa9\n\xc3\x89 a 2\xc3\x89\n\xc3\x89  a.2\xc3\x89\na\xc2\xa0b\na b\na\xc2 b\nA\xe2\x80\x83B\n"],
        "a CR LF document and its LF twin": [b"one\r\ntwo words\r\n\r\nthree\r\n", b"one\ntwo words\n\nthree\n"],
        "a document starts inside a white-space run": [b"tail  ", b"  head\ntail\nhead\n", b" \t", b"\t tail"],
    }
    for edge in (LANE, WAVE, T):
        out[f"white-space run over position {edge}"] = straddle(edge)
    return {k: (v, 4 if k.startswith("six") else 1) for k, v in out.items()}


@pytest.mark.parametrize("normalize", MASKS)
@pytest.mark.parametrize("name", list(batches()))
def test_two_calls_on_a_fresh_set(name, normalize):
    enc, (docs, min_bytes), seen = enc_of(), batches()[name], set()
    with enc.line_set(256, seed=5, min_bytes=min_bytes, normalize=normalize) as ls:
        assert ls.normalize == normalize
        same_host(ls.dedup_packed(*lr.pack(docs), add=True), ref.dedup(seen, docs, True, min_bytes, normalize), (name, normalize, "first, host"))
        assert len(ls) == len(seen)
        same_device(device_dedup(enc, ls, docs, shift=3), ref.dedup(seen, docs, True, min_bytes, normalize), (name, normalize, "second, device"))  # (keys older than the call)
        assert len(ls) == len(seen)


@pytest.mark.parametrize("normalize", (tiktoken.NORM_ALL, tiktoken.NORM_SPACE))
def test_filter_only(normalize):
    enc, seen = enc_of(), set()
    block = [b"Cookie  Banner!\nPage 1 of 9\n", b" licence footer"]
    docs = [b"page 7 of 3\nbody\nBODY\ncookie banner", b"", b"licence footer \nbody\n\nCookie Banner!\n"]
    ref.dedup(seen, block, True, 1, normalize)
    with enc.line_set(16, normalize=normalize) as ls:
        ls.add_packed(*lr.pack(block))
        assert len(ls) == 3
        want = ref.dedup(set(seen), docs, False, 1, normalize)
        assert want[0][0].startswith((b"body\nBODY", b"page 7 of 3\nbody\nBODY")) and want[2].sum() >= 2  # (duplicates within the batch stay)
        same_host(ls.dedup_packed(*lr.pack(docs), add=False), want, "host")
        same_device(device_dedup(enc, ls, docs, add=False), want, "device")
        assert len(ls) == 3


def test_a_mask_of_zero_is_the_plain_set():
    enc, docs = enc_of(), batches()["one normal form, different raw lengths"][0] * 2
    with enc.line_set(64, seed=9, normalize=0) as ls:
        want = line_set_ref.dedup(set(), docs)
        assert want[2].tolist() == [0, 12]
        same_device(device_dedup(enc, ls, docs), want, "normalize=0")


def test_refused_mask():
    with pytest.raises(ValueError):
        enc_of().line_set(8, normalize=16)
    assert "normalize" in lib_error()
