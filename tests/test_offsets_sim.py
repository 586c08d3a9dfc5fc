"""The token-span passes (tk_offsets.h) on the CPU: tests/hostsim/offsets_sim.cpp compiles the plain C++ they are made of
(tiktoken_amd/csrc/tk_span_rule.h) for the host and drives it the way the kernels do.  Compared with restatements in Python of the
reference's rule (Encoding.decode_with_offsets, tiktoken/core.py:312-335) and with Python's own strict UTF-8 decoder."""
import ctypes
import random

import numpy as np
import pytest

import helpers as h

NONE = (1 << 64) - 1
CONT = 0x80000000
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = h.build_sim("liboffsets_sim.so", ("offsets_sim.cpp", "tk_span_rule.h", "tk_common.h"), ("-Wall",))
        vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
        L.ofs_char_word.restype = u32
        L.ofs_char_word.argtypes = [ctypes.c_char_p, u32]
        L.ofs_spans.restype = u64
        L.ofs_spans.argtypes = [vp, vp, u64, vp, u64, u32, u64, vp, vp, vp, vp]
        L.ofs_utf8_first_invalid.restype = u64
        L.ofs_utf8_first_invalid.argtypes = [vp, u64, vp, u64, vp]
        _lib = L
    return _lib


def is_cont(b: int) -> bool:
    return 0x80 <= b < 0xC0


def word_of(tok: bytes) -> int:
    return sum(1 for b in tok if not is_cont(b)) | (CONT if is_cont(tok[0]) else 0)


# ---------------------------------------------------------------- the per-id word
@pytest.mark.parametrize("name", h.ENCODING_NAMES)
def test_char_word_of_every_token(name):
    L = lib()
    toks = list(h.load_vocab(name)) + [s.encode() for s in h.SPECIALS[name]]
    assert len(toks) > 50000
    for t in toks:
        assert L.ofs_char_word(t, len(t)) == word_of(t), t
    for t in (b"\x80", b"\xbf\xbf", b"\xa0\xe9\x99\xa4", b"\xe0\xae\xbf\xe0\xae", b"a", b"\xc3"):
        assert L.ofs_char_word(t, len(t)) == word_of(t), t


# ---------------------------------------------------------------- the span rule
def rule(docs: list[list[bytes]]):
    """The rule of the issue, per document: (byte_start, char_start, byte_off, char_off)."""
    bs, cs, boff, coff = [], [], [0], [0]
    for doc in docs:
        text_len = nbytes = 0
        for tok in doc:
            bs.append(nbytes)
            cs.append(max(0, text_len - (1 if is_cont(tok[0]) else 0)))
            text_len += sum(1 for b in tok if not is_cont(b))
            nbytes += len(tok)
        boff.append(boff[-1] + nbytes)
        coff.append(coff[-1] + text_len)
    return bs, cs, boff, coff


def run_spans(docs: list[list[bytes]], block: int, rng: int = 0):
    flat = [t for d in docs for t in d]
    n = len(flat)
    lens = np.array([len(t) for t in flat] or [0], np.uint32)
    words = np.array([word_of(t) for t in flat] or [0], np.uint32)
    tok_off = np.zeros(len(docs) + 1, np.uint64)
    tok_off[1:] = np.cumsum([len(d) for d in docs]) if docs else []
    bs, cs = np.full(n + 1, 0xDEAD, np.uint32), np.full(n + 1, 0xDEAD, np.uint32)
    boff, coff = np.full(len(docs) + 1, 0xDEAD, np.uint64), np.full(len(docs) + 1, 0xDEAD, np.uint64)
    rc = lib().ofs_spans(lens.ctypes.data, words.ctypes.data, n, tok_off.ctypes.data, len(docs), block, rng, bs.ctypes.data, cs.ctypes.data, boff.ctypes.data,
                         coff.ctypes.data)
    assert rc == 0
    return bs[:n].tolist(), cs[:n].tolist(), boff.tolist(), coff.tolist()


def check_spans(docs, blocks=(8, 16, 2048)):
    want = rule(docs)
    for block in blocks:
        for rng in (0, block, 3 * block):  # the batch in one range, a workgroup per range, three
            got = run_spans(docs, block, rng)
            for g, w, what in zip(got, want, ("byte_start", "char_start", "byte_off", "char_off")):
                assert g == w, (what, block, rng, [len(d) for d in docs][:20])


PIECES = [b"a", b"hello", b" world", "é".encode(), "中".encode(), b"\xe4", b"\xb8", b"\xad", b"\xb8\xad", b"\xe4\xb8", b"\xa0\xe9\x99\xa4", b"\xe0\xae\xbf\xe0\xae",
          b"\xaf\x8d", "😀".encode(), b"\xf0\x9f", b"\x98\x80", b"\x80", b"<|endoftext|>", b"x" * 37]


def test_span_rule_small_cases():
    check_spans([])
    check_spans([[]])
    check_spans([[], [], []])
    check_spans([[b"hello", b" world"]])
    check_spans([[b"\x80"]])  # a document of a single continuation-byte token
    check_spans([[b"\x80"], [b"\xbf"], [], [b"\x80"]])
    check_spans([[b"\x80", b"\xbf", b"\x80", b"a", b"\x80"]])  # starts with several such tokens: all clamp to 0
    check_spans([[b"a"], [b"\x80", b"\xbf", b"\xad", b"b", b"\xb8"], [b"\xb8\xad", b"\xad"]])  # the clamp is per document
    check_spans([[b"\xe4", b"\xb8", b"\xad", b"\xe4\xb8", b"\xad"]])
    check_spans([[], [b"a"], [], [], [b"b", b"c"], []])
    check_spans([[b"a"] * 5] + [[]] * 40 + [[b"b"] * 20] + [[]] * 70)  # runs of empty documents, inside and at the end of the batch


def test_span_rule_document_boundaries_around_a_block():
    """A document boundary at every position relative to a 2048-token workgroup (and to its lanes of eight)."""
    rng = random.Random(11)
    stream = [rng.choice(PIECES) for _ in range(2 * 2048 + 40)]
    for cut in list(range(2030, 2070)) + [0, 1, 7, 8, 9, 4095, 4096, 4097, len(stream)]:
        check_spans([stream[:cut], stream[cut:]], blocks=(2048,))
        check_spans([stream[:cut], [], stream[cut:cut + 3], stream[cut + 3:]], blocks=(2048,))
    for cut in range(0, 64):  # every position of a small workgroup
        check_spans([stream[:cut], stream[cut:100]], blocks=(16,))
    # a document longer than several workgroups, then short ones
    check_spans([stream[:4000], stream[4000:4001], [], stream[4001:]], blocks=(8, 2048))


def test_span_rule_random_batches():
    rng = random.Random(0x0FF5)
    for _ in range(300):
        docs = []
        for _ in range(rng.choice([1, 2, 5, 40])):
            r = rng.random()
            k = 0 if r < 0.15 else 1 if r < 0.3 else rng.choice([2, 7, 8, 9, 30, 200, 5000 if rng.random() < 0.1 else 60])
            docs.append([rng.choice(PIECES[-4:-2] + PIECES[5:8] if rng.random() < 0.2 else PIECES) for _ in range(k)])
        check_spans(docs, blocks=(8, 32, 2048))


# ---------------------------------------------------------------- strict UTF-8
def first_invalid(docs: list[bytes]):
    for d, doc in enumerate(docs):
        try:
            doc.decode("utf-8", "strict")
        except UnicodeDecodeError:
            return d
    return None


def sim_first_invalid(docs: list[bytes], order=None):
    blob, off = h.pack(docs)
    n = len(blob)
    buf = np.ascontiguousarray(blob) if n else np.zeros(1, np.uint8)
    lanes = None
    if order is not None:
        lanes = np.arange((n + 15) // 16, dtype=np.uint64)
        random.Random(order).shuffle(lanes)
    r = lib().ofs_utf8_first_invalid(buf.ctypes.data, n, off.ctypes.data, len(docs), lanes.ctypes.data if lanes is not None and len(lanes) else None)
    return None if r == NONE else int(r)


def check_utf8(docs: list[bytes], orders=(None, 1)):
    want = first_invalid(docs)
    for order in orders:
        got = sim_first_invalid(docs, order)
        assert got == want, (got, want, [d[:40] for d in docs][:8])


def check_one(seq: bytes):
    """One sequence as a document: alone, behind text that puts it at every offset of a lane, and between valid neighbours."""
    want = 0
    try:
        seq.decode("utf-8", "strict")
        want = None
    except UnicodeDecodeError:
        pass
    assert sim_first_invalid([seq]) == want, seq
    assert sim_first_invalid([b"ab", seq, "é".encode()]) == (None if want is None else 1), seq
    return want


def test_utf8_one_and_two_byte_sequences_exhaustively():
    for a in range(256):
        check_one(bytes([a]))
        for b in range(256):
            check_one(bytes([a, b]))
    for pad in range(0, 18):  # ... at every offset of a lane, and across two lanes
        for seq in (b"\xc3\xa9", b"\xc3", b"\xa9", b"\xc0\x80", b"\xc1\xbf", b"\xc2\x7f", b"\xdf\xbf", b"\xdf\xc0"):
            check_utf8([b"x" * pad + seq + b"y" * 20])
            check_utf8([b"x" * pad + seq])


def test_utf8_three_and_four_byte_forms():
    rng = random.Random(5)
    tails = [0x00, 0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC0, 0xFF]
    for lead in range(0xE0, 0x100):
        for second in range(256):
            for third in tails[:4] + [rng.randrange(256)] + tails[6:]:
                check_one(bytes([lead, second, third]))
                if lead >= 0xF0:
                    check_one(bytes([lead, second, third, rng.choice(tails + [rng.randrange(0x80, 0xC0)])]))
    # the edges by name: overlong forms, surrogates, the last code point and what lies above it
    for seq, ok in ((b"\xe0\x9f\xbf", False), (b"\xe0\xa0\x80", True), (b"\xed\x9f\xbf", True), (b"\xed\xa0\x80", False), (b"\xed\xbf\xbf", False), (b"\xee\x80\x80", True),
                    (b"\xf0\x8f\xbf\xbf", False), (b"\xf0\x90\x80\x80", True), (b"\xf4\x8f\xbf\xbf", True), (b"\xf4\x90\x80\x80", False), (b"\xf5\x80\x80\x80", False),
                    (b"\xef\xbf\xbf", True), (b"\xf8\x88\x80\x80\x80", False)):
        assert (check_one(seq) is None) == ok, seq
        for pad in range(0, 17):
            check_utf8([b"z" * pad + seq + b"z" * 3, b"ok"])


def test_utf8_document_boundary_inside_a_char():
    """A sequence cut by a document boundary is ill-formed in both documents: the first of them is reported."""
    for ch in ("é", "中", "😀"):
        seq = ch.encode()
        for cut in range(1, len(seq)):
            for pad in range(0, 34):
                docs = [b"p" * pad + seq[:cut], seq[cut:] + b"q" * 5]
                assert sim_first_invalid(docs) == 0 and first_invalid(docs) == 0
                assert sim_first_invalid([b"fine " * 3] + docs) == 1
                # only the second half is a document of its own kind: a stray continuation at a document's start
                check_utf8([b"p" * pad, seq[cut:] + b"q"])
                check_utf8([b"p" * pad + seq[:cut]])  # ... and an unfinished sequence at the end of the batch
                check_utf8([b"p" * pad + seq[:cut], b"", b""])
        for pad in range(0, 34):  # whole chars on both sides of the boundary are fine
            check_utf8([b"p" * pad + seq, seq + b"q", b"", seq])


def test_utf8_first_invalid_document_of_random_batches():
    rng = random.Random(0xBAD)
    units = [b"a", b"hello wor", "é".encode(), "中".encode(), "😀".encode(), b"\x80", b"\xbf", b"\xc2", b"\xe0\xa0", b"\xed\xa0\x80", b"\xf0\x90\x80", b"\xf4\x90", b"\xff",
             b"\xc0\x80", b"The quick brown fox jumps over the lazy dog. "]
    good = units[:5] + units[-1:]
    seen = set()
    for k in range(4000):
        docs = []
        for _ in range(rng.choice([1, 3, 8, 30])):
            pool = units if rng.random() < 0.15 else good
            docs.append(b"".join(rng.choice(pool) for _ in range(rng.choice([0, 1, 2, 5, 40]))))
        check_utf8(docs, orders=(None, k))
        seen.add(first_invalid(docs))
    assert None in seen and 0 in seen and len(seen) > 6
    for _ in range(2000):  # adversarial: random bytes, all documents
        docs = [bytes(rng.choice([rng.randrange(256), rng.randrange(0x80, 0x100), 0x41]) for _ in range(rng.randrange(0, 40))) for _ in range(rng.randrange(1, 6))]
        check_utf8(docs)
    big = ("The quick brown fox. " * 300 + "中文😀é").encode()
    check_utf8([big, big[:-1], big])
    check_utf8([big, big, big[1:]])
    check_utf8([big] * 3)
    check_utf8([])
    check_utf8([b"", b"", b""])
