"""Word statistics on the GPU (tk_words.h): the entries through CoreBPE and Encoding, value for value against tests/words_ref.py --
str.split, str.isalpha, bytes.count --, never against another run of the code under test.  Every batch goes through the host entry and
through the device entry on a side stream into poisoned outputs."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import tiktoken_amd as tiktoken
import words_ref as wr
from tiktoken_amd._lib import last_error as lib_error

pytestmark = pytest.mark.gpu
POISON = 0x55
T, LANE, WAVE = 4096, 16, 1024  # (checked against the shipped constants below: the batches are named at collection, before a core exists)


def enc_of():
    return tiktoken.get_encoding("gpt2_shaped")


@functools.lru_cache(maxsize=None)
def cases():
    """{name: (text, doc_off, stop words, terminal, the reference's result)}, computed once"""
    return {name: (*wr.pack(docs), stop, term, wr.stats(docs, stop, term)) for name, (docs, stop, term) in wr.batches(T, LANE, WAVE).items()}


def device_stats(enc, text, off, stop, term, skip=(), shift=0):
    """tk_word_stats_device on a side stream: uploads, poison, the call and the copies back are queued there; `shift`: the text starts
    that many bytes behind an aligned pointer"""
    dev = torch.device("cuda", enc._core_bpe.device)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        t_text = torch.from_numpy(np.concatenate([np.zeros(shift, np.uint8), text])).to(dev, non_blocking=True)[shift:]
        t_off = torch.from_numpy(off.view(np.int64).copy()).to(dev, non_blocking=True)
        outs = [torch.full((len(off) - 1,), POISON, dtype=torch.int64, device=dev) for _ in wr.Ref._fields]
        enc._core_bpe.word_stats_device(t_text, t_off, stop_words=stop, terminal=term, **{n: o for n, o in zip(wr.Ref._fields, outs) if n not in skip})
        pinned = [torch.empty(o.shape, dtype=o.dtype, pin_memory=True) for o in outs]
        for h, o in zip(pinned, outs):
            h.copy_(o, non_blocking=True)
    stream.synchronize()
    return wr.Ref(*[h.numpy().view(np.uint64) for h in pinned])


def same(got, want, what, skip=()):
    for f in wr.Ref._fields:
        a, b = getattr(got, f), getattr(want, f)
        if f in skip:
            assert (a == POISON).all(), (what, f, "written though not asked for")
        else:
            assert a.shape == b.shape and (a == b).all(), (what, f, np.argwhere(a != b)[:8].tolist(), a[a != b][:8], b[a != b][:8])


def test_shipped_constants():
    stat = enc_of()._core_bpe.stat
    assert (stat("words_tile"), stat("words_lane"), stat("words_wave")) == (T, LANE, WAVE)


@pytest.mark.parametrize("name", list(wr.batches(T, LANE, WAVE)))
def test_batch_through_host_and_device_entries(name):
    enc = enc_of()
    text, off, stop, term, want = cases()[name]
    got = enc.word_stats_packed(text, off, stop, term)
    assert (got.length == np.diff(off)).all()
    same(wr.Ref(*got[1:]), want, (name, "host"))
    same(device_stats(enc, text, off, stop, term), want, (name, "device"))


def test_expected_values_by_hand():
    """ill-formed text and patterns cut by a document boundary: what the rule says, written out, against what both entries give"""
    enc = enc_of()
    for way in ("host", "device"):
        got = {}
        for name in ("ill-formed", "cut patterns", "stop words"):
            text, off, stop, term, _ = cases()[name]
            got[name] = wr.Ref(*enc.word_stats_packed(text, off, stop, term)[1:]) if way == "host" else device_stats(enc, text, off, stop, term)
        ill, cut, stops = got["ill-formed"], got["cut patterns"], got["stop words"]
        assert ill.n_words.tolist() == [2, 1, 2, 1, 1, 1, 2, 2] and ill.word_chars.tolist() == [3, 2, 3, 2, 1, 1, 1, 3], way
        assert ill.n_alpha_words.tolist() == [2, 1, 1, 1, 1, 0, 1, 1] and ill.n_ellipsis.tolist() == [0, 0, 0, 0, 0, 0, 0, 1], way
        assert cut.n_words.tolist() == [1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 1, 1] and not cut.n_ellipsis.any() and not cut.stop_mask.any(), way
        assert cut.n_alpha_words.tolist() == [1] * 9 + [2, 1, 1], way  # (C3 | A9 is no letter: "k" and "l" are)
        assert stops.stop_mask.tolist() == [1, 0, 2, 0xC0000004, 0x80000000, 0x81], way


@pytest.mark.parametrize("name", ["words and symbols", "chars at lane edge +0", "chars at tile edge +1"])
def test_core_of_the_generic_engine_reads_unicodes_letters(name):
    """a pat_str without a hand-written scanner: that core's own class tables call every char a letter; the word statistics must not"""
    import helpers as h

    enc = tiktoken.Encoding("camel_words", pat_str=r"\p{Lu}?\p{Ll}+|\p{Lu}+(?!\p{Ll})|\d{1,3}|[^\s\p{L}\d]+|\s+|.", mergeable_ranks=h.golden_vocab("o200k_shaped"), special_tokens={})
    text, off, stop, term, want = cases()[name]
    same(wr.Ref(*enc.word_stats_packed(text, off, stop, term)[1:]), want, (name, "host"))
    same(device_stats(enc, text, off, stop, term), want, (name, "device"))


@pytest.mark.parametrize("shift", [1, 15])
def test_unaligned_device_pointer(shift):
    enc = enc_of()
    for name in ("words and symbols", "chars at tile edge +0", "a word over three tiles"):
        text, off, stop, term, want = cases()[name]
        same(device_stats(enc, text, off, stop, term, shift=shift), want, (name, shift))


def test_null_outputs():
    enc = enc_of()
    text, off, stop, term, want = cases()["words and symbols"]
    for f in wr.Ref._fields:
        same(device_stats(enc, text, off, stop, term, skip=(f,)), want, ("without", f), skip=(f,))


def test_text_entries_and_keep_mask():
    enc = enc_of()
    good = ("the quick brown foxes jumped over that lazy sleeping hound with great ease. " * 4)[:-1]
    texts = [good, "", "too short to pass the rule of fifty words", "a b c d e f g h i j the of " * 9, "the and " + "incomprehensibilities " * 60,
             good + " #" * 9, good + " wait..." * 7, "the and " + "1234 5678 " * 30, "cat dog hat mat sat rat bat " * 9, good + "\nno end\nnor here", "naïve – these words and that " * 10]
    want = wr.stats([t.encode() for t in texts])
    got = enc.word_stats_batch(texts)
    same(wr.Ref(*got[1:]), want, "str")
    same(wr.Ref(*enc.word_stats_batch([t.encode() for t in texts], stop_words=[s.encode() for s in tiktoken._tiktoken.GOPHER_STOP_WORDS])[1:]), want, "bytes")
    text, off = wr.pack([t.encode() for t in texts])
    dev = torch.device("cuda", enc._core_bpe.device)
    for first in (text.tobytes(), bytearray(text.tobytes()), memoryview(text.tobytes()), text, torch.from_numpy(text.copy()).to(dev)):
        same(wr.Ref(*enc.word_stats_packed(first, off)[1:]), want, type(first).__name__)
    ratio = lambda a, b: a / np.where(b > 0, b, 1).astype(np.float64)  # noqa: E731  (a is 0 wherever b is)
    n_stop = np.array([bin(int(m)).count("1") for m in want.stop_mask])
    mean = ratio(want.word_chars, want.n_words)
    rules = [want.n_words >= 50, want.n_words <= 100_000, mean >= 3, mean <= 10, ratio(want.n_hash, want.n_words) <= .1, ratio(want.n_ellipsis, want.n_words) <= .1,
             ratio(want.n_alpha_words, want.n_words) >= .8, n_stop >= 2]
    punct = ratio(want.n_punct_lines, want.n_lines) >= .5
    assert all((~r).any() for r in rules[:1] + rules[2:]) and (~punct).any() and np.logical_and.reduce(rules)[[0, 9, 10]].all()  # (every rule but max_words fails somewhere)
    mask = got.keep_mask()
    assert mask.dtype == np.uint8 and mask.tolist() == np.logical_and.reduce(rules).astype(int).tolist()
    assert got.keep_mask(max_words=60).tolist() == (np.logical_and.reduce(rules) & (want.n_words <= 60)).astype(int).tolist()
    assert got.keep_mask(*[None] * 8).all() and got.keep_mask(*[None] * 8, .5).tolist() == punct.astype(int).tolist()
    assert got.n_stop_words().tolist() == n_stop.tolist()


def test_refusals():
    core = enc_of()._core_bpe
    text, off = np.frombuffer(b"ab the\ncd", np.uint8), np.array([0, 4, 9], np.uint64)
    out = np.full(2, POISON, np.uint64)
    dev = torch.device("cuda", core.device)
    d_text, d_off, d_out = torch.from_numpy(text.copy()).to(dev), torch.from_numpy(off.view(np.int64).copy()).to(dev), torch.full((2,), POISON, dtype=torch.int64, device=dev)
    bad = [("at most 32", [b"w%02d" % i for i in range(33)], b"."), ("1 to 8 bytes", [b"the", b""], b"."), ("1 to 8 bytes", [b"abcdefghi"], b"."),
           ("repeated", [b"the", b"of", b"the"], b"."), ("white space", [b"a b"], b"."), ("white space", [b"a\xe3\x80\x80b"], b"."), ("white space", [b"\xc2\x85"], b"."),
           ("below 0x80", [b"the"], b".\x80"), ("at most 16", [b"the"], bytes(range(33, 50)))]
    for why, stop, term in bad:
        with pytest.raises(ValueError):
            core.word_stats_device(d_text, d_off, stop_words=stop, terminal=term, n_words=d_out)
        assert why in lib_error() and (d_out.cpu().numpy() == POISON).all(), why
        blob, soff, t, args = core._word_args(stop, term)
        assert core._L.tk_word_stats(core._h, text.ctypes.data, off.ctypes.data, 2, *args, out.ctypes.data, *[ctypes.c_void_p()] * 7) != 0
        assert why in lib_error() and (out == POISON).all(), why
    blob, soff, t, args = core._word_args([b"the"], b".")
    for o in ([1, 4, 9], [0, 5, 4, 9], [0, 0xFFFF0001]):  # (not from 0; does not ascend; above the cap -- the host entry's refusals)
        o = np.array(o, np.uint64)
        assert core._L.tk_word_stats(core._h, text.ctypes.data, o.ctypes.data, len(o) - 1, *args, out.ctypes.data, *[ctypes.c_void_p()] * 7) != 0
        assert ("0xFFFF0000" if o[-1] > 9 else "doc_off") in lib_error() and (out == POISON).all()
