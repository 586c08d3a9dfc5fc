"""The text passes on the GPU past 1024 and 2048 tiles (tk_words.h, tk_lines.h, tk_line_set.h, tk_clean.h): the two batches of
tests/text_wide_cases.py, at which a thread of the carry kernels takes a stretch of two and of three tiles, more than four of their
sixteen wavefronts hold an element, and the kept-byte scans make a second and a third trip.  Value for value and byte for byte against
the references of the passes' own test files -- words_ref, lines_ref, line_set_ref, clean_ref --, each computed once per batch and
shared by the host entry and the device entry; the device entries write into poisoned outputs.  Nothing expected comes from the GPU."""
import functools

import numpy as np
import pytest

import clean_ref as cr
import line_set_ref as sr
import lines_ref as lr
import text_wide_cases as tw
import tiktoken_amd as tiktoken
import words_ref as wr
from test_gpu_clean import device_clean
from test_gpu_line_set import device_dedup
from test_gpu_lines import device_stats as device_line_stats
from test_gpu_words import device_stats as device_word_stats

pytestmark = pytest.mark.gpu
POISON = 0x55
T, LANE, BLOCK, WAVE = tw.T, tw.LANE, tw.BLOCK, tw.WAVE  # (checked against the shipped constants below)


def enc_of():
    return tiktoken.get_encoding("gpt2_shaped")


@functools.lru_cache(maxsize=None)
def packed(name):
    return wr.pack(tw.batch(name)[0])


@functools.lru_cache(maxsize=None)
def words_want(name):
    return wr.stats(tw.batch(name)[0])


@functools.lru_cache(maxsize=None)
def lines_want(name):
    return lr.stats(tw.batch(name)[0])


@functools.lru_cache(maxsize=None)
def clean_want(name, max_word_chars):
    return cr.clean(tw.batch(name)[0], max_word_chars=max_word_chars)


def equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)[:8]
    assert not len(bad), (what, "first differences at", bad.tolist(), got[bad].tolist(), want[bad].tolist())


def text_equal(buffer, want, what):
    """the kept bytes, and the poison behind them untouched"""
    equal(buffer[:len(want)], want, (*what, "text_out"))
    equal(buffer[len(want):], np.full(len(buffer) - len(want), POISON, np.uint8), (*what, "behind text_out"))


def fields_equal(got, want, fields, what):
    for f in fields:
        equal(getattr(got, f), getattr(want, f), (*what, f))


def clean_equal(got, want, what, device):
    if device:
        text_equal(got.text, want.text, what)
        equal(got.counts, want.counts, (*what, "counts"))
    else:
        equal(got.text, want.text, (*what, "text"))
    fields_equal(got, want, ("doc_off", *cr.FIELDS), what)


@pytest.mark.parametrize("name", tw.NAMES)
def test_geometry_and_landmarks(name):
    stat = enc_of()._core_bpe.stat
    assert stat("words_tile") == stat("lines_tile") == stat("clean_tile") == T and stat("words_lane") == stat("lines_lane") == stat("clean_lane") == LANE
    docs, mark = tw.batch(name)
    text, off = packed(name)
    N = len(text)
    n_tiles = N // T + 1
    per = -(-n_tiles // BLOCK)
    assert per == {"per2": 2, "per3": 3}[name] == mark["per"] and n_tiles == mark["n_tiles"] and N % LANE != 0 and not docs[-1].endswith(b"\n")
    assert BLOCK < n_tiles <= 1100 if name == "per2" else (n_tiles >= 2 * BLOCK + 2 and n_tiles % 3 != 0)
    # a dropped line right behind every placed newline: before and behind tile 1024, in per3 behind tile 2048 too
    starts = [p + 1 for p in mark["newlines"]]
    assert all(cr.doc_clean(line, cr.C4)[0] == b"" for line in tw.DROPPED) and all(any(bytes(text[s:s + len(d)]) == d for d in tw.DROPPED) for s in starts)
    assert min(starts) // T < BLOCK < max(starts) // T and max(starts) // T >= n_tiles - 2 and (per < 3 or max(starts) // T > 2 * BLOCK)
    want, long_doc = clean_want(name, 1000), mark["long doc"]
    hit = np.flatnonzero(want.doc_hit)
    assert hit.tolist() == [mark["phrase doc"]] and off[hit[0]] > (BLOCK + 1) * T
    assert want.n_long[long_doc] == 2 and lines_want(name).n_dup_lines[long_doc] >= 1
    kept = clean_want(name, 0)
    assert kept.n_long.sum() == 0 and len(kept.text) - len(want.text) > 3 * WAVE * per * T  # (the three copies are kept: each more than 64 per tiles)


@pytest.mark.parametrize("name", tw.NAMES)
def test_word_statistics(name):
    enc = enc_of()
    text, off = packed(name)
    got = enc.word_stats_packed(text, off, wr.GOPHER, wr.TERMINAL)
    equal(got.length, np.diff(off), (name, "host", "length"))
    fields_equal(got, words_want(name), wr.Ref._fields, (name, "host"))
    fields_equal(device_word_stats(enc, text, off, wr.GOPHER, wr.TERMINAL), words_want(name), wr.Ref._fields, (name, "device"))


def test_word_statistics_on_the_core_of_the_generic_engine():
    """a pat_str without a hand-written scanner: that core uploads class tables of its own, the word statistics read the library's"""
    import helpers as h

    enc = tiktoken.Encoding("camel_words", pat_str=r"\p{Lu}?\p{Ll}+|\p{Lu}+(?!\p{Ll})|\d{1,3}|[^\s\p{L}\d]+|\s+|.", mergeable_ranks=h.golden_vocab("o200k_shaped"), special_tokens={})
    text, off = packed("per2")
    fields_equal(enc.word_stats_packed(text, off, wr.GOPHER, wr.TERMINAL), words_want("per2"), wr.Ref._fields, ("per2", "generic engine", "host"))
    fields_equal(device_word_stats(enc, text, off, wr.GOPHER, wr.TERMINAL), words_want("per2"), wr.Ref._fields, ("per2", "generic engine", "device"))


@pytest.mark.parametrize("name", tw.NAMES)
def test_line_statistics(name):
    enc = enc_of()
    text, off = packed(name)
    got = enc.line_stats_packed(text, off, seed=3)
    equal(got.length, np.diff(off), (name, "host", "length"))
    fields_equal(got, lines_want(name), lr.Ref._fields, (name, "host"))
    fields_equal(device_line_stats(enc, text, off, seed=5), lines_want(name), lr.Ref._fields, (name, "device"))


@pytest.mark.parametrize("max_word_chars", [1000, 0])
@pytest.mark.parametrize("name", tw.NAMES)
def test_cleaning(name, max_word_chars):
    """C4's defaults; and without the longest-word rule, so that the long line's copies are kept and go through the write pass"""
    enc = enc_of()
    text, off = packed(name)
    want, rules = clean_want(name, max_word_chars), dict(max_word_chars=max_word_chars)
    clean_equal(cr.Ref(*enc.clean_lines_packed(text, off, **rules), want.counts), want, (name, max_word_chars, "host"), device=False)
    clean_equal(device_clean(enc, text, off, rules), want, (name, max_word_chars, "device"), device=True)


def test_cleaning_counting_only():
    """text_out omitted: no write pass; its buffer and doc_off_out stay poisoned, counts = (0, lines not written)"""
    text, off = packed("per2")
    want = clean_want("per2", 1000)
    got = device_clean(enc_of(), text, off, {}, skip=("text_out", "doc_off_out"))
    assert (got.text == POISON).all() and (got.doc_off == POISON).all()
    fields_equal(got, want, cr.FIELDS, ("per2", "counting only"))
    equal(got.counts, [0, int(want.counts[1])], ("per2", "counting only", "counts"))


def test_cleaning_unaligned():
    text, off = packed("per2")
    clean_equal(device_clean(enc_of(), text, off, {}, shift=1), clean_want("per2", 1000), ("per2", "shift 1"), device=True)


def dedup_equal(got, want, what, device):
    docs, n_lines, n_dropped = want
    text, off = lr.pack(docs)
    if device:
        text_equal(got["text_out"], text, what)
        equal(got["counts"], [len(text), int(n_dropped.sum())], (*what, "counts"))
        got = (got["doc_off_out"], got["n_lines"], got["n_dropped"])
    else:
        equal(got.text, text, (*what, "text"))
        assert got.n_dropped_total == n_dropped.sum(), what
        got = (got.doc_off, got.n_lines, got.n_dropped)
    for a, b, f in zip(got, (off, n_lines, n_dropped), ("doc_off", "n_lines", "n_dropped")):
        equal(a, b, (*what, f))


@pytest.mark.parametrize("name", tw.NAMES)
def test_line_set_two_calls_on_a_fresh_set(name):
    """the first call through the host entry drops the long line's later copies and every other repeat; the second, through the device
    entry, drops every line.  The capacity holds the first call's distinct lines and the second call's lines (include/tiktoken_amd.h)."""
    enc, docs, seen = enc_of(), tw.batch(name)[0], set()
    first = sr.dedup(seen, docs)
    second = sr.dedup(seen, docs)
    long_line = bytes(packed(name)[0][tw.batch(name)[1]["long line"][0]:]).split(b"\n", 1)[0]
    assert b"".join(first[0]).count(long_line) == 1 and first[2].sum() > 2 and second[2].sum() == second[1].sum() < 100_000
    with enc.line_set(len(seen) + int(second[1].sum()), seed=3) as ls:
        dedup_equal(ls.dedup_packed(*packed(name), add=True), first, (name, "first, host"), device=False)
        assert len(ls) == len(seen)
        dedup_equal(device_dedup(enc, ls, docs), second, (name, "second, device"), device=True)
        assert len(ls) == len(seen)


def test_line_set_within_one_call_unaligned():
    enc, docs, seen = enc_of(), tw.batch("per2")[0], set()
    want = sr.dedup(seen, docs)
    with enc.line_set(int(want[1].sum())) as ls:
        dedup_equal(device_dedup(enc, ls, docs, shift=1), want, ("per2", "shift 1"), device=True)
        assert len(ls) == len(seen)
