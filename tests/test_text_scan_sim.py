"""The scan elements of the word statistics and of the line cleaning (tk_words.h, tk_clean.h) on the CPU: tests/hostsim/text_scan_sim.cpp
compiles the plain C++ they are made of (tk_words_rule.h, tk_clean_rule.h) for the host -- the masks of a lane, the 20-byte and 28-byte
elements, their joins, the words and lines handed out at the cuts -- and scans them in the kernels' order at any geometry: L lanes a
tile, P tiles a thread of the carry pass, W lanes a wavefront.  Compared, value for value, with tests/words_ref.py and
tests/clean_ref.py, at geometries that put a tile, stretch and group edge at nearly every 16th byte, at every shift against the 16-byte
grid, and geometry against geometry.  The same driver also runs as a program of its own under the address and undefined-behaviour
sanitizers."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import clean_ref as cr
import helpers as h
import words_ref as wr

SRCS = ("text_scan_sim.cpp", "tk_words_rule.h", "tk_clean_rule.h", "tk_line_set_rule.h", "tk_lines_rule.h", "tk_fingerprint_rule.h", "tk_rows_rule.h", "tk_common.h")
GEOMETRIES = [(256, 1, 64), (4, 1, 4), (4, 2, 4), (1, 3, 2), (16, 3, 4)]  # (lanes a tile, tiles a thread of the carry, lanes a wavefront)
T, LANE, WAVE = 4096, 16, 1024  # the shipped geometry the named batches are built from
WORD_FIELDS = ("n_words", "word_chars", "n_alpha_words", "stop_mask", "n_ellipsis")
CLEAN_FIELDS = ("n_lines", "n_short", "n_long", "n_no_end", "n_ellipsis", "n_phrase")
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = h.build_sim("libtext_scan_sim.so", SRCS, ("-Wall", "-Werror", "-Wno-unknown-pragmas"))
        vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
        _lib.text_scan_sim_words.restype = _lib.text_scan_sim_clean.restype = ctypes.c_int64
        _lib.text_scan_sim_words.argtypes = [vp, vp, u64, vp, vp, u64, vp, u32, u32, u32, vp]
        _lib.text_scan_sim_clean.argtypes = [vp, vp, u64, u64, u64, u32, vp, u64, vp, vp, u64, u32, u32, u32, vp, vp, u64]
    return _lib


@functools.lru_cache(maxsize=None)
def letters():
    """a bit per code point: str.isalpha"""
    return np.packbits(np.array([chr(c).isalpha() for c in range(0x110000)], np.uint8), bitorder="little")


def blob(items):
    """(bytes, offsets) of a list of byte strings, with a byte behind them so that no array is empty"""
    off = np.concatenate([[0], np.cumsum([len(s) for s in items])]).astype(np.uint64)
    return np.frombuffer(b"".join(items) + b"\0", np.uint8), off


def sim_words(docs, stop, geometry):
    text, off = wr.pack(docs)
    text, (sb, so), out = np.append(text, np.uint8(0)), blob(stop), np.full(5 * (len(docs) + 1), 7, np.uint64)
    rc = lib().text_scan_sim_words(text.ctypes.data, off.ctypes.data, len(docs), sb.ctypes.data, so.ctypes.data, len(stop), letters().ctypes.data, *geometry, out.ctypes.data)
    assert rc == 0 and (out[5 * len(docs):] == 7).all(), (rc, "or written behind the array")
    return dict(zip(WORD_FIELDS, out[:5 * len(docs)].reshape(5, -1)))


def sim_clean(docs, rules, geometry):
    """(the six counts per document, the starts of the dropped lines)"""
    r = {**cr.C4, **rules}
    text, off = cr.pack(docs)
    n, cap = len(docs), len(text) + 1
    text, (pb, po), term = np.append(text, np.uint8(0)), blob(list(r["line_phrases"])), np.frombuffer(bytes(r["terminal"]) + b"\0", np.uint8)
    out, starts = np.full(6 * (n + 1), 7, np.uint64), np.full(cap + 1, 7, np.uint64)
    rc = lib().text_scan_sim_clean(text.ctypes.data, off.ctypes.data, n, r["min_words"], r["max_word_chars"], int(r["drop_ellipsis"]), term.ctypes.data, len(r["terminal"]),
                                   pb.ctypes.data, po.ctypes.data, len(r["line_phrases"]), *geometry, out.ctypes.data, starts.ctypes.data, cap)
    assert rc >= 0 and (out[6 * n:] == 7).all() and (starts[rc:] == 7).all(), (rc, "or written behind an array")
    return dict(zip(CLEAN_FIELDS, out[:6 * n].reshape(6, -1))), starts[:rc]


def dropped_starts(docs, rules):
    """where the lines start that the reference drops: its pieces, each judged by the reference as a document of its own"""
    r, out, base = {**cr.C4, **rules, "doc_phrases": ()}, [], 0
    for t in docs:
        for m in re.finditer(rb"[^\n]+\n?|\n", bytes(t)):
            if m.group() != b"\n" and not cr.doc_clean(m.group(), r)[0]:
                out.append(base + m.start())
        base += len(t)
    return np.array(out, np.uint64)


@functools.lru_cache(maxsize=None)
def word_cases():
    return {name: (docs, stop, wr.stats(docs, stop, term)) for name, (docs, stop, term) in wr.batches(T, LANE, WAVE).items()}


@functools.lru_cache(maxsize=None)
def clean_cases():
    return {name: (docs, rules, cr.clean(docs, **rules), dropped_starts(docs, rules)) for name, (docs, rules) in cr.batches(T, LANE, WAVE).items()}


def same(got, want, fields, what):
    for f in fields:
        a, b = got[f], np.asarray(want[f] if isinstance(want, dict) else getattr(want, f))
        assert a.shape == b.shape and (a == b).all(), (what, f, np.argwhere(a != b)[:8].tolist(), a[a != b][:8], b[a != b][:8])


def same_starts(got, want, what):
    assert len(got) == len(want) and (got == want).all(), (what, "dropped starts", len(got), len(want), sorted(set(got.tolist()) ^ set(want.tolist()))[:8])


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "L%d-P%d-W%d" % g)
def test_named_batches_of_the_word_statistics(geometry):
    for name, (docs, stop, want) in word_cases().items():
        same(sim_words(docs, stop, geometry), want, WORD_FIELDS, (name, geometry))


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "L%d-P%d-W%d" % g)
def test_named_batches_of_the_line_cleaning(geometry):
    for name, (docs, rules, want, starts) in clean_cases().items():
        got, got_starts = sim_clean(docs, rules, geometry)
        same(got, want, CLEAN_FIELDS, (name, geometry))
        same_starts(got_starts, starts, (name, geometry))


def short_text():
    """a few hundred bytes in four documents: every white-space char, a word of continuation bytes alone, dot runs, the ellipsis char,
    a line phrase, and document boundaries inside a dot run, inside a white-space char and behind a newline"""
    u = lambda s: s.encode()  # noqa: E731
    spaces = "\t\x0b\x0c\r\x1c\x1d\x1e\x1f \x85\xa0\u1680\u2000\u2001\u2002\u2003\u2004\u2005\u2006\u2007\u2008\u2009\u200a\u2028\u2029\u202f\u205f\u3000"
    assert len(spaces) == 28 and all(c.isspace() for c in spaces)  # (and '\n', which ends the lines below)
    return [u("the w" + "x".join(spaces) + "end.\n") + b"aa \x96\x96 bb cc dd.\n\x96 alone and of that.\nto be... or not to be....\n" + u("wait\u2026 so it ends\u2026\n") +
            b"Our Privacy Policy is here today.\nfive words in this one..",
            b".... have \xc3\xa9t\xc3\xa9 with them all.\nshort.\n\nno end on this line\xe2\x80",
            b"\xa8and a cut space before.\n",
            u("\u4e2d\u6587 and \u03a9 of . .. ... .......\nlast line is open")]


@functools.lru_cache(maxsize=None)
def short_case():
    docs = short_text()
    return docs, wr.stats(docs), cr.clean(docs), dropped_starts(docs, {})


@pytest.mark.parametrize("geometry", [(1, 2, 2), (4, 1, 4)], ids=lambda g: "L%d-P%d-W%d" % g)
def test_every_feature_at_every_position_of_the_grid(geometry):
    """0 to 31 bytes of an earlier document before the short text: the results are the unshifted ones behind the prefix document's"""
    docs, w_want, c_want, starts = short_case()
    assert 200 < sum(map(len, docs)) < 1000 and w_want.n_ellipsis.sum() > 5 and all(getattr(c_want, f).sum() for f in CLEAN_FIELDS[1:] if f != "n_long")
    for k in range(32):
        prefix = (b"An earlier document of five words. " * 2)[:k]
        w_pre, c_pre = wr.stats([prefix]), cr.clean([prefix])
        what = ("a prefix of", k, geometry)
        same(sim_words([prefix] + docs, wr.GOPHER, geometry), {f: np.concatenate([getattr(w_pre, f), getattr(w_want, f)]) for f in WORD_FIELDS}, WORD_FIELDS, what)
        got, got_starts = sim_clean([prefix] + docs, {}, geometry)
        same(got, {f: np.concatenate([getattr(c_pre, f), getattr(c_want, f)]) for f in CLEAN_FIELDS}, CLEAN_FIELDS, what)
        same_starts(got_starts, np.concatenate([dropped_starts([prefix], {}), starts + np.uint64(k)]), what)


def random_batches(n_batches=40):
    """seeded batches over a small alphabet -- space, newline, '.', 'a', 'A', a continuation byte, C3, A9, U+2028 -- cut into documents
    at random positions, some of them empty"""
    rng = np.random.default_rng(0x7C5A)
    units = [b" ", b"\n", b".", b"a", b"A", b"\x96", b"\xc3", b"\xa9", b"\xe2\x80\xa8"]
    for i in range(n_batches):
        data = b"".join(units[3 if rng.integers(4) == 0 else rng.integers(9)] for _ in range(int(rng.integers(4 if i % 6 == 0 else 3000))))
        cuts = sorted(int(c) for c in rng.integers(0, len(data) + 1, int(rng.integers(1, 12))))
        cuts = [0] + [c for c in cuts for _ in range(1 + (rng.integers(3) == 0))] + [len(data)]  # (a cut twice: an empty document)
        yield [data[a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def test_the_grouping_does_not_matter():
    rules = dict(min_words=3, max_word_chars=3, terminal=b".a", line_phrases=(b"a A", b".."))
    n_words = n_dropped = 0
    for i, docs in enumerate(random_batches()):
        first = None
        for g in GEOMETRIES:
            w, (c, starts) = sim_words(docs, (b"a", b"aA", b"a.a"), g), sim_clean(docs, rules, g)
            first = first or (w, c, starts)
            same(w, first[0], WORD_FIELDS, (i, g))
            same(c, first[1], CLEAN_FIELDS, (i, g))
            same_starts(starts, first[2], (i, g))
        n_words, n_dropped = n_words + int(first[0]["n_words"].sum()), n_dropped + len(first[2])
    assert n_words > 1000 and n_dropped > 100  # (the batches are not trivial)


def test_refused_geometry():
    docs = [b"ab cd."]
    text, off = wr.pack(docs)
    out = np.zeros(8, np.uint64)
    sb, so = blob([b"the"])
    for g in ((0, 1, 4), (4, 0, 4), (4, 1, 0)):
        assert lib().text_scan_sim_words(text.ctypes.data, off.ctypes.data, 1, sb.ctypes.data, so.ctypes.data, 1, letters().ctypes.data, *g, out.ctypes.data) == -10


def test_random_batches_under_sanitizers(tmp_path):
    """tests/hostsim/text_scan_sanitize.cpp, built with -fsanitize=address,undefined and run directly: clean, and the same at every geometry."""
    exe = str(tmp_path / "text_scan_sanitize")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         os.path.join(h.HOSTSIM, "text_scan_sanitize.cpp"), "-o", exe], capture_output=True, text=True)
    if cc.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|cannot find lib(asan|ubsan)|lib(asan|ubsan)\S*: No such file", cc.stderr):
        pytest.skip("this g++ has no sanitizer runtime")  # (the linker says so; any other diagnostic is a failure)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "text_scan_sanitize ok" in run.stdout, run.stdout + run.stderr
