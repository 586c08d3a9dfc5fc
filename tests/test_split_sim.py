"""The split passes (tk_split.h) on the CPU: tests/hostsim/split_sim.cpp compiles the plain C++ they are made of
(tiktoken_amd/csrc/tk_split_rule.h) for the host and drives it the way the kernels do -- class planes by "wavefronts" of 64 in workgroups of
64 and 2048, a walk per block of K = 64, 128 and 4096, the stitch per document, fold and count with count blocks of 64 and 2048, scan, write.
Every array is read through a reader that checks the index and every output sits in front of a guard word.  Compared array for array with
tests/split_ref.py, the rule as a loop per document written from its description (include/tiktoken_amd.h).  The same driver also runs as a
program of its own under the address and undefined-behaviour sanitizers (host code only: nothing of it is loaded into Python)."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

import helpers as h
import split_ref as sr
from tiktoken_amd._tiktoken import CoreBPE

SRCS = ("split_sim.cpp", "sim_readers.h", "tk_split_rule.h", "tk_rows_rule.h", "tk_common.h")
_lib = None
G = 0xDEADBEEF
SHAPES = ((64, 64), (2048, 2048), (64, 2048))  # (workgroup of the class pass, count block)
KS = (64, 128, 4096)


def lib():
    global _lib
    if _lib is None:
        L = h.build_sim("libsplit_sim.so", SRCS, ("-Wall", "-Werror", "-I" + os.path.join(h.ROOT, "include")))
        vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
        L.split_sim.restype = ctypes.c_int64
        L.split_sim.argtypes = [vp, u64, vp, vp, u64, u64, vp, vp, vp, vp, vp, u32, u32, *[vp] * 10]
        _lib = L
    return _lib


def pack(docs, doc_lens):
    """the arrays a call takes: text, doc_off, tok_off and the spans"""
    text = np.frombuffer(b"".join(docs) + b"\0", np.uint8)[:-1].copy()
    doc_off = np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64)
    tok_off = np.cumsum([0] + [len(x) for x in doc_lens]).astype(np.uint64)
    bs, cs, byte_off, char_off = [], [], [0], [0]
    for t, lens in zip(docs, doc_lens):
        b, c = sr.spans(t, lens)
        bs += b[:-1]
        cs += c[:-1]
        byte_off.append(byte_off[-1] + b[-1])
        char_off.append(char_off[-1] + c[-1])
    return text, doc_off, tok_off, np.array(bs, np.uint32), np.array(cs, np.uint32), np.array(byte_off, np.uint64), np.array(char_off, np.uint64)


def run_sim(docs, doc_lens, N, M, O, separators, K, block, cb, tok_off=None):
    text, doc_off, real_off, bs, cs, byte_off, char_off = pack(docs, doc_lens)
    T, n_docs = int(real_off[-1]), len(docs)
    tok_off = real_off if tok_off is None else np.asarray(tok_off, np.uint64)
    spec = CoreBPE._split_spec(N, M, O, separators, K)
    outs = [np.full(T + 2, G, np.uint32) for _ in range(7)] + [np.full(T + 2, 0xAB, np.uint8), np.full(n_docs + 2, G, np.uint32)]
    stats = np.zeros(4, np.uint64)
    pad = [a if len(a) else np.zeros(1, a.dtype) for a in (text, bs, cs)]
    rc = lib().split_sim(pad[0].ctypes.data, len(text), doc_off.ctypes.data, tok_off.ctypes.data, n_docs, T, pad[1].ctypes.data, pad[2].ctypes.data, byte_off.ctypes.data,
                         char_off.ctypes.data, ctypes.byref(spec), block, cb, *[a.ctypes.data for a in outs], stats.ctypes.data)
    if rc < 0:
        return rc, None, stats
    C = int(rc)
    for a in outs[:8]:
        assert (a[C:] == (0xAB if a.dtype == np.uint8 else G)).all(), "written behind the last chunk"
    assert outs[8][-1] == G
    return 0, sr.Chunks(*[a[:C] for a in outs[:8]], outs[8][:n_docs + 1]), stats


def check(docs, doc_lens, N, M, O=0, separators=sr.DEFAULT, ks=KS, shapes=SHAPES):
    want = sr.split_rule(docs, doc_lens, N, M, O, separators)
    stats = None
    for K in ks:
        for block, cb in shapes:
            rc, got, stats = run_sim(docs, doc_lens, N, M, O, separators, K, block, cb)
            assert rc == 0, (rc, N, M, O, K, block, cb)
            sr.same(got, want, (N, M, O, K, block, cb))
    return want, stats


WORDS = ["a", "the", "of", "chunk", "token", "x", "splitting", "3.14", "é", "日本語", "😀", "naïve", "Zürich"]


def prose(rng, n_words, para=0.05, line=0.08, stop=0.15):
    out = []
    for _ in range(n_words):
        out.append(rng.choice(WORDS))
        r = rng.random()
        out.append("\n\n" if r < para else "\n" if r < para + line else rng.choice([". ", "? ", "! "]) if r < para + line + stop else " ")
    return "".join(out).encode("utf-8")


def tokenise(rng, text: bytes, longest=5):
    """random token lengths that add up to the text: tokens begin and end anywhere, inside chars too"""
    lens, p = [], 0
    while p < len(text):
        n = min(rng.randint(1, longest), len(text) - p)
        lens.append(n)
        p += n
    return lens


def test_a_case_worked_by_hand():
    """One document "aa bb. cc dd\\n\\nee ff gg" (22 bytes) in tokens of three bytes, the last of one: n = 8, boundaries 1 .. 7 at bytes
    3, 6, 9, 12, 15, 18, 21.  With the default separators boundary 2 lies behind "." and before " " (level 2; it also matches level 3, the
    lower wins), boundary 3 before " " (level 3), the others match nothing (boundary 4 lies before the blank line, not behind it).
    N = 5, M = 2: from s = 0 the window is 2 .. 5, its lowest level is 2, at e = 2.  From s = 2, 8 - 2 > 5, the window 4 .. 7 has no level:
    a hard cut at the last legal boundary, 7.  From s = 7 one token is left: the end.  Written down for the restatement and the simulation."""
    text = b"aa bb. cc dd\n\nee ff gg"
    lens = [3, 3, 3, 3, 3, 3, 3, 1]
    want = sr.split_rule([text], [lens], 5, 2)
    assert want.tok_begin.tolist() == [0, 2, 7] and want.tok_end.tolist() == [2, 7, 8] and want.doc.tolist() == [0, 0, 0]
    assert want.cut.tolist() == [2, sr.HARD, sr.END] and want.byte_begin.tolist() == [0, 6, 21] and want.byte_end.tolist() == [6, 21, 22]
    assert want.char_begin.tolist() == [0, 6, 21] and want.char_end.tolist() == [6, 21, 22] and want.doc_chunk.tolist() == [0, 3]
    check([text], [lens], 5, 2, ks=(64,))


def test_random_prose_every_block_shape():
    rng = random.Random(0x5117)
    docs = [prose(rng, n) for n in (0, 1, 40, 0, 200, 700, 3, 0)]
    lens = [tokenise(rng, d) for d in docs]
    for N, M, O in ((7, 2, 0), (7, 2, 1), (16, 8, 3), (200, 100, 0), (40, 37, 36)):
        check(docs, lens, N, M, O)


def test_segments_join_on_prose_and_not_on_separator_free_text():
    """K = 64: in prose the true chain meets the speculative walks (joined > 0).  In text without separators and with every boundary legal
    every cut is hard, so the true chain stands on the multiples of N and a speculative walk of block b on 64 b + (N - M) + j N: with
    N = 16, M = 8 these never meet (64 b + 8 is no multiple of 16), and the result is exact all the same."""
    rng = random.Random(7)
    text = prose(rng, 3000)
    _, stats = check([text], [tokenise(rng, text, 3)], 16, 8, ks=(64,), shapes=((64, 64),))
    assert stats[1] > 0 and stats[0] > 1
    flat = b"x" * 5000
    _, stats = check([flat], [[1] * 5000], 16, 8, ks=(64,), shapes=((64, 64),))
    assert stats[1] == 0 and stats[3] > 0 and stats[2] > 0


def test_steps_that_jump_whole_blocks():
    rng = random.Random(11)
    docs = [prose(rng, n) for n in (1, 30, 31, 32, 150, 2500)]
    docs = [b""] + [x for d in docs for x in (d, b"")]
    check(docs, [tokenise(rng, d, 2) for d in docs], 200, 100, ks=(64, 128))
    check(docs, [tokenise(rng, d, 2) for d in docs], 200, 150, 40, ks=(64,))


def test_separators_tail_head_both_and_document_edges():
    s16 = "0123456789abcdef"
    seps = [[(s16, "")], [("", s16)], [("ab", "cd")], [("\n", ""), ("", "\n")]]
    rng = random.Random(3)
    body = "".join(rng.choice(["x", "yy", s16, "abcd", "\n", "ab", "cd"]) for _ in range(600)).encode()
    docs = [s16.encode() + body + s16.encode(), b"cd" + body[:50] + b"ab", b"\n" * 30]
    lens = [tokenise(rng, d, 4) for d in docs]
    check(docs, lens, 9, 3, 0, seps, ks=(64,))
    check(docs, lens, 9, 3, 2, seps, ks=(128,), shapes=((64, 64),))
    check(docs, lens, 9, 3, 0, [], ks=(64,), shapes=((64, 64),))  # L = 0: hard cuts only
    four = [[(c + str(i), "") for i in range(4)] for c in "xy\nd"]
    check(docs, lens, 9, 3, 0, four, ks=(64,), shapes=((64, 64),))


def test_ill_formed_text_forces_cuts():
    text = b"ab " + b"\x80" * 40 + b" cd" * 10
    lens = [1] * len(text)
    want, _ = check([text], [lens], 7, 2, ks=(64,))
    assert sr.FORCED in want.cut.tolist()


def test_wide_windows_take_the_one_thread_search():
    """(N - M) / 64 + 2 words of L + 1 planes are more than 64: the window is searched word by word"""
    rng = random.Random(5)
    text = prose(rng, 4000)
    check([text], [tokenise(rng, text, 2)], 1200, 10, 9, ks=(4096, 64), shapes=((2048, 2048),))


def test_refusals():
    docs, lens = [b"abc def"], [[3, 4]]
    for N, M, O, K, why in ((5, 0, 0, 64, 1), (5, 3, 0, 64, 2), (9, 3, 3, 64, 3), (9, 3, 0, 65, 8)):
        rc, _, _ = run_sim(docs, lens, N, M, O, sr.DEFAULT, K, 64, 64)
        assert rc == -(16 + why)
    rc, _, _ = run_sim(docs, lens, 9, 3, 0, [[("", "")]], 64, 64, 64)
    assert rc == -(16 + 7)
    # tok_off: nothing is indexed with an array that does not ascend from 0 to T
    for off, key in (([1, 2], (0 << 2) | 1), ([0, 3], (0 << 2) | 3)):
        rc, _, _ = run_sim(docs, lens, 9, 3, 0, sr.DEFAULT, 64, 64, 64, tok_off=off)
        assert rc == -(64 + key), rc
    rc, _, _ = run_sim(docs * 2, lens * 2, 9, 3, 0, sr.DEFAULT, 64, 64, 64, tok_off=[0, 5, 4])
    assert rc == -(64 + ((1 << 2) | 2))


def test_case_list_under_sanitizers(tmp_path):
    """tests/hostsim/split_sanitize.cpp: the driver as a program of its own, built with -fsanitize=address,undefined, on random batches in
    heap blocks of exactly their size: it must run clean and find its own invariants (budget, tiling, ascending starts) intact."""
    exe = str(tmp_path / "split_sanitize")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         os.path.join(h.HOSTSIM, "split_sanitize.cpp"), "-o", exe], capture_output=True, text=True)
    if cc.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|cannot find lib(asan|ubsan)|lib(asan|ubsan)\S*: No such file", cc.stderr):
        pytest.skip("this g++ has no sanitizer runtime")  # (the linker says so; any other diagnostic is a failure)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "split_sanitize ok" in run.stdout
