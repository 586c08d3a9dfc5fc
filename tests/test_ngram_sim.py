"""The n-gram passes (tk_ngram.h) on the CPU: tests/hostsim/ngram_sim.cpp compiles the plain C++ they are made of
(tiktoken_amd/csrc/tk_ngram_rule.h) for the host -- the key, the probe, the smear across words, the counts per document -- and drives it
the way the kernels do, at tiles of 8 and 64 positions and at the shipped one.  Compared, value for value, with tests/ngram_ref.py, a
Python set of tuples.  The same driver also runs as a program of its own under the address and undefined-behaviour sanitizers."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import helpers as h
import ngram_ref as nr

SRCS = ("ngram_sim.cpp", "tk_ngram_rule.h", "tk_fingerprint_rule.h", "tk_rows_rule.h", "tk_common.h")
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = h.build_sim("libngram_sim.so", SRCS, ("-Wall", "-Werror", "-Wno-unknown-pragmas"))
        vp, u64, u32, i64 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int64
        for name, res, args in (("create", vp, [u32, u64, u64, ctypes.POINTER(i64)]), ("destroy", None, [vp]), ("count", u64, [vp]), ("add", i64, [vp, vp, u64, vp, u64, u32]),
                                ("overlap", i64, [vp, vp, u64, vp, u64, u32, vp, vp, vp, vp, vp]), ("tile", u32, [])):
            f = getattr(_lib, "ngram_sim_" + name)
            f.restype, f.argtypes = res, args
    return _lib


def sim(k, capacity, held, tok, off, tile, seed=5):
    """`held` added, one document an n-gram, then the batch asked: (the set's count, the overlap as a Ref); the status where refused"""
    rc = ctypes.c_int64()
    s = lib().ngram_sim_create(k, seed, capacity, ctypes.byref(rc))
    if not s:
        return rc.value
    try:
        a_tok, a_off = nr.as_docs(held, k)
        a_pad, pad = np.append(a_tok, np.uint32(0)), np.append(tok, np.uint32(0))  # (no empty array's pointer)
        rc = lib().ngram_sim_add(s, a_pad.ctypes.data, len(a_tok), a_off.ctypes.data, len(held), tile)
        if rc:
            return rc
        n, out = len(off) - 1, [np.full(len(off), 7, np.uint64) for _ in range(4)] + [np.full(len(tok) + 1, 7, np.uint8)]
        rc = lib().ngram_sim_overlap(s, pad.ctypes.data, len(tok), off.ctypes.data, n, tile, *[a.ctypes.data for a in out])
        assert rc == 0 and all(a[-1] == 7 for a in out), (rc, "or written behind an array")
        return lib().ngram_sim_count(s), nr.Ref(*[a[:n] for a in out[:4]], np.diff(off), out[4][:-1])
    finally:
        lib().ngram_sim_destroy(s)


@pytest.mark.parametrize("k", nr.KS)
def test_every_shape_at_every_tile(k):
    T = lib().ngram_sim_tile()
    cases = nr.batches(64, k) + [c for c in nr.batches(T, k) if c[0].startswith("edge")] + [(f"S{S}", *nr.small_table(k, S, seed=5)) for S in (4, 8)]
    for name, tok, off, held in cases:
        want = nr.overlap(held, tok, off, k)
        for tile in (8, 64, T):
            count, got = sim(k, int(name[1:]) // 2 if name[0] == "S" else max(len(held) * k, 1), held, tok, off, tile)
            assert count == len(held), (name, tile)
            for f in nr.Ref._fields:
                assert (getattr(got, f) == getattr(want, f)).all(), (name, tile, f, np.flatnonzero(getattr(got, f) != getattr(want, f))[:8])


def test_refusals_and_a_case_by_hand():
    tok, off = nr.pack([3, 4], 1)
    assert [sim(k, c, set(), tok, off, 64) for k, c in ((0, 8), (33, 8), (2, 0), (2, 2 ** 30 + 1))] == [-1, -1, -2, -2]
    assert sim(2, 3, {(1, 2), (3, 4)}, tok, off, 64) == -30 and sim(2, 4, set(), tok, off, 6) == -10
    count, got = sim(3, 16, {(5, 6, 7)}, np.array([5, 6, 7, 5, 6, 7, 7], np.uint32), np.array([0, 0, 5, 7], np.uint64), 8)
    assert (count, got.n_hit.tolist(), got.n_covered.tolist(), got.n_ngrams.tolist(), got.first_hit.tolist()) == (1, [0, 1, 0], [0, 3, 0], [0, 3, 0], [nr.NONE, 0, nr.NONE])
    assert got.mask.tolist() == [1, 1, 1, 0, 0, 0, 0]  # (5 6 7 | 5 6 ... 7 7: no n-gram crosses a document)


def test_case_list_under_sanitizers(tmp_path):
    """tests/hostsim/ngram_sanitize.cpp, built with -fsanitize=address,undefined and run directly: clean, and the same at every tile."""
    exe = str(tmp_path / "ngram_sanitize")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         os.path.join(h.HOSTSIM, "ngram_sanitize.cpp"), "-o", exe], capture_output=True, text=True)
    if cc.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|cannot find lib(asan|ubsan)|lib(asan|ubsan)\S*: No such file", cc.stderr):
        pytest.skip("this g++ has no sanitizer runtime")  # (the linker says so; any other diagnostic is a failure)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "ngram_sanitize ok" in run.stdout, run.stdout + run.stderr
