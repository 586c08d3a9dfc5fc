"""The scan value of the normalising line sets on the CPU (tests/hostsim/line_norm_sim.cpp over tk_lines_rule.h, tk_line_set_rule.h):
a line cut at given places and folded with the join in two groupings, against the plain hash of tests/line_norm_ref.py's normal form."""
import ctypes

import numpy as np
import pytest

import helpers as h
import line_norm_ref as ref

SRCS = ("line_norm_sim.cpp", "tk_line_set_rule.h", "tk_lines_rule.h", "tk_fingerprint_rule.h", "tk_rows_rule.h", "tk_common.h")
UNITS = [b" ", b" ", b"\t", b"\r", b"\x0b", b"\x0c", b",", b".", b"~", b"a", b"z", b"A", b"Z", b"@", b"[", b"`", b"{", b"0", b"9", b"/", b":", b"\xc3\x89", b"\xa0", b"\x1f", b"\x7f"]
_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = h.build_sim("libline_norm_sim.so", SRCS, ("-Wall", "-Werror", "-Wno-unknown-pragmas"))
        vp, u64 = ctypes.c_void_p, ctypes.c_uint64
        _lib.line_norm_sim_fold.restype = _lib.line_norm_sim_plain.restype = ctypes.c_int64
        _lib.line_norm_sim_fold.argtypes = [ctypes.c_char_p, u64, vp, u64, u64, ctypes.c_uint32, vp]
        _lib.line_norm_sim_plain.argtypes = [ctypes.c_char_p, u64, u64, vp]
    return _lib


def fold(line, cuts, seed, normalize):
    out, c = np.zeros(5, np.uint64), np.array(list(cuts) + [0], np.uint64)
    assert lib().line_norm_sim_fold(line, len(line), c.ctypes.data, len(cuts), seed, normalize, out.ctypes.data) == 0, (line, cuts, normalize, "the groupings differ")
    return out.tolist()


def plain(line, seed):
    out = np.zeros(5, np.uint64)
    assert lib().line_norm_sim_plain(line, len(line), seed, out.ctypes.data) == 0
    return out.tolist()


@pytest.mark.parametrize("normalize", range(16))
def test_random_lines_cut_at_random_places(normalize):
    rng = np.random.default_rng(0x4E4F + normalize)
    empty = 0
    for i in range(250):
        n = int(rng.integers(0, 4 if i % 5 == 0 else 90))
        line = b"".join(UNITS[int(rng.integers(len(UNITS)))] for _ in range(n))
        cuts = sorted(int(c) for c in rng.integers(0, len(line) + 1, int(rng.integers(0, 7))))
        want = ref.normal_form(line, normalize)
        empty += not want
        got, exp = fold(line, cuts, i, normalize), plain(want, i)
        assert got[:3] == exp[:3] and got[3] == len(line) and got[4] == exp[4], (line, cuts, want)
    assert empty > 5  # (lines without a body are among them)


@pytest.mark.parametrize("line, normalize, want", [
    (b"a , b", 12, b"a b"), (b"a , b", 8, b"a  b"), (b"a" + b"," * 40 + b"b", 8, b"ab"), (b"  Page 3 of 17\r", 15, b"page 0 of 00"), (b" \t ", 4, b""),
    (b"\xc3\x89A9", 3, b"\xc3\x89a0"), (b"@[`{/:", 1, b"@[`{/:"), (b"@[`{/:~!", 8, b"")])
def test_named_lines_at_every_cut(line, normalize, want):
    assert ref.normal_form(line, normalize) == want
    for c in range(len(line) + 1):
        assert fold(line, [c], 7, normalize)[:3] == plain(want, 7)[:3], c
