"""The UTF-8 repair passes (tk_utf8_repair.h) on the CPU: tests/hostsim/utf8_repair_sim.cpp compiles the plain C++ they are made of
(tiktoken_amd/csrc/tk_utf8_repair_rule.h) for the host and drives it the way the kernels do -- workgroups of 16, 256 (the kernels') and 2048 lanes, the lanes
in ascending, descending and shuffled order, a reader that refuses every index outside the contract, a writer that wants every output byte
stored exactly once.  Compared with the rule of include/tiktoken_amd.h restated in Python (tests/utf8_repair_ref.py), which is first
compared with CPython's own decoder on every input used here."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import helpers as h
import utf8_repair_ref as R

MODES = (R.REPLACE, R.IGNORE)
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = h.build_sim("libutf8_repair_sim.so", ("utf8_repair_sim.cpp", "tk_utf8_repair_rule.h", "tk_decode_rule.h", "tk_device.h", "tk_common.h"), ("-Wall", "-Werror"))
        vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
        L.u8r_run.restype = ctypes.c_int64
        L.u8r_run.argtypes = [vp, u64, vp, u64, u32, u32, u32, vp, vp, vp, vp, vp]
        _lib = L
    return _lib


def run(docs, mode, wg_lanes, order):
    blob, n, off = R.pack(docs)
    text = np.full(3 * n + 16, 0x5A, np.uint8)
    offs = np.full((3, len(docs) + 1), 0xDEAD, np.uint64)
    totals = np.zeros(5, np.uint64)
    rc = lib().u8r_run(blob.ctypes.data, n, off.ctypes.data, len(docs), mode, wg_lanes, order, text.ctypes.data, offs[0].ctypes.data, offs[1].ctypes.data, offs[2].ctypes.data,
                       totals.ctypes.data)
    return rc, text, offs, [int(t) for t in totals]


def check(docs, modes=MODES, wgs=(16, 256, 2048), orders=(0, 1, 2), cpython=True):
    for mode in modes:
        if cpython:
            R.check_against_cpython(docs, mode)
        want_text, *want_off = R.repair_batch(docs, mode)
        want_off = np.array(want_off, np.uint64)
        for wg in wgs:
            for order in orders:
                rc, text, offs, totals = run(docs, mode, wg, order)
                assert rc == 0, (rc, mode, wg, order)
                assert totals[0] == len(want_text) and totals[1] == want_off[1][-1] and totals[2] == want_off[2][-1], (totals, mode, wg, order)
                assert bytes(text[: totals[0]]) == want_text, (mode, wg, order, [d[:20] for d in docs][:6])
                assert np.array_equal(offs, want_off), (mode, wg, order)
                assert totals[3] == (1 if want_off[2][-1] else 0)  # the write pass runs exactly when a unit was replaced
    return totals


@pytest.fixture(scope="module")
def exhaustive():
    docs = R.exhaustive()
    assert len(docs) == 346201
    for mode in MODES:
        R.check_against_cpython(docs, mode)
    return docs


def test_exhaustive_small_sequences_each_a_document(exhaustive):
    assert 1_300_000 < sum(map(len, exhaustive)) < 1_400_000
    check(exhaustive, cpython=False)


def test_exhaustive_batch_as_one_document(exhaustive):
    check([b"".join(exhaustive)])


def test_sliding_sequences_and_boundaries_inside_them():
    """every case at workgroups of 16 lanes, of 256 (the kernels' geometry) and of 2048, each with its own edges, in all three orders"""
    for wg, wave in ((16, 64), (256, 1024), (2048, 1024)):
        for docs in R.sliding(16, wave, 16 * wg):
            check(docs, wgs=(wg,))


def test_runs_of_empty_documents():
    for docs in R.empties():
        check(docs)
    # a run of empty documents costs no lane more than one search
    e = [b""] * 70
    docs = e + [b"a" * 40] + e + [b"b" * 40] + e
    for order in (0, 2):
        rc, _, offs, totals = run(docs, R.REPLACE, 16, order)
        assert rc == 0 and totals[4] == 1
        assert offs[0].tolist() == R.repair_batch(docs, R.REPLACE)[1]


def test_growth_three_fold_over_several_workgroups():
    totals = check([b"\x80" * 5000])
    assert totals[2] == 5000
    rc, text, _, totals = run([b"\x80" * 5000], R.REPLACE, 16, 2)
    assert rc == 0 and totals[0] == 15000 and bytes(text[:15000]) == R.FFFD * 5000
    check([b"ab", b"\x80" * 5000, b"", b"\xbf" * 33, b"z"])


def test_growth_reaches_the_count_pass_s_bound():
    """R.growth: the most one workgroup leaves is 3 x its bytes + 3 -- the bound tk_k_u8r_count states for its 16-bit scan -- and the inputs
    reach it, by CPython's incremental decoder; the passes agree with the rule on them at the kernels' geometry and at a smaller one"""
    for block, wg in ((4096, 256), (256, 16)):
        most = []
        for docs in R.growth(block):
            per_wg = R.charged(docs, block)
            assert sum(per_wg) == len(R.repair_batch(docs, R.REPLACE)[0])
            most.append(max(per_wg))
            check(docs, wgs=(wg,), orders=(0, 2))
        assert most[0] == 3 * block and most[1:4] == [3 * block - 3 * k + 3 for k in (1, 2, 3)]  # a lead that its document's end cuts is charged there
        assert most[4:10] == [3 * block + 3] * 6 and max(most) == 3 * block + 3 < 1 << 16


def test_clean_text_takes_no_write_pass():
    clean = [("The quick brown fox. 中文😀é " * 40).encode(), b"", b"plain", "żółć".encode() * 500]
    for mode in MODES:
        for wg in (16, 256, 2048):
            rc, text, offs, totals = run(clean, mode, wg, 2)
            assert rc == 0 and totals[2] == 0 and totals[3] == 0
            assert bytes(text[: totals[0]]) == b"".join(clean)
            assert offs[1].tolist() == [0] + list(np.cumsum([len(d.decode()) for d in clean]))
    check(clean)


def test_same_length_does_not_mean_clean():
    docs = [b"abc\xf0\x9f\x98"]
    rc, text, offs, totals = run(docs, R.REPLACE, 16, 0)
    assert rc == 0 and totals[0] == 6 and totals[2] == 1 and totals[3] == 1
    assert bytes(text[:6]) == b"abc" + R.FFFD
    check(docs)
    check([b"\xf0\x9f\x98", b"\xf0\x9f\x98\x80"])


def test_degenerate_sizes():
    check([])  # n_docs == 0
    check([b""])
    check([b"", b"", b""])  # n_bytes == 0 with documents


def test_random_batches():
    for docs in R.random_batches(0x1CE, 300):
        check(docs, orders=(0, 2))


def test_offsets_that_do_not_ascend_to_n_are_refused():
    blob, n, off = R.pack([b"abc", b"de"])
    for bad, doc in (([0, 3, 4], 2), ([0, 4, 3], 1), ([1, 3, 5], 0), ([0, 3, 6], 2)):
        o = np.array(bad, np.uint64)
        out = np.zeros(64, np.uint8)
        offs = np.zeros((3, 3), np.uint64)
        totals = np.zeros(5, np.uint64)
        rc = lib().u8r_run(blob.ctypes.data, n, o.ctypes.data, 2, 0, 16, 0, out.ctypes.data, offs[0].ctypes.data, offs[1].ctypes.data, offs[2].ctypes.data, totals.ctypes.data)
        assert rc == 1000 + doc, (bad, rc)


# ---------------------------------------------------------------- the pooled batch of tests/test_gpu_text_passes_wide.py, without a GPU
WINDOWS = ((0, 5000), ((1 << 20) - 1070, (1 << 20) + 1030))  # a prefix, and the 2 100 documents around index 2^20, the last among them


def test_pooled_reference_is_the_per_document_one():
    pool, idx = R.wide_batch()
    assert len(idx) == R.WIDE_N == (1 << 20) + 1030 and R.WIDE_PREFIXES[-1] == R.WIDE_N
    for mode in MODES:
        R.check_against_cpython(pool, mode)  # ties the pooled reference to CPython's decoder: the GPU test compares with it alone
        text, *offs = R.pooled_repair(pool, idx, mode)
        assert all(len(o) == R.WIDE_N + 1 for o in offs) and len(text) == offs[0][-1]
        for lo, hi in WINDOWS:
            want_text, *want_offs = R.repair_batch(R.pooled_docs(pool, idx, lo, hi), mode)
            assert bytes(text[int(offs[0][lo]):int(offs[0][hi])]) == want_text, (mode, lo)
            for o, w in zip(offs, want_offs):
                assert (o[lo:hi + 1] - o[lo]).tolist() == w, (mode, lo)


def test_pooled_batch_holds_what_it_was_built_for():
    pool, idx = R.wide_batch()
    assert all(len(p) <= 12 for p in pool) and len(pool) <= 48
    assert np.array_equal(np.unique(idx), np.arange(len(pool)))  # every entry is drawn
    for whole in (b"", b"hello", "é".encode(), "中".encode(), "😀".encode()):
        assert whole in pool and R.repair(whole, R.REPLACE) == (whole, len(whole.decode()), 0)
    for cut, rest in ((b"x\xe4\xb8", b"\xad z"), (b"ab\xe4", b"\xb8\xad"), (b"\xf0\x9f\x98", b"\x80"), (b"\xf0\x9f", b"\x98\x80ok"), (b"\xc3", b"\xa9")):
        assert cut in pool and rest in pool and R.repair(cut + rest, R.REPLACE)[2] == 0  # together they are a char; apart, two ill-formed units at least
        assert R.repair(cut, R.IGNORE)[2] >= 1 and R.repair(rest, R.IGNORE)[2] >= 1
        a, b = pool.index(cut), pool.index(rest)
        assert ((idx[:-1] == a) & (idx[1:] == b)).any()  # ... and they are neighbours somewhere
    for lone in (b"\x80", b"\xbf\xbf", b"\xc0\x80", b"x\xf5y", b"\xff"):
        assert lone in pool
    ill = np.array([R.repair(p, R.REPLACE)[2] > 0 for p in pool])
    assert ill[idx[list(R.WIDE_FORCED)]].all()  # an ill-formed unit on both sides of every edge
    for n in R.WIDE_PREFIXES:
        assert 0.25 < ill[idx[:n]].mean() < 0.75, n


# ---------------------------------------------------------------- under the sanitizers, as a program of its own
def test_passes_under_the_sanitizers(tmp_path):
    """tests/hostsim/utf8_repair_sanitize.cpp: the same driver built with AddressSanitizer and UBSan, input and output allocated at exactly
    their contract sizes.  Host code only; nothing of it is loaded into Python."""
    d = h.HOSTSIM
    exe = str(tmp_path / "utf8_repair_sanitize")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         os.path.join(d, "utf8_repair_sanitize.cpp"), "-o", exe], capture_output=True, text=True)
    if cc.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|cannot find lib(asan|ubsan)|lib(asan|ubsan)\S*: No such file", cc.stderr):
        pytest.skip("this g++ has no sanitizer runtime")  # (the linker says so; any other diagnostic is a failure)
    assert cc.returncode == 0, cc.stderr[-3000:]
    small = [bytes(t) for t in R.exhaustive() if len(t) <= 3]
    batches = [small, [b"".join(small)], [b"\x80" * 5000], [b"abc\xf0\x9f\x98"], [], [b"", b""], [b"\x80" * 16], [b"a" * 15 + b"\xe4"], [b"a" * 16, b"\xb8"]]
    batches += R.empties() + R.sliding(16, 64, 256)[::7] + R.random_batches(7, 40)
    cases = []
    for k, docs in enumerate(batches):
        for mode in MODES:
            blob, n, off = R.pack(docs)
            text, to, co, ro = R.repair_batch(docs, mode)
            for wg, order in ((16, k % 3), (256, 2), (2048, 1)):
                cases.append(struct.pack("<7Q", n, len(docs), mode, wg, order, len(text), ro[-1]) + blob[: n + 16].tobytes() + off.tobytes() + text +
                             np.array([to, co, ro], np.uint64).tobytes())
    path = tmp_path / "cases.bin"
    path.write_bytes(struct.pack("<Q", len(cases)) + b"".join(cases))
    run_ = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert run_.returncode == 0, (run_.stdout[-2000:], run_.stderr[-4000:])
    assert run_.stdout.split()[:2] == ["ok", str(len(cases))]
