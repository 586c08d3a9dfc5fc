"""The stop-string passes (tk_stop_text.h) on the CPU: tests/hostsim/stop_text_sim.cpp compiles the plain C++ they are made of
(tiktoken_amd/csrc/tk_stop_text_rule.h) for the host and drives it the way the kernels do -- workgroups of 16, 256 (the kernels') and 2048
lanes, the lanes and workgroups in ascending, descending and shuffled order, readers that refuse every index outside [0, n_bytes + 16), a
writer that wants every output byte stored exactly once.  Compared with the rule of include/tiktoken_amd.h restated in Python
(tests/stop_text_ref.py: bytes.find per string, the least (position, index))."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import helpers as h
import stop_text_ref as S

GEOMETRY = ((16, 64), (256, 1024), (2048, 1024))  # (lanes of a workgroup, bytes of a wavefront)
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = h.build_sim("libstop_text_sim.so", ("stop_text_sim.cpp", "tk_stop_text_rule.h", "tk_device.h", "tk_common.h"), ("-Wall", "-Werror"))
        vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
        L.stops_run.restype = ctypes.c_int64
        L.stops_run.argtypes = [vp, u64, vp, u64, vp, vp, u32, u32, u32, u32, vp, vp, vp, vp]
        L.stops_ntok.restype = u32
        L.stops_ntok.argtypes = [vp, u64, u64, u64]
        _lib = L
    return _lib


def run_raw(blob, n, off, n_docs, stop_blob, stop_off, n_stops, flags, wg_lanes, order):
    text = np.full(n + 16, 0x5A, np.uint8)
    text_off = np.full(n_docs + 1, 0xDEAD, np.uint64)
    hit = np.full(max(n_docs, 1), 0xDEAD, np.uint32)
    totals = np.zeros(3, np.uint64)
    rc = lib().stops_run(blob.ctypes.data, n, off.ctypes.data, n_docs, stop_blob.ctypes.data, stop_off.ctypes.data, n_stops, flags, wg_lanes, order, text.ctypes.data,
                         text_off.ctypes.data, hit.ctypes.data, totals.ctypes.data)
    return rc, text, text_off, hit[:n_docs], [int(t) for t in totals]


def run(docs, stops, flags, wg_lanes, order):
    blob, n, off = S.pack(docs)
    stop_blob, stop_off = S.stop_arrays(stops)
    return run_raw(blob, n, off, len(docs), stop_blob, stop_off, len(stops), flags, wg_lanes, order)


def check(name, docs, stops, wgs=(16, 256, 2048), orders=(0, 1, 2)):
    for keep in (False, True):
        want_text, want_off, want_hit, want_n = S.cut_batch(docs, stops, keep)
        for wg in wgs:
            for order in orders:
                rc, text, text_off, hit, totals = run(docs, stops, S.KEEP if keep else 0, wg, order)
                ctx = (name, keep, wg, order)
                assert rc == 0, (rc, ctx)
                assert totals == [len(want_text), want_n, 1 if want_n else 0], (totals, ctx)  # the cut pass runs exactly when a document has a hit
                assert hit.tolist() == want_hit, ctx
                assert text_off.tolist() == want_off, ctx
                assert bytes(text[: totals[0]]) == want_text, ctx


def test_the_reference_is_what_the_rule_says():
    assert S.cut_doc(b"xxabcxx", [b"ab", b"abc"], False) == (2, 0) and S.cut_doc(b"xxabcxx", [b"abc", b"ab"], True) == (5, 0)
    assert S.cut_doc(b"xxBByyAA", [b"AA", b"BB"], False) == (2, 1)  # position decides before list order
    assert S.cut_doc(b"none", [b"AA"], True) == (4, S.NO_HIT) and S.cut_doc(b"", [], False) == (0, S.NO_HIT)
    assert S.cut_batch([b"aXb", b"", b"X"], [b"X"], True) == (b"aXX", [0, 2, 2, 3], [0, S.NO_HIT, 0], 2)


@pytest.mark.parametrize("wg,wave", GEOMETRY)
def test_edge_cases_at_every_geometry(wg, wave):
    """every case at workgroups of 16 lanes, of 256 (the kernels' geometry) and of 2048, each with its own edges, in all three orders"""
    for name, docs, stops in S.cases(16, wave, 16 * wg):
        check(name, docs, stops, wgs=(wg,))


def test_the_kernels_cases_at_the_other_geometries():
    for name, docs, stops in S.cases(16, 1024, 4096):
        check(name, docs, stops, wgs=(16, 2048), orders=(2,))


def test_random_batches():
    for name, docs, stops in S.random_cases(0x570B, 150):
        check(name, docs, stops, orders=(0, 2))


def test_no_hit_takes_no_cut_pass():
    docs = [b"The quick brown fox. " * 300, b"", "中文😀é".encode() * 50]
    for wg in (16, 256, 2048):
        rc, text, text_off, hit, totals = run(docs, [b"\n\n", b"###"], 0, wg, 2)
        assert rc == 0 and totals == [sum(map(len, docs)), 0, 0] and hit.tolist() == [S.NO_HIT] * 3
        assert bytes(text[: totals[0]]) == b"".join(docs)


def test_refusals():
    blob, n, off = S.pack([b"abc", b"de"])

    def refused(stops=(b"a",), flags=0, stop_off=None, offsets=None):
        stop_blob, so = S.stop_arrays(list(stops))
        if stop_off is not None:
            so = np.array(stop_off, np.uint32)
        o = off if offsets is None else np.array(offsets, np.uint64)
        return run_raw(blob, n, o, 2, stop_blob, so, len(so) - 1, flags, 16, 0)[0]

    assert refused() == 0
    assert refused(stops=[bytes([65 + i]) for i in range(17)]) == 2001
    assert refused(stops=[b"a", b"", b"b"]) == 2002
    assert refused(stops=[b"x" * 65]) == 2003
    assert refused(stops=[b"x" * 64]) == 0
    assert refused(stops=[b"abcd"], stop_off=[0, 3, 2]) == 2004
    assert refused(stops=[b"abcd"], stop_off=[1, 3]) == 2004
    assert refused(flags=2) == 2005
    for bad, doc in (([0, 3, 4], 2), ([0, 4, 3], 1), ([1, 3, 5], 0), ([0, 3, 6], 2)):
        assert refused(offsets=bad) == 1000 + doc, bad


def test_token_counts():
    rng = np.random.default_rng(5)
    for _ in range(200):
        lens = rng.choice([1, 1, 2, 3, 7, 300], size=int(rng.integers(0, 12))).tolist()
        base, t0 = int(rng.integers(0, 1000)), int(rng.integers(0, 5))
        starts = np.zeros(t0 + len(lens) + 1, np.uint64)  # (tokens of other rows before and behind)
        starts[t0:t0 + len(lens)] = base + np.concatenate([[0], np.cumsum(lens)[:-1]]) if lens else []
        starts[t0 + len(lens)] = base + sum(lens)
        for kept in sorted({0, 1, sum(lens), max(sum(lens) - 1, 0), *np.cumsum(lens).tolist(), *(np.cumsum(lens) + 1).tolist()}):
            if kept <= sum(lens):
                got = lib().stops_ntok(starts.ctypes.data, t0, t0 + len(lens), base + kept)
                assert got == S.n_tok_ref(lens, kept), (lens, kept)


# ---------------------------------------------------------------- the pooled batch of tests/test_gpu_text_passes_wide.py, without a GPU
WINDOWS = ((0, 5000), ((1 << 20) - 1070, (1 << 20) + 1030))  # a prefix, and the 2 100 documents around index 2^20, the last among them


def test_pooled_reference_is_the_per_document_one():
    pool, idx = S.wide_batch()
    assert len(idx) == S.WIDE_N == (1 << 20) + 1030 and S.WIDE_PREFIXES[-1] == S.WIDE_N
    for stops in (S.WIDE_STOPS, S.NO_STOPS):
        for keep in (False, True):
            text, text_off, hit = S.pooled_cut(pool, idx, stops, keep)
            assert len(text_off) == S.WIDE_N + 1 and len(hit) == S.WIDE_N and len(text) == text_off[-1]
            for lo, hi in WINDOWS:
                want_text, want_off, want_hit, _ = S.cut_batch(S.pooled_docs(pool, idx, lo, hi), stops, keep)
                assert bytes(text[int(text_off[lo]):int(text_off[hi])]) == want_text, (keep, lo)
                assert (text_off[lo:hi + 1] - text_off[lo]).tolist() == want_off, (keep, lo)
                assert hit[lo:hi].tolist() == want_hit, (keep, lo)


def test_pooled_batch_holds_what_it_was_built_for():
    pool, idx = S.wide_batch()
    stops = S.WIDE_STOPS
    assert all(len(p) <= 12 for p in pool) and len(pool) <= 48
    assert np.array_equal(np.unique(idx), np.arange(len(pool)))  # every entry is drawn
    cut = {p: S.cut_doc(p, stops, False) for p in pool}
    assert b"" in cut and cut[b"plain text"] == (10, S.NO_HIT)
    assert cut[b"<END>tail"] == (0, 0) and cut[b"ab<END>cd"] == (2, 0) and cut[b"abc<END>"] == (3, 0) and cut[b"##"] == (0, 1)
    assert cut[b"xy<E"][1] == S.NO_HIT and cut[b"ND>zz"][1] == S.NO_HIT and S.crosses(b"xy<E", b"ND>zz", stops)  # the halves of a stop string
    assert cut[b"a##b<END>"] == (1, 1) and cut[b"<END>##"] == (0, 0) and cut[b"<EN##"] == (0, 2) and cut[b"x<ENx"] == (1, 2)  # position, then list order
    for d in S.WIDE_FORCED:  # a hit in the middle, something kept, on both sides of every edge
        p = pool[idx[d]]
        for keep in (False, True):
            kept, k = S.cut_doc(p, stops, keep)
            assert k != S.NO_HIT and 1 <= kept < len(p), (d, p)
    cross = np.array([[S.crosses(a, b, stops) for b in pool] for a in pool])
    assert cross[idx[:-1], idx[1:]].sum() > 1000  # neighbours that form a stop string across their boundary ...
    assert not any(S.crosses(a, b, S.NO_STOPS) or S.cut_doc(a, S.NO_STOPS, False)[1] != S.NO_HIT for a in pool for b in pool)
    for n in S.WIDE_PREFIXES[:3]:  # ... already in the smallest prefixes
        assert cross[idx[:n - 1], idx[1:n]].any()
    has_hit = np.array([cut[p][1] != S.NO_HIT for p in pool])[idx]
    for n in S.WIDE_PREFIXES:
        assert 0.25 < has_hit[:n].mean() < 0.75, n


# ---------------------------------------------------------------- under the sanitizers, as a program of its own
def test_passes_under_the_sanitizers(tmp_path):
    """tests/hostsim/stop_text_sanitize.cpp: the same driver built with AddressSanitizer and UBSan, the input allocated so that it ends
    exactly 16 bytes behind the text.  Host code only; nothing of it is loaded into Python."""
    d = h.HOSTSIM
    exe = str(tmp_path / "stop_text_sanitize")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         os.path.join(d, "stop_text_sanitize.cpp"), "-o", exe], capture_output=True, text=True)
    if cc.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|cannot find lib(asan|ubsan)|lib(asan|ubsan)\S*: No such file", cc.stderr):
        pytest.skip("this g++ has no sanitizer runtime")  # (the linker says so; any other diagnostic is a failure)
    assert cc.returncode == 0, cc.stderr[-3000:]
    cases = []
    batches = S.cases(16, 64, 256) + S.cases(16, 1024, 4096)[::3] + S.random_cases(11, 40)
    for k, (_, docs, stops) in enumerate(batches):
        for keep in (0, 1):
            blob, n, off = S.pack(docs)
            stop_blob, stop_off = S.stop_arrays(stops)
            text, to, hit, n_hit = S.cut_batch(docs, stops, bool(keep))
            for wg, order in ((16, k % 3), (256, 2), (2048, 1)):
                cases.append(struct.pack("<9Q", n, len(docs), len(stops), int(stop_off[-1]), keep, wg, order, len(text), n_hit) + blob[: n + 16].tobytes() + off.tobytes() +
                             stop_blob[: int(stop_off[-1])].tobytes() + stop_off.tobytes() + text + np.array(to, np.uint64).tobytes() + np.array(hit, np.uint32).tobytes())
    path = tmp_path / "cases.bin"
    path.write_bytes(struct.pack("<Q", len(cases)) + b"".join(cases))
    run_ = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert run_.returncode == 0, (run_.stdout[-2000:], run_.stderr[-4000:])
    assert run_.stdout.split()[:2] == ["ok", str(len(cases))]
