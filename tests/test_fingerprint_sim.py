"""The fingerprint passes (tk_fingerprint.h) on the CPU: tests/hostsim/fingerprint_sim.cpp compiles the plain C++ they are made of
(tiktoken_amd/csrc/tk_fingerprint_rule.h) for the host and drives it tile by tile, segment by segment and lane by lane the way the kernels
do.  Compared, value for value, with tests/fingerprint_ref.py -- the rule in Python --, at the shipped tile and at tiles of 8 and 64
positions (the result must not depend on it).  The same driver also runs as a program of its own under the address and
undefined-behaviour sanitizers (nothing of it is loaded into Python)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import fingerprint_cases as fc
import fingerprint_ref as fr
import helpers as h

SRCS = ("fingerprint_sim.cpp", "tk_fingerprint_rule.h", "tk_rows_rule.h", "tk_common.h")
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = h.build_sim("libfingerprint_sim.so", SRCS, ("-Wall", "-Werror", "-Wno-unknown-pragmas"))
        vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
        L.fingerprint_sim.restype = ctypes.c_int64
        L.fingerprint_sim.argtypes = [vp, u64, vp, u64, u32, u32, u32, u64, u32, vp, vp, vp, vp]
        L.fingerprint_sim_tile.restype = u32
        _lib = L
    return _lib


def run_sim(tok, off, spec, tile):
    k, P, B, seed = spec
    n = len(off) - 1
    sig, band = np.full(n * max(P, 1) + 1, 7, np.uint32), np.full(n * max(B, 1) + 1, 7, np.uint64)
    exact, nsh = np.full(n + 1, 7, np.uint64), np.full(n + 1, 7, np.uint64)
    t = tok if len(tok) else np.zeros(1, np.uint32)
    rc = lib().fingerprint_sim(t.ctypes.data, len(tok), off.ctypes.data, n, k, P, B, seed, tile, *[a.ctypes.data for a in (sig, band, exact, nsh)])
    if rc != 0:
        return rc
    assert sig[n * P] == 7 and band[n * B] == 7 and exact[n] == 7 and nsh[n] == 7, "written behind an array"
    return fr.Ref(sig[:n * P].reshape(n, P), band[:n * B].reshape(n, B), exact[:n], nsh[:n], np.diff(off))


def same(got, want, what):
    assert not isinstance(got, int), (what, got)
    for name in fr.Ref._fields:
        a, b = getattr(got, name), getattr(want, name)
        assert a.shape == b.shape and a.dtype == b.dtype and (a == b).all(), (what, name, np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))[:8])


def tiles():
    return (lib().fingerprint_sim_tile(), 8, 64)


def test_the_numpy_form_of_the_reference_is_the_plain_one():
    assert fr.mix(0) == 0xE220A8397B1DCDAF  # (splitmix64's first output: the rule's mix is its finaliser behind the increment)
    for seed, spec in enumerate(fc.SPECS):
        tok, off = fc.pack([0, 1, 4, 5, 6, 0, 0, 37, 31, 32, 33, 3, 70], seed)
        same(fr.fingerprint(tok, off, *spec), fr.fingerprint_plain(tok, off, *spec), spec)


def test_a_case_worked_by_hand():
    tok, off = np.array([7, 8, 9, 7, 8, 9, 5], np.uint32), np.array([0, 0, 3, 6, 7], np.uint64)
    r = fr.fingerprint(tok, off, 2, 4, 2, 1)
    assert r.n_shingles.tolist() == [0, 2, 2, 1] and r.length.tolist() == [0, 3, 3, 1]
    assert (r.sig[0] == 0xFFFFFFFF).all() and (r.sig[1] == r.sig[2]).all() and r.exact[1] == r.exact[2] and (r.band[1] == r.band[2]).all()
    h78, h89 = fr.shingle_hash((7, 8), 1), fr.shingle_hash((8, 9), 1)
    assert r.sig[1].tolist() == [min(fr.perm_value(1, p, h78), fr.perm_value(1, p, h89)) for p in range(4)]
    assert r.sig[3].tolist() == [fr.perm_value(1, p, fr.shingle_hash((5,), 1)) for p in range(4)]
    assert fr.exact_groups(r) == [0, 1, 1, 3] and fr.duplicate_groups(r) == [0, 1, 1, 3] and fr.keep_mask(r) == [True, True, False, True]
    for tile in tiles():
        same(run_sim(tok, off, (2, 4, 2, 1), tile), r, tile)


@pytest.mark.parametrize("spec", fc.SPECS, ids=lambda s: f"k{s[0]}-P{s[1]}-B{s[2]}-{s[3] & 0xFF:x}")
def test_every_shape_at_every_tile(spec):
    """The shapes of fingerprint_cases built for a tile of 64 (run at all three tiles) and, the edge cases, for the shipped tile."""
    T = lib().fingerprint_sim_tile()
    for name, tok, off in fc.batches(64, spec[0]) + fc.batches(T, spec[0])[:2]:
        want = fr.fingerprint(tok, off, *spec)
        for tile in tiles():
            same(run_sim(tok, off, spec, tile), want, (name, tile))


def test_refusals_write_nothing():
    tok, off = fc.pack([3, 4], 1)
    for k, P, B in fc.REFUSED:
        with pytest.raises(ValueError):
            fr.check_spec(k, P, B)
        assert run_sim(tok, off, (k, P, B, 0), 64) in (-1, -2, -3), (k, P, B)
    assert run_sim(tok, off, (5, 16, 4, 0), 6) == -10


def test_case_list_under_sanitizers(tmp_path):
    """tests/hostsim/fingerprint_sanitize.cpp: the driver as a program of its own, built with -fsanitize=address,undefined, on seeded
    random batches in heap blocks of exactly their size: it must run clean and give the same result at every tile size."""
    exe = str(tmp_path / "fingerprint_sanitize")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         os.path.join(h.HOSTSIM, "fingerprint_sanitize.cpp"), "-o", exe], capture_output=True, text=True)
    if cc.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|cannot find lib(asan|ubsan)|lib(asan|ubsan)\S*: No such file", cc.stderr):
        pytest.skip("this g++ has no sanitizer runtime")  # (the linker says so; any other diagnostic is a failure)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "fingerprint_sanitize ok" in run.stdout


def helper_case(bands=None):
    """(tokens, tok_off, pairs, spec, the reference's result) of the helper batch, tokenised by the CPU oracle"""
    C = h.c_oracle_for("gpt2_shaped")
    tok, off, pairs = fc.helper_batch(lambda t: C.encode_ordinary(t.encode("utf-8")))
    k, P, B, seed = fc.HELPER_SPEC
    spec = (k, P, bands or B, seed)
    return tok, off, pairs, spec, fr.fingerprint(tok, off, *spec)


def test_the_reference_alone_keeps_the_jaccard_bound_on_the_helper_batch():
    """The condition of the GPU test: on every pair it looks at, the estimate lies within 4 sqrt(J (1 - J) / P) of the shingle sets' J."""
    tok, off, pairs, spec, r = helper_case()
    seen = set()
    for i, j in pairs:
        J = fr.true_jaccard(tok, off, i, j, spec[0])
        assert abs(fr.jaccard(r, i, j) - J) <= 4 * (J * (1 - J) / spec[1]) ** 0.5, (i, j, J, fr.jaccard(r, i, j))
        seen.add(0 if J == 1.0 else 1 if J > 0.2 else 2)
    assert seen == {0, 1, 2}  # (identical copies, noisy copies, different texts)


def test_the_numpy_helpers_are_the_dict_helpers():
    from tiktoken_amd import Fingerprints

    for bands in (None, 128):
        _, _, pairs, _, r = helper_case(bands)
        f = Fingerprints(*r)
        assert f.exact_groups().tolist() == fr.exact_groups(r)
        for th in (0.8, 0.3, 1.0, 0.0):
            want = fr.duplicate_groups(r, th)
            assert f.duplicate_groups(th).tolist() == want and f.keep_mask(th).tolist() == fr.keep_mask(r, th)
        assert all(f.jaccard(i, j) == fr.jaccard(r, i, j) for i, j in pairs)
    assert len(set(fr.duplicate_groups(r, 0.3))) < len(set(fr.duplicate_groups(r, 0.8))) < len(r.exact)  # (with one row per band the noisy copies meet)
    e = Fingerprints(*fr.fingerprint(np.zeros(0, np.uint32), np.zeros(1, np.uint64)))
    assert e.exact_groups().tolist() == [] and e.duplicate_groups().tolist() == [] and e.keep_mask().tolist() == []
