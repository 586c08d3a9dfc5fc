"""The passes that mark allowed special tokens (tk_k_spec_cand, tk_k_spec_resolve) on the CPU: tests/hostsim/spec_mark_sim.cpp compiles the
first one's per-thread body and tk_spec_resolve_one (tk_special.h) for the host and runs them lane by lane over packed batches, in buffers
of exactly the sizes the library gives them.  The three bitmaps they leave -- spec_start, spec_in, brk -- are compared bit for bit with
those of tests/spec_mark_ref.py, which states the rule (per document: the longest allowed special token at the leftmost position, then
on behind it) and knows nothing of candidates, clusters or walks.  Overlapping candidates are what this is about: no special token of the
form <|...|> can overlap another, so the device tests before this one never left the path "no earlier candidate covers me".
The same case list -- GROUPS below: every case, chunk and lane order -- runs a second time through the driver built as a program of its
own with the address and undefined-behaviour sanitizers (host code only: nothing of it is loaded into Python)."""
import ctypes
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import helpers as h
import spec_mark_ref as ref
from oracle import c_oracle

SRCS = ("spec_mark_sim.cpp", "tk_tables.cpp", "tk_pattern.cpp", "tk_regex.cpp", "tk_special.h", "tk_device.h", "tk_common.h", "tk_tables.h", "tk_regex.h",
        "tk_regex_host.h")
ORDERS = (0, 0x5EED)  # lanes and words ascending / shuffled (the kernels' threads run in no particular order)
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = h.build_sim("libspec_mark_sim.so", SRCS, ("-pthread",))
        vp, u64 = ctypes.c_void_p, ctypes.c_uint64
        L.sms_create.restype = vp
        L.sms_create.argtypes = [vp, vp, vp, u64, vp, vp, vp, u64, ctypes.c_char_p, ctypes.c_char_p, u64]
        L.sms_destroy.argtypes = [vp]
        L.sms_first_bytes.restype = ctypes.c_uint32
        L.sms_first_bytes.argtypes = [vp]
        L.sms_max_len.restype = ctypes.c_uint32
        L.sms_max_len.argtypes = [vp]
        L.sms_mark.restype = None
        L.sms_mark.argtypes = [vp, vp, u64, vp, u64, u64, vp, u64, u64, vp]
        _lib = L
    return _lib


class Sim:
    """The marking passes over the special tokens `specials` (a vocabulary of the 256 single bytes: the passes never look at it)."""

    def __init__(self, specials: dict[str, int]):
        self.specials = dict(specials)
        rb, ro, ri = c_oracle._pack([(bytes([b]), b) for b in range(256)])
        sb, so, si = c_oracle._pack([(k.encode(), v) for k, v in specials.items()])
        err = ctypes.create_string_buffer(512)
        self._h = lib().sms_create(rb.ctypes.data, ro.ctypes.data, ri.ctypes.data, len(ri), sb.ctypes.data, so.ctypes.data, si.ctypes.data, len(si),
                                   h.PAT_STR[0].encode(), err, 512)
        if not self._h:
            raise ValueError(err.value.decode())

    def __del__(self):
        if getattr(self, "_h", None):
            lib().sms_destroy(self._h)

    def first_bytes(self) -> int:
        return lib().sms_first_bytes(self._h)

    def max_len(self) -> int:
        return lib().sms_max_len(self._h)

    def mark(self, docs: list[bytes], allowed, order=0, d0=0, d1=None):
        """The words of spec_start, spec_in and brk (slack included) for documents [d0, d1) of the batch run as one chunk."""
        blob, off = h.pack(docs)
        d1 = len(docs) if d1 is None else d1
        base, end = int(off[d0]), int(off[d1])
        text = np.ascontiguousarray(blob[base:end]) if end > base else np.zeros(1, np.uint8)
        sub = np.ascontiguousarray(off[d0:d1 + 1])
        ids = np.asarray([self.specials[s] for s in allowed] or [0], np.uint32)
        nwords = (end - base + 31) // 32
        out = np.full(3 * (nwords + 2) + 8, 0xA5A5A5A5, np.uint32)
        lib().sms_mark(self._h, text.ctypes.data, end - base, sub.ctypes.data, d1 - d0, base, ids.ctypes.data, len(allowed), order, out.ctypes.data)
        assert (out[3 * (nwords + 2):] == 0xA5A5A5A5).all()
        return out[:3 * (nwords + 2)].reshape(3, nwords + 2)


def same(words: np.ndarray, want, n: int, what):
    """The sim's three bitmaps against the reference's; every bit at and behind n is zero."""
    for name, w, b in zip(("spec_start", "spec_in", "brk"), words, want):
        bits = np.unpackbits(np.ascontiguousarray(w).view(np.uint8), bitorder="little").astype(bool)
        assert not bits[n:].any(), (what, name, "a mark behind the text")
        if not np.array_equal(bits[:n], b):
            at = int(np.flatnonzero(bits[:n] != b)[0])
            raise AssertionError((what, name, "first difference at byte", at, "got", bits[max(0, at - 8):at + 8].astype(int).tolist(), "want",
                                  b[max(0, at - 8):at + 8].astype(int).tolist()))


def runs_of(c: ref.Case):
    """(d0, d1) of the whole batch and of the case's chunks"""
    return [(0, len(c.docs))] + list(c.chunks)


def found_of(c: ref.Case):
    """(start, length) of the special tokens per document, by the reference (a case may bring them: the joined documents)"""
    if getattr(c, "found", None) is None:
        allowed_b = [s.encode() for s in c.allowed]
        c.found = [ref.find_specials(d, allowed_b) for d in c.docs]
    return c.found


def runs_list(cases):
    """Everything that is run for a list of cases: (case, d0, d1, order) -- the whole batch and every chunk, in both orders."""
    return [(c, d0, d1, order) for c in cases for d0, d1 in runs_of(c) for order in ORDERS]


def expect(c: ref.Case, d0: int, d1: int):
    return ref.bitmaps(c.docs, c.allowed, d0, d1, found_of(c)), sum(len(d) for d in c.docs[d0:d1])


def check(c: ref.Case) -> int:
    """One case through the simulation loaded into Python; returns the number of special tokens taken."""
    sim = Sim(c.specials)
    taken = 0
    for _, d0, d1, order in runs_list([c]):
        want, n = expect(c, d0, d1)
        same(sim.mark(c.docs, c.allowed, order, d0, d1), want, n, (c.name, d0, d1, order))
        taken += int(want[0].sum()) if order == ORDERS[0] else 0
    return taken


def longest_cluster(c: ref.Case) -> int:
    """An upper bound: the longest stretch of a document in which every byte lies in some match of a registered special token."""
    toks = [s.encode() for s in c.specials]
    best = 0
    for d in set(c.docs):
        if len(d) <= 64:
            continue
        cov = np.zeros(len(d) + 1, np.int64)
        for t in toks:
            i = d.find(t)
            while i >= 0:
                cov[i] += 1
                cov[i + len(t)] -= 1
                i = d.find(t, i + 1)
        run = 0
        for x in np.cumsum(cov)[:-1] > 0:
            run = run + 1 if x else 0
            best = max(best, run)
    return best


def test_reference_against_the_oracle():
    """The reference of this file and oracle/tk_oracle.c agree on where special tokens lie: under a vocabulary of the 256 bytes a document's
    ids are its bytes, with the special tokens' ids where the reference finds them."""
    for c in ref.cases_a()[:1] + ref.small_cases():
        C = c_oracle.COracle(0, {bytes([b]): b for b in range(256)}, c.specials)
        toks, toff = C.encode_batch(*h.pack(c.docs), set(c.allowed), 8)
        for d, doc in enumerate(c.docs):
            assert toks[int(toff[d]):int(toff[d + 1])].tolist() == ref.plain_walk(doc, c.specials, c.allowed), (c.name, d, doc[:60])


def test_forms():
    """The cases reach what they are meant to reach: both forms of the first-byte test, both forms of the head walk, every cluster
    within the bound."""
    assert Sim({s: 1 + k for k, s in enumerate(ref.S3)}).first_bytes() == 2
    six = next(c for c in ref.cases_f() if c.name == "f: seven first bytes")
    assert Sim(six.specials).first_bytes() == 0xFF
    a = ref.cases_a()[0]
    assert Sim(a.specials).max_len() == 3 and Sim(a.also(ref.NEVER65, "").specials).max_len() == 65 and Sim(a.also(ref.NEVER66, "").specials).max_len() == 66
    assert sorted({Sim(c.specials).max_len() for c in ref.cases_d()}) == [33, 65, 67, 70, 105, 201]
    for c in ref.cases_b() + ref.small_cases():
        assert longest_cluster(c) <= ref.MAX_CLUSTER, c.name
    assert longest_cluster(ref.cases_b()[0]) == 4096


REGRESSIONS: list = []  # inputs on which a marking pass was found wrong once, by name (none so far)


def with_forms(cases):
    """(c): every case, then the same case in the core with a 65-byte special token and in the one with a 66-byte one"""
    for c in cases:
        found_of(c)  # (once per case: the forms share it, their extra special token occurs nowhere)
    return [v for c in cases for v in [c] + ref.head_walk_forms([c])]


@functools.lru_cache(maxsize=None)
def joined_cases(k: int):
    """(a) joined: one case per prefix 0 .. 70.  'c' is in no special token, so the prefix moves every match by its length: the reference
    walks the document once (and test_joined_reference_moves_with_the_prefix walks a prefixed one)."""
    allowed = ref.S3_ALLOWED[k]
    found = ref.find_specials(ref.joined_a(0).encode(), [s.encode() for s in allowed])
    assert len(found) > 5000
    out = []
    for p in ref.JOINED_PREFIXES:
        c = ref.Case(f"a: joined behind {p}, allowed {'+'.join(allowed)}", ref.S3, allowed, [ref.joined_a(p)])
        c.found = [[(a + p, ln) for a, ln in found]]
        out.append(c)
    return out


# The case list, by groups: what test_group runs through the simulation loaded into Python, test_group_under_sanitizers runs through the
# stand-alone program -- the same cases, chunks and orders.
GROUPS = {
    **{f"a-documents-{k}": (lambda k=k: with_forms(ref.cases_a()[k:k + 1])) for k in range(3)},
    **{f"a-joined-{k}": (lambda k=k: with_forms(joined_cases(k))) for k in range(3)},
    **{f"b-runs-{k}": (lambda k=k: with_forms(ref.cases_b()[k:k + 1])) for k in range(3)},
    **{g: (lambda g=g: with_forms(getattr(ref, "cases_" + g)())) for g in "defg"},
    "regressions": lambda: list(REGRESSIONS),
}
MIN_TAKEN = {"a-documents": 10000, "a-joined": 5000, "b-runs": 1000}  # (a case that marks nothing checks nothing)


def test_joined_reference_moves_with_the_prefix():
    for k in range(3):
        c = joined_cases(k)[7]
        for got, want in zip(ref.bitmaps(c.docs, c.allowed), ref.bitmaps(c.docs, c.allowed, found=c.found)):
            assert np.array_equal(got, want)


@pytest.mark.parametrize("group", list(GROUPS))
def test_group(group):
    """(a) - (g) with (c) for each: every case, whole and by its chunks, lanes and words in ascending and in shuffled order"""
    cases = GROUPS[group]()
    taken = [check(c) for c in cases]
    if group != "regressions":
        assert len(cases) % 3 == 0
        for i in range(0, len(cases), 3):  # (c): the three forms of a core mark the same special tokens
            assert taken[i] == taken[i + 1] == taken[i + 2] >= MIN_TAKEN.get(group[:-2], 0), cases[i].name


def write_cases(path, todo):
    with open(path, "wb") as f:
        pat = h.PAT_STR[0].encode()
        f.write(struct.pack("<Q", len(pat)) + pat)
        for c, d0, d1, order in todo:
            blob, off = h.pack(c.docs)
            f.write(struct.pack("<Q", len(c.specials)))
            for s, i in c.specials.items():
                f.write(struct.pack("<II", i, len(s.encode())) + s.encode())
            f.write(struct.pack("<Q", len(c.allowed)) + np.asarray([c.specials[s] for s in c.allowed], np.uint32).tobytes())
            base, end = int(off[d0]), int(off[d1])
            f.write(struct.pack("<4Q", end - base, d1 - d0, base, order) + off[d0:d1 + 1].tobytes() + blob[base:end].tobytes())


@pytest.mark.parametrize("group", list(GROUPS))
def test_group_under_sanitizers(group, tmp_path):
    """The driver as a program of its own, built with -fsanitize=address,undefined, on the same list as test_group -- runs_list of the same
    cases: it must run clean and leave the same bitmaps.  The list is dealt out to a few processes that run side by side."""
    exe = h.build_once("spec_mark_sim_san", SRCS, ["-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSPEC_MARK_SIM_MAIN"])
    todo = runs_list(GROUPS[group]())
    order = sorted(range(len(todo)), key=lambda i: -sum(len(d) for d in todo[i][0].docs[todo[i][1]:todo[i][2]]))  # (the long ones first, one to each)
    n_proc = max(1, min(8, len(os.sched_getaffinity(0)), len(todo)))
    parts = [[todo[i] for i in order[k::n_proc]] for k in range(n_proc)]
    procs = []
    for k, part in enumerate(parts):
        write_cases(tmp_path / f"cases{k}.bin", part)
        procs.append(subprocess.Popen([exe, str(tmp_path / f"cases{k}.bin"), str(tmp_path / f"results{k}.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    ends = [p.communicate() + (p.returncode,) for p in procs]
    for k, (part, (out, err, rc)) in enumerate(zip(parts, ends)):
        assert rc == 0 and err == "", (rc, err[-3000:])
        assert out.strip() == f"{len(part)} cases"
        raw = open(tmp_path / f"results{k}.bin", "rb").read()
        at = 0
        for c, d0, d1, order_ in part:
            _, max_len, nwords = struct.unpack_from("<IIQ", raw, at)
            at += 16
            assert max_len == max(len(s.encode()) for s in c.specials)
            words = np.frombuffer(raw, np.uint32, 3 * (nwords + 2), at).reshape(3, nwords + 2)
            at += 12 * (nwords + 2)
            want, n = expect(c, d0, d1)
            same(words, want, n, (c.name, d0, d1, order_))
        assert at == len(raw)
