"""The JSON Lines passes (tk_jsonl.h) on the CPU: tests/hostsim/jsonl_sim.cpp compiles the plain C++ they are made of
(tiktoken_amd/csrc/tk_jsonl_rule.h) for the host and drives it tile by tile the way the kernels do.  Compared, status for status and byte for
byte, with tests/jsonl_ref.py -- the rule as a byte scanner --, at TK_JSONL_TILE and at a tile of 64 bytes (the result must not depend on
it); the rule itself is tied to Python's parser: every generated line json.loads accepts as a dict gives json.loads(line).get(field).  The
same driver also runs as a program of its own under the address and undefined-behaviour sanitizers (nothing of it is loaded into Python)."""
import ctypes
import json
import os
import random
import re
import subprocess

import numpy as np
import pytest

import helpers as h
import jsonl_cases as jc
import jsonl_ref as jr
from tiktoken_amd.core import _repair_surrogates

SRCS = ("jsonl_sim.cpp", "tk_jsonl_rule.h", "tk_utf8_repair_rule.h", "tk_decode_rule.h", "tk_device.h", "tk_common.h")
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = h.build_sim("libjsonl_sim.so", SRCS, ("-Wall", "-Werror", "-Wno-unknown-pragmas", "-I" + os.path.join(h.ROOT, "include")))
        vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
        L.jsonl_sim.restype = ctypes.c_int64
        L.jsonl_sim.argtypes = [vp, u64, vp, u64, u32, u32, u64, *[vp] * 7]
        L.jsonl_sim_tile.restype = u32
        _lib = L
    return _lib


def run_sim(buf: bytes, field: bytes, mode: int, tile: int):
    n, cap = len(buf), buf.count(b"\n") + 1
    src = np.frombuffer(buf + b"\0", np.uint8)[:-1].copy() if n else np.zeros(1, np.uint8)
    text = np.full(n + 1, 0xCD, np.uint8)
    doc_off, line_off = np.full(cap + 1, 7, np.uint64), np.full(cap + 1, 7, np.uint64)
    line, status = np.full(cap, 7, np.uint64), np.full(cap, 0xCD, np.uint8)
    counts, bad = np.zeros(3, np.uint64), np.zeros(3, np.uint64)
    f = np.frombuffer(field, np.uint8).copy() if field else np.zeros(1, np.uint8)
    rc = lib().jsonl_sim(src.ctypes.data, n, f.ctypes.data, len(field), mode, tile, cap, *[a.ctypes.data for a in (text, doc_off, line, line_off, status, counts, bad)])
    if rc == 1:
        return jr.Extract(None, None, None, None, None, tuple(int(x) for x in bad))
    assert rc == 0, rc
    n_docs, n_lines, n_text = (int(x) for x in counts)
    assert (text[n_text:] == 0xCD).all(), "written behind the text"
    return jr.Extract(text[:n_text], doc_off[:n_docs + 1], line[:n_docs], line_off[:n_lines + 1], status[:n_lines], None)


def same(got: jr.Extract, want: jr.Extract, what):
    assert got.bad == want.bad, what
    if want.bad is not None:
        return
    for name in ("status", "line_off", "line", "doc_off", "text"):
        a, b = getattr(got, name), getattr(want, name)
        assert a.shape == b.shape and (a == b).all(), (what, name, a[:40], b[:40])


def check(buf: bytes, field: bytes = b"text", what=None, tiles=None):
    tiles = tiles or (lib().jsonl_sim_tile(), 64)
    for mode in (jr.SKIP, jr.EMPTY, jr.RAISE):
        want = jr.extract(buf, field, mode)
        for tile in tiles:
            same(run_sim(buf, field, mode, tile), want, (what, mode, tile))
    return jr.extract(buf, field, jr.SKIP)


def test_cases_worked_by_hand():
    r = check(b'{"id":1,"text":"a\\n\\u00e9\\ud83d\\ude00\\ud83d"}\n\n{"text":null}\r\n{"id":2}\n[1]\n{"text":"x","text":"y"} ')
    assert r.status.tolist() == [jr.OK, jr.BLANK, jr.NOT_STRING, jr.MISSING, jr.BAD, jr.OK]
    assert r.texts() == ["a\né😀�".encode(), b"y"] and r.line.tolist() == [0, 5]
    assert r.line_off.tolist() == [0, 46, 47, 62, 71, 75, 99]
    e = jr.extract(b'{"text":"a"}\n{"id":2}\n', b"text", jr.RAISE)
    assert e.bad == (1, 13, jr.MISSING)
    e = jr.extract(b'{"text":"a"}\n\n{"id":2}\n', b"text", jr.EMPTY)
    assert e.doc_off.tolist() == [0, 1, 1] and e.line.tolist() == [0, 2]


def test_edge_cases_at_both_tiles():
    for T in (lib().jsonl_sim_tile(), 64):
        for name, buf in jc.edge_buffers(T):
            check(buf, what=(T, name), tiles=(T, 64) if len(buf) < 40000 else (T,))
    T = lib().jsonl_sim_tile()
    r = check(jc.straddle(T, b"\\ud83d\\ude00", T - 5), tiles=(T,))
    assert r.texts()[0].endswith("😀".encode())
    r = check(b'{"text":"' + b"\\\\" * 32768 + b'"}\n', tiles=(T,))
    assert r.texts() == [b"\\" * 32768]
    r = check(b'{"text":""}\n' * 700, tiles=(T, 64))
    assert len(r.line) == 700 and int(r.doc_off[-1]) == 0


def test_random_buffers_match_the_rule_and_do_not_depend_on_the_tile():
    rng = random.Random(0x7501)
    for k in range(60):
        field = rng.choice(["text", "t", "content", "a b"])
        buf = jc.buffer(rng, rng.randint(0, 40), rng.choice([0.0, 0.1, 0.5, 1.0]), field)
        check(buf, field.encode(), what=k, tiles=(lib().jsonl_sim_tile(), 64, 128))


def test_the_rule_agrees_with_json_loads_on_every_line_it_accepts_as_a_dict():
    rng = random.Random(0x7502)
    seen = {jr.OK: 0, jr.MISSING: 0, jr.NOT_STRING: 0}
    for _ in range(3000):
        line = jc.dumps(rng, jc.record(rng))
        if rng.random() < 0.6:
            line = jc.mutate(rng, line)
        try:  # (the line as strict UTF-8: json.loads on bytes decodes with "surrogatepass", which the rule's UTF-8 check does not)
            obj = json.loads(line.decode("utf-8"))
        except ValueError:
            continue
        if not isinstance(obj, dict):
            continue
        st, text = jr.scan_line(line, b"text")
        v = obj.get("text")
        if isinstance(v, str):
            assert st == jr.OK and text == _repair_surrogates(v).encode("utf-8"), line
        else:
            assert st == (jr.MISSING if "text" not in obj else jr.NOT_STRING) and text is None, line
        seen[st] += 1
    assert all(n > 20 for n in seen.values()), seen


def test_refusals():
    src = np.zeros(8, np.uint8)
    outs = [np.zeros(16, np.uint64) for _ in range(7)]

    def rc(field: bytes, mode=0, tile=64):
        f = np.frombuffer(field + b"\0", np.uint8).copy()
        return lib().jsonl_sim(src.ctypes.data, 0, f.ctypes.data, len(field), mode, tile, 1, *[a.ctypes.data for a in outs])
    assert rc(b"") == -17 and rc(b"x" * 65) == -17 and rc(b'a"b') == -18 and rc(b"a\\") == -18 and rc(b"a\x1f") == -18
    assert rc(b"text", 3) == -19 and rc(b"text", 0, 96) == -21 and rc(b"x" * 64) == 0


def test_case_list_under_sanitizers(tmp_path):
    """tests/hostsim/jsonl_sanitize.cpp: the driver as a program of its own, built with -fsanitize=address,undefined, on seeded random
    buffers in heap blocks of exactly their size: it must run clean and give the same result at every tile size."""
    exe = str(tmp_path / "jsonl_sanitize")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I" + os.path.join(h.ROOT, "include"), os.path.join(h.HOSTSIM, "jsonl_sanitize.cpp"), "-o", exe], capture_output=True, text=True)
    if cc.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|cannot find lib(asan|ubsan)|lib(asan|ubsan)\S*: No such file", cc.stderr):
        pytest.skip("this g++ has no sanitizer runtime")  # (the linker says so; any other diagnostic is a failure)
    assert cc.returncode == 0, cc.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "jsonl_sanitize ok" in run.stdout
