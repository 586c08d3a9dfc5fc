"""The packed-sample-rows passes (tk_sample_rows.h) on the CPU: tests/hostsim/sample_rows_sim.cpp compiles the plain C++ they are made of
(tiktoken_amd/csrc/tk_sample_rows_rule.h on top of tk_samples_rule.h) for the host and drives it the way the kernels do -- one entry per
sample, the rounds of pointer doubling with their entries in either order, lanes of eight positions, workgroups of 16 and 2048, every array
behind a reader that checks the index; the write pass runs through tk_srow_lane, the function the kernel itself calls.  Compared with the
restatement of the rule as Python loops in tests/sample_rows_ref.py, which is written from the rule's description
(include/tiktoken_amd.h), not from the kernels.  The same driver also runs as a program of its own under the address and
undefined-behaviour sanitizers (host code only: nothing of it is loaded into Python)."""
import ctypes
import struct
import subprocess

import numpy as np
import pytest

import helpers as h
import sample_rows_ref as rr
import samples_ref as sr
from test_samples_sim import role_table

_lib = None
BLOCKS = (16, 2048)
KEEP_TAIL, LEFT, SKIP_LONG, IGNORE_FIRST = 1, 2, 4, 8
NONE = 0xFFFFFFFF
SRCS = ("sample_rows_sim.cpp", "sim_readers.h", "tk_sample_rows_rule.h", "tk_samples_rule.h", "tk_rows_rule.h", "tk_common.h")
BAD_SOFF, BAD_ROLE = 1 << 40, 1 << 41
G32, G64 = 0xDEADBEEF, 0xDEADBEEFDEADBEEF


def lib():
    global _lib
    if _lib is None:
        L = h.build_sim("libsample_rows_sim.so", SRCS, ("-Wall", "-Werror",))
        vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int32
        L.sample_rows_sim_place.restype = ctypes.c_int64
        L.sample_rows_sim_place.argtypes = [u64, vp, u64, vp, vp, u64, u64, vp, vp, vp, u32, u32, u32, u32, u32, i32, u32, u32] + [vp] * 11
        L.sample_rows_sim_write.restype = ctypes.c_int64
        L.sample_rows_sim_write.argtypes = [vp, u64, vp, u64, vp, vp, u64, u64, vp, vp, vp, u32, u32, u32, u32, i32, u32, u32, vp, vp, vp, vp, vp, u64, u64] + [vp] * 5
        _lib = L
    return _lib


def spec_of(max_len, width_multiple=0, bos=None, eos=None, pad=0, ignore=sr.IGNORE, keep_tail=False, left=False, skip_long=False, ignore_first=False):
    flags = (KEEP_TAIL if keep_tail else 0) | (LEFT if left else 0) | (SKIP_LONG if skip_long else 0) | (IGNORE_FIRST if ignore_first else 0)
    return (max_len, width_multiple, NONE if bos is None else bos, NONE if eos is None else eos, pad, ignore, flags)


def run_sim(tokens, tok_off, part_role, sample_off, roles, max_len, block, *, order=0, T=None, n_roles=None, **kw):
    """(rc, SampleRows or None) of the simulation; every output sits in front of a guard word that must survive."""
    tokens = np.ascontiguousarray(tokens, np.uint32)
    tok_off, sample_off = np.ascontiguousarray(tok_off, np.uint64), np.ascontiguousarray(sample_off, np.uint64)
    part_role = np.ascontiguousarray(part_role, np.uint8)
    T, n_parts, n = len(tokens) if T is None else T, len(tok_off) - 1, len(sample_off) - 1
    ids_t, off_t, train_t = role_table(roles)
    n_roles = len(roles) if n_roles is None else n_roles
    spec = spec_of(max_len, **kw)
    pstart, full, c, f = np.full(n_parts + 2, G64, np.uint64), np.full(n + 1, G64, np.uint64), np.full(n + 2, G64, np.uint64), np.full(n + 2, G64, np.uint64)
    ln, ntr, srow, scol = (np.full(n + 1, G32, np.uint32) for _ in range(4))
    rsmp, rseg = np.full(n + 2, G32, np.uint32), np.full(n + 2, G32, np.uint32)
    counts = np.zeros(2, np.uint64)
    roles_p = part_role if n_parts else np.zeros(1, np.uint8)
    table = (n_roles, ids_t.ctypes.data, off_t.ctypes.data, train_t.ctypes.data)
    ptr = lambda *arrays: [a.ctypes.data for a in arrays]  # noqa: E731
    rc = lib().sample_rows_sim_place(T, tok_off.ctypes.data, n_parts, roles_p.ctypes.data, sample_off.ctypes.data, n, *table, *spec, order,
                                     *ptr(pstart, full, ln, ntr, c, f, srow, scol, rsmp, rseg, counts))
    if rc:
        return rc, None
    R, S = int(counts[0]), int(counts[1])
    L = max_len
    ids, seg, pos, cu = np.full(R * L + 1, G32, np.uint32), np.full(R * L + 1, G32, np.uint32), np.full(R * L + 1, G32, np.uint32), np.full(S + 2, G32, np.uint32)
    lab = np.full(R * L + 1, 0x5A5A5A5A, np.int32)
    src = tokens if T else np.zeros(1, np.uint32)
    rc = lib().sample_rows_sim_write(src.ctypes.data, T, tok_off.ctypes.data, n_parts, roles_p.ctypes.data, sample_off.ctypes.data, n, *table, spec[0], *spec[2:], block,
                                     *ptr(pstart, c, f, rsmp, rseg), R, S, *ptr(ids, lab, seg, pos, cu))
    if rc:
        return rc, None
    assert ids[-1] == G32 and seg[-1] == G32 and pos[-1] == G32 and cu[-1] == G32 and lab[-1] == 0x5A5A5A5A
    assert pstart[-1] == G64 and full[-1] == G64 and c[-1] == G64 and f[-1] == G64 and all(a[-1] == G32 for a in (ln, ntr, srow, scol, rsmp, rseg))
    assert (rsmp[R + 1:] == G32).all() and (rseg[R + 1:] == G32).all()
    grid = lambda a: a[:-1].reshape(R, L)  # noqa: E731
    return 0, rr.SampleRows(grid(ids), grid(lab), grid(seg), grid(pos), cu[:-1], rseg[: R + 1], rsmp[: R + 1], ln[:-1], full[:-1], ntr[:-1], srow[:-1], scol[:-1])


def check(samples, L, kws, blocks=BLOCKS, roles=sr.CHAT, pad=7, ignore=sr.IGNORE, ctx=""):
    arrays = sr.pack(samples)
    for kw in kws:
        want = rr.rows_rule(*arrays, roles, L, pad=pad, ignore=ignore, **kw)
        if ignore == sr.IGNORE:
            rr.invariants(want, L)
        for block in blocks:
            for order in (0, 1):
                rc, got = run_sim(*arrays, roles, L, block, order=order, pad=pad, ignore=ignore, **kw)
                assert rc == 0, (rc, ctx, L, kw, block)
                rr.same(got, want, (ctx, L, kw, block, order))


def test_a_case_worked_by_hand():
    """L = 8, no bos, eos 2, role 0 = before [50], untrained; role 1 = after [52], trained.  Samples: A = user [10, 11] assistant [20]:
    50 10 11 20 52 2 (6 elements, 20 52 2 trained); B = assistant [30 .. 36]: 30 .. 36 52 2 (9 elements: cut to 30 .. 36 52, or left out);
    C = empty: 2 alone (untrained); D = assistant [40]: 40 52 2.  Next-fit: A | B | C D, written down from the rule's text."""
    roles = (sr.Role((50,), (), False), sr.Role((), (52,), True))
    arrays = sr.pack([[(0, [10, 11]), (1, [20])], [(1, [30, 31, 32, 33, 34, 35, 36])], [], [(1, [40])]])
    I, N = sr.IGNORE, NONE
    for got in (rr.rows_rule(*arrays, roles, 8, eos=2, pad=0), run_sim(*arrays, roles, 8, 16, eos=2, pad=0)[1]):
        assert got.ids.tolist() == [[50, 10, 11, 20, 52, 2, 0, 0], [30, 31, 32, 33, 34, 35, 36, 52], [2, 40, 52, 2, 0, 0, 0, 0]]
        assert got.labels.tolist() == [[I, I, I, 20, 52, 2, I, I], [30, 31, 32, 33, 34, 35, 36, 52], [I, 40, 52, 2, I, I, I, I]]
        assert got.seg.tolist() == [[0] * 6 + [N] * 2, [1] * 8, [2, 3, 3, 3, N, N, N, N]]
        assert got.pos.tolist() == [[0, 1, 2, 3, 4, 5, 0, 1], [0, 1, 2, 3, 4, 5, 6, 7], [0, 0, 1, 2, 0, 1, 2, 3]]
        assert got.cu_seqlens.tolist() == [0, 6, 8, 16, 17, 20, 24] and got.row_seg.tolist() == [0, 2, 3, 6] and got.row_sample.tolist() == [0, 1, 2, 4]
        assert got.len.tolist() == [6, 8, 1, 3] and got.full_len.tolist() == [6, 9, 1, 3] and got.n_trained.tolist() == [3, 8, 0, 3]
        assert got.sample_row.tolist() == [0, 1, 2, 2] and got.sample_col.tolist() == [0, 0, 0, 1]
    # skip_long leaves B out, and C fits behind A (6 + 1 <= 8) while D does not (7 + 3 > 8): A C | D; ignore_first masks D's 40 (A's first
    # is a before id, C's an untrained eos)
    for got in (rr.rows_rule(*arrays, roles, 8, eos=2, pad=0, skip_long=True, ignore_first=True),
                run_sim(*arrays, roles, 8, 16, eos=2, pad=0, skip_long=True, ignore_first=True)[1]):
        assert got.ids.tolist() == [[50, 10, 11, 20, 52, 2, 2, 0], [40, 52, 2, 0, 0, 0, 0, 0]]
        assert got.labels.tolist() == [[I, I, I, 20, 52, 2, I, I], [I, 52, 2, I, I, I, I, I]]
        assert got.seg.tolist() == [[0] * 6 + [2, N], [3, 3, 3, N, N, N, N, N]] and got.pos.tolist() == [[0, 1, 2, 3, 4, 5, 0, 0], [0, 1, 2, 0, 1, 2, 3, 4]]
        assert got.cu_seqlens.tolist() == [0, 6, 7, 8, 11, 16] and got.row_seg.tolist() == [0, 3, 5] and got.row_sample.tolist() == [0, 3, 4]
        assert got.len.tolist() == [6, 8, 1, 3] and got.full_len.tolist() == [6, 9, 1, 3] and got.n_trained.tolist() == [3, 0, 0, 2]
        assert got.sample_row.tolist() == [0, N, 0, 1] and got.sample_col.tolist() == [0, 0, 6, 0]


def test_case_list():
    rng = np.random.default_rng(2048)
    for name, samples, L, kws in rr.cases(rng):
        big = len(samples) > 1500
        check(samples, L, kws[:1] if big else kws, blocks=BLOCKS[1:] if big else BLOCKS, ctx=name)


@pytest.mark.parametrize("roles", [sr.ALL_TRAINED, sr.NONE_TRAINED], ids=["all", "none"])
def test_training_flags_and_ignore_index(roles):
    rng = np.random.default_rng(3)
    samples = [[(int(rng.integers(0, 6)), rng.integers(0, 50000, size=int(k)).tolist()) for k in rng.integers(0, 12, size=3)] for _ in range(20)]
    for ignore in (-100, 0, -1):
        check(samples, 24, [dict(bos=1, eos=2, ignore_first=True), dict(keep_tail=True, ignore_first=True), dict(eos=2)], roles=roles, ignore=ignore, blocks=(16,))


def test_token_pointer_that_is_not_16_byte_aligned():
    """tk_srow_lane fetches eight body tokens at once where their address is a multiple of 16: the token array at every offset from one"""
    rng = np.random.default_rng(6)
    arrays = sr.pack([[(2, rng.integers(0, 50000, size=70).tolist()), (0, [])], [(3, rng.integers(0, 50000, size=150).tolist()), (1, [5] * 9)], [(3, [9] * 40)]])
    tokens = arrays[0]
    room = np.zeros(len(tokens) + 8, np.uint32)
    first = (-room.ctypes.data // 4) % 4  # the element of `room` that lies on a 16-byte boundary
    for shift in range(4):
        held = room[first + shift: first + shift + len(tokens)]
        held[:] = tokens
        assert held.ctypes.data % 16 == 4 * shift
        for L, kw in ((128, dict(bos=1)), (300, dict(eos=2, keep_tail=True)), (64, dict())):
            rc, got = run_sim(held, *arrays[1:], sr.CHAT, L, 16, pad=7, **kw)
            assert rc == 0
            rr.same(got, rr.rows_rule(*arrays, sr.CHAT, L, pad=7, **kw), (shift, L, kw))


def test_random_sweep():
    rng = np.random.default_rng(0x5A3)
    for _ in range(150):
        samples = []
        for _ in range(int(rng.choice([1, 2, 5, 30, 90]))):
            parts = []
            for _ in range(int(rng.choice([0, 0, 1, 2, 3, 8]))):
                k = 0 if rng.random() < 0.3 else int(rng.choice([1, 2, 7, 8, 9, 30]))
                parts.append((int(rng.integers(0, 6)), rng.integers(0, 60000, size=k).tolist()))
            samples.append(parts)
        bos, eos = sr.SPECIALS[int(rng.integers(0, 4))]
        kw = dict(bos=bos, eos=eos, keep_tail=bool(rng.integers(0, 2)), skip_long=bool(rng.integers(0, 2)), ignore_first=bool(rng.integers(0, 2)))
        check(samples, int(rng.choice([1, 2, 3, 8, 13, 64, 100, 2048])), [kw], roles=(sr.CHAT, sr.ALL_TRAINED)[int(rng.integers(0, 2))], blocks=(16,))


def test_refusals():
    arrays = sr.pack([[(0, [1, 2, 3]), (2, [4])], [(1, [5, 6])]])
    tokens, tok_off, part_role, sample_off = arrays
    assert run_sim(*arrays, sr.CHAT, 4, 16)[0] == 0
    assert run_sim(*arrays, sr.CHAT, 0, 16)[0] == 1  # everything the samples pass refuses: max_len == 0
    assert run_sim(*arrays, (), 4, 16)[0] == 2
    assert run_sim(*arrays, sr.CHAT * 43, 4, 16)[0] == 3
    assert run_sim(*arrays, (sr.Role(tuple(range(4000)), tuple(range(97)), True),) * 3, 4, 16, n_roles=1)[0] == 5
    assert run_sim(*arrays, sr.CHAT, 4, 16, width_multiple=8)[0] == 11  # ... and the two of this pass
    assert run_sim(*arrays, sr.CHAT, 4, 16, left=True)[0] == 12
    L_, n = lib(), None
    ids_t, off_t, train_t = role_table(sr.CHAT)
    table = (len(sr.CHAT), ids_t.ctypes.data, off_t.ctypes.data, train_t.ctypes.data)
    nothing = [n] * 11
    assert L_.sample_rows_sim_place(1 << 32, n, 3, n, n, 2, *table, *spec_of(4), 0, *nothing) == 6
    assert L_.sample_rows_sim_place(7, n, (1 << 32) - 1, n, n, 2, *table, *spec_of(4), 0, *nothing) == 7
    assert L_.sample_rows_sim_place(7, n, 3, n, n, (1 << 32) - 1, *table, *spec_of(4), 0, *nothing) == 8
    # R * L reaches 2^32 through the figures alone: two samples of 2^30 + 1 tokens do not share a row of 2^31 (T is not the array's)
    two = np.array([0, (1 << 30) + 1, (1 << 31) + 2], np.uint64)
    plain = (sr.Role(),)
    args = (two, np.zeros(2, np.uint8), np.array([0, 1, 2], np.uint64), plain)
    assert run_sim(tokens, *args, 1 << 31, 16, T=(1 << 31) + 2)[0] == 10
    assert run_sim(tokens, *args, 1 << 31, 16, T=(1 << 31) + 2, skip_long=True, ignore_first=True)[0] == 10
    big = np.array([0, (1 << 32) - 2, (1 << 32) - 2, (1 << 32) - 1], np.uint64)
    assert run_sim(tokens, big, part_role, sample_off, sr.CHAT, 4, 16, T=(1 << 32) - 1)[0] == 9
    for bad, part, why in (([1, 3, 4, 6], 0, 1), ([0, 4, 3, 6], 1, 2), ([0, 3, 4, 7], 2, 3), ([0, 1 << 40, 4, 6], 1, 2), ([0, 3, 1 << 63, 6], 2, 2)):
        for kw in (dict(), dict(bos=1, eos=2, keep_tail=True, skip_long=True, ignore_first=True)):
            assert run_sim(tokens, np.array(bad, np.uint64), part_role, sample_off, sr.CHAT, 5, 16, **kw)[0] == 16 + (part << 2 | why), bad
    for bad, sample, why in (([1, 2, 3], 0, 1), ([0, 3, 2], 1, 2), ([0, 2, 4], 1, 3), ([0, 1 << 50, 3], 1, 2), ([0, 1, 0, 3], 1, 2)):
        for kw in (dict(), dict(bos=1, eos=2, keep_tail=True, skip_long=True, ignore_first=True)):
            assert run_sim(tokens, tok_off, part_role, np.array(bad, np.uint64), sr.CHAT, 5, 16, **kw)[0] == BAD_SOFF + (sample << 2 | why), bad
    for bad, part in (([6, 0, 1], 0), ([0, 200, 255], 1), ([0, 1, 6], 2)):
        assert run_sim(tokens, tok_off, np.array(bad, np.uint8), sample_off, sr.CHAT, 5, 16, ignore_first=True)[0] == BAD_ROLE + part


def todo_for_the_sanitizers():
    out = []
    rng = np.random.default_rng(2048)
    for i, (name, samples, L, kws) in enumerate(rr.cases(rng)):
        for j, kw in enumerate(kws):
            out.append((sr.pack(samples), sr.CHAT, BLOCKS[(i + j) % 2], (i + j) % 2, L, dict(pad=7, **kw)))
    arrays = sr.pack([[(0, [1, 2, 3]), (2, [4])], [(1, [5, 6])]])
    for bad in ([0, 4, 3, 6], [0, 3, 1 << 63, 6]):  # refusals run through the same checks
        out.append(((arrays[0], np.array(bad, np.uint64), arrays[2], arrays[3]), sr.CHAT, 16, 0, 5, dict()))
    out.append(((arrays[0], arrays[1], np.array([0, 200, 1], np.uint8), arrays[3]), sr.CHAT, 16, 0, 5, dict(ignore_first=True)))
    out.append(((arrays[0], arrays[1], arrays[2], np.array([0, 1 << 50, 3], np.uint64)), sr.CHAT, 16, 1, 5, dict(skip_long=True)))
    return out


def test_case_list_under_sanitizers(tmp_path):
    """The driver as a program of its own, built with -fsanitize=address,undefined, on the case list and on refused calls: it must run
    clean and give the results of the restatement."""
    exe = h.build_once("sample_rows_sim_san", SRCS, ["-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSAMPLE_ROWS_SIM_MAIN"])
    todo = todo_for_the_sanitizers()
    src, dst = tmp_path / "cases.bin", tmp_path / "results.bin"
    with open(src, "wb") as f:
        for (tokens, tok_off, part_role, sample_off), roles, block, order, L, kw in todo:
            ids_t, off_t, train_t = role_table(roles)
            spec = spec_of(L, **kw)
            f.write(struct.pack("<16Q", len(tokens), len(tok_off) - 1, len(sample_off) - 1, len(roles), len(ids_t) - 1, *spec[:5], spec[5] & 0xFFFFFFFF, spec[6], block, order, 0, 0))
            f.write(tok_off.tobytes() + sample_off.tobytes() + off_t.tobytes() + ids_t[:-1].tobytes() + tokens.tobytes() + part_role.tobytes() + train_t[:-1].tobytes())
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    assert r.stdout.strip() == f"{len(todo)} cases"
    raw = open(dst, "rb").read()
    at = 0
    for arrays, roles, block, order, L, kw in todo:
        rc, R, S = struct.unpack_from("<qQQ", raw, at)
        at += 24
        try:
            want = rr.rows_rule(*arrays, roles, L, **kw)
        except rr.Refused:
            assert rc > 0
            continue
        n = len(arrays[3]) - 1
        assert rc == 0 and (R, L) == want.ids.shape and S + 1 == len(want.cu_seqlens)
        got = []
        for dtype, count in ((np.uint32, R * L), (np.int32, R * L), (np.uint32, R * L), (np.uint32, R * L), (np.uint32, S + 1), (np.uint32, R + 1), (np.uint32, R + 1),
                             (np.uint32, n), (np.uint64, n), (np.uint32, n), (np.uint32, n), (np.uint32, n)):
            got.append(np.frombuffer(raw, dtype, count, at))
            at += count * np.dtype(dtype).itemsize
        rr.same(rr.SampleRows(*[g.reshape(R, L) for g in got[:4]], *got[4:]), want, (block, order, L, kw))
    assert at == len(raw)
