"""The samples passes (tk_samples.h) on the CPU: tests/hostsim/samples_sim.cpp compiles the plain C++ they are made of
(tiktoken_amd/csrc/tk_samples_rule.h) for the host and drives it the way the kernels do -- lanes of eight positions, workgroups of 16 and
2048, every array behind a reader that checks the index; the write pass runs through tk_smp_lane, the function the kernel itself calls.
Compared with the restatement of the rule as Python loops in tests/samples_ref.py, which is written from the rule's description
(include/tiktoken_amd.h), not from the kernels.  The same driver also runs as a program of its own under the address and
undefined-behaviour sanitizers (host code only: nothing of it is loaded into Python)."""
import ctypes
import struct
import subprocess

import numpy as np
import pytest

import helpers as h
import samples_ref as sr

_lib = None
BLOCKS = (16, 2048)
KEEP_TAIL, LEFT = 1, 2
NONE = 0xFFFFFFFF
SRCS = ("samples_sim.cpp", "sim_readers.h", "tk_samples_rule.h", "tk_rows_rule.h", "tk_common.h")
BAD_SOFF, BAD_ROLE = 1 << 40, 1 << 41


def lib():
    global _lib
    if _lib is None:
        L = h.build_sim("libsamples_sim.so", SRCS, ("-Wall", "-Werror",))
        vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int32
        L.samples_sim_count.restype = ctypes.c_int64
        L.samples_sim_count.argtypes = [u64, vp, u64, vp, vp, u64, u64, vp, vp, vp, u32, u32, u32, u32, u32, i32, u32, vp, vp, vp, vp, vp]
        L.samples_sim.restype = ctypes.c_int64
        L.samples_sim.argtypes = [vp, u64, vp, u64, vp, vp, u64, u64, vp, vp, vp, u32, u32, u32, u32, u32, i32, u32, u32, vp, u32, vp, vp, vp]
        _lib = L
    return _lib


def role_table(roles):
    ids, off, train = [], [0], []
    for r in roles:
        ids += list(r.before)
        off.append(len(ids))
        ids += list(r.after)
        off.append(len(ids))
        train.append(1 if r.train else 0)
    return np.array(ids + [0], np.uint32), np.array(off, np.uint32), np.array(train + [0], np.uint8)


def spec_of(max_len, width_multiple=0, bos=None, eos=None, pad=0, ignore=sr.IGNORE, keep_tail=False, left=False):
    return (max_len, width_multiple, NONE if bos is None else bos, NONE if eos is None else eos, pad, ignore, (KEEP_TAIL if keep_tail else 0) | (LEFT if left else 0))


def run_sim(tokens, tok_off, part_role, sample_off, roles, max_len, block, *, T=None, n_roles=None, **kw):
    """(rc, Samples or None) of the simulation; the arrays sit in front of guard words that must survive."""
    tokens = np.ascontiguousarray(tokens, np.uint32)
    tok_off, sample_off = np.ascontiguousarray(tok_off, np.uint64), np.ascontiguousarray(sample_off, np.uint64)
    part_role = np.ascontiguousarray(part_role, np.uint8)
    T, n_parts, R = len(tokens) if T is None else T, len(tok_off) - 1, len(sample_off) - 1
    ids_t, off_t, train_t = role_table(roles)
    n_roles = len(roles) if n_roles is None else n_roles
    G = 0xDEADBEEF
    spec = spec_of(max_len, **kw)
    pstart, full = np.full(n_parts + 2, G, np.uint64), np.full(R + 1, G, np.uint64)
    ln, ntr = np.full(R + 1, G, np.uint32), np.full(R + 1, G, np.uint32)
    counts = np.zeros(2, np.uint64)
    roles_p = part_role if n_parts else np.zeros(1, np.uint8)
    table = (n_roles, ids_t.ctypes.data, off_t.ctypes.data, train_t.ctypes.data)
    rc = lib().samples_sim_count(T, tok_off.ctypes.data, n_parts, roles_p.ctypes.data, sample_off.ctypes.data, R, *table, *spec, pstart.ctypes.data, full.ctypes.data,
                                 ln.ctypes.data, ntr.ctypes.data, counts.ctypes.data)
    if rc:
        return rc, None
    assert int(counts[0]) == R
    W = int(counts[1])
    ids, lab, mask = np.full(R * W + 1, G, np.uint32), np.full(R * W + 1, 0x5A5A5A5A, np.int32), np.full(R * W + 1, 0xAB, np.uint8)
    src = tokens if T else np.zeros(1, np.uint32)
    rc = lib().samples_sim(src.ctypes.data, T, tok_off.ctypes.data, n_parts, roles_p.ctypes.data, sample_off.ctypes.data, R, *table, *spec, block, pstart.ctypes.data, W,
                           ids.ctypes.data, lab.ctypes.data, mask.ctypes.data)
    if rc:
        return rc, None
    assert ids[-1] == G and lab[-1] == 0x5A5A5A5A and mask[-1] == 0xAB and pstart[-1] == G and full[-1] == G and ln[-1] == G and ntr[-1] == G
    return 0, sr.Samples(ids[:-1].reshape(R, W), mask[:-1].reshape(R, W), lab[:-1].reshape(R, W), ln[:-1], full[:-1], ntr[:-1])


def check(samples, max_lens, blocks=BLOCKS, specials=sr.SPECIALS, roles=sr.CHAT, pad=7, settings=None, ignore=sr.IGNORE):
    arrays = sr.pack(samples)
    for bos, eos in specials:
        for max_len in max_lens:
            for kw in (settings if settings is not None else sr.settings()):
                want = sr.samples_rule(*arrays, roles, max_len, bos=bos, eos=eos, pad=pad, ignore=ignore, **kw)
                for block in blocks:
                    rc, got = run_sim(*arrays, roles, max_len, block, bos=bos, eos=eos, pad=pad, ignore=ignore, **kw)
                    assert rc == 0, (rc, max_len, bos, eos, kw, block)
                    sr.same(got, want, (max_len, bos, eos, kw, block))


def test_a_case_worked_by_hand():
    """Two roles: user = before [50, 51], after [52], untrained; assistant = before [50, 53], after [52], trained.  One conversation
    user [10, 11], assistant [20, 21, 22] with bos 1 and eos 2: the stream is
    1 | 50 51 10 11 52 | 50 53 20 21 22 52 | 2, thirteen elements, the last five of them trained.  Written down from the rule's text, for
    the restatement and for the simulation."""
    roles = (sr.Role((50, 51), (52,), False), sr.Role((50, 53), (52,), True))
    arrays = sr.pack([[(0, [10, 11]), (1, [20, 21, 22])], [], [(1, [])]])
    stream = [1, 50, 51, 10, 11, 52, 50, 53, 20, 21, 22, 52, 2]
    I = sr.IGNORE
    labels = [I] * 8 + [20, 21, 22, 52, 2]
    for got in (sr.samples_rule(*arrays, roles, 16, bos=1, eos=2, pad=0), run_sim(*arrays, roles, 16, 16, bos=1, eos=2, pad=0)[1]):
        assert got.ids.tolist() == [stream + [0] * 3, [1, 2] + [0] * 14, [1, 50, 53, 52, 2] + [0] * 11]
        assert got.labels.tolist() == [labels + [I] * 3, [I] * 16, [I, I, I, 52, 2] + [I] * 11]
        assert got.mask.sum(1).tolist() == [13, 2, 5] and got.len.tolist() == [13, 2, 5] and got.full_len.tolist() == [13, 2, 5] and got.n_trained.tolist() == [5, 0, 2]
    # the head under max_len 9: the cut falls on the first body token of the trained part -- one trained element survives
    for got in (sr.samples_rule(*arrays, roles, 9, bos=1, eos=2, pad=0), run_sim(*arrays, roles, 9, 16, bos=1, eos=2, pad=0)[1]):
        assert got.ids[0].tolist() == stream[:9] and got.labels[0].tolist() == [I] * 8 + [20]
        assert got.len.tolist() == [9, 2, 5] and got.full_len.tolist() == [13, 2, 5] and got.n_trained.tolist() == [1, 0, 2]
    # the tail under max_len 6 with padding in front: the cut falls inside a before run, nothing is put back in
    for got in (sr.samples_rule(*arrays, roles, 6, bos=1, eos=2, pad=0, keep_tail=True, left=True, width_multiple=8),
                run_sim(*arrays, roles, 6, 16, bos=1, eos=2, pad=0, keep_tail=True, left=True, width_multiple=8)[1]):
        assert got.ids.tolist() == [[53, 20, 21, 22, 52, 2], [0, 0, 0, 0, 1, 2], [0, 1, 50, 53, 52, 2]]
        assert got.labels.tolist() == [[I, 20, 21, 22, 52, 2], [I] * 6, [I, I, I, I, 52, 2]] and got.n_trained.tolist() == [5, 0, 2]
    # W == 0: only samples without elements, no bos / eos, width_multiple 1 -- the per-sample arrays are still there
    none = sr.pack([[], [(0, [])], []])
    bare = (sr.Role(),)
    for got in (sr.samples_rule(*none, bare, 5, width_multiple=1), run_sim(*none, bare, 5, 16, width_multiple=1)[1]):
        assert got.ids.shape == (3, 0) and got.labels.shape == (3, 0) and got.len.tolist() == [0, 0, 0] and got.full_len.tolist() == [0, 0, 0]


@pytest.mark.parametrize("block", BLOCKS)
def test_case_list(block):
    rng = np.random.default_rng(block)
    for name, samples, max_lens in sr.cases(block, rng):
        check(samples, max_lens, blocks=(block,))


@pytest.mark.parametrize("roles", [sr.ALL_TRAINED, sr.NONE_TRAINED], ids=["all", "none"])
def test_training_flags_and_ignore_index(roles):
    rng = np.random.default_rng(3)
    samples = [[(int(rng.integers(0, 6)), rng.integers(0, 50000, size=int(n)).tolist()) for n in rng.integers(0, 12, size=4)] for _ in range(12)]
    for ignore in (-100, 0, -1):
        check(samples, [5, 24, 64], roles=roles, ignore=ignore, settings=sr.settings()[::5])
    got = run_sim(*sr.pack(samples), sr.NONE_TRAINED, 24, 16, bos=1, eos=2)[1]
    assert (got.labels == sr.IGNORE).all() and not got.n_trained.any()


def test_where_the_cut_falls():
    """One sample, bos | before(3) body(4) after(2) | before(2) body(3) after(1) | eos = 17 elements: every max_len from 1 to 18, head and tail
    -- the cut on the first and the last id of a before run, of a body, of an after run, and on eos"""
    roles = (sr.Role((61, 62, 63), (64, 65), True), sr.Role((66, 67), (68,), False), sr.Role((66, 67), (68,), True))
    for second in (1, 2):
        samples = [[(0, [10, 11, 12, 13]), (second, [20, 21, 22])]]
        check(samples, list(range(1, 19)), roles=roles, blocks=(16,))


def test_lengths_around_the_cap():
    rng = np.random.default_rng(11)
    for max_len in (7, 8, 9, 64):
        for bos, eos in sr.SPECIALS:
            k = (bos is not None) + (eos is not None)
            samples = [[(3, rng.integers(0, 50000, size=n - k).tolist())] for n in (max_len - 1, max_len, max_len + 1) if n - k >= 0]
            check(samples, [max_len], specials=[(bos, eos)])


def test_role_ids_up_to_2_32_minus_2_and_256_roles():
    rng = np.random.default_rng(256)
    roles = tuple(sr.Role(tuple(int(x) for x in rng.integers(2**31, 2**32 - 1, size=i % 4)), ((2**32 - 2,) if i % 3 == 0 else ()), i % 2 == 0) for i in range(256))
    samples = [[(r, rng.integers(0, 50000, size=r % 5).tolist()) for r in range(s, 256, 8)] for s in range(8)]
    check(samples, [9, 200], roles=roles, settings=sr.settings()[::3], specials=sr.SPECIALS[::3])


def test_token_pointer_that_is_not_16_byte_aligned():
    """tk_smp_lane fetches eight body tokens at once where their address is a multiple of 16: the token array at every offset from one"""
    rng = np.random.default_rng(6)
    arrays = sr.pack([[(2, rng.integers(0, 50000, size=70).tolist()), (0, [])], [(3, rng.integers(0, 50000, size=150).tolist()), (1, [5] * 9)]])
    tokens = arrays[0]
    room = np.zeros(len(tokens) + 8, np.uint32)
    first = (-room.ctypes.data // 4) % 4  # the element of `room` that lies on a 16-byte boundary
    for shift in range(4):
        held = room[first + shift: first + shift + len(tokens)]
        held[:] = tokens
        assert held.ctypes.data % 16 == 4 * shift
        for bos, eos in sr.SPECIALS:
            for kw in sr.settings()[::3]:
                for max_len in (48, 300):
                    rc, got = run_sim(held, *arrays[1:], sr.CHAT, max_len, 16, bos=bos, eos=eos, pad=7, **kw)
                    assert rc == 0
                    sr.same(got, sr.samples_rule(*arrays, sr.CHAT, max_len, bos=bos, eos=eos, pad=7, **kw), (shift, bos, eos, kw, max_len))


def test_random_sweep():
    rng = np.random.default_rng(0x5A3)
    for _ in range(120):
        samples = []
        for _ in range(int(rng.choice([1, 2, 5, 30]))):
            parts = []
            for _ in range(int(rng.choice([0, 1, 2, 3, 8, 25]))):
                u = rng.random()
                n = 0 if u < 0.3 else int(rng.choice([1, 2, 7, 8, 9, 30, 200]))
                parts.append((int(rng.integers(0, 6)), rng.integers(0, 60000, size=n).tolist()))
            samples.append(parts)
        bos, eos = sr.SPECIALS[int(rng.integers(0, 4))]
        kw = dict(left=bool(rng.integers(0, 2)), keep_tail=bool(rng.integers(0, 2)), width_multiple=int(rng.choice([0, 1, 3, 8, 64])))
        check(samples, [int(rng.choice([1, 2, 3, 8, 13, 64, 100, 2048]))], specials=[(bos, eos)], settings=[kw], roles=(sr.CHAT, sr.ALL_TRAINED)[int(rng.integers(0, 2))])


def test_refusals():
    arrays = sr.pack([[(0, [1, 2, 3]), (2, [4])], [(1, [5, 6])]])
    tokens, tok_off, part_role, sample_off = arrays
    assert run_sim(*arrays, sr.CHAT, 4, 16)[0] == 0
    assert run_sim(*arrays, sr.CHAT, 0, 16)[0] == 1  # max_len == 0
    assert run_sim(*arrays, (), 4, 16)[0] == 2  # no roles, but parts
    assert run_sim(*sr.pack([[], []]), (), 4, 16)[0] == 0  # ... and none needed
    assert run_sim(*arrays, sr.CHAT * 43, 4, 16)[0] == 3  # 258 roles
    assert run_sim(*arrays, (sr.Role(tuple(range(4000)), tuple(range(97)), True),) * 3, 4, 16, n_roles=1)[0] == 5  # 4097 ids
    assert run_sim(*arrays, (sr.Role(tuple(range(4000)), tuple(range(96)), True),) * 3, 4, 16, n_roles=3)[0] == 5
    assert run_sim(tokens, tok_off, np.zeros(3, np.uint8), sample_off, (sr.Role(tuple(range(4000)), tuple(range(96)), True),), 4, 16)[0] == 0
    L, n = lib(), None
    ids_t, off_t, train_t = role_table(sr.CHAT)
    bad_off = off_t.copy()
    bad_off[3] = bad_off[2] - 1
    table = (len(sr.CHAT), ids_t.ctypes.data, off_t.ctypes.data, train_t.ctypes.data)
    assert L.samples_sim_count(7, n, 3, n, n, 2, len(sr.CHAT), n, bad_off.ctypes.data, n, *spec_of(4), n, n, n, n, n) == 4  # role_off descends
    # 32-bit outputs, refused from the figures alone (nothing is read): tokens, parts, samples
    assert L.samples_sim_count(1 << 32, n, 3, n, n, 2, *table, *spec_of(4), n, n, n, n, n) == 6
    assert L.samples_sim_count(7, n, (1 << 32) - 1, n, n, 2, *table, *spec_of(4), n, n, n, n, n) == 7
    assert L.samples_sim_count(7, n, 3, n, n, (1 << 32) - 1, *table, *spec_of(4), n, n, n, n, n) == 8
    # ... and after the counts: rows times width (two rows of 2^31; the figures alone), and the same batch one bit narrower
    assert run_sim(*arrays, sr.CHAT, 1 << 31, 16)[0] == 10
    # the elements of all parts: T below 2^32, the role ids carry the sum over it (the figures alone: T is not the array's)
    big = np.array([0, (1 << 32) - 2, (1 << 32) - 2, (1 << 32) - 1], np.uint64)
    assert run_sim(tokens, big, part_role, sample_off, sr.CHAT, 4, 16, T=(1 << 32) - 1)[0] == 9
    # a tok_off that does not describe the batch: the first offending part, and no access out of bounds on the way (rc -1 would say so)
    for bad, part, why in (([1, 3, 4, 6], 0, 1), ([0, 4, 3, 6], 1, 2), ([0, 3, 4, 5], 2, 3), ([0, 3, 4, 7], 2, 3), ([0, 1 << 40, 4, 6], 1, 2), ([0, 3, 1 << 63, 6], 2, 2),
                           ([2, 1, 0, 9], 0, 1)):
        for kw in (dict(), dict(bos=1, eos=2, keep_tail=True, left=True, width_multiple=8)):
            assert run_sim(tokens, np.array(bad, np.uint64), part_role, sample_off, sr.CHAT, 5, 16, **kw)[0] == 16 + (part << 2 | why), bad
    # a sample_off that does not: the first offending sample
    for bad, sample, why in (([1, 2, 3], 0, 1), ([0, 3, 2], 1, 2), ([0, 2, 2], 1, 3), ([0, 2, 4], 1, 3), ([0, 1 << 50, 3], 1, 2), ([0, 2], 0, 3), ([0, 1, 0, 3], 1, 2)):
        for kw in (dict(), dict(bos=1, eos=2, keep_tail=True, left=True, width_multiple=8)):
            assert run_sim(tokens, tok_off, part_role, np.array(bad, np.uint64), sr.CHAT, 5, 16, **kw)[0] == BAD_SOFF + (sample << 2 | why), bad
    # ... both: tok_off speaks first; a part whose role is none: the first such part
    assert run_sim(tokens, np.array([0, 4, 3, 6], np.uint64), part_role, np.array([0, 3, 2], np.uint64), sr.CHAT, 5, 16)[0] == 16 + (1 << 2 | 2)
    for bad, part in (([6, 0, 1], 0), ([0, 200, 255], 1), ([0, 1, 6], 2)):
        assert run_sim(tokens, tok_off, np.array(bad, np.uint8), sample_off, sr.CHAT, 5, 16)[0] == BAD_ROLE + part
    assert run_sim(tokens, tok_off, np.array([0, 1, 5], np.uint8), sample_off, sr.CHAT, 5, 16)[0] == 0


def todo_for_the_sanitizers():
    out = []
    for block in BLOCKS:
        rng = np.random.default_rng(block)
        for name, samples, max_lens in sr.cases(block, rng):
            for i, max_len in enumerate(max_lens):
                bos, eos = sr.SPECIALS[(i + len(name)) % 4]
                kw = sr.settings()[(i * 5 + len(samples)) % 12]
                out.append((sr.pack(samples), sr.CHAT, block, max_len, dict(bos=bos, eos=eos, pad=7, **kw)))
    arrays = sr.pack([[(0, [1, 2, 3]), (2, [4])], [(1, [5, 6])]])
    for bad in ([0, 4, 3, 6], [0, 3, 1 << 63, 6]):  # refusals run through the same checks
        out.append(((arrays[0], np.array(bad, np.uint64), arrays[2], arrays[3]), sr.CHAT, 16, 5, dict()))
    out.append(((arrays[0], arrays[1], np.array([0, 200, 1], np.uint8), arrays[3]), sr.CHAT, 16, 5, dict()))
    out.append(((arrays[0], arrays[1], arrays[2], np.array([0, 1 << 50, 3], np.uint64)), sr.CHAT, 16, 5, dict()))
    return out


def test_case_list_under_sanitizers(tmp_path):
    """The driver as a program of its own, built with -fsanitize=address,undefined, on the case list and on refused calls: it must run
    clean and give the results of the restatement."""
    exe = h.build_once("samples_sim_san", SRCS, ["-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSAMPLES_SIM_MAIN"])
    todo = todo_for_the_sanitizers()
    src, dst = tmp_path / "cases.bin", tmp_path / "results.bin"
    with open(src, "wb") as f:
        for (tokens, tok_off, part_role, sample_off), roles, block, max_len, kw in todo:
            ids_t, off_t, train_t = role_table(roles)
            spec = spec_of(max_len, **kw)
            f.write(struct.pack("<16Q", len(tokens), len(tok_off) - 1, len(sample_off) - 1, len(roles), len(ids_t) - 1, *spec[:5], spec[5] & 0xFFFFFFFF, spec[6], block, 0, 0, 0))
            f.write(tok_off.tobytes() + sample_off.tobytes() + off_t.tobytes() + ids_t[:-1].tobytes() + tokens.tobytes() + part_role.tobytes() + train_t[:-1].tobytes())
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    assert r.stdout.strip() == f"{len(todo)} cases"
    raw = open(dst, "rb").read()
    at = 0
    for arrays, roles, block, max_len, kw in todo:
        rc, R, W = struct.unpack_from("<qQQ", raw, at)
        at += 24
        try:
            want = sr.samples_rule(*arrays, roles, max_len, **kw)
        except sr.Refused:
            assert rc > 0
            continue
        assert rc == 0 and (R, W) == want.ids.shape
        got = []
        for dtype, count in ((np.uint32, R * W), (np.int32, R * W), (np.uint8, R * W), (np.uint32, R), (np.uint64, R), (np.uint32, R)):
            got.append(np.frombuffer(raw, dtype, count, at))
            at += count * np.dtype(dtype).itemsize
        sr.same(sr.Samples(got[0].reshape(R, W), got[2].reshape(R, W), got[1].reshape(R, W), *got[3:]), want, (block, max_len, kw))
    assert at == len(raw)
