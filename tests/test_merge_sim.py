"""The long-piece merges (tk_k_merge_rounds, tk_k_merge_rounds_wide, tk_k_merge_long) on the CPU: tests/hostsim/merge_sim.cpp compiles the
plain C++ they are made of (tiktoken_amd/csrc/tk_merge_rule.h) for the host and drives it the way the kernels do -- a piece shared by 1, 2,
16 or 1024 wavefronts (the last: the wide geometry, 64 workgroups of 16), rows of 512 parts, lanes of eight, phase by phase with a barrier
count per wavefront, the wavefronts, lanes and threads of a phase ascending, descending and shuffled, exact-size buffers with every index
checked and every survivor slot of a round written exactly once.  A round that is not valid sends the piece through the simulated level
tree, one merge at a time.  The tokens are compared with the oracles' byte_pair_merge (oracle/c_oracle.py, oracle/py_oracle.py), never
with the code under test."""
import ctypes
import os
import random
import re
import struct
import subprocess

import numpy as np
import pytest

import helpers as h
from oracle import c_oracle, py_oracle

_lib = None
NWVS = ((1, 0), (2, 0), (16, 0), (1024, 1), (16, 1))  # (wavefronts, the prefix in the wide form)
SEEDS = (0, 1, 7)  # ascending, descending, shuffled
N_RESULTS = 11
BETWEEN, LASTING = 1, 2
SRCS = ("merge_sim.cpp", "tk_merge_rule.h", "tk_common.h")
LENGTHS = (2, 3, 8, 9, 63 * 8 - 1, 63 * 8 + 1, 511, 512, 513, 1023, 1024, 1025)
# one part either side of the boundaries between wavefront ranges: ranges are multiples of 512 parts -- 1024 and 16 wavefronts: 512, 1024,
# 1536 (up to 8192 parts), two wavefronts: 512 (up to 1024 parts), 1024 (up to 2048), 1536 (up to 3072)
BOUNDARIES = (1535, 1536, 1537, 2047, 2048, 2049, 3071, 3072, 3073)


def lib():
    global _lib
    if _lib is None:
        L = h.build_sim("libmerge_sim.so", SRCS, ("-Wall", "-Werror"))
        vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
        L.merge_sim.restype = ctypes.c_int64
        L.merge_sim.argtypes = [vp, u32, vp, vp, vp, vp, u64, u32, i32, u64, i32, vp, vp]
        L.merge_sim_levels.restype = i32
        L.merge_sim_levels.argtypes = [u32, vp, vp]
        _lib = L
    return _lib


class Vocab:
    """What the kernels have of a vocabulary: the rank of every byte, of every pair of bytes, and of every pair of tokens (the pair table,
    here a sorted array).  Bytes that are no token get ids nothing else has; the texts do not contain them."""

    def __init__(self, ranks: dict[bytes, int]):
        self.ranks = ranks
        self.byte_rank = np.array([ranks.get(bytes([b]), 0x7FFF0000 + b) for b in range(256)], np.uint32)
        self.pair2 = np.full(65536, 0xFFFFFFFF, np.uint32)
        pairs = {}
        for t, r in ranks.items():
            if len(t) == 2:
                self.pair2[(t[0] << 8) | t[1]] = r
            for k in range(1, len(t)):
                a, b = ranks.get(t[:k]), ranks.get(t[k:])
                if a is not None and b is not None:
                    pairs[(a << 32) | b] = r
        self.keys = np.array(sorted(pairs), np.uint64)
        self.vals = np.array([pairs[k] for k in sorted(pairs)], np.uint32)
        self.oracle = c_oracle.COracle(0, ranks, {})

    def reference(self, piece: bytes) -> list[int]:
        """byte_pair_merge's tokens: the C oracle's; where the piece itself is a token (the oracle's encode_piece answers that before it
        merges, as the front kernel does, so such a piece never reaches a merge kernel) and for short pieces also the Python oracle's"""
        want = None
        if len(piece) <= 64 or piece in self.ranks:
            cuts = py_oracle.byte_pair_merge(self.ranks, piece)
            want = [self.ranks[piece[a:b]] for a, b in zip(cuts, cuts[1:])]
        if piece not in self.ranks:
            got = self.oracle.encode_piece(piece)
            assert want is None or got == want
            want = got
        return want


def run_sim(V: Vocab, piece: bytes, nwv=1, wide=0, seed=0, force_long=False):
    n = len(piece)
    text = np.frombuffer(piece, np.uint8)
    out = np.full(n + 1, 0xDEADBEEF, np.uint32)
    result = np.zeros(N_RESULTS, np.uint64)
    rc = lib().merge_sim(text.ctypes.data, n, V.byte_rank.ctypes.data, V.pair2.ctypes.data, V.keys.ctypes.data if len(V.keys) else None,
                         V.vals.ctypes.data if len(V.keys) else None, len(V.keys), nwv, wide, seed, int(force_long), out.ctypes.data, result.ctypes.data)
    assert out[n] == 0xDEADBEEF
    res = [int(x) for x in result]
    return rc, out[:res[0]].tolist(), res


def check(V: Vocab, piece: bytes, k: int = 0, every_seed: bool = False, what=None) -> int:
    """The piece on every geometry -- one seed each, chosen by k, or all three -- against the oracle; returns the violation bits"""
    want = V.reference(piece)
    viol = set()
    for g, (nwv, wide) in enumerate(NWVS):
        for seed in SEEDS if every_seed else (SEEDS[(k + g) % 3],):
            rc, got, res = run_sim(V, piece, nwv, wide, seed)
            assert rc == 0, (rc, nwv, wide, seed, what, piece[:40])
            assert got == want, (nwv, wide, seed, what, piece[:40])
            viol.add(res[2])
    assert len(viol) == 1, (viol, what)  # (whether a round is valid does not depend on who shares the piece)
    return viol.pop()


@pytest.fixture(scope="module")
def gpt2():
    return Vocab(h.golden_vocab("gpt2_shaped"))


def test_a_round_worked_by_hand():
    """{aa: 0, aaaa: 1, b: .., ab: 2}: "aaaaab" -- the pairs aa at 0 .. 3 rank 0, ab ranks 2.  Round one picks the even ones of the run of
    four: parts 0 and 2, then parts aa aa a b; the pair (aa, aa) ranks 1, (a, b) 2.  Round two: aaaa a b.  Round three: aaaa ab.  Three
    rounds, no violation; the simulation has 1 phase boundary at the start, 3 per round and 1 at the end (its own count of where the kernel
    synchronises, not of the kernel's barrier instructions)."""
    ranks = {bytes([b]): 10 + b for b in range(256)}
    ranks.update({b"aa": 0, b"aaaa": 1, b"ab": 2})
    V = Vocab(ranks)
    assert V.reference(b"aaaaab") == [1, 2]
    for nwv, wide in NWVS:
        rc, got, res = run_sim(V, b"aaaaab", nwv, wide)
        assert rc == 0 and got == [1, 2] and res[1:4] == [3, 0, 1 + 3 * 3 + 1]
    # a longer token that ranks BELOW its parts' pair: {aa: 5, aaa: 1}: "aaaa" -- the reference merges aa at 0, then (aa, a) -> aaa before
    # the second aa: between the two picks of the round the pair (merged part, right neighbour) ranks below m
    ranks = {bytes([b]): 10 + b for b in range(256)}
    ranks.update({b"aa": 5, b"aaa": 1})
    V = Vocab(ranks)
    assert V.reference(b"aaaa") == [1, 10 + ord("a")]
    rc, got, res = run_sim(V, b"aaaa")
    assert rc == 0 and got == [1, 10 + ord("a")] and res[2] == BETWEEN and res[4] == 2
    # ... and one that only a lasting pair shows: {ab: 5, abc: 1}: "abc" -> (ab, c) ranks 1 < 5
    ranks = {bytes([b]): 10 + b for b in range(256)}
    ranks.update({b"ab": 5, b"abc": 1})
    V = Vocab(ranks)
    rc, got, res = run_sim(V, b"xabcx")
    assert rc == 0 and got == V.reference(b"xabcx") and res[2] == LASTING


def forms(rng: random.Random, n: int):
    yield "run", b"a" * n
    yield "abab", (b"ab" * n)[:n]
    yield "aab", (b"aab" * n)[:n]
    yield "two letters", bytes(rng.choice(b"ab") for _ in range(n))
    yield "three letters", bytes(rng.choice(b"ets") for _ in range(n))


def test_lengths_and_range_boundaries(gpt2):
    rng = random.Random(11)
    redone = 0
    for k, n in enumerate(LENGTHS + BOUNDARIES + (8191, 8192, 8193, 20001)):
        for name, piece in forms(rng, n):
            redone += check(gpt2, piece, k, every_seed=n in (9, 513, 1025), what=(n, name)) != 0
    assert redone == 0  # (a trained vocabulary: a longer token is learnt after its parts)


def test_runs_of_one_byte(gpt2):
    """Runs of 2 .. 20 and 508 .. 516 times one byte inside other letters, starting at every offset mod 8 around the first lane, the end of
    the first row (also the end of a wavefront's range for 16 and 1024 wavefronts) and the end of the second row (the range boundary of
    two wavefronts): odd and even parity crossing lanes, rows and ranges under a trained vocabulary, where earlier rounds shift the run.
    (A range of nothing but rank-m pairs entered by an odd run: test_an_odd_run_enters_a_range_of_nothing_but_rank_m_pairs.)"""
    rng = random.Random(12)
    redone = k = 0
    for length in list(range(2, 21)) + list(range(508, 517)):
        for start in list(range(0, 9)) + list(range(512 - 12, 512 + 5)) + list(range(1024 - 12, 1024 + 5)):
            if length > 20 and start % 8 not in (0, 3, 4, 7) and start > 8:
                continue
            n = max(start + length + rng.choice((0, 1, 5, 8)), 1030)
            fill = bytes(rng.choice(b"etn") for _ in range(n))
            piece = fill[:start] + b"x" * length + fill[start + length:]
            redone += check(gpt2, piece, k, what=(length, start)) != 0
            k += 1
    assert k > 1000 and redone == 0


def test_an_odd_run_enters_a_range_of_nothing_but_rank_m_pairs():
    """{aa: 0}: the run's pair is the lowest rank there is, so round one meets the text as written.  "b" * s + "a" * L + "b" * tail with 16
    and 1024 wavefronts (ranges of 512 parts): the run enters the second range with the parity of 512 - s, even and odd, and its last pair
    is two parts before the range's end, one before, the range's last part (the leading run is then as long as the range: every part of it
    is affected, not one more) and beyond it, into the third range.  With {aaaa: 1} as well a second round walks the halved run."""
    k = 0
    for extra in ({}, {b"aaaa": 1}):
        ranks = {bytes([b]): 10 + b for b in range(256)}
        ranks.update({b"aa": 0, **extra})
        V = Vocab(ranks)
        for s in (0, 1, 2, 3):
            for end in range(1021, 1029):  # the run's parts are s .. end - 1, its pairs s .. end - 2
                for tail in (0, 1, 4):
                    piece = b"b" * s + b"a" * (end - s) + b"b" * tail
                    assert check(V, piece, k, every_seed=end == 1024, what=(s, end, tail)) == 0
                    k += 1
    # the same at the first boundary, the run starting inside the first range's last lane: short leading runs of either parity
    V = Vocab({**{bytes([b]): 10 + b for b in range(256)}, b"aa": 0})
    for s in range(504, 513):
        for L in range(2, 12):
            assert check(V, b"b" * s + b"a" * L + b"b" * 600, s + L, what=(s, L)) == 0


def adversarial(rng: random.Random) -> dict[bytes, int]:
    """The generator of tests/test_merge_schedule_sim.py: tokens are concatenations of tokens, their ranks shuffled -- a longer token may
    rank below its parts' pair"""
    alpha = b"abc"[: rng.choice([2, 3])]
    V = {bytes([b]): 1000 + b for b in range(256)}
    toks = [bytes([c]) for c in alpha]
    for _ in range(rng.randint(3, 14)):
        t = rng.choice(toks) + rng.choice(toks)
        if t not in V and len(t) <= 8:
            toks.append(t)
            V[t] = -1
    extra = [t for t in toks if len(t) > 1]
    rng.shuffle(extra)
    V.update({t: r for r, t in enumerate(extra)})
    return V, alpha


def test_adversarial_vocabularies():
    rng = random.Random(1)
    counts = {0: 0, BETWEEN: 0, LASTING: 0, BETWEEN | LASTING: 0}
    k = 0
    for _ in range(120):
        ranks, alpha = adversarial(rng)
        V = Vocab(ranks)
        for n in (2, 3, 5, 8, 9, 17, 40, 100, rng.choice((505, 512, 513)), rng.choice((1023, 1025, 1537))):
            piece = bytes(rng.choice(alpha) for _ in range(n))
            counts[check(V, piece, k, what=(ranks, n))] += 1
            k += 1
    total = sum(counts.values())
    assert counts[BETWEEN] + counts[BETWEEN | LASTING] >= 1 and counts[LASTING] + counts[BETWEEN | LASTING] >= 1, counts
    assert counts[0] * 10 >= total, counts


def levels_ref(n: int):
    cnt, off, o = [n], [0], 0
    while True:
        cnt.append((cnt[-1] + 63) // 64)
        off.append(o)
        o += cnt[-1]
        if cnt[-1] <= 64:
            return len(cnt) - 1, cnt, off


def test_level_counts_and_offsets():
    for n, nl in ((2, 1), (64, 1), (65, 1), (4096, 1), (4097, 2), (262144, 2), (262145, 3), (1 << 24, 3), (1 << 30, 4)):
        cnt, off = np.zeros(7, np.uint32), np.zeros(7, np.uint32)
        got = lib().merge_sim_levels(n, cnt.ctypes.data, off.ctypes.data)
        want = levels_ref(n)
        assert got == nl == want[0] and cnt[:nl + 1].tolist() == want[1] and off[:nl + 1].tolist() == want[2], n


def test_one_merge_at_a_time_through_the_level_tree(gpt2):
    """Every piece straight through the simulated tk_k_merge_long: top levels of 1, 2, 64 and 65 entries (one and two levels), three
    levels once; merges whose i, j and pp lie in one, two and three blocks of 64; merges at the first and with the last part.  After every
    merge the simulation compares the whole tree with one built from the ranks."""
    rng = random.Random(13)
    seen = np.zeros(N_RESULTS, np.int64)
    for k, n in enumerate((2, 3, 63, 64, 65, 66, 127, 128, 129, 130, 1025, 4095, 4096, 4097, 4161)):
        for name, piece in forms(rng, n):
            want = gpt2.reference(piece)
            rc, got, res = run_sim(gpt2, piece, seed=SEEDS[k % 3], force_long=True)
            assert rc == 0 and got == want, (rc, n, name)
            assert res[10] == (1 if n <= 4096 else 2) and res[4] == n - len(want)
            seen += np.array(res, np.int64)
    # i, j and pp in three blocks of 64: a part of 64 bytes and more between them -- a vocabulary with the runs of 2, 4, .. 128 times "a"
    ranks = {bytes([b]): 10 + b for b in range(256)}
    ranks.update({b"a" * (2 << k): k for k in range(7)})
    V = Vocab(ranks)
    for n in (129, 200, 4161):
        rc, got, res = run_sim(V, b"a" * n, force_long=True)
        assert rc == 0 and got == V.reference(b"a" * n)
        seen += np.array(res, np.int64)
        check(V, b"a" * n, n)
    assert all(seen[5:10] > 0), seen
    piece = bytes(rng.choice(b"etaoin shr") for _ in range(262145))
    rc, got, res = run_sim(gpt2, piece, force_long=True)
    assert rc == 0 and res[10] == 3 and got == gpt2.reference(piece)
    ranks, _ = adversarial(random.Random(5))
    V = Vocab(ranks)
    for n in (65, 130, 4097):
        piece = bytes(rng.choice(b"ab") for _ in range(n))
        rc, got, res = run_sim(V, piece, force_long=True)
        assert rc == 0 and got == V.reference(piece)


# ---------------------------------------------------------------- under the sanitizers, as a program of its own
def test_pieces_under_the_sanitizers(tmp_path, gpt2):
    """tests/hostsim/merge_sanitize.cpp: the same driver with unchecked buffers -- heap blocks of exactly n entries -- built with
    AddressSanitizer and UBSan, so that an index beyond a block ends the run there.  Host code in a program of its own: nothing is loaded
    into Python."""
    exe = str(tmp_path / "merge_sanitize")
    d = os.path.join(h.ROOT, "tests", "hostsim")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         os.path.join(d, "merge_sanitize.cpp"), "-o", exe], capture_output=True, text=True)
    if cc.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|cannot find lib(asan|ubsan)|lib(asan|ubsan)\S*: No such file", cc.stderr):
        pytest.skip("this g++ has no sanitizer runtime")  # (the linker says so; any other diagnostic is a failure)
    assert cc.returncode == 0, cc.stderr[-2000:]
    rng = random.Random(14)
    adv = Vocab(adversarial(random.Random(5))[0])
    n_cases = n_tokens = 0
    for name, V in (("gpt2", gpt2), ("adv", adv)):
        cases = []
        for k, n in enumerate((2, 9, 505, 512, 513, 1023, 1024, 1025, 1537, 8193)):
            for _, piece in forms(rng, n):
                for g, (nwv, wide) in enumerate(NWVS):
                    cases.append((piece, nwv, wide, SEEDS[(k + g) % 3], 0))
                cases.append((piece, 1, 0, 0, 1))
        path = tmp_path / f"{name}.bin"
        with open(path, "wb") as f:
            f.write(struct.pack("<2Q", len(V.keys), len(cases)) + V.byte_rank.tobytes() + V.pair2.tobytes() + V.keys.tobytes() + V.vals.tobytes())
            for piece, nwv, wide, seed, force_long in cases:
                want = np.array(V.reference(piece), np.uint32)
                f.write(struct.pack("<6Q", len(piece), nwv, wide, seed, force_long, len(want)) + piece + want.tobytes())
                n_tokens += len(want)
        n_cases += len(cases)
        run = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
        assert run.returncode == 0 and run.stdout.split()[:2] == ["ok", str(len(cases))], (run.stdout[-300:], run.stderr[-3000:])
    assert n_cases > 500 and n_tokens > 0
