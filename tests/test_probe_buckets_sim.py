"""The bucketed whole-piece tables (tk_common.h, "bucketed tables") on the CPU: the builder of tk_tables.cpp and the probes the device
runs, through the simulations of tests/hostsim (tk_hostsim.cpp; probe_sim.cpp for the probes themselves).  Every token of at most 23 bytes is found with its rank and every near-miss is absent, on
the vocabulary shapes of tests/vocab_shapes.py, the shaped vocabularies and a vocabulary made to collide (tests/probe_vocab.py); the
builder's bound is an error, not a long walk; and the builder and the probes run under the sanitizers in a program of their own.
The same vocabularies on the device: tests/test_gpu_probe_buckets.py."""
import ctypes
import functools
import os
import random
import re
import subprocess

import numpy as np
import pytest

import helpers as h
import probe_vocab as pv
import vocab_shapes as vs

ABSENT = 0xFFFFFFFF
SHAPES = [(s, m) for s in vs.TOKEN_SETS for m in vs.ID_MAPS]
CLS = {"short": 0, "mid": 1, "xl": 2}
BW = {"short": pv.SHORT_BW, "mid": pv.MID_BW, "xl": pv.XL_BW}


@functools.lru_cache(maxsize=None)
def probe_lib():
    """tests/hostsim/probe_sim.cpp: the builder and the bucket probes themselves, a whole vocabulary checked in one call"""
    L = h.build_sim("libtk_probe_sim.so", ("probe_sim.cpp", "tk_tables.cpp", "tk_pattern.cpp", "tk_regex.cpp", "tk_common.h", "tk_tables.h"), ("-pthread",))
    vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    L.pbs_create.restype = vp
    L.pbs_create.argtypes = [vp, vp, vp, u64, ctypes.c_char_p, ctypes.c_char_p, u64]
    L.pbs_destroy.argtypes = [vp]
    L.pbs_home.restype = u64
    L.pbs_home.argtypes = [vp, vp, u32]
    L.pbs_home_stats.argtypes = [vp, vp]
    L.pbs_probe.restype = u32
    L.pbs_probe.argtypes = [vp, vp, u32]
    L.pbs_digest.restype = u64
    L.pbs_digest.argtypes = [vp]
    L.pbs_check_all.argtypes = [vp, u64, vp, vp]
    return L


class ProbeSim:
    def __init__(self, pat_str, ranks):
        toks = list(ranks.items())
        blob = np.frombuffer(b"".join(t for t, _ in toks) + b"\0" * 16, np.uint8)
        off = np.cumsum([0] + [len(t) for t, _ in toks], dtype=np.uint64)
        ids = np.array([r for _, r in toks], np.uint32)
        err = ctypes.create_string_buffer(512)
        self._h = probe_lib().pbs_create(blob.ctypes.data, off.ctypes.data, ids.ctypes.data, len(ids), pat_str.encode(), err, 512)
        if not self._h:
            raise ValueError(err.value.decode())

    def __del__(self):
        if getattr(self, "_h", None):
            probe_lib().pbs_destroy(self._h)

    def home(self, key: bytes):
        """(class, home bucket) of a string of 1..23 bytes, by the product's own hashes"""
        v = probe_lib().pbs_home(self._h, np.frombuffer(key, np.uint8).ctypes.data, len(key))
        return v >> 32, v & 0xFFFFFFFF

    def home_stats(self):
        """per class (slots, buckets, the most tokens with one home bucket, that bucket)"""
        out = np.zeros(12, np.uint64)
        probe_lib().pbs_home_stats(self._h, out.ctypes.data)
        return [tuple(int(x) for x in out[4 * c:4 * c + 4]) for c in range(3)]

    def probe(self, key: bytes) -> int:
        return probe_lib().pbs_probe(self._h, np.frombuffer(key, np.uint8).ctypes.data, len(key))

    def digest(self) -> int:
        return probe_lib().pbs_digest(self._h)

    def check_all(self, seed: int):
        """(tokens checked, neighbours checked, failures, index of the first token at which one failed)"""
        out, bad = np.zeros(3, np.uint64), np.zeros(1, np.uint64)
        probe_lib().pbs_check_all(self._h, seed, out.ctypes.data, bad.ctypes.data)
        return int(out[0]), int(out[1]), int(out[2]), int(bad[0])


def neighbours(tok: bytes, rng: random.Random):
    """Every proper prefix, an extension by one byte and a one-byte mutation"""
    yield from (tok[:k] for k in range(1, len(tok)))
    yield tok + bytes([rng.randrange(256)])
    i = rng.randrange(len(tok))
    yield tok[:i] + bytes([tok[i] ^ (1 << rng.randrange(8))]) + tok[i + 1:]


def check_lookups(sim, ranks, seed, every=1):
    rng = random.Random(seed)
    for n, (t, r) in enumerate(ranks.items()):
        if len(t) > 23:
            continue
        assert sim.lookup(t) == r, t
        if len(t) >= 9:
            assert sim.lookup_xl(t)[0] == r, t  # (the by-identity table: tks_lookup takes the hashed table for these lengths)
        if n % every:
            continue
        for c in neighbours(t, rng):
            if c not in ranks and len(c) <= 23:
                assert sim.lookup(c) == ABSENT, (t, c)
                if len(c) >= 9:
                    assert sim.lookup_xl(c)[0] == ABSENT, (t, c)


@pytest.mark.parametrize("set_name,map_name", SHAPES)
def test_tokens_found_neighbours_absent_on_the_shapes(set_name, map_name):
    ranks, specials = vs.vocab(set_name, map_name)
    check_lookups(h.HostSim(h.PAT_STR[0], ranks, specials), ranks, 1)


@pytest.mark.parametrize("name,pat", [("gpt2_shaped", 0), ("cl100k_shaped", 1), ("o200k_shaped", 2)])
def test_tokens_found_neighbours_absent_on_the_shaped_vocabularies(name, pat):
    """The tables of real size, where full buckets and buckets that keys were carried past occur: every token of at most 23 bytes, and EVERY
    proper prefix, an extension by one byte and a one-byte mutation of every one of them that is not a token -- one call of the simulation
    (tests/hostsim/probe_sim.cpp), which asks a hash set of the token strings what is a token"""
    ranks = h.golden_vocab(name)
    sim = ProbeSim(h.PAT_STR[pat], ranks)
    n_tok, n_abs, failures, first_bad = sim.check_all(2)
    assert failures == 0, (failures, list(ranks)[first_bad])
    assert n_tok == sum(len(t) <= 23 for t in ranks) and n_abs >= 2 * n_tok  # (most tokens have more than two neighbours that are not tokens)
    for cls, (slots, buckets, most, _) in zip(CLS, sim.home_stats()):  # some home bucket has more tokens than a bucket holds: keys were carried on
        assert most > BW[cls], (name, cls, most)


def test_collision_vocabulary():
    """Three buckets' worth and more of each table's tokens share the table's last bucket -- by the product's own hashes, not only by their
    restatement in probe_vocab --: all are found, beyond the wrap-around; strings of the same bucket that are not tokens, and every
    neighbour, end absent"""
    ranks, colliding, absent, slots = pv.collision_vocab()
    sim, psim = h.HostSim(h.PAT_STR[2], ranks, {}), ProbeSim(h.PAT_STR[2], ranks)
    stats = psim.home_stats()
    for cls, bw in BW.items():
        n_slots, buckets, most, at = stats[CLS[cls]]
        assert n_slots == slots[cls] and buckets == n_slots // bw  # (the sizing rules restated in probe_vocab are the builder's)
        assert len(colliding[cls]) >= 3 * bw and len(absent[cls]) == pv.N_ABSENT
        assert most >= len(colliding[cls]) and at == buckets - 1  # the fullest home bucket is the last one
        for t in colliding[cls] + absent[cls]:
            assert psim.home(t) == (CLS[cls], buckets - 1), t
        for t in colliding[cls]:
            assert sim.lookup(t) == ranks[t] == psim.probe(t)
        for t in absent[cls]:
            assert t not in ranks and sim.lookup(t) == ABSENT == psim.probe(t)
    for t in colliding["xl"]:
        assert sim.lookup_xl(t)[0] == ranks[t]
    for t in absent["xl"]:
        assert sim.lookup_xl(t)[0] == ABSENT
    check_lookups(sim, ranks, 3)
    assert psim.check_all(3)[2] == 0


def test_tables_are_the_same_from_build_to_build():
    """Every word a probe depends on -- the by-identity slots' `passed` word among them -- is the same in two builds of the same vocabulary"""
    ranks = h.golden_vocab("cl100k_shaped")
    assert ProbeSim(h.PAT_STR[1], ranks).digest() == ProbeSim(h.PAT_STR[1], ranks).digest()
    other = dict(list(ranks.items())[:-1])
    assert ProbeSim(h.PAT_STR[1], other).digest() != ProbeSim(h.PAT_STR[1], ranks).digest()


def colliding_short_keys(n_keys: int, n_short: int) -> list[bytes]:
    """n_keys four-byte keys with one home bucket in the short table of n_short tokens: the multiplier is odd, so the hash is inverted"""
    slots = pv.pow2_for(n_short)
    shift = 32 - slots.bit_length() + 1
    inv = pow(pv.SHORT_MUL, -1, 1 << 32)
    bucket = slots // pv.SHORT_BW // 2
    keys = [(((bucket * pv.SHORT_BW) << shift | low) * inv) & pv.M32 for low in range(n_keys)]
    out = [k.to_bytes(4, "little") for k in keys]
    assert len(set(out)) == n_keys and {pv.short_slot(k, slots) // pv.SHORT_BW for k in out} == {bucket}
    return out


def test_builder_bound_is_an_error():
    """More keys with one home bucket than TK_BUCKET_BOUND buckets hold: tk_build_tables says so.  Half as many: every one is found."""
    singles = {bytes([b]): b for b in range(256)}
    over = pv.BUCKET_BOUND * pv.SHORT_BW + 1
    keys = colliding_short_keys(over, 256 + over)
    with pytest.raises(ValueError, match="the short token table.*full buckets in a row"):
        h.HostSim(h.PAT_STR[0], {**{k: 256 + i for i, k in enumerate(keys)}, **singles}, {})
    half = pv.BUCKET_BOUND * pv.SHORT_BW // 2
    keys = colliding_short_keys(half, 256 + half)
    ranks = {**{k: 256 + i for i, k in enumerate(keys)}, **singles}
    sim = h.HostSim(h.PAT_STR[0], ranks, {})
    for t, r in ranks.items():
        assert sim.lookup(t) == r
    assert sim.lookup(keys[0][:3] + bytes([keys[0][3] ^ 0x80])) == ABSENT


def searched_keys(cls: str, n_keys: int, lengths) -> list[bytes]:
    """n_keys strings of the class with one home bucket in the table of n_keys tokens of that class, found by search over random bytes"""
    slots = pv.pow2_for(n_keys) if cls == "mid" else pv.xl_slots(n_keys)
    slot_of = pv.mid_slot if cls == "mid" else pv.xl_slot
    rng = random.Random(len(cls) + n_keys)
    out = set()
    while len(out) < n_keys:
        k = rng.randbytes(rng.choice(lengths))
        if slot_of(k, slots) // BW[cls] == 5:
            out.add(k)
    return sorted(out)


@pytest.mark.parametrize("cls,lengths,name", [("mid", (5, 6, 7, 8), "mid"), ("xl", (9, 12, 16, 17, 23), "by-identity")])
def test_builder_bound_of_the_mid_and_by_identity_tables(cls, lengths, name):
    """The same for the two other tables, with searched keys: one key more than TK_BUCKET_BOUND buckets hold is the error that names the
    table; half as many are all found, and so absent are their neighbours"""
    singles = {bytes([b]): b for b in range(256)}
    over = pv.BUCKET_BOUND * BW[cls] + 1
    keys = searched_keys(cls, over, lengths)
    with pytest.raises(ValueError, match=f"the {name} token table.*full buckets in a row"):
        ProbeSim(h.PAT_STR[0], {**{k: 256 + i for i, k in enumerate(keys)}, **singles})
    half = pv.BUCKET_BOUND * BW[cls] // 2
    keys = searched_keys(cls, half, lengths)
    ranks = {**{k: 256 + i for i, k in enumerate(keys)}, **singles}
    sim = ProbeSim(h.PAT_STR[0], ranks)
    assert sim.home_stats()[CLS[cls]][2] == half and {sim.home(k) for k in keys} == {(CLS[cls], 5)}
    for t, r in ranks.items():
        assert sim.probe(t) == r
    assert sim.check_all(5)[2] == 0


def test_builder_and_probes_under_the_sanitizers(tmp_path):
    """tests/hostsim/probe_sanitize.cpp: tk_build_tables and the three probes on the collision vocabulary, built with AddressSanitizer and
    UBSan, every table a heap block of exactly its bytes.  The probed keys: every token, every colliding string that is not one, every
    neighbour -- the last bucket of each table, where the sequences wrap around, among them.  Host code in a program of its own: nothing
    is loaded into Python."""
    exe = str(tmp_path / "probe_sanitize")
    src = [os.path.join(h.HOSTSIM, "probe_sanitize.cpp")] + [os.path.join(h.CSRC, f) for f in ("tk_tables.cpp", "tk_pattern.cpp", "tk_regex.cpp")]
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *src, "-pthread", "-o", exe],
                        capture_output=True, text=True)
    if cc.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|cannot find lib(asan|ubsan)|lib(asan|ubsan)\S*: No such file", cc.stderr):
        pytest.skip("this g++ has no sanitizer runtime")  # (the linker says so; any other diagnostic is a failure)
    assert cc.returncode == 0, cc.stderr[-2000:]
    ranks, colliding, absent, slots = pv.collision_vocab()
    rng = random.Random(4)
    probes = {t: r for t, r in ranks.items()}
    for cls in pv.CLASSES:
        probes.update({t: ABSENT for t in absent[cls]})
    for t in list(ranks):
        probes.update({c: ABSENT for c in neighbours(t, rng) if c not in ranks and len(c) <= 23})
    toks, keys = list(ranks.items()), list(probes.items())
    off = np.cumsum([0] + [len(t) for t, _ in toks], dtype=np.uint64)
    koff = np.cumsum([0] + [len(t) for t, _ in keys], dtype=np.uint64)
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        f.write(np.array([len(toks), int(off[-1]), len(keys), int(koff[-1])], np.uint64).tobytes())
        f.write(off.tobytes() + np.array([r for _, r in toks], np.uint32).tobytes() + b"".join(t for t, _ in toks))
        f.write(koff.tobytes() + np.array([r for _, r in keys], np.uint32).tobytes() + b"".join(t for t, _ in keys))
    run = subprocess.run([exe, str(path), h.PAT_STR[2]], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout, run.stderr[-3000:])
    out = run.stdout.split()
    assert out[0] == "ok" and int(out[1]) == len(keys)
    for i, (cls, bw) in enumerate((("short", pv.SHORT_BW), ("mid", pv.MID_BW), ("xl", pv.XL_BW))):
        name, n_slots, most, at_last = out[2 + 4 * i], int(out[3 + 4 * i]), int(out[4 + 4 * i]), int(out[5 + 4 * i])
        # by the product's own hashes: the table is as large as probe_vocab says, three buckets' worth of tokens share a home bucket, and
        # the last bucket is the home of probed tokens and of probed strings that are not tokens
        assert name == cls and n_slots == slots[cls] and most >= 3 * bw and at_last >= len(colliding[cls]) + pv.N_ABSENT, out
