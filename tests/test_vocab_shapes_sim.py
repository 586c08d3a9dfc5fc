"""The tables of tk_build_tables and the shared host / device probes on vocabularies of other shapes than the trained, dense ones the
rest of the suite uses (tests/vocab_shapes.py): wide and sparse ids, no short table, no device decode table, untrained token sets, the
256 bytes alone.  CPU only: the simulation of tests/hostsim against the dictionaries themselves, the C oracle and py_oracle.  The same
shapes on the device: tests/test_gpu_vocab_shapes.py."""
import functools
import random
import zlib

import pytest

import helpers as h
import vocab_shapes as vs
from oracle import c_oracle, py_oracle

ABSENT = 0xFFFFFFFF
SHAPES = [(s, m) for s in vs.TOKEN_SETS for m in vs.ID_MAPS]
shapes = pytest.mark.parametrize("set_name,map_name", SHAPES)


def _seed(*what) -> int:
    return zlib.crc32(repr(what).encode())


@functools.lru_cache(maxsize=4)  # (a test at a time walks the shapes in order: a shape's tables are built once per test, not kept for all 27)
def sim_of(set_name, map_name):
    ranks, specials = vs.vocab(set_name, map_name)
    return h.HostSim(h.PAT_STR[0], ranks, specials)


def test_constants_are_the_headers():
    assert vs.TK_PAIR8_MAX_ID == (1 << 21) - 2 and vs.TK_SHORT_MAX_RANK == 0x3FFFFFFE
    assert [vs.bin_of(n) for n in (2, 16, 17, 24, 25, 64, 65, 128, 129, 512, 513, 1024)] == [0, 0, 1, 1, 2, 4, 5, 5, 6, 7, 8, 8]


@shapes
def test_lookup_finds_every_token_and_nothing_else(set_name, map_name):
    ranks, _ = vs.vocab(set_name, map_name)
    sim = sim_of(set_name, map_name)
    for t, r in ranks.items():
        assert sim.lookup(t) == r, t
    for c in vs.non_tokens(set_name, random.Random(_seed("non", set_name)), 5000):
        assert sim.lookup(c) == ABSENT, c


def count_pairs(ranks) -> int:
    return sum(1 for t in ranks for s in range(1, len(t)) if t[:s] in ranks and t[s:] in ranks)


@shapes
def test_pair_table_is_exact(set_name, map_name):
    ranks, _ = vs.vocab(set_name, map_name)
    sim = sim_of(set_name, map_name)
    n = 0
    for t, r in ranks.items():
        for s in range(1, len(t)):
            a, b = ranks.get(t[:s]), ranks.get(t[s:])
            if a is not None and b is not None:
                n += 1
                assert sim.lookup_pair(a, b) == r, (t, s)
    assert sim.n_pairs() == n == count_pairs(ranks)
    rng = random.Random(_seed("pairs", set_name, map_name))
    toks = list(ranks)
    ids = sorted(ranks.values())
    used = set(ids)
    tried = 0
    while tried < 20000:
        a, b = rng.choice(toks), rng.choice(toks)
        if a + b in ranks:
            continue
        tried += 1
        assert sim.lookup_pair(ranks[a], ranks[b]) == ABSENT, (a, b)
    for _ in range(2000):  # ids that belong to no token: holes of the map, ids beyond it
        a, b = rng.choice(ids) + rng.choice((0, 1)), rng.randrange(0, ids[-1] + 2)
        if a in used and b in used:
            continue
        assert sim.lookup_pair(a, b) == ABSENT, (a, b)


@shapes
def test_table_format_is_what_the_ids_call_for(set_name, map_name):
    want = vs.expected_format(set_name, map_name)
    fmt = sim_of(set_name, map_name).table_format()
    assert bool(fmt & vs.FMT_SHORT) == want["short_table"]
    assert bool(fmt & vs.FMT_PAIR_PACKED) == want["pair_table_packed"]
    assert bool(fmt & vs.FMT_DEC_DENSE) == want["dec_dense"]


@pytest.mark.parametrize("set_name", vs.TOKEN_SETS)
def test_table_format_flips_exactly_at_the_edges(set_name):
    """Without special tokens, so that the largest rank is the largest id of all"""
    def fmt(map_name):
        return h.HostSim(h.PAT_STR[0], vs.vocab(set_name, map_name)[0], {}).table_format()

    assert fmt("dense") == vs.FMT_SHORT | vs.FMT_PAIR_PACKED | vs.FMT_DEC_DENSE
    assert fmt("packed_edge") & vs.FMT_PAIR_PACKED and not fmt("wide_edge") & vs.FMT_PAIR_PACKED
    assert fmt("packed_edge") & vs.FMT_SHORT and fmt("wide_edge") & vs.FMT_SHORT
    assert fmt("short_edge") & vs.FMT_SHORT and not fmt("no_short") & vs.FMT_SHORT
    assert not fmt("top") & (vs.FMT_SHORT | vs.FMT_PAIR_PACKED | vs.FMT_DEC_DENSE)
    # a special token's id counts for the short table (its id has to fit the table's rank field no more than a rank does, yet
    # tk_build_tables takes the largest id of all): one above TK_SHORT_MAX_RANK takes the table away
    ranks = vs.vocab(set_name, "short_edge")[0]
    assert not h.HostSim(h.PAT_STR[0], ranks, {"<|above|>": vs.TK_SHORT_MAX_RANK + 1}).table_format() & vs.FMT_SHORT


@shapes
def test_encode_piece_equals_the_c_oracle(set_name, map_name):
    ranks, specials = vs.vocab(set_name, map_name)
    sim, C = sim_of(set_name, map_name), c_oracle.COracle(0, ranks, specials)
    for p in vs.pieces(set_name, random.Random(_seed("pieces", set_name)), 3000, n_long=50):
        assert sim.encode_piece(p) == C.encode_piece(p), p


@pytest.mark.parametrize("set_name,map_name,count", [("bytes_only", "dense", 300), ("bytes_only", "top", 300), ("untrained", "dense", 300)])
def test_encode_piece_equals_py_oracle(set_name, map_name, count):
    """A second witness on vocabularies the C oracle has never seen either"""
    ranks, specials = vs.vocab(set_name, map_name)
    sim, C = sim_of(set_name, map_name), c_oracle.COracle(0, ranks, specials)
    for p in vs.pieces(set_name, random.Random(_seed("py", set_name)), count, n_long=5):
        want = py_oracle.encode_single_piece(p, ranks)
        assert sim.encode_piece(p) == want and C.encode_piece(p) == want, p


BYTES = {bytes([b]): b for b in range(256)}


def test_ids_of_2_to_the_31_minus_1_are_refused():
    with pytest.raises(ValueError, match="not supported"):
        h.HostSim(h.PAT_STR[0], {**BYTES, b"ab": 0x7FFFFFFF}, {})
    with pytest.raises(ValueError, match="not supported"):
        h.HostSim(h.PAT_STR[0], BYTES, {"<|s|>": 0x7FFFFFFF})
    sim = h.HostSim(h.PAT_STR[0], {**BYTES, b"ab": 0x7FFFFFFE}, {"<|s|>": 0x7FFFFFFD})
    assert sim.lookup(b"ab") == 0x7FFFFFFE and sim.lookup_pair(ord("a"), ord("b")) == 0x7FFFFFFE and sim.encode_piece(b"cab") == [ord("c"), 0x7FFFFFFE]


def test_a_four_byte_token_of_rank_0x3fffffff_is_found():
    """Regression (found by trained x short_edge): rank 0x3FFFFFFF with a length of 4 made a short slot's value TK_SHORT_EMPTY -- the
    token was never found, and its slot could be given away.  The short table now ends at 0x3FFFFFFE."""
    for rank, short in ((0x3FFFFFFF, 0), (0x3FFFFFFE, vs.FMT_SHORT)):
        for tok in (b"abcd", b"abc", b"ab"):
            ranks = {**BYTES, tok: rank, b"cd": 300}
            sim, C = h.HostSim(h.PAT_STR[0], ranks, {}), c_oracle.COracle(0, ranks, {})
            assert sim.table_format() & vs.FMT_SHORT == short
            assert sim.lookup(tok) == rank and sim.lookup(b"cd") == 300 and sim.encode_piece(tok) == [rank]
            assert sim.encode_piece(b"x" + tok + b"cd") == C.encode_piece(b"x" + tok + b"cd")


def test_the_text_of_the_gpu_tests_meets_its_conditions():
    """Counted with the oracle's split alone (the GPU file asserts the same before it encodes)"""
    docs = vs.shape_docs()
    for set_name in vs.TOKEN_SETS:
        ranks, specials = vs.vocab(set_name, "dense")
        census = vs.text_census(c_oracle.COracle(0, ranks, specials), docs, ranks)
        assert min(census["bins"]) >= 32 and census["over_1k"] >= 5, (set_name, census)
        if set_name == "untrained":  # (the only set with tokens of more than 23 bytes that are letter runs)
            assert census["long_tokens"] >= 20, census
    assert any(len(d) == vs.ONE_PIECE_DOC and len(c_oracle.COracle(0, ranks, {}).split(d)) == 1 for d in docs)
