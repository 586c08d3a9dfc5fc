"""The decode passes (tk_decode.h) on the CPU: tests/hostsim/decode_sim.cpp compiles the plain C++ they are made of
(tiktoken_amd/csrc/tk_decode_rule.h) for the host and drives it the way the kernels do -- workgroups of 16 and 2048 tokens, lanes of eight,
the length pass, the scan, the copy pass through tk_dec_lane, the function the kernel itself calls -- with the lanes in ascending,
descending and shuffled order and a writer that checks every store: 8-byte stores aligned and inside the output, every output byte stored
exactly once, nothing outside.  Compared with tests/decode_ref.py, which is written from the reference's rule, not from the kernels."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import decode_ref as dr
import helpers as h

_lib = None
BLOCKS = (16, 2048)
SEEDS = (0, 1, 7)  # ascending, descending, shuffled
BAD_ID, OOB = 1, -1
SRCS = ("decode_sim.cpp", "sim_readers.h", "tk_decode_rule.h", "tk_device.h", "tk_common.h")


def lib():
    global _lib
    if _lib is None:
        L = h.build_sim("libdecode_sim.so", SRCS, ("-Wall", "-Werror"))
        vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
        L.decode_sim.restype = ctypes.c_int64
        L.decode_sim.argtypes = [vp, u64, vp, u32, u64, vp, vp, u32, u64, u32, u64, u64, vp, u64, vp, vp, u64, vp]
        L.decode_sim_docoff.restype = ctypes.c_int64
        L.decode_sim_docoff.argtypes = [vp, u64, u64, u64, vp, u64, vp]
        _lib = L
    return _lib


def run_sim(table, tokens, block, seed=0, *, extra_blocks=0, pos_base=0, off_base=0, dec_len=None, room=None, want_log=False):
    """(rc, bytes, tok_byte_off, first bad position, log) of the simulation; the caller's arrays sit before guard words that must survive"""
    tokens = np.ascontiguousarray(tokens, np.uint32)
    n = len(tokens)
    if room is None:
        room = sum(table.len_of.get(int(t), 0) for t in tokens)
    G = 0xDEADBEEFDEADBEEF
    out = np.full(room + 8, 0xAB, np.uint8)
    tbo = np.full(n + 1, G, np.uint64)
    log = np.zeros(room + 8 if want_log else 1, np.uint64)
    result = np.zeros(3, np.uint64)
    src = tokens if n else np.zeros(1, np.uint32)
    dec = np.ascontiguousarray(table.dec if dec_len is None else table.dec[:dec_len].copy())
    rc = lib().decode_sim(src.ctypes.data, n, dec.ctypes.data, table.n_ids, len(dec), table.tok_blob.ctypes.data, table.spec_blob.ctypes.data, block, seed, extra_blocks,
                          pos_base, off_base, out.ctypes.data, room, tbo.ctypes.data, log.ctypes.data if want_log else None, len(log), result.ctypes.data)
    total, bad, n_log = (int(x) for x in result)
    assert tbo[-1] == G and (out[room:] == 0xAB).all()
    if rc:
        return rc, None, None, None if bad == 0xFFFFFFFFFFFFFFFF else bad, None
    assert total <= room
    return 0, out[:total].tobytes(), tbo[:-1], None, log[:n_log].tolist() if want_log else None


def check(table, tokens, blocks=BLOCKS, seeds=SEEDS, what=None, **kw):
    want, off, bad = dr.decode_ref(table, tokens)
    assert bad is None
    for block in blocks:
        for seed in seeds:
            rc, got, tbo, _, _ = run_sim(table, tokens, block, seed, **kw)
            assert rc == 0, (rc, block, seed, what)
            assert got == want, (block, seed, what)
            assert np.array_equal(tbo, off[:-1] + np.uint64(kw.get("off_base", 0))), (block, seed, what)


@pytest.fixture(scope="module")
def table():
    return dr.edge_table()


def test_the_table_builder_accepts_the_edge_vocabulary():
    """The product's own table builder (tk_tables.cpp, through the host simulation) takes the vocabulary: sparse ranks, tokens of up to 300
    bytes, special tokens of 1 to 40 bytes with a gap of ids in front of the last"""
    ranks, specials = dr.edge_vocab()
    sim = h.HostSim(h.PAT_STR[1], ranks, specials)
    for t, r in ranks.items():
        assert sim.lookup(t) == r
    t = dr.edge_table()
    assert sorted(len(b) for i, b in t.by_id.items() if i not in t.special_ids and len(b) > 1) == dr.LONG_LENGTHS
    assert sorted(len(t.by_id[i]) for i in t.special_ids) == dr.SPECIAL_LENGTHS
    assert len(t.holes) > 50 and any(hole < max(ranks.values()) for hole in t.holes)
    # the last-ranked token ends the ordinary blob, the special token with the largest id ends the other
    for special, blob in ((False, t.tok_blob), (True, t.spec_blob)):
        i = t.last_of_blob(special)
        assert i == (max(specials.values()) if special else max(ranks.values()))
        o, n = int(t.dec[i][0]) & ~dr.SPEC_BIT, int(t.dec[i][1])
        assert o + n + dr.PAD == len(blob) and blob[o:o + n].tobytes() == t.by_id[i]


@pytest.mark.parametrize("block", BLOCKS)
def test_a_case_worked_by_hand(block):
    """Ten tokens over a table of five: "a", "bc", a token of nine bytes, one of eight, the special token "<|x|>" (id 5; id 4 has no
    entry).  Two lanes.  Lane 0 owns bytes [0, 29): its first word goes out byte by byte (the first word of a stretch always does), words
    8 and 16 as 8-byte stores, the rest 24 .. 28 byte by byte.  Lane 1 owns [29, 39): it starts at byte 5 of word 24 -- bytes 29, 30, 31 --
    and ends inside word 32: bytes 32 .. 38."""
    t = dr.Table({b"a": 0, b"bc": 1, b"defghijkl": 2, b"MNOPQRST": 3}, {"<|x|>": 5})
    assert t.dec.tolist() == [[0, 1], [1, 2], [3, 9], [12, 8], [0, 0], [0x80000000, 5]] and t.n_ids == 6
    tokens = [1, 0, 2, 3, 5, 0, 0, 1, 2, 0]
    want = b"bcadefghijklMNOPQRST<|x|>aabcdefghijkla"
    offsets = [0, 2, 3, 12, 20, 25, 26, 27, 29, 38]
    stores = [(b, 1) for b in range(8)] + [(8, 8), (16, 8)] + [(b, 1) for b in range(24, 29)] + [(b, 1) for b in range(29, 32)] + [(b, 1) for b in range(32, 39)]
    ref = dr.decode_ref(t, tokens)
    assert ref[0] == want and ref[1].tolist() == offsets + [39]
    rc, got, tbo, _, log = run_sim(t, tokens, block, 0, want_log=True)
    assert rc == 0 and got == want and tbo.tolist() == offsets
    assert [(e >> 1, 8 if e & 1 else 1) for e in log] == stores
    rc, got, tbo, _, log = run_sim(t, tokens, block, 1, want_log=True)  # lane 1 first
    assert rc == 0 and got == want and [(e >> 1, 8 if e & 1 else 1) for e in log] == stores[15:] + stores[:15]
    assert run_sim(t, [1, 0, 4, 3], block)[0::3] == (BAD_ID, 2)


def test_alignment_sweep(table):
    tokens = dr.alignment_sweep(table)
    assert 50_000 < len(tokens) < 100_000
    check(table, tokens, what="sweep")
    # the same with a special token as the 8-byte filler: the source blob switches on both sides of every token
    check(table, dr.alignment_sweep(table, table.id_of_len(8, special=True)), seeds=(7,), what="sweep, special fillers")


@pytest.mark.parametrize("block", BLOCKS)
def test_runs_of_one_length(table, block):
    for n_bytes in (1, 7, 8, 9):
        ids = [table.id_of_len(n_bytes)] if n_bytes > 1 else [0x41, 0x42]
        ids.append(table.id_of_len(n_bytes, special=True))
        for i in ids:
            for count in (1, 8, 9, 63, 64, 65, 3 * block + 5):
                check(table, [i] * count, blocks=(block,), what=(n_bytes, i, count))


@pytest.mark.parametrize("block", BLOCKS)
def test_lanes_inside_one_word(table, block):
    """Lanes whose eight tokens total fewer than 8 bytes cannot be: a token has a byte at least.  Lanes of exactly 8 single bytes at every
    alignment, so that each lane's stretch is the tail of one word and the head of the next and goes out byte by byte; and the batch's
    last lanes of 1 .. 7 tokens, several of which share one word with their neighbour."""
    for lead in range(8):
        for tail in range(1, 8):
            tokens = [(lead * 8 + k) & 0xFF for k in range(lead)] + [table.id_of_len(8)] * (8 - lead) if lead else []
            tokens += [(17 * k + lead) & 0xFF for k in range(64)] + [(tail + k) & 0xFF for k in range(tail)]
            check(table, tokens, blocks=(block,), what=(lead, tail))
    # a lane of 1 .. 7 single bytes behind a long token: its whole stretch lies inside one word, both neighbours in the same word
    for L in (9, 10, 11, 12, 13, 14, 15, 17):
        for k in range(1, 8):
            tokens = [table.id_of_len(L)] + [0x30 + j for j in range(7)] + [0x61 + j for j in range(k)]
            check(table, tokens, blocks=(block,), what=(L, k))


@pytest.mark.parametrize("block", BLOCKS)
def test_a_stretch_that_ends_on_a_word_boundary(table, block):
    for first in range(8):  # the stretch starts at byte `first` of a word and ends exactly at the end of a word, one to three words on
        for words in (1, 2, 3):
            lead = [table.id_of_len(8)] * (8 - first) + [(first + k) & 0xFF for k in range(first)] if first else []
            body = 8 * words - first
            lane = [table.id_of_len(body - 7)] + [0x41 + k for k in range(7)] if body - 7 >= 2 else None
            if lane is None:
                continue
            check(table, lead + lane + [table.id_of_len(16, special=True)] * 3, blocks=(block,), what=(first, words))
            check(table, lead + lane, blocks=(block,), what=(first, words, "last"))  # ... and the batch ends there


@pytest.mark.parametrize("block", BLOCKS)
def test_token_counts(table, block):
    rng = np.random.default_rng(block)
    for n in (0, 1, 7, 8, 9, block - 1, block, block + 1, 2 * block, 3 * block + 5):
        tokens = dr.random_batch(table, rng, n)
        check(table, tokens, blocks=(block,), what=n)
        check(table, tokens, blocks=(block,), seeds=(7,), extra_blocks=1, what=(n, "an empty workgroup behind"))
        check(table, tokens, blocks=(block,), seeds=(1,), pos_base=block * 4, off_base=(1 << 33) + 5, what=(n, "a later range"))


@pytest.mark.parametrize("block", BLOCKS)
def test_the_last_token_of_each_blob_ends_the_batch(table, block):
    for special in (False, True):
        last = table.last_of_blob(special)
        for lead in range(9):
            check(table, [0x41] * lead + [last], blocks=(block,), what=(special, lead))
            check(table, [table.last_of_blob(not special)] * 2 + [0x41] * lead + [last], blocks=(block,), what=(special, lead))


@pytest.mark.parametrize("block", BLOCKS)
def test_bad_ids(table, block):
    rng = np.random.default_rng(3)
    hole = next(x for x in table.holes if x < 400)
    gap = table.holes[-1]  # in the gap in front of the last special token
    base = dr.random_batch(table, rng, 3 * block + 5)
    check(table, np.concatenate([base, [table.n_ids - 1]]), blocks=(block,), what="n_ids - 1 is valid")
    for bad_id in (hole, gap, table.n_ids, table.n_ids + 1, 0x7FFFFFFF, 0x80000000 | 5, 0xFFFFFFFF):
        for pos in (0, 7, 8, block - 1, block, 2 * block + 3, len(base) - 1):
            tokens = base.copy()
            tokens[pos] = bad_id
            assert dr.decode_ref(table, tokens)[2] == pos
            for seed in SEEDS:
                assert run_sim(table, tokens, block, seed)[0::3] == (BAD_ID, pos), (bad_id, pos, seed)
            assert run_sim(table, tokens, block, 1, pos_base=1 << 35)[0::3] == (BAD_ID, (1 << 35) + pos)
    # two bad ids in different workgroups, the later workgroup visited first, the larger id first: the first position is reported
    for a, b in ((3, 2 * block + 1), (block - 1, block), (block + 2, 3 * block + 4)):
        tokens = base.copy()
        tokens[a], tokens[b] = 0xFFFFFFFF, hole
        assert dr.decode_ref(table, tokens)[2] == a
        for seed in SEEDS + (11, 12):
            assert run_sim(table, tokens, block, seed)[0::3] == (BAD_ID, a)


@pytest.mark.parametrize("block", BLOCKS)
def test_nothing_is_read_from_the_table_beyond_n_ids(table, block):
    """The table reaches the rule through a reader that checks every index: with an array of exactly n_ids entries the ids n_ids and
    0xFFFFFFFF are bad ids, not reads -- and the reader does say so when an entry the rule needs is missing (the array one entry short)"""
    tokens = np.array([0x41, table.n_ids - 1, table.n_ids, 0xFFFFFFFF, 5], np.uint32)
    assert run_sim(table, tokens, block)[0::3] == (BAD_ID, 2)
    assert run_sim(table, tokens[:2], block)[0] == 0
    assert run_sim(table, tokens[:2], block, dec_len=table.n_ids - 1)[0] == OOB


def test_random_sweep(table):
    rng = np.random.default_rng(0xDEC)
    for k in range(300):
        n = int(rng.choice([1, 5, 8, 13, 40, 130, 300, 700]))
        tokens = dr.random_batch(table, rng, n, long_share=float(rng.choice([0.1, 0.4, 0.8])), special_share=float(rng.choice([0.0, 0.15, 0.2])))
        check(table, tokens, blocks=(BLOCKS[k % 2],) if n > 300 else BLOCKS, seeds=(k % 2, 2 + k), what=k)
    check(table, dr.random_batch(table, rng, 5 * 2048 + 3), seeds=(9,))


def docoff(tok_off, n, tok_byte_off, total, short=False):
    tok_off = np.ascontiguousarray(tok_off, np.uint64)
    n_docs = len(tok_off) - 1
    out = np.full(n_docs + 2, 0xDEADBEEF, np.uint64)
    tbo = np.ascontiguousarray(tok_byte_off, np.uint64)
    off_in = tok_off[:-1].copy() if short else tok_off
    rc = lib().decode_sim_docoff(off_in.ctypes.data, len(off_in), n_docs, n, (tbo if n else np.zeros(1, np.uint64)).ctypes.data, total, out.ctypes.data)
    assert out[-1] == 0xDEADBEEF
    return rc, out[:-1]


def test_document_offsets(table):
    rng = np.random.default_rng(5)
    tokens = dr.random_batch(table, rng, 100)
    _, off, _ = dr.decode_ref(table, tokens)
    total = int(off[-1])
    for sizes in ([0, 0, 3, 0, 0, 0, 50, 1, 0, 46, 0, 0], [100], [0], [0, 0, 0, 100], [100, 0, 0], [1] * 100, [7, 0, 93]):
        n = sum(sizes)
        tok_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        rc, got = docoff(tok_off, n, off[:n], int(off[n]))
        assert rc == 0 and np.array_equal(got, dr.doc_offsets_ref(off, tok_off)), sizes
        assert got[-1] == off[n]  # tok_off[d] == n takes the total (tok_byte_off has no entry n)
    assert docoff([0, 40, 100], 100, off[:100], total, short=True)[0] == OOB


# ---------------------------------------------------------------- under the sanitizers, as a program of its own
def test_sweeps_under_the_sanitizers(tmp_path, table):
    """tests/hostsim/decode_sanitize.cpp: the same driver with the kernel's own writer (raw stores), built with AddressSanitizer and UBSan.
    Each blob is a heap block of exactly its bytes plus the 16 the table builder leaves behind them, the output one of exactly total + 16
    (what tk_api.hip allocates): tk_load8's read past a token's end and the byte-wise tails stay inside what the host allocates.  Host code
    in a program of its own: nothing is loaded into Python."""
    exe = str(tmp_path / "decode_sanitize")
    d = os.path.join(h.ROOT, "tests", "hostsim")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         os.path.join(d, "decode_sanitize.cpp"), "-o", exe], capture_output=True, text=True)
    if cc.returncode != 0 and "sanitize" in cc.stderr:
        pytest.skip("this g++ has no sanitizer runtime")
    assert cc.returncode == 0, cc.stderr[-2000:]
    rng = np.random.default_rng(0x5A)
    cases = [(dr.alignment_sweep(table), 2048, 0), (dr.alignment_sweep(table, table.id_of_len(8, special=True)), 16, 5)]
    for special in (False, True):  # the last token of each blob as the very last token
        cases += [(np.array([0x41] * lead + [table.last_of_blob(special)], np.uint32), 16, 1) for lead in range(9)]
    for k in range(200):
        cases.append((dr.random_batch(table, rng, int(rng.choice([0, 1, 9, 40, 300, 2500])), long_share=0.5, special_share=0.2), BLOCKS[k % 2], k))
    path = tmp_path / "cases.bin"
    n_bytes = 0
    with open(path, "wb") as f:
        f.write(struct.pack("<4Q", table.n_ids, len(table.tok_blob), len(table.spec_blob), len(cases)))
        f.write(table.dec.tobytes() + table.tok_blob.tobytes() + table.spec_blob.tobytes())
        for tokens, block, seed in cases:
            want = dr.decode_ref(table, tokens)[0]
            f.write(struct.pack("<4Q", len(tokens), block, seed, len(want)) + np.ascontiguousarray(tokens, np.uint32).tobytes() + want)
            n_bytes += len(want)
    run = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.split() == ["ok", str(len(cases)), str(n_bytes)], (run.stdout[-300:], run.stderr[-3000:])
