"""The back end of the encode pipeline (tk_k_count_tiles, the scan, tk_k_place, tk_k_bigcopy) on the CPU: tests/hostsim/back_sim.cpp compiles
the rules the kernels take from tiktoken_amd/csrc/tk_back_rule.h (expression macros: the kernels' own text) for the host and drives them
in the kernels' frame, which it writes again.  Compared with the restatement of the rule in tests/back_ref.py, which is written from the
rule, not from the kernels.  The simulation reads the start bitmap, the result words and the count bytes through index-checked readers
over exactly the words stage_front gives the device buffers."""
import ctypes

import numpy as np
import pytest

import back_ref as br
import helpers as h
from back_ref import Piece

_lib = None
STAGE, BIGCOPY = 1024, 4096


def lib():
    global _lib
    if _lib is None:
        L = h.build_sim("libback_sim.so", ("back_sim.cpp", "sim_readers.h", "tk_back_rule.h", "tk_common.h"), ("-Wall", "-Werror",))
        vp, u64 = ctypes.c_void_p, ctypes.c_uint64
        L.back_sim.restype = ctypes.c_int64
        L.back_sim.argtypes = [u64, u64, vp, vp, vp, vp, vp, vp, vp, vp, u64, vp, u64, u64, vp, vp, vp, vp, vp]
        L.back_sim_res_words.restype = L.back_sim_starts_words.restype = u64
        L.back_sim_res_words.argtypes = [u64]
        L.back_sim_starts_words.argtypes = [u64, u64]
        _lib = L
    return _lib


def run_sim(pieces, doc_off, n, rows=1, waves=1, ovf_base=64, tok_base=0, starts_words=None, rng=None):
    """(rc, tokens, tok_off, stats) of the simulation; outputs sit before guard words that must survive"""
    ntiles = max(1, -(-n // br.TILE))
    if starts_words is None:
        starts_words = lib().back_sim_starts_words(n, ntiles)
    dev = br.build(pieces, doc_off, n, lib().back_sim_res_words(n), starts_words, ovf_base, rng)
    total = sum(len(p.tokens) for p in pieces)
    G = 0xDEADBEEF
    out, tok_off = np.full(total + 1, G, np.uint32), np.full(len(doc_off) + 1, G, np.uint64)
    tile_nt, stats = np.zeros(ntiles, np.uint32), np.zeros(4, np.uint64)
    sizes = np.array([len(dev.res), len(dev.starts), ovf_base, len(dev.ovf) // 4, len(dev.cnt8), len(dev.staging), total, rows, waves], np.uint64)
    ptr = lambda a: a.ctypes.data
    rc = lib().back_sim(n, ntiles, ptr(dev.tile_np), ptr(dev.res), ptr(dev.tab), ptr(dev.ovf), ptr(dev.cnt8), ptr(dev.staging), ptr(dev.starts), ptr(dev.doc_off),
                        len(doc_off) - 1, ptr(dev.doc_first), 0, tok_base, ptr(sizes), ptr(out), ptr(tok_off), ptr(tile_nt), ptr(stats))
    if rc == 0:
        assert out[-1] == G and tok_off[-1] == G
    return rc, out[:-1], tok_off[:-1], [int(x) for x in stats]


def check(pieces, doc_off, n, ctx=None, **kw):
    want_tok, want_off = br.rule(pieces, doc_off, n, kw.get("tok_base", 0))
    stats = None
    for rows in (1, 3):
        for waves in (1, 3):
            rc, tok, off, stats = run_sim(pieces, doc_off, n, rows=rows, waves=waves, **kw)
            assert rc == 0, (rc, rows, waves, ctx)
            assert stats[0] == len(want_tok) and stats[1] == len(pieces), (stats, ctx)
            assert np.array_equal(tok, want_tok), (ctx, rows, waves, np.flatnonzero(tok != want_tok)[:5])
            assert np.array_equal(off, want_off), (ctx, rows, waves, np.flatnonzero(off != want_off)[:5], off[:8], want_off[:8])
    return stats


def toks(rng, k):
    return rng.integers(1, 200000, size=k).tolist()


def words(rng, n, counts, first=0, step=2):
    """pieces of the given token counts, `step` bytes apart from `first` on; the text ends `step` bytes behind the last"""
    assert first + step * len(counts) <= n
    return [Piece(first + step * i, toks(rng, c)) for i, c in enumerate(counts)]


def test_restatement_on_a_case_worked_by_hand():
    """A guard on tests/back_ref.py only: it touches neither the simulation nor the library."""
    pieces = [Piece(0, [5]), Piece(1, []), Piece(2, [7, 8, 9]), Piece(6, [4])]
    tok, off = br.rule(pieces, [0, 2, 6, 9, 9], 9, tok_base=100)
    assert tok.tolist() == [5, 7, 8, 9, 4] and off.tolist() == [100, 101, 104, 105, 105]


def test_one_tile_of_one_hundred_bytes_and_the_size_of_the_start_bitmap():
    """n = 100: tk_k_place reads all 120 words of the tile's start bitmap.  With the size stage_front gives it the reader stays quiet; with
    (nwords + 2) words, the size before, the simulation trips it."""
    rng = np.random.default_rng(100)
    pieces = words(rng, 100, [1, 2, 1, 0, 3, 1, 14, 1] * 6)
    docs = [0, 8, 50, 100]
    check(pieces, docs, 100)
    assert lib().back_sim_starts_words(100, 1) == 122
    rc, *_ = run_sim(pieces, docs, 100, starts_words=(100 + 31) // 32 + 2)
    assert rc == -1


@pytest.mark.parametrize("cnt", [0, 1, 2, 13, 14, 254, 255, 256])
def test_token_counts_around_the_inline_entry_and_the_count_byte(cnt):
    """a gap char, a token, TKD_INLINE and one beyond, the count byte's escape at 255 -- as a table entry and as an overflow entry"""
    rng = np.random.default_rng(cnt)
    for kind in ("auto", "table", "ovf") if cnt else ("gap",):
        n = 64
        pieces = [Piece(0, toks(rng, 1)), Piece(3, toks(rng, cnt), kind), Piece(9, toks(rng, 2)), Piece(20, toks(rng, cnt), kind), Piece(40, toks(rng, 1))]
        check(pieces, [0, 3, 9, 20, 40, 64, 64], n, ctx=(cnt, kind))
        check(pieces, [0, 20, 64], n, ctx=(cnt, kind, "no table"), ovf_base=0)


def test_a_missed_piece_without_an_entry_counts_as_its_one_token():
    pieces = [Piece(0, [9]), Piece(2, [0], "noentry"), Piece(4, [7, 7]), Piece(8, [0], "noentry"), Piece(10, [3])]
    check(pieces, [0, 2, 4, 8, 10, 12], 12)


@pytest.mark.parametrize("cnt", [BIGCOPY - 1, BIGCOPY])
def test_very_long_pieces_in_a_tile_that_is_not_staged(cnt):
    rng = np.random.default_rng(cnt)
    for kind in ("table", "ovf"):
        pieces = [Piece(0, toks(rng, 1)), Piece(2, toks(rng, cnt), kind), Piece(3000, toks(rng, 3)), Piece(3839, toks(rng, 1)), Piece(3840, toks(rng, 2))]
        stats = check(pieces, [0, 2, 3000, 3839, 3840, 3850], 3850, ctx=(cnt, kind))
        assert stats[2] == 0 and stats[3] == (1 if cnt >= BIGCOPY else 0), stats


@pytest.mark.parametrize("nt", [STAGE, STAGE + 1])
def test_a_tile_of_exactly_the_staged_size_and_one_more(nt):
    rng = np.random.default_rng(nt)
    counts = [1, 2, 0, 5, 1, 1, 14, 3] * 30
    counts.append(nt - sum(counts))  # (a long last piece: the staging area's copy into LDS)
    pieces = words(rng, 3840, counts) + [Piece(3840, toks(rng, 2)), Piece(3845, toks(rng, 1))]
    stats = check(pieces, [0, 6, 3840, 3845, 3850], 3850, ctx=nt)
    assert stats[2] == (1 if nt <= STAGE else 0), stats  # (the chunk's last tile is never staged)


@pytest.mark.parametrize("np_", [255, 256, 257, 513])
def test_pieces_around_a_step_of_256(np_):
    rng = np.random.default_rng(np_)
    counts = [int(c) for c in rng.choice([0, 1, 1, 1, 2, 5, 14], size=np_)]
    counts[-1] = 3
    pieces = words(rng, 3840, counts, step=3) + [Piece(3840, toks(rng, 1))]
    docs = sorted({0, 3 * 254, 3 * (np_ - 1), 3840}) + [3841]
    check(pieces, docs, 3841, ctx=np_)


@pytest.mark.parametrize("nd", [64, 65, 200])
def test_many_documents_starting_in_one_tile(nd):
    rng = np.random.default_rng(nd)
    counts = [int(c) for c in rng.choice([0, 1, 1, 2, 3, 14], size=600)]
    pieces = words(rng, 7700, counts, first=3840, step=5) + [Piece(7680 + 1, toks(rng, 2))]
    pieces = [Piece(7, toks(rng, 2))] + pieces
    at = sorted(int(x) for x in rng.choice(600, size=nd, replace=False))
    docs = [3840 + 5 * i for i in at] + [7700]
    check(pieces, docs, 7700, ctx=nd, tok_base=1 << 33)


def test_documents_at_the_first_and_last_byte_of_a_tile_and_empty_ones_at_the_end():
    rng = np.random.default_rng(5)
    for n in (3840, 3841, 7680):
        pieces = [Piece(0, toks(rng, 2)), Piece(100, toks(rng, 1)), Piece(3839, toks(rng, 3))]
        if n > 3840:
            pieces.append(Piece(3840, toks(rng, 2)))
        if n == 7680:
            pieces += [Piece(5000, toks(rng, 14)), Piece(7679, toks(rng, 1))]
        docs = [0, 3839] + [s for s in (3840, 7679) if s < n] + [n] * 6
        check(pieces, docs, n, ctx=n)
        check(pieces, [0] * 3 + docs[1:], n, ctx=(n, "empty documents at the front"))


def test_a_gap_char_right_before_a_document_start():
    """behind gap chars the sum over the listed pieces is negative: a document offset and a token place that only work modulo 2^32"""
    rng = np.random.default_rng(6)
    pieces = [Piece(0, []), Piece(1, []), Piece(2, toks(rng, 1)), Piece(3, []), Piece(4, toks(rng, 2)), Piece(6, []), Piece(7, toks(rng, 1))]
    check(pieces, [0, 2, 4, 7, 8], 8)
    check(pieces, [2, 7, 8], 8, tok_base=(1 << 32) - 1)
    pieces = [Piece(i, []) for i in range(300)] + [Piece(300, toks(rng, 1)), Piece(301, []), Piece(302, toks(rng, 20))]
    check(pieces, [0, 300, 302, 310], 310)


def test_random_sweep():
    rng = np.random.default_rng(0xBAC)
    for it in range(300):
        ntiles = int(rng.choice([1, 1, 2, 3]))
        n = int((ntiles - 1) * br.TILE + rng.integers(1, br.TILE + 1))
        k = int(min(rng.choice([1, 3, 20, 300, 700]), n))
        at = sorted(int(x) for x in rng.choice(n, size=k, replace=False))
        pieces = []
        for s in at:
            u = rng.random()
            cnt = 1 if u < 0.6 else 0 if u < 0.68 else int(rng.choice([2, 3, 13, 14, 40, 255, 300])) if u < 0.97 else 1
            kind = "auto" if u < 0.97 else "table" if u < 0.985 else "ovf"
            pieces.append(Piece(s, toks(rng, cnt), kind))
        nd = int(rng.choice([1, 2, 5, 70]))
        docs = sorted(int(x) for x in rng.choice(at, size=min(nd, k), replace=False)) + [n] * int(rng.integers(1, 4))
        check(pieces, docs, n, ctx=it, ovf_base=int(rng.choice([0, 16, 64])), tok_base=int(rng.choice([0, 12345, 1 << 40])), rng=rng)
