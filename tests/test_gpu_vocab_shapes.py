"""Encode and decode on the device with vocabularies of other shapes than the trained, dense ones (tests/vocab_shapes.py): a wide pair
table -- the merge kernel per length bin is then the production path --, no short table, no device decode table, a sparse host decoder,
untrained token sets, the 256 bytes alone, ids up to 0x7FFFFFFE.  The reference is the C oracle on the same packed batch (its own hash
map, no table code shared with the library): every token and every tok_off.  Each test asserts through tk_stat that the core has the
tables the shape is meant to give it.  The CPU side of the same shapes: tests/test_vocab_shapes_sim.py."""
import functools

import numpy as np
import pytest
import regex

import decode_ref as dr
import helpers as h
import padded_ref as pr
import rows_ref as rr
import samples_ref as sr
import vocab_shapes as vs
from oracle import c_oracle

pytestmark = pytest.mark.gpu

GPU_SHAPES = [("untrained", m) for m in ("dense", "wide_edge", "wide", "dec_edge_hi", "no_short", "top")] + [("trained", "wide"), ("bytes_only", "dense"), ("bytes_only", "wide")]
shapes = pytest.mark.parametrize("shape", GPU_SHAPES, ids="-".join)
PAT = h.PAT_STR[0]
DBG_MERGE_PER_BIN, DBG_ONE_MERGE = 0x800000, 1024  # TK_DBG_MERGE_PER_BIN, TK_DBG_ONE_MERGE (tk_common.h); the variable is read as a decimal number


@functools.lru_cache(maxsize=None)
def encoding_of(shape, pat=PAT):
    """One Encoding, and so one core, per shape for the whole module"""
    from tiktoken_amd import Encoding

    ranks, specials = vs.vocab(*shape)
    return Encoding("-".join(shape), pat_str=pat, mergeable_ranks=ranks, special_tokens=specials)


def core_of(shape, pat=PAT):
    return encoding_of(shape, pat)._core_bpe


@functools.lru_cache(maxsize=None)
def oracle_of(shape):
    return c_oracle.COracle(0, *vs.vocab(*shape))


@functools.lru_cache(maxsize=None)
def batch():
    """The text (vocab_shapes.shape_docs) as a packed batch, once it is known to hold what the tests are about"""
    docs = vs.shape_docs()
    for set_name in vs.TOKEN_SETS:
        ranks, specials = vs.vocab(set_name, "dense")
        census = vs.text_census(oracle_of((set_name, "dense")), docs, ranks)
        assert min(census["bins"]) >= 32 and census["over_1k"] >= 5, (set_name, census)
        assert set_name != "untrained" or census["long_tokens"] >= 20, census
    return (docs, *h.pack(list(docs)))


@functools.lru_cache(maxsize=None)
def reference(shape):
    """The oracle's (tokens, tok_off) of the batch: computed once per shape, never written to"""
    _, blob, off = batch()
    toks, toff = oracle_of(shape).encode_batch(blob, off)
    toks.setflags(write=False)
    toff.setflags(write=False)
    return toks, toff


def pieces_of(C, doc):
    ends = C.split(doc)
    return [doc[a:b] for a, b in zip([0] + ends[:-1], ends)]


def assert_path(core, shape):
    """The core took the tables the shape calls for (tk_stat): packed or wide pair table, short table or none, the device decode table's ids"""
    want = vs.expected_format(*shape)
    got = {k: core.stat(k) for k in ("pair_table_packed", "short_table", "decode_table_ids")}
    assert got == {"pair_table_packed": int(want["pair_table_packed"]), "short_table": int(want["short_table"]), "decode_table_ids": want["decode_table_ids"]}, shape
    return want


def same(got, want, what):
    toks, toff = got
    assert np.array_equal(toff, want[1]), (what, np.flatnonzero(toff != want[1])[:5].tolist())
    assert toks.dtype == np.uint32 and np.array_equal(toks, want[0]), (what, np.flatnonzero(toks != want[0][: len(toks)])[:5].tolist() if len(toks) >= len(want[0]) else (len(toks), len(want[0])))


def test_the_shapes_cover_the_branches():
    fmt = {s: vs.expected_format(*s) for s in GPU_SHAPES}
    assert {f["pair_table_packed"] for f in fmt.values()} == {True, False} and {f["short_table"] for f in fmt.values()} == {True, False}
    assert {bool(f["decode_table_ids"]) for f in fmt.values()} == {True, False} and {f["dec_dense"] for f in fmt.values()} == {True, False}
    assert not fmt[("untrained", "wide_edge")]["pair_table_packed"] and fmt[("untrained", "wide_edge")]["short_table"]


@shapes
def test_whole_batch(shape):
    core = core_of(shape)
    assert_path(core, shape)
    _, blob, off = batch()
    same(core.encode_batch_packed(blob, off), reference(shape), shape)


@shapes
def test_small_calls(shape):
    """Every document of at most 2 KiB by itself: the one-launch path (tk_k_small)"""
    core = core_of(shape)
    assert_path(core, shape)
    docs, _, _ = batch()
    toks, toff = reference(shape)
    before, n = core.stat("small_calls"), 0
    for d, doc in enumerate(docs):
        if len(doc) <= 2048:
            n += len(doc) > 0
            assert core.encode_ordinary(doc.decode()) == toks[int(toff[d]):int(toff[d + 1])].tolist(), (shape, d)
    assert n > 200 and core.stat("small_calls") - before == n


@shapes
def test_mid_size_calls(shape):
    """The documents of 8, 40, 100 and 12 KiB by themselves: cut into segments at the pattern's certain starts, the segments encoded in
    one launch (encode_mid) -- their pieces are tokens or short, as that path wants them"""
    core = core_of(shape)
    assert_path(core, shape)
    docs, _, _ = batch()
    toks, toff = reference(shape)
    sim = h.HostSim(PAT, {bytes([b]): b for b in range(256)}, {})
    mids = [d for d, doc in enumerate(docs) if len(doc) in vs.MID_DOCS and len(oracle_of(shape).split(doc)) > 1]
    assert len(mids) == 4 and all(sim.mid_plan(docs[d])[0] is not None for d in mids)
    ranks = vs.vocab(*shape)[0]
    # a segment gives the document up at a piece of more than 24 bytes that is not a token (untrained: the text has none; the others: the
    # last document has none), and the calls after such a document do not try: those that go through first
    gives_up = {d: any(len(p) > 24 and p not in ranks for p in pieces_of(oracle_of(shape), docs[d])) for d in mids}
    for d in sorted(mids, key=gives_up.get):
        given_up = gives_up[d]
        assert given_up == (shape[0] != "untrained" and len(docs[d]) != vs.MID_DOCS[3])
        before = core.stat("mid_calls")
        assert core.encode_ordinary(docs[d].decode()) == toks[int(toff[d]):int(toff[d + 1])].tolist(), (shape, d)
        if not given_up:
            assert core.stat("mid_calls") - before == 1, (shape, len(docs[d]))


@pytest.mark.parametrize("dbg", [DBG_MERGE_PER_BIN, DBG_ONE_MERGE])
@pytest.mark.parametrize("shape", [s for s in GPU_SHAPES if vs.expected_format(*s)["pair_table_packed"]], ids="-".join)
def test_merge_forms_of_the_packed_table(shape, dbg, monkeypatch):
    """A packed pair table through the kernel per length bin, and with one merge at a time on the long pieces.  (A wide table takes the
    kernels per bin by itself: test_whole_batch, where pair_table_packed is 0 -- stage_back has no other branch for it.)"""
    from tiktoken_amd import CoreBPE

    monkeypatch.setenv("TIKTOKEN_AMD_DEBUG", str(dbg))
    core = CoreBPE(*vs.vocab(*shape), PAT)
    monkeypatch.delenv("TIKTOKEN_AMD_DEBUG")
    assert_path(core, shape)
    _, blob, off = batch()
    same(core.encode_batch_packed(blob, off), reference(shape), (shape, dbg))
    core.close()


@functools.lru_cache(maxsize=None)
def batch_with_specials():
    """The documents of up to 3000 bytes with the two special tokens and near misses of them put in at char boundaries"""
    rng = np.random.default_rng(0x5BEC)
    docs = []
    units = [vs.SPECIAL_HI.encode(), vs.SPECIAL_LO.encode(), vs.SPECIAL_HI.encode()[:-1], b"<|shape_mid|>", b"<|", b"|>"]
    for doc in vs.shape_docs():
        if len(doc) > 3000:
            continue
        text = doc.decode()
        out, at = [], 0
        for _ in range(int(rng.integers(0, 4))):
            cut = int(rng.integers(at, len(text) + 1))
            out += [text[at:cut].encode(), units[int(rng.integers(0, len(units)))]]
            at = cut
        docs.append(b"".join(out) + text[at:].encode())
    return (docs, *h.pack(docs))


def first_hit(docs):
    for d, doc in enumerate(docs):
        hits = [(doc.find(s.encode()), s) for s in (vs.SPECIAL_HI, vs.SPECIAL_LO) if s.encode() in doc]
        if hits:
            return (d, *min(hits))


@shapes
def test_special_tokens(shape):
    from tiktoken_amd import DisallowedSpecialError

    core, C = core_of(shape), oracle_of(shape)
    assert_path(core, shape)
    docs, blob, off = batch_with_specials()
    want = C.encode_batch(blob, off, "all")
    ids = set(vs.vocab(*shape)[1].values())
    assert sum(int(t) in ids for t in want[0]) > 100
    same(core.encode_batch_packed(blob, off, "all"), want, shape)
    same(core.encode_batch_packed(blob, off, {vs.SPECIAL_LO}), C.encode_batch(blob, off, {vs.SPECIAL_LO}), (shape, "one allowed"))
    with pytest.raises(DisallowedSpecialError) as e:
        core.encode_batch_packed(blob, off, None, disallowed_special="all")
    assert (e.value.doc, e.value.pos, e.value.token) == first_hit(docs)


def test_a_pattern_of_the_generic_engine_with_wide_ids():
    """The first pat_str of tests/golden/generic_patterns.json.gz on untrained x wide: Python `regex` for the split, the oracle's
    byte_pair_encode for the tokens"""
    from test_regex_engine import _generic_golden

    shape = ("untrained", "wide")
    pat = _generic_golden()[0]["pat_str"]
    core, C = core_of(shape, pat), oracle_of(shape)
    assert_path(core, shape)
    docs, blob, off = batch()
    toks, toff, cache = [], [0], {}
    for doc in docs:
        for m in regex.finditer(pat, doc.decode()):
            p = m.group().encode()
            if p not in cache:
                cache[p] = C.encode_piece(p)
            toks += cache[p]
        toff.append(len(toks))
    same(core.encode_batch_packed(blob, off), (np.array(toks, np.uint32), np.array(toff, np.uint64)), pat)


class Table:
    """What decode_ref.decode_ref reads of a table: id -> bytes, the special tokens' decoder behind the ordinary one"""

    def __init__(self, ranks, specials):
        self.by_id = {v: k.encode() for k, v in specials.items()}
        self.by_id.update({r: t for t, r in ranks.items()})


DECODE_SHAPES = GPU_SHAPES + [("untrained", "dec_edge_lo")]


@pytest.mark.parametrize("shape", DECODE_SHAPES, ids="-".join)
def test_decode(shape):
    ranks, specials = vs.vocab(*shape)
    enc, core = encoding_of(shape), core_of(shape)
    want_fmt = assert_path(core, shape)
    table = Table(ranks, specials)
    _, sblob, soff = batch_with_specials()
    tokens, tok_off = oracle_of(shape).encode_batch(sblob, soff, "all")
    assert len(tokens) >= 10_000 and set(specials.values()) <= set(tokens.tolist())
    # decode_bytes gives the text back: beyond 8192 ids on the device where there is a table, and below
    assert core.decode_bytes(tokens.tolist()) == sblob.tobytes()
    assert core.decode_bytes(tokens[:8191].tolist()) == dr.decode_ref(table, tokens[:8191])[0]
    want, off, _ = dr.decode_ref(table, tokens)
    want_off = dr.doc_offsets_ref(off, tok_off)
    lists = [tokens[int(a):int(b)].tolist() for a, b in zip(tok_off[:-1], tok_off[1:])]
    texts = [want[int(a):int(b)].decode() for a, b in zip(want_off[:-1], want_off[1:])]
    # an id without bytes: in a hole of the map, beyond the last id where it has none
    ok, hole = ranks[b"a"], next((i for i in range(max(table.by_id) - 1, 0, -1) if i not in table.by_id), max(table.by_id) + 1)
    assert (hole < max(table.by_id)) == (shape[1] != "dense") and dr.decode_ref(table, [ok, hole])[2] == 1
    if want_fmt["decode_table_ids"]:
        assert shape[1] in ("dense", "wide_edge", "wide", "dec_edge_lo")
        data, byte_off = core.decode_batch_packed(tokens, tok_off)
        assert data == want and np.array_equal(byte_off, want_off)
        data, byte_off, _, byte_start, char_start, bad = core.decode_batch_spans_packed(tokens, tok_off)
        doc = np.repeat(np.arange(len(tok_off) - 1), np.diff(tok_off.astype(np.int64)))
        assert bad is None and data.tobytes() == want and np.array_equal(byte_off, want_off)
        assert np.array_equal(byte_start.astype(np.uint64), off[:-1] - want_off[doc])
        with pytest.raises(KeyError, match=f"Invalid token for decoding: {hole}\\b"):
            core.decode_batch_packed(np.array([ok, hole], np.uint32), np.array([0, 2], np.uint64))
        assert enc.decode_with_offsets_batch(lists[:40]) == [decode_with_offsets_ref(table, t) for t in lists[:40]]
    else:
        assert shape[1] in ("dec_edge_hi", "no_short", "top")
        import torch

        d_tok = torch.from_numpy(tokens.view(np.int32).copy()).cuda()
        d_off = torch.from_numpy(tok_off.view(np.int64).copy()).cuda()
        torch.cuda.synchronize()
        for call in (lambda: core.decode_batch_packed(tokens, tok_off), lambda: core.decode_batch_spans_packed(tokens, tok_off),
                     lambda: core.decode_batch_device(d_tok.data_ptr(), len(tokens), d_off.data_ptr(), len(tok_off) - 1),
                     lambda: core.token_spans_device(d_tok.data_ptr(), len(tokens), d_off.data_ptr(), len(tok_off) - 1)):
            with pytest.raises(ValueError, match="too sparse"):
                call()
    # Encoding: the reference's results either way (core.py falls back to the host where there is no table)
    assert enc.decode(tokens.tolist()) == sblob.tobytes().decode()
    assert enc.decode_batch(lists) == texts
    assert enc.decode_bytes_batch(lists[:50]) == [t.encode() for t in texts[:50]]
    for t in lists[:40]:
        assert enc.decode_with_offsets(t) == decode_with_offsets_ref(table, t)
    with pytest.raises(KeyError, match=f"{hole}"):
        enc.decode([ok, hole])
    with pytest.raises(KeyError, match=f"Invalid token for decoding: {hole}\\b"):
        core.decode_bytes([ok, hole] * 5000)


def decode_with_offsets_ref(table, tokens):
    """Encoding.decode_with_offsets of the reference (core.py:303-335) restated"""
    pieces = [table.by_id[t] for t in tokens]
    offsets, n = [], 0
    for p in pieces:
        offsets.append(max(0, n - (0x80 <= p[0] < 0xC0)))
        n += sum(1 for b in p if not 0x80 <= b < 0xC0)
    return b"".join(pieces).decode("utf-8", "strict"), offsets


def test_rows_padded_and_samples_with_wide_ids():
    """The three batch forms on untrained x wide with bos, eos and pad beyond 16 bits, bos and pad beyond 2^21: 32-bit results equal the rules restated in
    rows_ref, padded_ref and samples_ref; 16-bit ids are refused"""
    shape = ("untrained", "wide")
    core = core_of(shape)
    assert_path(core, shape)
    ranks, specials = vs.vocab(*shape)
    docs = [d for d in vs.shape_docs() if len(d) <= 700][:60]
    blob, off = h.pack(docs)
    tokens, tok_off = oracle_of(shape).encode_batch(blob, off)
    bos, eos, pad = specials[vs.SPECIAL_HI], specials[vs.SPECIAL_LO], max(ranks.values())
    assert min(bos, eos, pad) > 0xFFFF and min(bos, pad, int(tokens.max())) > vs.TK_PAIR8_MAX_ID
    got = core.encode_batch_rows_packed(blob, off, seq_len=67, bos=bos, eos=eos, pad=pad)
    want = rr.rows_rule(tokens, tok_off, 67, bos, eos, pad)
    assert got.ids.dtype == np.uint32 and got.ids.shape == (want.n_rows, 67) and got.n_stream == want.n_stream
    for name in ("ids", "doc", "pos"):
        assert np.array_equal(getattr(got, name).ravel(), getattr(want, name)), name
    assert np.array_equal(got.cu_seqlens, want.cu_seqlens) and np.array_equal(got.row_seg, want.row_seg)
    got = core.encode_batch_padded_packed(blob, off, max_length=50, stride=7, windows=True, padding_side="left", pad_to_multiple_of=8, bos=bos, eos=eos, pad=pad)
    pr.same(pr.Padded(*got), pr.padded_rule(tokens, tok_off, 50, stride=7, width_multiple=8, bos=bos, eos=eos, pad=pad, windows=True, left=True), "padded")
    from tiktoken_amd import Role

    roles = [sr.Role((bos, pad), (eos,), False), sr.Role((bos,), (eos, eos), True)]
    part_role = [i % 2 for i in range(len(docs))]
    sample_off = np.arange(0, len(docs) + 1, 3, dtype=np.uint64)
    assert int(sample_off[-1]) == len(docs)
    got = core.encode_batch_samples_packed(blob, off, part_role=part_role, sample_off=sample_off, roles=[Role(*r) for r in roles], max_length=120, keep="tail",
                                           pad_to_multiple_of=8, bos=bos, eos=eos, pad=pad)
    sr.same(sr.Samples(*got), sr.samples_rule(tokens, tok_off, part_role, sample_off, roles, 120, width_multiple=8, bos=bos, eos=eos, pad=pad, keep_tail=True), "samples")
    with pytest.raises(ValueError):
        core.encode_batch_rows_packed(blob, off, seq_len=67, bos=bos, eos=eos, pad=pad, dtype=np.uint16)
    with pytest.raises(ValueError):
        core.encode_batch_padded_packed(blob, off, max_length=50, bos=bos, eos=eos, pad=pad, dtype=np.uint16)
    with pytest.raises(ValueError):  # (no id of the call's own above 16 bits: the batch's tokens are)
        core.encode_batch_rows_packed(blob, off, seq_len=67, pad=0, dtype=np.uint16)


def test_ids_of_2_to_the_31_minus_1_are_refused():
    from tiktoken_amd import CoreBPE

    single = {bytes([b]): b for b in range(256)}
    with pytest.raises(ValueError, match="not supported"):
        CoreBPE({**single, b"ab": 0x7FFFFFFF}, {}, PAT)
    with pytest.raises(ValueError, match="not supported"):
        CoreBPE(single, {"<|s|>": 0x7FFFFFFF}, PAT)
    core = CoreBPE({**single, b"ab": 0x7FFFFFFE}, {"<|s|>": 0x7FFFFFFD}, PAT)
    assert core.encode("cab<|s|>ab", "all") == [ord("c"), 0x7FFFFFFE, 0x7FFFFFFD, 0x7FFFFFFE]
    assert core.decode_bytes([0x7FFFFFFE, 0x7FFFFFFD]) == b"ab<|s|>"


def test_a_four_byte_token_of_rank_0x3fffffff():
    """Regression: with a short table that rank and a length of 4 made the slot's value the empty mark, and the token was never found.
    The short table now ends one rank earlier (TK_SHORT_MAX_RANK)."""
    from tiktoken_amd import CoreBPE

    single = {bytes([b]): b for b in range(256)}
    for rank, short in ((0x3FFFFFFF, 0), (0x3FFFFFFE, 1)):
        ranks = {**single, b"abcd": rank, b"ab": 300}
        core, C = CoreBPE(ranks, {}, PAT), c_oracle.COracle(0, ranks, {})
        assert core.stat("short_table") == short
        text = b"abcd xabcd ab abcd"
        assert core.encode_ordinary(text.decode()) == C.encode_ordinary(text).tolist() and core.encode_ordinary("abcd") == [rank]
        blob, off = h.pack([b"abcd", b"abcd\n" * 4000, text * 500])
        toks, toff = core.encode_batch_packed(blob, off)
        assert toks[0] == rank and toks[1:8001].tolist() == [rank, 10] * 4000
        same((toks, toff), C.encode_batch(blob, off), rank)
