"""The decode kernels (tk_decode.h) on the device, at the shapes natural text never brings: one CoreBPE over decode_ref.edge_vocab() --
tokens of 2 .. 300 bytes, special tokens of 1 .. 40 bytes, ranks with holes -- and every comparison against tests/decode_ref.py (a join
over a Python table), never against another entry point of the library.  The CPU side of the same cases: tests/test_decode_sim.py."""
import ctypes

import numpy as np
import pytest

import decode_ref as dr
import helpers as h
import tiktoken_amd as tiktoken

pytestmark = pytest.mark.gpu
BLOCK = 2048


@pytest.fixture(scope="module")
def table():
    return dr.edge_table()


@pytest.fixture(scope="module")
def core():
    ranks, specials = dr.edge_vocab()
    return tiktoken.CoreBPE(ranks, specials, h.PAT_STR[1])


@pytest.fixture(scope="module")
def sweep(table):
    """(ids, tok_off, reference bytes, reference byte offsets) of the alignment sweep, its documents cut every 13 tokens -- inside the
    lanes of eight -- with empty documents first, last and in runs"""
    tokens = dr.alignment_sweep(table)
    cuts = list(range(0, len(tokens), 13)) + [len(tokens)]
    tok_off = np.array([0, 0] + cuts[1:40] + [cuts[40]] * 3 + cuts[41:] + [len(tokens)] * 2, np.uint64)
    want, off, bad = dr.decode_ref(table, tokens)
    assert bad is None and len(tokens) < 100_000
    return tokens, tok_off, want, off


def dev_bytes(ptr, n):
    import torch

    return bytes(torch.as_tensor(h._DevArray(ptr, n, "|u1"), device="cuda").cpu().numpy()) if n else b""


def on_device(core, tokens, tok_off=None, stream=0, shift=0):
    """decode_batch_device: (bytes, byte offsets or None).  shift: the ids start that many elements into their buffer."""
    import torch

    n = len(tokens)
    room = torch.zeros(n + shift + 4, dtype=torch.int32, device="cuda")
    if n:
        room[shift:shift + n] = torch.from_numpy(np.ascontiguousarray(tokens, np.uint32).view(np.int32)).cuda()
    d_tok = room[shift:]
    d_off = torch.from_numpy(np.ascontiguousarray(tok_off, np.uint64).view(np.int64)).cuda() if tok_off is not None else None
    torch.cuda.synchronize()
    db, nb, do = core.decode_batch_device(d_tok.data_ptr() if n else 0, n, d_off.data_ptr() if d_off is not None else 0, len(tok_off) - 1 if tok_off is not None else 0, stream)
    assert (do != 0) == (tok_off is not None)
    return dev_bytes(db, nb), (h.dev_u64(do, len(tok_off)) if tok_off is not None else None), d_tok


def check_three(core, tokens, tok_off, want, off, what=None):
    """The three batch entry points against the reference: bytes and the documents' byte offsets, byte_start for the spans"""
    tokens, tok_off = np.ascontiguousarray(tokens, np.uint32), np.ascontiguousarray(tok_off, np.uint64)
    want_off = dr.doc_offsets_ref(off, tok_off)
    data, byte_off = core.decode_batch_packed(tokens, tok_off)
    assert data == want and np.array_equal(byte_off, want_off), (what, "packed")
    data, byte_off, _, byte_start, _, bad = core.decode_batch_spans_packed(tokens, tok_off, validate=False)
    doc = np.repeat(np.arange(len(tok_off) - 1), np.diff(tok_off.astype(np.int64)))
    assert bad is None and data.tobytes() == want and np.array_equal(byte_off, want_off), (what, "spans")
    assert np.array_equal(byte_start.astype(np.uint64), off[:-1] - want_off[doc]), (what, "byte_start")
    data, byte_off, _ = on_device(core, tokens, tok_off)
    assert data == want and np.array_equal(byte_off, want_off), (what, "device")


def test_alignment_sweep_through_the_three_entry_points(core, sweep):
    check_three(core, *sweep)


def test_token_counts(core, table):
    rng = np.random.default_rng(12)
    for n in (0, 1, 7, 8, 9, 2047, 2048, 2049, 4096, 3 * BLOCK + 5):
        tokens = dr.random_batch(table, rng, n)
        want, off, _ = dr.decode_ref(table, tokens)
        check_three(core, tokens, [0, n], want, off, n)
        check_three(core, tokens, [0, 0, n // 2, n // 2, n, n], want, off, n)


def test_decode_bytes_on_both_sides_of_the_switch_to_the_device(core, table):
    tokens = dr.random_batch(table, np.random.default_rng(13), 8192, long_share=0.5, special_share=0.2)
    for n in (8191, 8192):
        assert core.decode_bytes(tokens[:n].tolist()) == dr.decode_ref(table, tokens[:n])[0], n


def test_device_resident_entry(core, table, sweep):
    tokens, _, want, off = sweep
    n = 20_011
    tok_off = np.array([0, 0, 0, 5, 5, 4000, 4000, 4000, 12345, n, n, n], np.uint64)  # empty documents first, last and in runs
    data, byte_off, _ = on_device(core, tokens[:n], tok_off)
    assert data == want[: int(off[n])] and np.array_equal(byte_off, dr.doc_offsets_ref(off, tok_off))
    data, byte_off, _ = on_device(core, tokens[:n])  # without offsets
    assert data == want[: int(off[n])] and byte_off is None
    # the id pointer 4 bytes off a 16-byte boundary: a view from element 1
    data, _, d_tok = on_device(core, tokens[:n], shift=1)
    assert d_tok.data_ptr() % 16 == 4 and data == want[: int(off[n])]
    # a stream of the caller's, created by the HIP runtime the library itself links (its symbols resolve through the library's handle)
    L = tiktoken._lib.lib()
    L.hipStreamCreate.argtypes, L.hipStreamDestroy.argtypes = [ctypes.POINTER(ctypes.c_void_p)], [ctypes.c_void_p]
    s = ctypes.c_void_p()
    assert L.hipStreamCreate(ctypes.byref(s)) == 0 and s.value
    try:
        data, byte_off, _ = on_device(core, tokens[:n], tok_off, stream=s.value)
        assert data == want[: int(off[n])] and np.array_equal(byte_off, dr.doc_offsets_ref(off, tok_off))
    finally:
        assert L.hipStreamDestroy(s) == 0


def test_a_small_batch_after_a_large_one(core, table, sweep):
    """The core's buffers are reused: lengths and workgroup sums of the 60 000 tokens before must not leak into the nine"""
    tokens, _, want, off = sweep
    n = 60_000
    check_three(core, tokens[:n], [0, n], want[: int(off[n])], off[: n + 1])
    small = np.array([table.id_of_len(300), 0x41, table.id_of_len(17, special=True), table.id_of_len(9), 0x42, table.id_of_len(1, special=True), 0x43,
                      table.id_of_len(64), table.id_of_len(40, special=True)], np.uint32)
    w, o, _ = dr.decode_ref(table, small)
    check_three(core, small, [0, 4, 9], w, o)


def raises_key_error(core, tokens, bad_id, entry):
    tokens = np.ascontiguousarray(tokens, np.uint32)
    with pytest.raises(KeyError, match=f"Invalid token for decoding: {bad_id}$|Invalid token for decoding: {bad_id}\\D"):
        if entry == "packed":
            core.decode_batch_packed(tokens, np.array([0, len(tokens)], np.uint64))
        elif entry == "spans":
            core.decode_batch_spans_packed(tokens, np.array([0, 3, len(tokens)], np.uint64), validate=False)
        elif entry == "device":
            on_device(core, tokens, np.array([0, len(tokens)], np.uint64))
        else:
            core.decode_bytes(tokens.tolist())


@pytest.mark.parametrize("entry", ("packed", "spans", "device", "decode_bytes"))
def test_ids_without_an_entry(core, table, sweep, entry):
    rng = np.random.default_rng(14)
    base = dr.random_batch(table, rng, 4 * BLOCK + 100)  # (at least 8192: decode_bytes takes the device path)
    hole = next(x for x in table.holes if x < 400)
    top = max(table.by_id)
    assert dr.decode_ref(table, [top])[2] is None and dr.decode_ref(table, [top + 1])[2] == 0
    for bad_id, pos in ((hole, 5), (table.holes[-1], BLOCK), (top + 1, 3 * BLOCK - 1), (0xFFFFFFFF, len(base) - 1), (0xFFFFFFFF, 0)):
        tokens = base.copy()
        tokens[pos] = bad_id
        assert dr.decode_ref(table, tokens)[2] == pos
        raises_key_error(core, tokens, bad_id, entry)
    # two bad ids in different workgroups, the larger id first: the error names the id at the first position
    tokens = base.copy()
    tokens[BLOCK + 7], tokens[3 * BLOCK + 9] = 0xFFFFFFFF, hole
    raises_key_error(core, tokens, 0xFFFFFFFF, entry)
    tokens[BLOCK + 7], tokens[3 * BLOCK + 9] = top + 1, top + 2
    raises_key_error(core, tokens, top + 1, entry)
    # after the errors the same core decodes the alignment batch exactly
    check_three(core, *sweep)


def test_a_refused_device_decode_leaves_no_launch_for_the_next_call_to_pay(core, table):
    """Profiling on: the event pair of tk_k_dec_len in a call that ends in KeyError goes with that call, not into the next one's count"""
    good = dr.random_batch(table, np.random.default_rng(16), 9)
    bad = good.copy()
    bad[4] = next(x for x in table.holes if x < 400)
    tok_off = np.array([0, 9], np.uint64)
    core.set_profiling(True)
    try:
        core.reset_kernel_ms()
        with pytest.raises(KeyError):
            on_device(core, bad, tok_off)
        core.reset_kernel_ms()
        data, _, _ = on_device(core, good, tok_off)
        assert data == dr.decode_ref(table, good)[0]
        assert core.kernel_ms("tk_k_dec_len")[1] == 1
        assert core.kernel_ms("tk_k_dec_copy")[1] == 1
    finally:
        core.set_profiling(False)


def test_ids_too_sparse_for_the_device_table():
    """A special token at id 2^26: there is no device table.  decode_batch_packed says so; Encoding's batch forms fall back to the host
    loop and equal the reference."""
    ranks = {bytes([b]): b for b in range(256)}
    ranks.update({b"ab": 256, b"hello world!": 257, b"0123456789abcdefg": 259})
    specials = {"<|big|>": 1 << 26}
    t = dr.Table(ranks, specials)
    enc = tiktoken.Encoding("sparse_ids", pat_str=h.PAT_STR[1], mergeable_ranks=ranks, special_tokens=specials)
    rng = np.random.default_rng(15)
    ids = np.array([0x61, 0x20, 256, 257, 259, 1 << 26], np.uint32)
    docs = [ids[rng.integers(0, len(ids), size=n)].tolist() for n in (0, 1, 9, 300, 0, 8200)]
    flat = np.array([x for d in docs for x in d], np.uint32)
    tok_off = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.uint64)
    with pytest.raises(ValueError, match="too sparse"):
        enc._core_bpe.decode_batch_packed(flat, tok_off)
    want = [dr.decode_ref(t, d)[0] for d in docs]
    assert enc.decode_bytes_batch(docs) == want
    assert enc.decode_batch(docs) == [w.decode() for w in want]
    assert enc.decode_bytes(docs[5]) == want[5] and len(docs[5]) >= 8192
    assert enc.decode_tokens_bytes(docs[3]) == [t.by_id[i] for i in docs[3]]
    text, offsets = enc.decode_with_offsets(docs[3])
    assert text == want[3].decode() and offsets == dr.decode_ref(t, docs[3])[1][:-1].tolist()  # (ASCII: chars are bytes)
    for bad in ([0x61, 258], [1 << 25], [0x61] * 8192 + [(1 << 26) + 1]):
        with pytest.raises(KeyError):
            enc.decode_bytes(bad)
    with pytest.raises(KeyError):
        enc.decode_bytes_batch([[0x61], [258]])
    with pytest.raises(KeyError):
        enc.decode_tokens_bytes([258])


def test_a_special_token_whose_id_is_a_rank():
    """The constructor accepts such a vocabulary, as the reference does; lib.rs:347-351 asks the ordinary decoder first: the ordinary
    token's bytes win, on the host path and on the device"""
    ranks = {bytes([b]): b for b in range(256)}
    ranks.update({b"ab": 256, b"abcdefghijk": 257})
    core = tiktoken.CoreBPE(ranks, {"<|dup|>": 257, "<|end|>": 258}, h.PAT_STR[1])
    t = dr.Table(ranks, {"<|dup|>": 257, "<|end|>": 258})
    assert t.by_id[257] == b"abcdefghijk"
    tokens = np.array([257, 258, 0x41, 257, 256, 258, 257, 257, 257, 258], np.uint32)
    want, off, _ = dr.decode_ref(t, tokens)
    assert core.decode_bytes(tokens.tolist()) == want  # the host loop
    check_three(core, tokens, [0, 4, 10], want, off)
    long = np.tile(tokens, 900)  # (at least 8192 ids: decode_bytes on the device)
    assert core.decode_bytes(long.tolist()) == want * 900
