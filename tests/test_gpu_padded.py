"""Padded model inputs on the GPU (tk_padded.h): tk_pad_batch_device and tk_encode_batch_padded through CoreBPE and Encoding, against the
numpy restatement of the rule in tests/padded_ref.py (written from the rule's description in include/tiktoken_amd.h, not from the kernels)."""
import numpy as np
import pytest

import helpers as h
import padded_ref as pr
import tiktoken_amd as tiktoken

pytestmark = pytest.mark.gpu
BLOCK = 2048  # TK_DEC_BLOCK: positions per workgroup


def to_device(tokens, tok_off):
    import torch

    d_tok = torch.from_numpy(np.ascontiguousarray(tokens, np.uint32).view(np.int32).copy()).cuda() if len(tokens) else torch.zeros(4, dtype=torch.int32, device="cuda")
    d_off = torch.from_numpy(np.ascontiguousarray(tok_off, np.uint64).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return d_tok, d_off


def dev(ptr: int, n: int, typestr: str, dtype) -> np.ndarray:
    import torch

    if not n:
        return np.zeros(0, dtype)
    return torch.as_tensor(h._DevArray(ptr, n, typestr), device="cuda").cpu().numpy().view(dtype)


def shim_args(kw):
    """padded_ref's keywords as pad_batch_device's"""
    return dict(stride=kw.get("stride", 0), windows=kw.get("windows", False), keep="tail" if kw.get("keep_tail") else "head",
                padding_side="left" if kw.get("left") else "right", pad_to_multiple_of=kw.get("width_multiple") or None)


def pad_device(core, tokens, tok_off, max_len, bos=None, eos=None, pad=0, dtype=np.uint32, held=None, **kw):
    """pad_batch_device on arrays copied to the device, read back as a padded_ref.Padded"""
    d_tok, d_off = held if held is not None else to_device(tokens, tok_off)
    n_docs = len(tok_off) - 1
    r = core.pad_batch_device(d_tok.data_ptr(), len(tokens), d_off.data_ptr(), n_docs, max_length=max_len, bos=bos, eos=eos, pad=pad, dtype=dtype, **shim_args(kw))
    R, W = r.n_rows, r.width
    ids = dev(r.input_ids, R * W, "<i2", np.uint16) if np.dtype(dtype) == np.uint16 else h.dev_u32(r.input_ids, R * W)
    return pr.Padded(ids.reshape(R, W), dev(r.attention_mask, R * W, "|u1", np.uint8).reshape(R, W), h.dev_u32(r.lengths, R), h.dev_u32(r.row_doc, R),
                     h.dev_u32(r.row_tok, R), h.dev_u32(r.doc_row, n_docs + 1))


def core_of(name="gpt2_shaped"):
    return tiktoken.get_encoding(name)._core_bpe


def check(core, docs, max_lens, specials=pr.SPECIALS, pad=7, settings=None, ctx=""):
    tokens, tok_off = pr.pack_docs(docs)
    held = to_device(tokens, tok_off)
    for bos, eos in specials:
        k = (bos is not None) + (eos is not None)
        for max_len in max_lens:
            for kw in (settings if settings is not None else pr.settings(max_len, k)):
                want = pr.padded_rule(tokens, tok_off, max_len, bos=bos, eos=eos, pad=pad, **kw)
                pr.same(pad_device(core, tokens, tok_off, max_len, bos, eos, pad, held=held, **kw), want, (ctx, max_len, bos, eos, kw))


# ---------------------------------------------------------------- the device entry against the restatement
MODES = (dict(), dict(left=True, keep_tail=True), dict(windows=True, stride=1, left=True), dict(windows=True, width_multiple=8), dict(keep_tail=True, width_multiple=64),
         dict(left=True, width_multiple=1))  # head / tail / windows, padding behind and in front


@pytest.mark.parametrize("bos,eos", pr.SPECIALS)
def test_device_entry_case_list(bos, eos):
    """Empty batch, only empty documents (W == 0 among them), runs of 40 and 70 empty documents, one document of 5 * 2048 + 11 tokens in
    windows, row boundaries at 2047 / 2048 / 2049 positions -- every max_len of a case crossed with the padding side, head / tail / windows,
    stride in {0, 1, c - 1} and width_multiple in {0, 1, 8, 64} (padded_ref.settings)."""
    core = core_of()
    rng = np.random.default_rng(BLOCK)
    k = (bos is not None) + (eos is not None)
    for name, docs, max_lens in pr.cases(BLOCK, rng):
        for max_len in max_lens:
            check(core, docs, [max_len], specials=[(bos, eos)], settings=pr.settings(max_len, k, max(map(len, docs), default=0)), ctx=name)


@pytest.mark.parametrize("bos,eos", pr.SPECIALS)
def test_documents_around_the_capacity(bos, eos):
    """n_d in {c - 1, c, c + 1, c + step - 1, c + step, c + step + 1}, stride in {0, 1, c - 1}, max_len in {1 + k, 7, 8, 9, 64, 2048, 2049}"""
    core = core_of()
    rng = np.random.default_rng(7)
    k = (bos is not None) + (eos is not None)
    for max_len in (1 + k, 7, 8, 9, 64, 2048, 2049):
        c = max_len - k
        for stride in sorted({0, 1, c - 1}):
            if stride >= c:
                continue
            docs = pr.around_capacity(max_len, k, stride, rng)
            sets = [dict(left=left, width_multiple=wm, windows=True, stride=stride) for left in (False, True) for wm in (0, 8)]
            if stride == 0:
                sets += [dict(left=left, keep_tail=kt, width_multiple=wm) for left in (False, True) for kt in (False, True) for wm in (0, 1, 64)]
            check(core, docs, [max_len], specials=[(bos, eos)], settings=sets)


def test_only_empty_documents_and_width_zero():
    core = core_of()
    tokens, tok_off = pr.pack_docs([[]] * 5)
    got = pad_device(core, tokens, tok_off, 9, width_multiple=1)
    assert got.ids.shape == (5, 0) and got.mask.shape == (5, 0)
    assert got.len.tolist() == [0] * 5 and got.row_doc.tolist() == [0, 1, 2, 3, 4] and got.row_tok.tolist() == [0] * 5 and got.doc_row.tolist() == [0, 1, 2, 3, 4, 5]
    check(core, [[]] * 5, [1, 9])
    got = pad_device(core, tokens, tok_off, 9, bos=1, eos=2, pad=3, width_multiple=8, left=True)
    assert got.ids.tolist() == [[3] * 6 + [1, 2]] * 5 and got.len.tolist() == [2] * 5
    got = pad_device(core, *pr.pack_docs([]), 9, eos=2, width_multiple=8)  # the empty batch: no row, longest 0
    assert got.ids.shape == (0, 0) and got.doc_row.tolist() == [0]
    assert pad_device(core, *pr.pack_docs([]), 9, eos=2).ids.shape == (0, 9)


@pytest.mark.parametrize("bos,eos", pr.SPECIALS)
def test_width_multiple_with_the_longest_row_below_at_and_above_max_len(bos, eos):
    core = core_of()
    rng = np.random.default_rng(5)
    for longest in (5, 15, 16, 17, 24, 40):  # max_len 16: below, just below, at, above
        docs = [rng.integers(0, 50000, size=n).tolist() for n in (3, 0, longest, 1)]
        sets = [dict(width_multiple=wm, left=left, **m) for wm in (0, 1, 8, 64) for left in (False, True) for m in (dict(), dict(keep_tail=True), dict(windows=True, stride=3))]
        check(core, docs, [16], specials=[(bos, eos)], settings=sets)


@pytest.mark.parametrize("bos,eos", pr.SPECIALS)
def test_token_pointer_that_is_not_16_byte_aligned(bos, eos):
    """A lane loads eight body tokens as two 16-byte words where their address allows it: shifting the array moves the lanes that can, and
    so does a bos, which moves every body index by one."""
    import torch

    core = core_of()
    rng = np.random.default_rng(5)
    tokens, tok_off = pr.pack_docs([rng.integers(0, 50000, size=n).tolist() for n in (700, 0, 1500, 9)])
    buf = torch.zeros(len(tokens) + 8, dtype=torch.int32, device="cuda")
    d_off = torch.from_numpy(tok_off.view(np.int64).copy()).cuda()
    wants = {(max_len, i): pr.padded_rule(tokens, tok_off, max_len, bos=bos, eos=eos, pad=7, **kw) for max_len in (64, 67) for i, kw in enumerate(MODES)}
    for shift in (0, 1, 2, 3):
        buf[shift: shift + len(tokens)] = torch.from_numpy(tokens.view(np.int32).copy()).cuda()
        torch.cuda.synchronize()
        for (max_len, i), want in wants.items():
            pr.same(pad_device(core, tokens, tok_off, max_len, bos, eos, 7, held=(buf[shift:], d_off), **MODES[i]), want, (shift, max_len, MODES[i]))


@pytest.fixture(scope="module")
def short_documents():
    """300 000 documents of one and two tokens, on the host and on the device"""
    rng = np.random.default_rng(300000)
    n_docs = 300_000
    sizes = rng.integers(1, 3, size=n_docs)
    tok_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    tokens = rng.integers(0, 50000, size=int(tok_off[-1])).astype(np.uint32)
    return tokens, tok_off, to_device(tokens, tok_off)


@pytest.mark.parametrize("bos,eos", pr.SPECIALS)
def test_300000_short_documents(short_documents, bos, eos):
    """More than 1024 workgroups in the write pass (300 000 rows of 8 = 1172 of them) and more than 1024 * 256 documents in the count
    pass and in the scan, whose loop takes 1024 counts at a time: one- and two-token documents with max_len 8 -- and with max_len 1 + k in
    windows, a row per token, where a lane's eight positions span several rows and documents."""
    core = core_of()
    tokens, tok_off, held = short_documents
    n_docs = len(tok_off) - 1
    assert n_docs > 1024 * 256 and n_docs * 8 > 1024 * BLOCK
    k = (bos is not None) + (eos is not None)
    for max_len, kw in ((8, dict()), (8, dict(left=True, keep_tail=True)), (8, dict(windows=True, stride=1, left=True, width_multiple=8)), (1 + k, dict(windows=True))):
        got = pad_device(core, tokens, tok_off, max_len, bos, eos, 50255, held=held, **kw)
        pr.same(got, pr.padded_rule(tokens, tok_off, max_len, bos=bos, eos=eos, pad=50255, **kw), (max_len, kw))
    assert got.ids.shape == (len(tokens), 1 + k) and np.array_equal(got.doc_row, tok_off.astype(np.uint32))


@pytest.mark.parametrize("bos,eos", pr.SPECIALS)
def test_ids_16_bit(bos, eos):
    enc = tiktoken.get_encoding("gpt2_shaped")
    core = enc._core_bpe
    assert enc.max_token_value < 65536
    rng = np.random.default_rng(16)
    docs = [rng.integers(0, 50000, size=n).tolist() for n in (100, 0, 31, 700, 1, 64, 63)]
    tokens, tok_off = pr.pack_docs(docs)
    held = to_device(tokens, tok_off)
    for max_len in (7, 64, 65):
        for kw in MODES:
            got = pad_device(core, tokens, tok_off, max_len, bos, eos, 9, dtype=np.uint16, held=held, **kw)
            assert got.ids.dtype == np.uint16
            pr.same(got._replace(ids=got.ids.astype(np.uint32)), pr.padded_rule(tokens, tok_off, max_len, bos=bos, eos=eos, pad=9, **kw), (max_len, kw))


def test_ids_16_bit_refusals():
    enc = tiktoken.get_encoding("gpt2_shaped")
    core = enc._core_bpe
    tokens, tok_off = pr.pack_docs([[1, 2, 3], [4]])
    held = to_device(tokens, tok_off)
    for bad in (dict(bos=65536, pad=0), dict(eos=70000, pad=0), dict(eos=50256, pad=1 << 20)):
        with pytest.raises(ValueError, match="16-bit"):
            core.pad_batch_device(held[0].data_ptr(), len(tokens), held[1].data_ptr(), 2, max_length=16, dtype=np.uint16, **bad)
    with pytest.raises(ValueError, match="16-bit"):
        tiktoken.get_encoding("o200k_shaped").encode_ordinary_batch_padded(["a b"], 16, eos=1, dtype=np.uint16)
    narrow = enc.encode_ordinary_batch_padded(["a b c d", "", "e"], 4, eos=enc.eot_token, dtype=np.uint16)
    wide = enc.encode_ordinary_batch_padded(["a b c d", "", "e"], 4, eos=enc.eot_token)
    assert narrow.input_ids.dtype == np.uint16 and np.array_equal(narrow.input_ids, wide.input_ids.astype(np.uint16))
    assert narrow.attention_mask.flags.writeable and wide.attention_mask.flags.writeable and wide.input_ids.flags.writeable


# ---------------------------------------------------------------- invariants on a random batch
def test_invariants_on_a_random_batch():
    core = core_of("cl100k_shaped")
    rng = np.random.default_rng(0x20000)
    sizes = [0 if rng.random() < 0.15 else int(rng.integers(1, 400)) for _ in range(300)]
    docs = [rng.integers(0, 100000, size=n).tolist() for n in sizes]
    tokens, tok_off = pr.pack_docs(docs)
    held = to_device(tokens, tok_off)
    BOS, EOS, PAD, L, STRIDE = 100258, 100257, 100276, 128, 16
    for bos, eos in ((None, EOS), (BOS, EOS), (None, None)):
        for left in (False, True):
            got = pad_device(core, tokens, tok_off, L, bos, eos, PAD, held=held, windows=True, stride=STRIDE, left=left, width_multiple=8)
            k = (bos is not None) + (eos is not None)
            R, W = got.ids.shape
            assert np.array_equal(got.mask.sum(1), got.len) and np.all(np.diff(got.doc_row.astype(np.int64)) > 0) and got.doc_row[-1] == R
            assert np.all(got.ids[got.mask == 0] == PAD)
            for r in range(R):
                d, t, n = int(got.row_doc[r]), int(got.row_tok[r]), int(got.len[r])
                elems = got.ids[r, W - n:] if left else got.ids[r, :n]
                want = ([bos] if bos is not None else []) + docs[d][t:t + n - k] + ([eos] if eos is not None else [])
                assert elems.tolist() == want, (r, d, t)
                if r and got.row_doc[r - 1] == d:  # consecutive windows of a document overlap in exactly `stride` tokens
                    assert int(got.row_tok[r - 1]) + int(got.len[r - 1]) - k - t == STRIDE
            ends = got.row_tok.astype(np.int64) + got.len - k  # the last window of every document reaches its end
            assert np.array_equal(ends[got.doc_row[1:].astype(np.int64) - 1], np.diff(tok_off.astype(np.int64)))
            pr.same(got, pr.padded_rule(tokens, tok_off, L, bos=bos, eos=eos, pad=PAD, windows=True, stride=STRIDE, left=left, width_multiple=8), (bos, eos, left))


# ---------------------------------------------------------------- end to end
@pytest.mark.parametrize("name", h.ENCODING_NAMES)
def test_end_to_end_against_the_oracle(name):
    enc = tiktoken.get_encoding(name)
    C = h.c_oracle_for(name)
    eot = enc.eot_token
    texts = [d.decode() for d in h.fuzz_batch(0xE2E + len(name), 48 << 10)] + ["", "tail"]
    with_specials = [t + s for t, s in zip(texts, ["<|endoftext|>", "", " <|endoftext|> x"] * len(texts))]
    blob, off = enc._pack(with_specials)
    tokens, tok_off = C.encode_batch(blob, off, "all", 8)
    assert eot in tokens and len(tokens) > 4000
    for max_len, kw in ((64, dict(eos=eot)), (128, dict(bos=eot, eos=eot, pad=0, windows=True, stride=16)), (50, dict(pad=5, keep_tail=True, left=True, width_multiple=8)),
                        (len(tokens) + 3, dict(pad=5, width_multiple=64))):
        got = enc.encode_batch_padded(with_specials, max_len, allowed_special="all", **{**shim_args(kw), **{x: kw[x] for x in ("bos", "eos", "pad") if x in kw}})
        want = pr.padded_rule(tokens, tok_off, max_len, **{"pad": kw.get("eos", 0), **kw})
        pr.same(pr.Padded(*got), want, (max_len, kw))
    tokens, tok_off = C.encode_batch(*enc._pack(texts), None, 8)
    got = enc.encode_ordinary_batch_padded(texts, 96, eos=eot, windows=True, stride=8, pad_to_multiple_of=8)
    pr.same(pr.Padded(*got), pr.padded_rule(tokens, tok_off, 96, eos=eot, pad=eot, windows=True, stride=8, width_multiple=8), "ordinary")
    # a disallowed special token: the error of encode_batch_packed, and nothing returned
    with pytest.raises(ValueError) as want_err:
        enc.encode_batch_packed(with_specials)
    with pytest.raises(ValueError) as got_err:
        enc.encode_batch_padded(with_specials, 64, eos=eot)
    assert str(got_err.value) == str(want_err.value)
    with pytest.raises(tiktoken.DisallowedSpecialError) as want_hit:
        enc._core_bpe.encode_batch_packed(blob, off, None, disallowed_special="all")
    with pytest.raises(tiktoken.DisallowedSpecialError) as got_hit:
        enc._core_bpe.encode_batch_padded_packed(blob, off, None, disallowed_special="all", max_length=64, eos=eot)
    assert (got_hit.value.doc, got_hit.value.pos, got_hit.value.token) == (want_hit.value.doc, want_hit.value.pos, want_hit.value.token)
    # padding that nothing was named for -- and none needed
    with pytest.raises(ValueError, match="pad"):
        enc.encode_ordinary_batch_padded(texts, 64)
    assert enc.encode_ordinary_batch_padded(["a b c d e f g h i j k"], 4).input_ids.shape == (1, 4)
    assert enc.encode_ordinary_batch_padded([], 8).input_ids.shape == (0, 8)


# ---------------------------------------------------------------- buffer lifetimes
def test_padding_leaves_the_encode_result_intact():
    import torch

    enc = tiktoken.get_encoding("o200k_shaped")
    core = enc._core_bpe
    texts = [d.decode() for d in h.fuzz_batch(0xB0F, 48 << 10)]
    blob, off = enc._pack(texts)
    tokens, tok_off = enc.encode_ordinary_batch_packed(texts)
    d_text = torch.zeros(len(blob) + 256, dtype=torch.uint8, device="cuda")
    d_text[: len(blob)] = torch.from_numpy(blob.copy()).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    dt, nt, dof = core.encode_batch_device(d_text.data_ptr(), len(blob), d_off.data_ptr(), off, len(texts))
    assert nt == len(tokens)
    for kw in (dict(eos=enc.eot_token), dict(pad=3, windows=True, stride=7, left=True), dict(bos=1, eos=2, pad=3, width_multiple=64)):
        r = core.pad_batch_device(dt, nt, dof, len(texts), max_length=256, **{**shim_args(kw), **{x: kw[x] for x in ("bos", "eos", "pad") if x in kw}})
        assert np.array_equal(h.dev_u32(dt, nt), tokens) and np.array_equal(h.dev_u64(dof, len(tok_off)), tok_off)
        R, W = r.n_rows, r.width
        got = pr.Padded(h.dev_u32(r.input_ids, R * W).reshape(R, W), dev(r.attention_mask, R * W, "|u1", np.uint8).reshape(R, W), h.dev_u32(r.lengths, R),
                        h.dev_u32(r.row_doc, R), h.dev_u32(r.row_tok, R), h.dev_u32(r.doc_row, len(texts) + 1))
        pr.same(got, pr.padded_rule(tokens, tok_off, 256, **{"pad": kw.get("eos", 0), **kw}), kw)


# ---------------------------------------------------------------- refusals
def test_bad_tok_off_is_refused_by_the_device_check():
    """Refusals, not faults: the count pass checks every entry and indexes nothing with it, and it counts in a scratch array: nothing is
    written into the buffers of the previous result."""
    core = core_of()
    rng = np.random.default_rng(9)
    docs = [rng.integers(0, 50000, size=n).tolist() for n in (30, 0, 2100, 12, 5)]
    tokens, tok_off = pr.pack_docs(docs)
    d_tok, d_good = to_device(tokens, tok_off)
    n = len(tokens)
    good = core.pad_batch_device(d_tok.data_ptr(), n, d_good.data_ptr(), len(docs), max_length=64, eos=1)
    def result():
        return (h.dev_u32(good.input_ids, good.n_rows * 64), dev(good.attention_mask, good.n_rows * 64, "|u1", np.uint8), h.dev_u32(good.lengths, good.n_rows),
                h.dev_u32(good.row_doc, good.n_rows), h.dev_u32(good.row_tok, good.n_rows), h.dev_u32(good.doc_row, len(docs) + 1))

    before = result()
    for bad, doc in (([0, 30, 30, 2130, 2100, n], 3), ([0, 30, 30, 2130, 2142, n - 1], 4), ([0, 30, 30, 2130, 2142, n + 1], 4), ([1, 30, 30, 2130, 2142, n], 0),
                     ([0, 40, 30, 2130, 2142, n], 1), ([0, 30, 1 << 40, 2130, 2142, n], 2)):
        _, d_bad = to_device(tokens, np.array(bad, np.uint64))
        for kw in (dict(eos=1), dict(pad=0, windows=True, stride=3), dict(pad=0, keep="tail", padding_side="left", pad_to_multiple_of=8)):
            with pytest.raises(ValueError, match=f"document {doc}\\b"):
                core.pad_batch_device(d_tok.data_ptr(), n, d_bad.data_ptr(), len(docs), max_length=64, **kw)
        assert all(np.array_equal(a, b) for a, b in zip(before, result()))  # the previous result, doc_row included, is whole
    pr.same(pad_device(core, tokens, tok_off, 64, eos=1, pad=1, held=(d_tok, d_good)), pr.padded_rule(tokens, tok_off, 64, eos=1, pad=1), "after a refusal")


def test_remaining_refusals():
    enc = tiktoken.get_encoding("gpt2_shaped")
    core = enc._core_bpe
    tokens, tok_off = pr.pack_docs([[1, 2, 3], [4]])
    d_tok, d_off = to_device(tokens, tok_off)
    args = (d_tok.data_ptr(), 4, d_off.data_ptr(), 2)
    for kw, what in ((dict(max_length=0, pad=0), "max_len"), (dict(max_length=1, eos=5), "max_len"), (dict(max_length=2, bos=4, eos=5), "max_len"),
                     (dict(max_length=4, pad=0, windows=True, stride=4), "stride"), (dict(max_length=4, eos=1, windows=True, stride=3), "stride"),
                     (dict(max_length=4, pad=0, stride=1), "stride"), (dict(max_length=4, pad=0, windows=True, keep="tail"), "KEEP_TAIL")):
        with pytest.raises(ValueError, match=what):
            core.pad_batch_device(*args, **kw)
    with pytest.raises(ValueError, match="max_len"):
        enc.encode_ordinary_batch_padded(["a b c"], 1, eos=5)
    with pytest.raises(ValueError, match="stride"):  # (before anything is encoded)
        enc.encode_batch_padded(["a <|endoftext|>"], 4, eos=5, stride=2)
    with pytest.raises(ValueError, match="32-bit"):  # (refused from the figures alone: nothing is read)
        core.pad_batch_device(d_tok.data_ptr(), 1 << 32, d_off.data_ptr(), 2, max_length=4, eos=1)
    with pytest.raises(ValueError, match="32-bit"):
        core.pad_batch_device(d_tok.data_ptr(), 4, d_off.data_ptr(), (1 << 32) - 1, max_length=4, eos=1)
    with pytest.raises(ValueError, match="32-bit"):  # R * W: two rows of 2^31, found after the count; nothing that large is allocated
        core.pad_batch_device(*args, max_length=1 << 31, pad=0)
    with pytest.raises(ValueError, match="pad"):
        core.pad_batch_device(*args, max_length=3)
    for kw in (dict(dtype=np.int64), dict(keep="middle"), dict(padding_side="up"), dict(pad_to_multiple_of=0)):
        with pytest.raises(ValueError):
            enc.encode_ordinary_batch_padded(["a"], 4, eos=1, **kw)
    pr.same(pad_device(core, tokens, tok_off, 3, eos=9, pad=9, held=(d_tok, d_off)), pr.padded_rule(tokens, tok_off, 3, eos=9, pad=9), "after the refusals")
    several = tiktoken.CoreBPE(enc._mergeable_ranks, enc._special_tokens, enc._pat_str, devices=[0, 0])
    with pytest.raises(ValueError, match="one device"):
        several.pad_batch_device(*args, max_length=2, pad=0)
    with pytest.raises(ValueError, match="one device"):
        several.encode_batch_padded_packed(np.frombuffer(b"ab", np.uint8), np.array([0, 2], np.uint64), max_length=2)


# ---------------------------------------------------------------- the id store the row passes and the padded passes share
@pytest.mark.parametrize("dtype", [np.uint32, np.uint16])
def test_last_lane_stores_three_ids_and_nothing_behind_them(dtype):
    """2048 + 3 positions through both write passes: two workgroups, whose last lane writes three elements one by one where every other
    lane writes eight at once.  The library's arrays hold a multiple of 8 elements each, so the five behind the result exist: they are
    painted between two calls of the same shape and must come through the second one untouched."""
    import torch

    import rows_ref as rr

    core = core_of()
    rng = np.random.default_rng(2051)
    n, n8 = BLOCK + 3, BLOCK + 8
    ids_t, ids_np, paint = ("<i2", np.uint16, 0x5A5A) if np.dtype(dtype) == np.uint16 else ("<i4", np.uint32, 0x5A5A5A5A)

    def behind(ptr, typestr, size, value=None):
        """the five elements behind the n of an array of the library: painted, or read"""
        t = torch.as_tensor(h._DevArray(ptr + n * size, n8 - n, typestr), device="cuda")
        if value is not None:
            t.fill_(value)
            torch.cuda.synchronize()
        return t.cpu().numpy()

    # rows: no bos / eos and drop_last, so the positions written are the tokens
    tokens, tok_off = rr.pack_docs([rng.integers(0, 50000, size=k).tolist() for k in (700, 0, 1340, 11)])
    assert len(tokens) == n
    d_tok, d_off = to_device(tokens, tok_off)
    want = rr.rows_rule(tokens, tok_off, 64, None, None, 7, True)
    seen = None
    for call in range(2):
        r = core.pack_rows_device(d_tok.data_ptr(), n, d_off.data_ptr(), len(tok_off) - 1, seq_len=64, pad=7, drop_last=True, dtype=dtype)
        arrays = ((r.ids, ids_t, np.dtype(ids_np).itemsize, paint), (r.doc, "<i4", 4, 0x5A5A5A5A), (r.pos, "<i4", 4, 0x5A5A5A5A))
        assert r.n_rows * 64 + r.n_tail == n and seen in (None, (r.ids, r.doc, r.pos))
        seen = (r.ids, r.doc, r.pos)
        for ptr, typestr, size, value in arrays:
            if call == 0:
                behind(ptr, typestr, size, value)
            else:
                assert (behind(ptr, typestr, size).astype(np.int64) & (256 ** size - 1) == value).all(), (typestr, ptr == r.ids)
        assert np.array_equal(dev(r.ids, n, ids_t, ids_np), want.ids) and np.array_equal(h.dev_u32(r.doc, n), want.doc) and np.array_equal(h.dev_u32(r.pos, n), want.pos)
        assert np.array_equal(h.dev_u32(r.cu_seqlens, r.n_segs + 1), want.cu_seqlens) and np.array_equal(h.dev_u32(r.row_seg, r.n_rows + 1), want.row_seg)

    # padded: 7 rows of 293
    tokens, tok_off = pr.pack_docs([rng.integers(0, 50000, size=k).tolist() for k in (293, 10, 300, 0, 1000, 294, 292)])
    d_tok, d_off = to_device(tokens, tok_off)
    want = pr.padded_rule(tokens, tok_off, 293, bos=None, eos=None, pad=7)
    seen = None
    for call in range(2):
        r = core.pad_batch_device(d_tok.data_ptr(), len(tokens), d_off.data_ptr(), 7, max_length=293, pad=7, dtype=dtype)
        assert r.n_rows * r.width == n and seen in (None, (r.input_ids, r.attention_mask))
        seen = (r.input_ids, r.attention_mask)
        for ptr, typestr, size, value in ((r.input_ids, ids_t, np.dtype(ids_np).itemsize, paint), (r.attention_mask, "|u1", 1, 0x5A)):
            if call == 0:
                behind(ptr, typestr, size, value)
            else:
                assert (behind(ptr, typestr, size).astype(np.int64) & (256 ** size - 1) == value).all(), (typestr, ptr == r.input_ids)
        pr.same(pad_device(core, tokens, tok_off, 293, None, None, 7, dtype=dtype, held=(d_tok, d_off)), want, ("store", np.dtype(dtype).name))
        assert (r.n_rows, r.width) == (7, 293)
