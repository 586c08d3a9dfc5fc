"""Training rows on the GPU (tk_rows.h): tk_pack_rows_device and tk_encode_batch_rows through CoreBPE and Encoding, against the numpy
restatement of the rule in tests/rows_ref.py (written from the rule's description in include/tiktoken_amd.h, not from the kernels)."""
import numpy as np
import pytest

import helpers as h
import rows_ref as rr
import tiktoken_amd as tiktoken

pytestmark = pytest.mark.gpu
BLOCK = 2048  # TK_DEC_BLOCK: positions per workgroup


def to_device(tokens, tok_off):
    import torch

    d_tok = torch.from_numpy(np.ascontiguousarray(tokens, np.uint32).view(np.int32).copy()).cuda() if len(tokens) else torch.zeros(4, dtype=torch.int32, device="cuda")
    d_off = torch.from_numpy(np.ascontiguousarray(tok_off, np.uint64).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return d_tok, d_off


def dev_u16(ptr: int, n: int) -> np.ndarray:
    import torch

    if not n:
        return np.zeros(0, np.uint16)
    return torch.as_tensor(h._DevArray(ptr, n, "<i2"), device="cuda").cpu().numpy().view(np.uint16)


def pack_device(core, tokens, tok_off, L, bos=None, eos=None, pad=None, drop_last=False, dtype=np.uint32, held=None):
    """pack_rows_device on arrays copied to the device, read back as a rows_ref.Rows"""
    d_tok, d_off = held if held is not None else to_device(tokens, tok_off)
    r = core.pack_rows_device(d_tok.data_ptr(), len(tokens), d_off.data_ptr(), len(tok_off) - 1, seq_len=L, bos=bos, eos=eos, pad=pad, drop_last=drop_last, dtype=dtype)
    m = r.n_rows * L + r.n_tail
    ids = dev_u16(r.ids, m) if np.dtype(dtype) == np.uint16 else h.dev_u32(r.ids, m)
    return rr.Rows(ids, h.dev_u32(r.doc, m), h.dev_u32(r.pos, m), h.dev_u32(r.cu_seqlens, r.n_segs + 1), h.dev_u32(r.row_seg, r.n_rows + 1), r.n_rows, r.n_segs,
                   r.n_stream, r.n_tail)


def same(got: rr.Rows, want: rr.Rows, ctx):
    assert (got.n_rows, got.n_segs, got.n_stream, got.n_tail) == (want.n_rows, want.n_segs, want.n_stream, want.n_tail), ctx
    for name in ("ids", "doc", "pos", "cu_seqlens", "row_seg"):
        g, w = getattr(got, name), getattr(want, name)
        assert g.shape == w.shape and np.array_equal(g, w), (name, ctx, np.flatnonzero(g != w)[:5] if g.shape == w.shape else (g.shape, w.shape))


def core_of(name="gpt2_shaped"):
    return tiktoken.get_encoding(name)._core_bpe


# ---------------------------------------------------------------- the device entry against the restatement
def batch_of_three_workgroups(rng):
    """About 5 000 tokens: document boundaries at token 2047, 2048 and 2049, a document across the second boundary of workgroups, a partial
    last workgroup; empty documents inside and at the end."""
    sizes = [2047, 1, 1, 0, 0, 300, 1800, 7, 0, 850, 1, 0, 0]
    assert np.cumsum(sizes).tolist()[:3] == [2047, 2048, 2049] and 2 * BLOCK < sum(sizes) < 3 * BLOCK
    return [rng.integers(0, 50000, size=n).tolist() for n in sizes]


@pytest.mark.parametrize("bos,eos", rr.SPECIALS)
def test_device_entry_three_workgroups(bos, eos):
    core = core_of()
    rng = np.random.default_rng(11)
    docs = batch_of_three_workgroups(rng)
    tokens, tok_off = rr.pack_docs(docs)
    held = to_device(tokens, tok_off)
    S = len(tokens) + len(docs) * ((bos is not None) + (eos is not None))
    for L in (1, 7, 64, 2048, 4096, S + 3):
        for drop_last in (False, True):
            want = rr.rows_rule(tokens, tok_off, L, bos, eos, 3, drop_last)
            same(pack_device(core, tokens, tok_off, L, bos, eos, 3, drop_last, held=held), want, (L, bos, eos, drop_last))
    for L in {S, S // 2 if S % 2 == 0 else S, S // 3 if S % 3 == 0 else S}:  # the stream an exact multiple of the row
        for drop_last in (False, True):
            same(pack_device(core, tokens, tok_off, L, bos, eos, 3, drop_last, held=held), rr.rows_rule(tokens, tok_off, L, bos, eos, 3, drop_last), (L, drop_last))


def test_device_entry_case_list():
    core = core_of()
    rng = np.random.default_rng(BLOCK)
    for name, docs, seq_lens in rr.cases(BLOCK, rng):
        tokens, tok_off = rr.pack_docs(docs)
        held = to_device(tokens, tok_off)
        for bos, eos in rr.SPECIALS:
            S = len(tokens) + len(docs) * ((bos is not None) + (eos is not None))
            for L in sorted(set(seq_lens) | {S + 3, max(S, 1)}):
                for drop_last in (False, True):
                    want = rr.rows_rule(tokens, tok_off, L, bos, eos, 9, drop_last)
                    same(pack_device(core, tokens, tok_off, L, bos, eos, 9, drop_last, held=held), want, (name, L, bos, eos, drop_last))


def test_token_pointer_that_is_not_16_byte_aligned():
    """With k == 0 a lane loads its eight ids as two 16-byte words where the caller's pointer allows it: here it does not."""
    import torch

    core = core_of()
    rng = np.random.default_rng(5)
    tokens, tok_off = rr.pack_docs([rng.integers(0, 50000, size=n).tolist() for n in (700, 0, 1500, 9)])
    buf = torch.zeros(len(tokens) + 8, dtype=torch.int32, device="cuda")
    d_off = torch.from_numpy(tok_off.view(np.int64).copy()).cuda()
    for shift in (0, 1, 3):
        buf[shift: shift + len(tokens)] = torch.from_numpy(tokens.view(np.int32).copy()).cuda()
        torch.cuda.synchronize()
        got = pack_device(core, tokens, tok_off, 64, held=(buf[shift:], d_off), pad=0)
        same(got, rr.rows_rule(tokens, tok_off, 64, pad=0), shift)


def test_more_than_1024_workgroups():
    """tk_k_rows_scan takes the counts of 1024 workgroups at a time: 1024 * 2048 + 2049 positions are 1026 workgroups, the last one partial,
    so its loop runs twice and the segments of the first 1024 workgroups are carried into the rest."""
    core = core_of()
    rng = np.random.default_rng(1026)
    n = 1024 * BLOCK + 2049
    cuts = rng.integers(0, n + 1, size=260)
    cuts = np.sort(np.concatenate([cuts, rng.choice(cuts, size=40), [n, n]]))  # 303 documents, 42 and more of them empty
    tok_off = np.concatenate([[0], cuts, [n]]).astype(np.uint64)
    tokens = rng.integers(0, 50000, size=n).astype(np.uint32)
    assert int((np.diff(tok_off.astype(np.int64)) == 0).sum()) >= 42 and int((cuts > 1024 * BLOCK).sum()) >= 2
    want = rr.rows_rule(tokens, tok_off, 1000, None, None, 7, True)
    assert want.n_stream == n and want.n_tail == n % 1000 and -(-(want.n_rows * 1000 + want.n_tail) // BLOCK) == 1026
    same(pack_device(core, tokens, tok_off, 1000, None, None, 7, True), want, "1026 workgroups")


# ---------------------------------------------------------------- invariants on a random batch
def test_invariants_on_a_random_batch():
    core = core_of("cl100k_shaped")
    rng = np.random.default_rng(0x20000)
    sizes = [0 if rng.random() < 0.15 else int(rng.integers(1, 160)) for _ in range(300)]
    docs = [rng.integers(0, 100000, size=n).tolist() for n in sizes]
    tokens, tok_off = rr.pack_docs(docs)
    assert 15000 < len(tokens) < 30000 and sizes.count(0) > 20
    held = to_device(tokens, tok_off)
    BOS, EOS, PAD, L = 100258, 100257, 100276, 512
    for bos, eos in ((None, EOS), (BOS, EOS), (None, None)):
        got = pack_device(core, tokens, tok_off, L, bos, eos, PAD, False, held=held)
        assert np.array_equal(got.cu_seqlens[:-1], np.flatnonzero(got.pos == 0)) and got.cu_seqlens[-1] == got.n_rows * L
        # the documents come back: strip bos, eos and pad, regroup by doc
        body = (got.doc != rr.NONE) & ~np.isin(got.ids, [x for x in (bos, eos) if x is not None])
        assert not np.any(got.ids[got.doc == rr.NONE] != PAD)
        back = [got.ids[body & (got.doc == d)].tolist() for d in range(len(docs))]
        assert back == docs
        # row_seg: the cu_seqlens of rows a .. b on their own
        for a, b in ((0, 1), (0, got.n_rows), (3, 4), (5, 17), (got.n_rows - 1, got.n_rows)):
            part = got.cu_seqlens[got.row_seg[a]: got.row_seg[b] + 1].astype(np.int64) - a * L
            pos = got.pos[a * L: b * L]
            assert np.array_equal(part, np.concatenate([np.flatnonzero(pos == 0), [(b - a) * L]])), (a, b)
        same(got, rr.rows_rule(tokens, tok_off, L, bos, eos, PAD), (bos, eos))


# ---------------------------------------------------------------- 16-bit ids
def test_ids_16_bit():
    enc = tiktoken.get_encoding("gpt2_shaped")
    assert enc.max_token_value < 65536
    texts = [d.decode() for d in h.fuzz_batch(0x16, 24 << 10)]
    eot = enc.eot_token
    for drop_last in (False, True):
        wide = enc.encode_ordinary_batch_rows(texts, 128, eos=eot, drop_last=drop_last)
        narrow = enc.encode_ordinary_batch_rows(texts, 128, eos=eot, drop_last=drop_last, dtype=np.uint16)
        assert narrow.ids.dtype == np.uint16 and narrow.tail_ids.dtype == np.uint16 and wide.ids.size > 3000
        assert np.array_equal(narrow.ids, wide.ids.astype(np.uint16)) and np.array_equal(narrow.tail_ids, wide.tail_ids.astype(np.uint16))
        for name in ("doc", "pos", "cu_seqlens", "row_seg", "tail_doc", "tail_pos"):
            assert np.array_equal(getattr(narrow, name), getattr(wide, name)), name
    tokens, tok_off = enc.encode_ordinary_batch_packed(texts)
    got = pack_device(enc._core_bpe, np.array(tokens), tok_off, 77, bos=eot, pad=0, dtype=np.uint16)
    want = rr.rows_rule(tokens, tok_off, 77, bos=eot, pad=0)
    same(got._replace(ids=got.ids.astype(np.uint32)), want, "device, 16-bit")
    for bad in (dict(bos=65536), dict(eos=70000), dict(eos=eot, pad=1 << 20)):
        with pytest.raises(ValueError, match="16-bit"):
            enc.encode_ordinary_batch_rows(texts[:3], 16, dtype=np.uint16, drop_last=True, **bad)
    with pytest.raises(ValueError, match="16-bit"):
        tiktoken.get_encoding("o200k_shaped").encode_ordinary_batch_rows(texts[:3], 16, dtype=np.uint16, drop_last=True)
    assert enc.encode_ordinary_batch_rows(texts[:3], 16, dtype=np.uint16, drop_last=True).ids.dtype == np.uint16  # (still usable)


# ---------------------------------------------------------------- end to end
def rows_result_as_ref(p, L) -> rr.Rows:
    flat = [np.concatenate([a.reshape(-1), t]) for a, t in ((p.ids, p.tail_ids), (p.doc, p.tail_doc), (p.pos, p.tail_pos))]
    assert p.ids.shape == p.doc.shape == p.pos.shape and p.ids.ndim == 2 and (p.ids.shape[1] == L or p.ids.size == 0)
    return rr.Rows(*flat, p.cu_seqlens, p.row_seg, p.ids.shape[0], len(p.cu_seqlens) - 1, p.n_stream, len(p.tail_ids))


@pytest.mark.parametrize("name", h.ENCODING_NAMES)
def test_end_to_end(name):
    enc = tiktoken.get_encoding(name)
    eot = enc.eot_token
    texts = [d.decode() for d in h.fuzz_batch(0xE2E + len(name), 64 << 10)] + ["", "tail"]
    tokens, tok_off = enc.encode_ordinary_batch_packed(texts)
    assert len(tokens) > 5000
    for L, kw in ((256, dict(eos=eot)), (1000, dict(bos=eot, eos=eot, pad=0, drop_last=True)), (64, dict(drop_last=True)), (len(tokens) + 3, dict(pad=5))):
        got = enc.encode_ordinary_batch_rows(texts, L, **kw)
        want = rr.rows_rule(tokens, tok_off, L, kw.get("bos"), kw.get("eos"), kw.get("pad", kw.get("eos", 0)), kw.get("drop_last", False))
        same(rows_result_as_ref(got, L), want, (L, kw))
    with_specials = [t + s for t, s in zip(texts, ["<|endoftext|>", "", " <|endoftext|> x"] * len(texts))]
    tokens, tok_off = enc.encode_batch_packed(with_specials, allowed_special="all")
    assert eot in tokens
    got = enc.encode_batch_rows(with_specials, 333, allowed_special="all", eos=eot)
    same(rows_result_as_ref(got, 333), rr.rows_rule(tokens, tok_off, 333, None, eot, eot), "allowed specials")
    # a disallowed special token: the error of encode_batch_packed
    with pytest.raises(ValueError) as want_err:
        enc.encode_batch_packed(with_specials)
    with pytest.raises(ValueError) as got_err:
        enc.encode_batch_rows(with_specials, 333, eos=eot)
    assert str(got_err.value) == str(want_err.value)
    blob, off = enc._pack(with_specials)
    with pytest.raises(tiktoken.DisallowedSpecialError) as want_hit:
        enc._core_bpe.encode_batch_packed(blob, off, None, disallowed_special="all")
    with pytest.raises(tiktoken.DisallowedSpecialError) as got_hit:
        enc._core_bpe.encode_batch_rows_packed(blob, off, None, disallowed_special="all", seq_len=333, eos=eot)
    assert (got_hit.value.doc, got_hit.value.pos, got_hit.value.token) == (want_hit.value.doc, want_hit.value.pos, want_hit.value.token)
    # padding that nothing was named for
    with pytest.raises(ValueError, match="pad"):
        enc.encode_ordinary_batch_rows(texts, len(tokens) + 3)
    assert enc.encode_ordinary_batch_rows([], 8).ids.shape == (0, 8)
    assert enc.encode_ordinary_batch_rows([], 8).cu_seqlens.tolist() == [0]


# ---------------------------------------------------------------- buffer lifetimes
def test_packing_leaves_the_encode_result_intact():
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
    for kw in (dict(eos=enc.eot_token), dict(drop_last=True), dict(bos=1, eos=2, pad=3, dtype=np.uint32)):
        r = core.pack_rows_device(dt, nt, dof, len(texts), seq_len=512, **kw)
        assert np.array_equal(h.dev_u32(dt, nt), tokens) and np.array_equal(h.dev_u64(dof, len(tok_off)), tok_off)
        m = r.n_rows * 512 + r.n_tail
        got = rr.Rows(h.dev_u32(r.ids, m), h.dev_u32(r.doc, m), h.dev_u32(r.pos, m), h.dev_u32(r.cu_seqlens, r.n_segs + 1), h.dev_u32(r.row_seg, r.n_rows + 1), *r[5:])
        same(got, rr.rows_rule(tokens, tok_off, 512, kw.get("bos"), kw.get("eos"), kw.get("pad", kw.get("eos", 0)), kw.get("drop_last", False)), kw)


# ---------------------------------------------------------------- refusals
def test_bad_tok_off_is_refused_by_the_device_check():
    """Refusals, not faults: the marking pass compares every entry with n_tokens before anything is indexed with it."""
    core = core_of()
    rng = np.random.default_rng(9)
    docs = [rng.integers(0, 50000, size=n).tolist() for n in (30, 0, 2100, 12, 5)]
    tokens, tok_off = rr.pack_docs(docs)
    d_tok, d_good = to_device(tokens, tok_off)
    n = len(tokens)
    for bad, doc in (([0, 30, 30, 2130, 2100, n], 3), ([0, 30, 30, 2130, 2142, n - 1], 4), ([0, 30, 30, 2130, 2142, n + 1], 4), ([1, 30, 30, 2130, 2142, n], 0),
                     ([0, 40, 30, 2130, 2142, n], 1)):
        _, d_bad = to_device(tokens, np.array(bad, np.uint64))
        for kw in (dict(eos=1), dict(drop_last=True)):
            with pytest.raises(ValueError, match=f"document {doc}\\b"):
                core.pack_rows_device(d_tok.data_ptr(), n, d_bad.data_ptr(), len(docs), seq_len=64, **kw)
        same(pack_device(core, tokens, tok_off, 64, eos=1, held=(d_tok, d_good)), rr.rows_rule(tokens, tok_off, 64, eos=1, pad=1), "after a refusal")


def test_remaining_refusals():
    enc = tiktoken.get_encoding("gpt2_shaped")
    core = enc._core_bpe
    tokens, tok_off = rr.pack_docs([[1, 2, 3], [4]])
    d_tok, d_off = to_device(tokens, tok_off)
    with pytest.raises(ValueError, match="seq_len"):
        core.pack_rows_device(d_tok.data_ptr(), 4, d_off.data_ptr(), 2, seq_len=0, drop_last=True)
    with pytest.raises(ValueError, match="seq_len"):
        enc.encode_ordinary_batch_rows(["a b c"], 0, drop_last=True)
    with pytest.raises(ValueError, match="pad"):
        core.pack_rows_device(d_tok.data_ptr(), 4, d_off.data_ptr(), 2, seq_len=3)
    with pytest.raises(ValueError, match="32-bit"):  # (refused from the figures alone: nothing is read)
        core.pack_rows_device(d_tok.data_ptr(), (1 << 32) - 1, d_off.data_ptr(), 2, seq_len=4, eos=1)
    with pytest.raises(ValueError, match="dtype"):
        enc.encode_ordinary_batch_rows(["a"], 4, eos=1, dtype=np.int64)
    same(pack_device(core, tokens, tok_off, 3, eos=9, held=(d_tok, d_off)), rr.rows_rule(tokens, tok_off, 3, eos=9, pad=9), "after the refusals")
    several = tiktoken.CoreBPE(enc._mergeable_ranks, enc._special_tokens, enc._pat_str, devices=[0, 0])
    with pytest.raises(ValueError, match="one device"):
        several.pack_rows_device(d_tok.data_ptr(), 4, d_off.data_ptr(), 2, seq_len=2)
    with pytest.raises(ValueError, match="one device"):
        several.encode_batch_rows_packed(np.frombuffer(b"ab", np.uint8), np.array([0, 2], np.uint64), seq_len=2)
