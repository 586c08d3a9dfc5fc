"""Disallowed special tokens checked on the GPU, in the batch encode's own call (tk_encode_batch_checked / tk_k_spec_find), against
what the reference does on the host before it encodes (tiktoken/core.py:116-124): the same ValueError for the same document, the
same tokens when nothing is found, and the scan really taken (a launch counter) exactly when the policy can be checked on the device."""
import numpy as np
import pytest

import helpers as h

pytestmark = pytest.mark.gpu

MIB = 1 << 20


def make_encoding(name: str, specials=None):
    from tiktoken_amd import Encoding

    g = h.load_golden(name)
    return Encoding(name + "_disallowed_test", pat_str=g["pat_str"], mergeable_ranks=h.golden_vocab(name),
                    special_tokens=dict(specials if specials is not None else g["special_tokens"]))


@pytest.fixture(scope="module")
def encs():
    return {"o200k_custom8": make_encoding("o200k_shaped", h.CUSTOM8), "cl100k_shaped": make_encoding("cl100k_shaped")}


def launches(enc) -> int:
    return enc._core_bpe.stat("spec_find_launches")


def host_error(enc, text: str, disallowed) -> str:
    """What the host search says about one document: the parent's code path."""
    with pytest.raises(ValueError) as e:
        enc._reject_disallowed(text, disallowed)
    return str(e.value)


def texts_of(blob, off) -> list[str]:
    bb = blob.tobytes()
    return [bb[int(a):int(b)].decode("utf-8") for a, b in zip(off[:-1], off[1:])]


def first_hit(specials: dict[str, int], docs: list[bytes], disallowed):
    """(doc, byte offset, token): the CPU answer -- the first document with an occurrence, the leftmost one in it, the longest token there."""
    toks = sorted((s.encode() for s in disallowed), key=len, reverse=True)
    for d, t in enumerate(docs):
        at = min((p for p in (t.find(s) for s in toks) if p >= 0), default=-1)
        if at >= 0:
            return d, at, next(s for s in toks if t.startswith(s, at)).decode()
    return None


@pytest.mark.parametrize("name", ["o200k_custom8", "cl100k_shaped"])
def test_default_arguments_raise_the_host_error(encs, name):
    enc = encs[name]
    tok = "<|custom_5|>" if name == "o200k_custom8" else "<|fim_middle|>"
    clean = texts_of(*h.gen_corpus(0xD15A, 1, 1 * MIB))
    assert len(clean) > 20
    n = len(clean)
    for where in (0, n // 2, n - 1):  # the first, a middle, the last document
        texts = list(clean)
        texts[where] = texts[where][:100] + tok + texts[where][100:]
        before = launches(enc)
        with pytest.raises(ValueError) as e:
            enc.encode_batch(texts)
        assert str(e.value) == host_error(enc, texts[where], enc.special_tokens_set)
        assert tok in str(e.value)
        assert launches(enc) > before
        with pytest.raises(ValueError) as e:
            enc.encode_batch_packed(texts)
        assert str(e.value) == host_error(enc, texts[where], enc.special_tokens_set)
    # two offending documents: the earlier one is named
    texts = list(clean)
    texts[n // 3] += "<|endoftext|>"
    texts[2 * n // 3] = tok + texts[2 * n // 3]
    with pytest.raises(ValueError) as e:
        enc.encode_batch(texts)
    assert str(e.value) == host_error(enc, texts[n // 3], enc.special_tokens_set) and "<|endoftext|>" in str(e.value)
    # ... and the batch without them encodes as ever
    C = h.c_oracle_for("o200k_shaped" if name == "o200k_custom8" else name)
    blob, off = h.pack([t.encode() for t in clean])
    want, woff = C.encode_batch(blob, off, None, 8)
    got, goff = enc.encode_batch_packed(clean)
    assert np.array_equal(got, want) and np.array_equal(goff, woff)


def test_allowed_overrides_disallowed(encs):
    enc = encs["o200k_custom8"]
    a = ["some text <|custom_1|> more", "plain", "tail <|custom_1|>"]
    got = enc.encode_batch(a, allowed_special={"<|custom_1|>"}, disallowed_special="all")
    assert got[0].count(h.CUSTOM8["<|custom_1|>"]) == 1 and got[2][-1] == h.CUSTOM8["<|custom_1|>"]
    assert got == [enc.encode(t, allowed_special={"<|custom_1|>"}) for t in a]
    b = a + ["and <|custom_2|> here"]
    with pytest.raises(ValueError) as e:
        enc.encode_batch(b, allowed_special={"<|custom_1|>"}, disallowed_special="all")
    assert str(e.value) == host_error(enc, b[3], enc.special_tokens_set - {"<|custom_1|>"}) and "<|custom_2|>" in str(e.value)
    # disallowed_special=() never raises: everything is text
    before = launches(enc)
    assert enc.encode_batch(b, disallowed_special=()) == [enc.encode_ordinary(t) for t in b]
    assert launches(enc) == before
    # an explicit set of one token ignores the others
    assert enc.encode_batch(a, disallowed_special={"<|custom_2|>"}) == [enc.encode_ordinary(t) for t in a]
    with pytest.raises(ValueError) as e:
        enc.encode_batch(b, disallowed_special={"<|custom_2|>"})
    assert str(e.value) == host_error(enc, b[3], {"<|custom_2|>"})
    # the same token allowed and disallowed raises, as the reference does (it searches before it encodes)
    with pytest.raises(ValueError) as e:
        enc.encode_batch(a, allowed_special={"<|custom_1|>"}, disallowed_special={"<|custom_1|>"})
    assert str(e.value) == host_error(enc, a[0], {"<|custom_1|>"})


def test_scan_is_taken_exactly_when_the_device_can_check(encs):
    enc = encs["o200k_custom8"]
    texts = ["hello world " * 50, "", "more text <|custom_9|> <|endoftext"] * 4
    want = [enc.encode_ordinary(t) for t in texts]
    n0 = launches(enc)
    assert enc.encode_batch(texts) == want  # default arguments: disallowed_special="all"
    n1 = launches(enc)
    assert n1 > n0
    assert enc.encode_batch(texts, disallowed_special=()) == want
    assert launches(enc) == n1
    assert enc.encode_batch(texts, disallowed_special={"<|custom_1|>", "not a special token"}) == want  # any string may be disallowed: host search
    assert launches(enc) == n1
    with pytest.raises(ValueError, match="not a special token"):
        enc.encode_batch(texts + ["this is not a special token, or is it"], disallowed_special={"<|custom_1|>", "not a special token"})
    assert launches(enc) == n1
    lone = texts + ["lone \ud83d surrogate"]
    assert enc.encode_batch(lone) == want + [enc.encode_ordinary("lone \ufffd surrogate")]  # surrogate repair: host search
    assert launches(enc) == n1
    with pytest.raises(ValueError, match="custom_3"):
        enc.encode_batch(lone + ["<|custom_3|>"])
    assert launches(enc) == n1
    assert enc.encode_batch(texts, disallowed_special=["<|custom_1|>", "<|endofprompt|>"]) == want  # (any collection)
    assert launches(enc) > n1
    # the single-text calls keep the host search
    n2 = launches(enc)
    with pytest.raises(ValueError):
        enc.encode("a <|custom_1|>")
    assert enc.encode("hello") == enc.encode_ordinary("hello") and launches(enc) == n2


def test_kernel_is_profiled(encs):
    core = encs["o200k_custom8"]._core_bpe
    core.set_profiling(True)
    try:
        core.reset_kernel_ms()
        encs["o200k_custom8"].encode_batch(["some text"] * 100)
        ms, n = core.kernel_ms("tk_k_spec_find")
        assert n >= 1 and ms > 0
    finally:
        core.set_profiling(False)


@pytest.mark.parametrize("name", ["o200k_custom8", "cl100k_shaped"])
def test_no_hit_equals_the_oracle(encs, name):
    """6 MiB of text with decoys -- for cl100k every <|custom_N|> that helpers.insert_specials puts in is one: none is registered."""
    enc = encs[name]
    C = h.c_oracle_for("o200k_shaped" if name == "o200k_custom8" else name)
    blob, off = h.gen_corpus(0x6A8, 1, 6 * MIB)
    if name == "cl100k_shaped":
        blob, off = h.insert_specials(blob, off)
    else:  # decoys only
        docs = [d + b" <|custom_9|> <|endoftext <|custom_3| <| |>" for d in texts_bytes(blob, off)]
        blob, off = h.pack(docs)
    want, woff = C.encode_batch(blob, off, None, 8)
    before = launches(enc)
    got, goff = enc.encode_batch_packed(texts_of(blob, off))
    assert launches(enc) > before
    assert np.array_equal(goff, woff) and np.array_equal(got, want)


def texts_bytes(blob, off) -> list[bytes]:
    bb = blob.tobytes()
    return [bb[int(a):int(b)] for a, b in zip(off[:-1], off[1:])]


# ---------------------------------------------------------------- the pipelined host path (32 MiB chunks)
@pytest.fixture(scope="module")
def big(encs):
    """Five documents of 30 MiB each, a multiple of 16 bytes: at least 2 * TK_STAGE_BYTES in all, so the batch takes the pipelined path, and
    the cuts next to j/5 of the bytes make every document a chunk of its own (asserted through the "chunks" figure)."""
    enc = encs["cl100k_shaped"]
    stage = enc._core_bpe.stat("stage_bytes")
    assert stage == 64 * MIB
    L, n = 30 * MIB, 5
    assert n * L >= 2 * stage
    blob, off = h.insert_specials(*h.gen_corpus(0xB16B16, 1, n * L + MIB, threads=16))  # (decoys: cl100k registers no <|custom_N|>)
    bb = blob.tobytes()
    docs = []
    for k in range(n):
        a = int(off[np.searchsorted(off, k * L, side="left")])  # a document start: a char boundary
        body = bb[a:a + L - 64]
        while body and (body[-1] & 0xC0) == 0x80:
            body = body[:-1]
        if body and body[-1] >= 0xC0:
            body = body[:-1]
        docs.append(body + b"x" * (L - len(body)))
    assert all(len(d) == L for d in docs)
    return docs


def test_pipelined_no_hit_and_token_across_chunks(encs, big):
    enc = encs["cl100k_shaped"]
    C = h.c_oracle_for("cl100k_shaped")
    tok = b"<|fim_suffix|>"
    docs = list(big)
    for k in range(len(docs) - 1):  # every chunk ends with one half of a token and the next one starts with the other
        docs[k] = docs[k][:-7] + tok[:7]
        docs[k + 1] = tok[7:] + docs[k + 1][:-7]  # (the documents end in padding)
    blob, off = h.pack(docs)
    want, woff = C.encode_batch(blob, off, None, 8)
    before = launches(enc)
    got, goff = enc.encode_batch_packed([d.decode() for d in docs])
    assert enc._core_bpe.stat("chunks") == len(docs)
    assert launches(enc) >= before + len(docs)  # one per chunk
    assert np.array_equal(goff, woff) and np.array_equal(got, want)


def test_pipelined_hits(encs, big):
    enc = encs["cl100k_shaped"]
    core = enc._core_bpe
    from tiktoken_amd import DisallowedSpecialError

    tok = b"<|fim_suffix|>"
    L = len(big[0])
    cases = {
        "in the last chunk": (4, 12345),
        "ends on a chunk's last byte": (2, L - len(tok)),
        "starts a chunk": (3, 0),
        "ends on the batch's last byte": (4, L - len(tok)),
    }
    for what, (d, at) in cases.items():
        docs = list(big)
        docs[d] = docs[d][:at] + tok + docs[d][at + len(tok):]
        blob, off = h.pack(docs)
        with pytest.raises(DisallowedSpecialError) as e:
            core.encode_batch_packed(blob, off, set(), disallowed_special="all")
        assert (e.value.doc, e.value.pos, e.value.token) == (d, at, tok.decode()), what
        assert (d, at, tok.decode()) == first_hit(enc._special_tokens, docs, enc.special_tokens_set), what
    # ... through Encoding, and the core is fine afterwards
    texts = [x.decode() for x in docs]
    with pytest.raises(ValueError) as e:
        enc.encode_batch_packed(texts)
    assert str(e.value) == host_error(enc, texts[4], enc.special_tokens_set)
    small = ["after the hit", "all is well"]
    assert enc.encode_batch(small) == [enc.encode_ordinary(t) for t in small]


# ---------------------------------------------------------------- packed bytes: CoreBPE
def test_corebpe_packed_hit_fields_and_core_stays_usable(encs):
    from tiktoken_amd import DisallowedSpecialError

    enc = encs["o200k_custom8"]
    core = enc._core_bpe
    C = h.c_oracle_for("o200k_shaped")
    clean = texts_bytes(*h.gen_corpus(0xFEED, 0, 2 * MIB))
    cb, co = h.pack(clean)
    want, woff = C.encode_batch(cb, co, None, 8)
    dirty = list(clean)
    dirty[7] = b""
    dirty[8] = "é中".encode() + b"<|custom_9|><|custom_6|>" + dirty[8] + b"<|endoftext|>"
    dirty[30] = b"<|endofprompt|>"
    db, do = h.pack(dirty)
    hit = first_hit(h.CUSTOM8, dirty, h.CUSTOM8)
    assert hit == (8, 5 + 12, "<|custom_6|>")
    for _ in range(2):  # both orders, twice
        with pytest.raises(DisallowedSpecialError) as e:
            core.encode_batch_packed(db, do, disallowed_special="all")
        assert (e.value.doc, e.value.pos, e.value.token) == hit and isinstance(e.value, ValueError)
        assert str(e.value) == host_error(enc, "<|custom_6|>", {"<|custom_6|>"})
        got, goff = core.encode_batch_packed(cb, co, disallowed_special="all")
        assert np.array_equal(got, want) and np.array_equal(goff, woff)
        got, goff = core.encode_batch_packed(cb, co)
        assert np.array_equal(got, want) and np.array_equal(goff, woff)
        with pytest.raises(DisallowedSpecialError) as e:
            core.encode_batch_packed(db, do, None, disallowed_special={"<|endofprompt|>", "<|endoftext|>"})
        assert (e.value.doc, e.value.pos, e.value.token) == first_hit(h.CUSTOM8, dirty, {"<|endofprompt|>", "<|endoftext|>"})
        assert e.value.doc == 8 and e.value.token == "<|endoftext|>"
    # one document, short: a checked call does not take the one-launch path
    with pytest.raises(DisallowedSpecialError) as e:
        core.encode_batch_packed(*h.pack([b"tiny <|custom_0|>"]), disallowed_special="all")
    assert (e.value.doc, e.value.pos, e.value.token) == (0, 5, "<|custom_0|>")
    t, o = core.encode_batch_packed(*h.pack([b"tiny text"]), disallowed_special="all")
    assert t.tolist() == enc.encode_ordinary("tiny text") and o.tolist() == [0, len(t)]
    # an allowed token overlapping a disallowed one: the search looks at the raw text
    with pytest.raises(DisallowedSpecialError) as e:
        core.encode_batch_packed(*h.pack([b"a <|custom_1|> b", b"<|custom_2|>"]), {"<|custom_1|>"}, disallowed_special={"<|custom_1|>", "<|custom_2|>"})
    assert (e.value.doc, e.value.pos) == (0, 2)
    # empty batch, empty documents; a string that is no special token of the core
    t, o = core.encode_batch_packed(*h.pack([b"", b""]), disallowed_special="all")
    assert len(t) == 0 and o.tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match="not a special token"):
        core.encode_batch_packed(cb, co, disallowed_special={"<|nope|>"})


def test_device_resident_checked(encs):
    import torch

    from tiktoken_amd import DisallowedSpecialError

    enc = encs["o200k_custom8"]
    core = enc._core_bpe
    clean = texts_bytes(*h.gen_corpus(0xFEED, 0, 2 * MIB))
    want, woff = h.c_oracle_for("o200k_shaped").encode_batch(*h.pack(clean), None, 8)
    dirty = list(clean)
    dirty[11] = dirty[11][:64] + b"<|custom_3|>" + dirty[11][64:]
    for docs, hit in ((clean, None), (dirty, (11, 64, "<|custom_3|>")), (clean, None)):
        blob, off = h.pack(docs)
        d_text = torch.zeros(len(blob) + 256, dtype=torch.uint8, device="cuda")
        d_text[: len(blob)] = torch.from_numpy(blob.copy()).cuda()
        d_off = torch.from_numpy(off.astype(np.int64)).cuda()
        torch.cuda.synchronize()
        for h_off in (off, None):
            if hit:
                with pytest.raises(DisallowedSpecialError) as e:
                    core.encode_batch_device(d_text.data_ptr(), len(blob), d_off.data_ptr(), h_off, len(docs), disallowed_special="all")
                assert (e.value.doc, e.value.pos, e.value.token) == hit
            else:
                dt, nt, dof = core.encode_batch_device(d_text.data_ptr(), len(blob), d_off.data_ptr(), h_off, len(docs), disallowed_special="all")
                assert nt == len(want)
                assert np.array_equal(h.dev_u32(dt, nt), want) and np.array_equal(h.dev_u64(dof, len(off)), woff)


def test_virtual_ranks_same_hit_same_tokens(encs):
    from tiktoken_amd import CoreBPE, DisallowedSpecialError

    g = h.load_golden("o200k_shaped")
    clean = texts_bytes(*h.gen_corpus(0x6A9, 0, 6 * MIB))
    cb, co = h.pack(clean)
    want, woff = h.c_oracle_for("o200k_shaped").encode_batch(cb, co, None, 8)
    n = len(clean)
    for devices in ([0, 0], [0, 0, 0]):
        core = CoreBPE(h.golden_vocab("o200k_shaped"), h.CUSTOM8, g["pat_str"], devices=devices)
        got, goff = core.encode_batch_packed(cb, co, disallowed_special="all")
        assert np.array_equal(got, want) and np.array_equal(goff, woff)
        for where in ([5], [n - 3], [n // 2, n - 3], [n // 5, n // 2, n - 1]):  # hits in one shard, in the last, in several: the lowest document
            dirty = list(clean)
            for d in where:
                dirty[d] = dirty[d][:40] + b"<|custom_%d|>" % (d % 8) + dirty[d][40:]
            with pytest.raises(DisallowedSpecialError) as e:
                core.encode_batch_packed(*h.pack(dirty), disallowed_special="all")
            assert (e.value.doc, e.value.pos, e.value.token) == first_hit(h.CUSTOM8, dirty, h.CUSTOM8) == (where[0], 40, "<|custom_%d|>" % (where[0] % 8))
        got, goff = core.encode_batch_packed(cb, co, disallowed_special="all")
        assert np.array_equal(got, want) and np.array_equal(goff, woff)
        core.close()
