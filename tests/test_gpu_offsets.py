"""Token offsets for whole batches on the GPU (tk_offsets.h): Encoding.decode_with_offsets / decode_tokens_bytes of the reference
(tiktoken/core.py:303-335) as batch calls, and the same spans for the tokens an encode call has just produced.  Expected values: the
reference's own results recorded in tests/golden/offsets.json.gz (tools/gen_golden_offsets.py), the property its tests/test_offsets.py
checks, a numpy restatement of its rule, and Python's strict UTF-8 decoder."""
import gzip
import json
import os
import random

import numpy as np
import pytest

import helpers as h
import tiktoken_amd as tiktoken

pytestmark = pytest.mark.gpu
ENCS = h.ENCODING_NAMES


def golden():
    with gzip.open(os.path.join(h.ROOT, "tests", "golden", "offsets.json.gz")) as f:
        return json.loads(f.read())["encodings"]


def byte_ids(enc, data: bytes) -> list[int]:
    return [enc._mergeable_ranks[bytes([b])] for b in data]


# ---------------------------------------------------------------- the reference's recorded results
@pytest.mark.parametrize("name", ENCS)
def test_golden_offsets(name):
    enc = tiktoken.get_encoding(name)
    cases = golden()[name]
    assert len(cases) > 60 and any(not c["tokens"] for c in cases) and any(c["text"] is None for c in cases)
    good = [c for c in cases if c["text"] is not None]
    for c in cases:
        if c["text"] is None:
            with pytest.raises(UnicodeDecodeError):
                enc.decode_with_offsets(c["tokens"])
        else:
            assert enc.decode_with_offsets(c["tokens"]) == (c["text"], c["offsets"]), c["tokens"]
    assert enc.decode_with_offsets_batch([c["tokens"] for c in good]) == [(c["text"], c["offsets"]) for c in good]
    flat = np.array([t for c in good for t in c["tokens"]], np.uint32)
    tok_off = np.zeros(len(good) + 1, np.uint64)
    tok_off[1:] = np.cumsum([len(c["tokens"]) for c in good])
    data, byte_off, char_off, byte_start, char_start = enc.decode_with_offsets_packed(flat, tok_off)
    assert data.tobytes() == "".join(c["text"] for c in good).encode()
    assert byte_off.tolist() == [0] + np.cumsum([len(c["text"].encode()) for c in good]).tolist()
    assert char_off.tolist() == [0] + np.cumsum([len(c["text"]) for c in good]).tolist()
    assert char_start.tolist() == [o for c in good for o in c["offsets"]]
    for d, c in enumerate(good):  # byte_start: where the token's bytes lie in its document
        at = 0
        for i, t in enumerate(c["tokens"]):
            assert byte_start[int(tok_off[d]) + i] == at
            at += len(enc.decode_single_token_bytes(t))


@pytest.mark.parametrize("name", ENCS)
def test_offset_is_first_char_holding_a_byte_of_the_token(name):
    """tests/test_offsets.py of the reference: offset i = length of the common prefix of the text and decode(tokens[:i], errors="ignore")."""
    enc = tiktoken.get_encoding(name)
    rng = random.Random(17)
    units = ["hello", " world", "中", "文", "é", "😀", "ந", "ி", "டி", " ", "\n", "1234", "<|endoftext|>", "’", "ǅ", "́", "テキスト", "한국어", "🇩🇪", "👩‍👩‍👧‍👦"]
    batch = []
    for _ in range(60):
        text = "".join(rng.choice(units) for _ in range(rng.randrange(1, 20)))
        batch.append(enc.encode(text, allowed_special="all"))
    got = enc.decode_with_offsets_batch(batch)
    for tokens, (text, offsets) in zip(batch, got):
        assert text == enc.decode(tokens, errors="strict")
        want = []
        for i in range(len(tokens)):
            prefix = enc.decode(tokens[:i], errors="ignore")
            k = 0
            while k < len(text) and k < len(prefix) and text[k] == prefix[k]:
                k += 1
            want.append(k)
        assert offsets == want, (text, tokens)


# ---------------------------------------------------------------- a large batch against numpy
def numpy_spans(enc, tokens, tok_off):
    n_ids = enc.max_token_value + 1
    length, chars, cont = np.zeros(n_ids, np.int64), np.zeros(n_ids, np.int64), np.zeros(n_ids, bool)
    table = [(enc._mergeable_ranks[t], t) for t in enc.token_byte_values()] + [(i, s.encode()) for s, i in enc._special_tokens.items()]
    for i, t in table:
        a = np.frombuffer(t, np.uint8)
        c = (a & 0xC0) == 0x80
        length[i], chars[i], cont[i] = len(t), int((~c).sum()), bool(c[0])
    tl, tc = length[tokens], chars[tokens]
    gb, gc = np.concatenate([[0], np.cumsum(tl)]), np.concatenate([[0], np.cumsum(tc)])
    t_off = tok_off.astype(np.int64)
    byte_off, char_off = gb[t_off], gc[t_off]
    doc = np.repeat(np.arange(len(tok_off) - 1), np.diff(t_off))
    rel = gc[:-1] - char_off[doc]
    return byte_off, char_off, gb[:-1] - byte_off[doc], np.where(cont[tokens] & (rel > 0), rel - 1, rel)


def numpy_bytes(enc, tokens):
    """The decoded bytes as a gather over a numpy table of the vocabulary's token bytes (nothing of the library's decode in it)"""
    n_ids = enc.max_token_value + 1
    table = [(enc._mergeable_ranks[t], t) for t in enc.token_byte_values()] + [(i, s.encode()) for s, i in enc._special_tokens.items()]
    start, length = np.zeros(n_ids, np.int64), np.zeros(n_ids, np.int64)
    at = 0
    for i, t in table:
        start[i], length[i] = at, len(t)
        at += len(t)
    blob = np.frombuffer(b"".join(t for _, t in table), np.uint8)
    tl = length[tokens]
    ends = np.cumsum(tl)
    return blob[np.arange(int(ends[-1])) + np.repeat(start[tokens] - (ends - tl), tl)]


def test_large_batch_against_numpy():
    enc = tiktoken.get_encoding("o200k_shaped")
    blob, off = h.gen_corpus(0x0FF5, 1, 12 << 20)
    tokens, _ = enc._core_bpe.encode_batch_packed(blob, off, None)
    tokens = np.array(tokens)
    assert len(tokens) >= 2_000_000
    rng = np.random.default_rng(3)
    # documents of mixed sizes over the token stream: empty ones, single tokens, a few hundred, several workgroups of 2048
    sizes = []
    total = 0
    while total < len(tokens):
        k = int(rng.choice([0, 0, 1, 2, 7, 8, 9, 60, 150, 400, 2047, 2048, 2049, 9000], p=[.06, .06, .1, .1, .05, .05, .05, .2, .2, .11, .005, .005, .005, .005]))
        sizes.append(min(k, len(tokens) - total))
        total += sizes[-1]
    sizes += [0, 0]
    tok_off = np.zeros(len(sizes) + 1, np.uint64)
    tok_off[1:] = np.cumsum(sizes)
    assert len(sizes) >= 10_000 and max(sizes) > 4 * 2048 and sizes.count(0) > 500
    # (documents cut anywhere in the token stream need not be UTF-8: no validation here)
    data, byte_off, char_off, byte_start, char_start, bad = enc._core_bpe.decode_batch_spans_packed(tokens, tok_off, validate=False)
    assert bad is None
    w_boff, w_coff, w_bs, w_cs = numpy_spans(enc, tokens, tok_off)
    assert np.array_equal(byte_off, w_boff) and np.array_equal(char_off, w_coff)
    assert np.array_equal(byte_start, w_bs) and np.array_equal(char_start, w_cs)
    w_bytes = numpy_bytes(enc, tokens)
    ref_bytes, ref_off = enc._core_bpe.decode_batch_packed(tokens, tok_off, as_array=True)
    assert np.array_equal(ref_off, w_boff) and np.array_equal(ref_bytes, w_bytes) and np.array_equal(data, w_bytes)
    # spans only: the same arrays, no bytes
    only = enc._core_bpe.decode_batch_spans_packed(tokens, tok_off, want_bytes=False, validate=False)
    assert only[0] is None and np.array_equal(only[3], w_bs) and np.array_equal(only[4], w_cs) and np.array_equal(only[2], w_coff)
    # the corpus's own documents are valid UTF-8: the validated call agrees
    tokens2, tok_off2 = enc._core_bpe.encode_batch_packed(blob, off, None)
    data2, byte_off2, _, _, cs2 = enc.decode_with_offsets_packed(tokens2, tok_off2)
    assert np.array_equal(data2, blob) and np.array_equal(byte_off2, off)
    assert np.array_equal(cs2, numpy_spans(enc, np.array(tokens2), tok_off2)[3])
    # decode_tokens_bytes_batch against the per-token method, on a sample of the documents
    lo = len(sizes) // 2
    sample = [tokens[int(tok_off[d]):int(tok_off[d + 1])].tolist() for d in range(lo, lo + 120)]
    assert sum(map(len, sample)) > 1000
    assert enc.decode_tokens_bytes_batch(sample) == [[enc.decode_single_token_bytes(t) for t in doc] for doc in sample]
    assert enc.decode_tokens_bytes(sample[3]) == [enc.decode_single_token_bytes(t) for t in sample[3]]


def test_batch_of_several_ranges_against_numpy():
    """More than 2 x 16 Mi ids: tk_decode_batch_spans runs in overlapped ranges; documents lie across the ranges' boundaries."""
    enc = tiktoken.get_encoding("o200k_shaped")
    blob, off = h.gen_corpus(0x0FF6, 1, 12 << 20)
    tokens, tok_off = enc._core_bpe.encode_batch_packed(blob, off, None)
    reps = (34 << 20) // len(tokens) + 1
    counts = np.diff(tok_off.astype(np.int64))
    tokens = np.tile(np.array(tokens), reps)
    tok_off = np.concatenate([[0], np.cumsum(np.tile(counts, reps))]).astype(np.uint64)
    assert len(tokens) > 2 * (16 << 20) and (16 << 20) not in tok_off and (32 << 20) not in tok_off
    data, byte_off, char_off, byte_start, char_start = enc.decode_with_offsets_packed(tokens, tok_off)  # (validated: the documents are the corpus's)
    w_boff, w_coff, w_bs, w_cs = numpy_spans(enc, tokens, tok_off)
    assert np.array_equal(byte_off, w_boff) and np.array_equal(char_off, w_coff)
    assert np.array_equal(byte_start, w_bs) and np.array_equal(char_start, w_cs)
    assert len(data) == reps * len(blob) and all(np.array_equal(data[k * len(blob):(k + 1) * len(blob)], blob) for k in (0, reps // 2, reps - 1))
    only = enc._core_bpe.decode_batch_spans_packed(tokens, tok_off, want_bytes=False, validate=False)
    assert only[0] is None and np.array_equal(only[3], w_bs) and np.array_equal(only[4], w_cs) and np.array_equal(only[1], w_boff)
    # an ill-formed document and an id without an entry, both in the last range
    cut = int(tok_off[-3])
    bad = np.concatenate([tokens[:cut], np.array([enc._mergeable_ranks[b"\xe4"]], np.uint32), tokens[cut:]])
    bad_off = tok_off.copy()
    bad_off[-2:] += 1
    got = enc._core_bpe.decode_batch_spans_packed(bad, bad_off, want_bytes=False)
    assert got[5] == len(tok_off) - 3
    with pytest.raises(UnicodeDecodeError):
        enc.decode_with_offsets_packed(bad, bad_off)
    bad[cut] = enc.max_token_value + 7
    with pytest.raises(KeyError, match=str(enc.max_token_value + 7)):
        enc._core_bpe.decode_batch_spans_packed(bad, bad_off, validate=False)


def test_long_runs_of_empty_documents():
    enc = tiktoken.get_encoding("gpt2_shaped")
    ok = enc.encode("hello world, hello")
    batch = [[]] * 100_000 + [ok] + [[]] * 150_000 + [ok[:2]] + [[]] * 50_000
    flat, tok_off = enc._flatten(batch)
    data, byte_off, char_off, bs, cs = enc.decode_with_offsets_packed(flat, tok_off)
    text = enc.decode(ok)
    assert data.tobytes().decode() == text + enc.decode(ok[:2])
    want = np.zeros(len(batch) + 1, np.uint64)
    want[100_001:] = len(text)
    want[250_002:] = len(text) + len(enc.decode(ok[:2]))
    assert np.array_equal(byte_off, want) and np.array_equal(char_off, want)
    assert cs.tolist() == enc.decode_with_offsets(ok)[1] + enc.decode_with_offsets(ok[:2])[1]


# ---------------------------------------------------------------- invalid UTF-8, unknown ids, empty batches
def test_invalid_utf8_raises_pythons_error():
    enc = tiktoken.get_encoding("cl100k_shaped")
    ok = enc.encode("fine text 中文 😀 " * 40)
    bad_docs = [byte_ids(enc, b"ab\xe4\xb8"), byte_ids(enc, b"\x80abc"), enc.encode("x" * 50) + byte_ids(enc, b"\xed\xa0\x80") + enc.encode(" tail"),
                byte_ids(enc, b"\xf4\x90\x80\x80"), byte_ids(enc, b"\xc0\xaf")]
    for bad in bad_docs:
        raw = enc.decode_bytes(bad)
        try:
            raw.decode("utf-8", "strict")
            raise AssertionError("the case is meant to be invalid")
        except UnicodeDecodeError as e:
            want = (e.start, e.end, e.reason, e.object)
        for batch in ([bad, ok, ok], [ok, [], bad, ok], [ok, ok, bad], [ok, bad, bad_docs[0]]):  # first, middle, last; two bad ones: the first
            with pytest.raises(UnicodeDecodeError) as e:
                enc.decode_with_offsets_batch(batch)
            assert (e.value.start, e.value.end, e.value.reason, e.value.object) == want
        with pytest.raises(UnicodeDecodeError) as e:
            enc.decode_with_offsets(bad)
        assert (e.value.start, e.value.end, e.value.reason, e.value.object) == want
    # a sequence split across two documents: both are invalid, the first is reported
    a, b = enc.encode("head ") + byte_ids(enc, b"\xe4\xb8"), byte_ids(enc, b"\xad") + enc.encode(" rest")
    assert enc.decode_with_offsets(a + b)[0] == "head 中 rest"
    for batch, first in (([ok, a, b], a), ([b, ok], b), ([ok, [], a, [], b], a)):
        with pytest.raises(UnicodeDecodeError) as e:
            enc.decode_with_offsets_batch(batch)
        try:
            enc.decode_bytes(first).decode("utf-8", "strict")
        except UnicodeDecodeError as w:
            assert (e.value.start, e.value.end, e.value.reason, e.value.object) == (w.start, w.end, w.reason, w.object)
    # validate=False: the spans, no exception
    flat, tok_off = enc._flatten([ok, a, b])
    data, byte_off, char_off, bs, cs, bad = enc._core_bpe.decode_batch_spans_packed(flat, tok_off, validate=False)
    assert bad is None and data.tobytes() == b"".join(enc.decode_bytes(t) for t in (ok, a, b))
    assert cs[int(tok_off[2])] == 0 and bs[int(tok_off[2])] == 0 and cs[int(tok_off[2]) + 1] == 0  # the clamp: the continuation byte, then " rest"... both in char 0
    assert enc._core_bpe.decode_batch_spans_packed(flat, tok_off, validate=True)[5] == 1
    assert enc.decode_tokens_bytes_batch([a, b]) == [[enc.decode_single_token_bytes(t) for t in doc] for doc in (a, b)]


def test_unknown_id_and_empty_batches():
    enc = tiktoken.get_encoding("cl100k_shaped")
    missing = 100261  # between the special tokens of the shaped vocabulary
    with pytest.raises(KeyError):
        enc.decode_single_token_bytes(missing)
    ok = enc.encode("hello world")
    for batch in ([ok, ok + [missing] + [missing + 1], ok], [[missing]]):
        with pytest.raises(KeyError, match=str(missing)):
            enc.decode_with_offsets_batch(batch)
        with pytest.raises(KeyError, match=str(missing)):
            enc.decode_tokens_bytes_batch(batch)
    with pytest.raises(KeyError, match=str(missing)):
        enc.decode_with_offsets(ok + [missing])
    with pytest.raises(KeyError, match=str(missing)):
        enc.decode_tokens_bytes([missing])
    with pytest.raises(KeyError):
        enc.decode_with_offsets_batch([[enc.max_token_value + 5]])
    assert enc.decode_with_offsets_batch([]) == []
    assert enc.decode_with_offsets_batch([[], [], []]) == [("", [])] * 3
    assert enc.decode_tokens_bytes_batch([]) == [] and enc.decode_tokens_bytes_batch([[], []]) == [[], []]
    assert enc.decode_with_offsets([]) == ("", []) and enc.decode_tokens_bytes([]) == []
    data, byte_off, char_off, bs, cs = enc.decode_with_offsets_packed(np.zeros(0, np.uint32), np.zeros(4, np.uint64))
    assert len(data) == 0 and byte_off.tolist() == [0] * 4 and char_off.tolist() == [0] * 4 and len(bs) == 0 and len(cs) == 0
    # documents of continuation bytes only: every token of them lies in char 0
    conts = byte_ids(enc, b"\x80\xbf\x80")
    flat, tok_off = enc._flatten([conts[:1], conts, [], conts[:2] + ok])
    _, _, char_off, bs, cs, _ = enc._core_bpe.decode_batch_spans_packed(flat, tok_off, validate=False)
    assert cs.tolist()[:6] == [0] * 6 and bs.tolist()[:6] == [0, 0, 1, 2, 0, 1] and char_off.tolist()[:4] == [0, 0, 0, 0]


def test_several_devices_are_refused():
    enc = tiktoken.get_encoding("gpt2_shaped")
    core = tiktoken.CoreBPE(enc._mergeable_ranks, enc._special_tokens, enc._pat_str, devices=[0, 0])
    with pytest.raises(ValueError, match="one device"):
        core.decode_batch_spans_packed(np.zeros(1, np.uint32), np.array([0, 1], np.uint64))
    with pytest.raises(ValueError, match="one device"):
        core.encode_batch_spans_packed(np.frombuffer(b"ab", np.uint8), np.array([0, 2], np.uint64))
    with pytest.raises(ValueError, match="one device"):
        core.token_spans_device(0, 0, 0, 0)


# ---------------------------------------------------------------- the encode side
def check_encode_side(enc, texts, **kw):
    tokens, tok_off, byte_start, char_start = enc.encode_batch_offsets_packed(texts, **kw) if kw else enc.encode_ordinary_batch_offsets_packed(texts)
    w_tokens, w_off = enc.encode_batch_packed(texts, **kw) if kw else enc.encode_ordinary_batch_packed(texts)
    assert np.array_equal(tokens, w_tokens) and np.array_equal(tok_off, w_off)
    blob, doc_off = enc._pack(texts)
    raw = blob.tobytes()
    docs = [tokens[int(a):int(b)].tolist() for a, b in zip(tok_off[:-1], tok_off[1:])]
    for d, doc in enumerate(docs):
        for k, t in enumerate(doc):
            i = int(tok_off[d]) + k
            piece = enc.decode_single_token_bytes(t)
            at = int(doc_off[d]) + int(byte_start[i])
            assert raw[at:at + len(piece)] == piece, (d, k)
    want = enc.decode_with_offsets_batch(docs)
    assert [w[0] for w in want] == [_repaired(t) for t in texts]
    assert char_start.tolist() == [o for w in want for o in w[1]]
    for d in sorted({0, len(docs) // 2, len(docs) - 1}) if docs else ():
        assert enc.decode_with_offsets(docs[d])[1] == char_start[int(tok_off[d]):int(tok_off[d + 1])].tolist()
    return tokens


def _repaired(t: str) -> str:
    return t.encode("utf-8", "surrogatepass").decode("utf-8", "replace") if any(0xD800 <= ord(c) < 0xE000 for c in t) else t


def fuzz_texts(seed, nbytes=48 << 10):
    return [d.decode() for d in h.fuzz_batch(seed, nbytes)] + ["", "நடிகர் சூர்யா", "我非常渴望与人工智能一起工作", " Ġ除", ""]


@pytest.mark.parametrize("name", ENCS)
def test_encode_side_stock_families(name):
    enc = tiktoken.get_encoding(name)
    toks = check_encode_side(enc, fuzz_texts(0xE0 + len(name)))
    assert len(toks) > 5000
    check_encode_side(enc, fuzz_texts(0xE1), allowed_special="all")
    check_encode_side(enc, ["hello world<|endoftext|> green cow", "<|endoftext|>", "", "x<|endoftext|>"], allowed_special="all")
    check_encode_side(enc, ["plain", "text only"], allowed_special=set(), disallowed_special="all")
    with pytest.raises(ValueError, match="disallowed special token"):
        enc.encode_batch_offsets_packed(["fine", "not <|endoftext|> fine"])
    check_encode_side(enc, [])
    check_encode_side(enc, ["", ""])


def test_encode_side_generic_pattern():
    base = tiktoken.get_encoding("cl100k_shaped")
    enc = tiktoken.Encoding("everything", pat_str=r"\s+|\S+", mergeable_ranks=base._mergeable_ranks, special_tokens=base._special_tokens)
    assert tiktoken._lib.lib().tk_pattern_id(enc._pat_str.encode()) == 3
    check_encode_side(enc, fuzz_texts(0xE7, 24 << 10))
    check_encode_side(enc, fuzz_texts(0xE8, 24 << 10), allowed_special="all")
    # a pattern that leaves characters unmatched: they yield no token, the spans would be off -- refused, naming the document
    gaps = tiktoken.Encoding("words_only", pat_str=r"\w+", mergeable_ranks=base._mergeable_ranks, special_tokens=base._special_tokens)
    assert gaps.encode_ordinary_batch(["ab cd", "efgh"]) == [gaps.encode_ordinary("ab") + gaps.encode_ordinary("cd"), gaps.encode_ordinary("efgh")]
    check_encode_side(gaps, ["abcd", "efgh", ""])
    with pytest.raises(ValueError, match="document 1"):
        gaps.encode_ordinary_batch_offsets_packed(["abcd", "ef gh", "ij kl"])
    check_encode_side(gaps, ["still", "usable"])


def test_device_resident_spans():
    import torch

    enc = tiktoken.get_encoding("o200k_shaped")
    core = enc._core_bpe
    texts = fuzz_texts(0xD0, 96 << 10)
    blob, off = enc._pack(texts)
    tokens, tok_off, byte_start, char_start = enc.encode_ordinary_batch_offsets_packed(texts)
    d_text = torch.zeros(len(blob) + 256, dtype=torch.uint8, device="cuda")
    d_text[: len(blob)] = torch.from_numpy(blob.copy()).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    dt, nt, dof = core.encode_batch_device(d_text.data_ptr(), len(blob), d_off.data_ptr(), off, len(texts))
    assert nt == len(tokens)
    for d_doc_off in (d_off.data_ptr(), 0):
        dbs, dcs, dbo, dco = core.token_spans_device(dt, nt, dof, len(texts), d_doc_off)
        assert np.array_equal(h.dev_u32(dbs, nt), byte_start) and np.array_equal(h.dev_u32(dcs, nt), char_start)
        assert np.array_equal(h.dev_u64(dbo, len(off)), off)
        assert h.dev_u64(dco, len(off)).tolist() == [0] + np.cumsum([len(_repaired(t)) for t in texts]).tolist()
    # ... and the bytes follow from the same ids with the device-resident decode
    db, nb, dbo2 = core.decode_batch_device(dt, nt, dof, len(texts))
    assert nb == len(blob) and np.array_equal(h.dev_u64(dbo2, len(off)), off)
