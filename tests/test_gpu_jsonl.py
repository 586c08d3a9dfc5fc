"""JSON Lines on the GPU (tk_jsonl.h): tk_jsonl_extract, tk_jsonl_extract_device and tk_encode_jsonl through CoreBPE and Encoding, status
for status and byte for byte against tests/jsonl_ref.py -- the rule as a byte scanner -- and, for the encode entries, against
encode_ordinary_batch_packed on the texts of the reference route; never against another run of the code under test.  The shapes: every
item that can straddle a tile's edge cut at every byte, lines of several tiles, more lines than tiles, every status under every on_error."""
import random

import numpy as np
import pytest

import jsonl_cases as jc
import jsonl_ref as jr
import tiktoken_amd as tiktoken
from tiktoken_amd import JsonlError, _tiktoken

pytestmark = pytest.mark.gpu


def enc_of(name="gpt2_shaped"):
    return tiktoken.get_encoding(name)


def tile_of(enc) -> int:
    return int(enc._core_bpe.stat("jsonl_tile"))


def same(got, want: jr.Extract, what):
    assert got.n_lines == len(want.status), what
    for name in ("status", "line_off", "line", "doc_off", "text"):
        a, b = np.asarray(getattr(got, name)), getattr(want, name)
        assert a.shape == b.shape and (a == b).all(), (what, name, a[:40], b[:40])


def check(enc, buf: bytes, field="text", what=None, modes=("skip", "empty", "raise")):
    for mode in modes:
        want = jr.extract(buf, field.encode(), jr.MODES[mode])
        if want.bad is not None:
            with pytest.raises(JsonlError) as e:
                enc.extract_jsonl(buf, field, mode)
            assert (e.value.line, e.value.pos, e.value.status) == want.bad, (what, mode)
        else:
            same(enc.extract_jsonl(buf, field, mode), want, (what, mode))
    return jr.extract(buf, field.encode(), jr.SKIP)


def test_every_tile_edge_case_long_lines_and_edge_statuses():
    enc = enc_of()
    T = tile_of(enc)
    assert T % 64 == 0 and T >= 64
    for name, buf in jc.edge_buffers(T):
        check(enc, buf, what=name, modes=("skip", "raise") if len(buf) > 60000 else ("skip", "empty", "raise"))
    r = check(enc, jc.straddle(T, b"\\ud83d\\ude00", T - 5), modes=("skip",))
    assert r.texts()[0].endswith("😀".encode())


def test_more_lines_than_tiles_and_empty_documents():
    enc = enc_of()
    buf = b'{"text":""}\n' * 70000
    assert 70000 > len(buf) // tile_of(enc)
    got = enc.extract_jsonl(buf)
    same(got, jr.extract(buf, b"text", jr.RAISE), "70000 empty")
    assert len(got.line) == 70000 and int(got.doc_off[-1]) == 0 and got.texts()[:2] == ["", ""]


def test_every_status_under_every_on_error_and_a_refused_call_changes_nothing():
    enc = enc_of()
    good = b'{"text":"kept \\u00e9"}\n{"id":1,"text":"second"}\n'
    import torch

    # the device entry keeps its result in the core: a refused call must leave it whole
    t_good = torch.frombuffer(bytearray(good), dtype=torch.uint8).to(f"cuda:{enc._core_bpe.device}")
    lines =[b'{"text":"ok"}', b"  \t", b'{"id":2}', b'{"text":17}', b'{"text":"open}', b'{"text":"bad \\q"}', b'{"text":"\xff"}', b'["text"]', b'{"text":"last"}']
    want_status = [jr.OK, jr.BLANK, jr.MISSING, jr.NOT_STRING, jr.BAD, jr.BAD, jr.BAD, jr.BAD, jr.OK]
    buf = b"\n".join(lines) + b"\n"
    r = check(enc, buf)
    assert r.status.tolist() == want_status
    got = enc.extract_jsonl(buf, on_error="skip")
    assert got.line.tolist() == [0, 8] and got.texts() == ["ok", "last"]
    got = enc.extract_jsonl(buf, on_error="empty")
    assert got.line.tolist() == [0, 2, 3, 4, 5, 6, 7, 8] and got.texts() == ["ok", "", "", "", "", "", "", "last"]
    before = enc._core_bpe.jsonl_extract_device(t_good.data_ptr(), t_good.numel())
    assert (before.n_docs, before.n_lines, before.n_text) == (2, 2, 13)
    with pytest.raises(JsonlError) as e:
        enc.extract_jsonl(buf)
    assert (e.value.line, e.value.pos, e.value.status) == (2, len(lines[0]) + len(lines[1]) + 2, jr.MISSING)
    want = jr.extract(good, b"text", jr.RAISE)
    assert (enc._from_device(t_good, before.text, before.n_text, "|u1") == want.text).all()
    assert (enc._from_device(t_good, before.doc_off, before.n_docs + 1, "<u8") == want.doc_off).all()
    assert (enc._from_device(t_good, before.line, before.n_docs, "<u8") == want.line).all()
    assert (enc._from_device(t_good, before.status, before.n_lines, "|u1") == want.status).all()
    same(enc.extract_jsonl(good), jr.extract(good, b"text", jr.RAISE), "after a refusal")
    for field in ("", "x" * 65, 'a"b', "a\\b"):
        with pytest.raises(ValueError):
            enc.extract_jsonl(good, field)
    with pytest.raises(ValueError):
        enc.extract_jsonl(good, on_error="ignore")


def test_skip_cannot_hide_a_failure():
    """at most 10 % of the lines are not OK, by construction and checked against the restatement; the status array is compared in full"""
    enc = enc_of()
    rng = random.Random(0x7503)
    buf = jc.buffer(rng, 4000, 0.08, final_newline=True, bom=False)
    want = jr.extract(buf, b"text", jr.SKIP)
    n_bad = int((want.status != jr.OK).sum())
    assert 0 < n_bad <= 400, n_bad
    got = enc.extract_jsonl(buf, on_error="skip")
    same(got, want, "skip")
    assert len(got.line) == 4000 - n_bad
    for field in ("t", "a b", "content"):
        check(enc, jc.buffer(rng, 300, 0.3, field), field, what=field)


def test_other_inputs_memoryview_bytearray_numpy_and_a_device_tensor():
    import torch

    enc = enc_of()
    rng = random.Random(0x7504)
    buf = jc.buffer(rng, 500, 0.1)
    want = jr.extract(buf, b"text", jr.SKIP)
    for data in (bytearray(buf), memoryview(buf), np.frombuffer(buf, np.uint8)):
        same(enc.extract_jsonl(data, on_error="skip"), want, type(data))
    t = torch.frombuffer(bytearray(buf), dtype=torch.uint8).to(f"cuda:{enc._core_bpe.device}")
    same(enc.extract_jsonl(t, on_error="skip"), want, "tensor")
    tok = enc.encode_ordinary_jsonl_packed(t, on_error="skip")
    ref_tok, ref_off = enc.encode_ordinary_batch_packed([x.decode("utf-8") for x in want.texts()])
    assert (np.asarray(tok.tokens) == ref_tok).all() and (np.asarray(tok.tok_off) == ref_off).all()


def test_encode_jsonl_equals_the_reference_route_on_mixed_scripts():
    enc = enc_of()
    rng = random.Random(0x7505)
    parts = []
    size = 0
    while size < (2 << 20):
        parts.append(jc.buffer(rng, 200, 0.05, final_newline=True, bom=False))
        size += len(parts[-1])
    buf = b"".join(parts)
    want = jr.extract(buf, b"text", jr.SKIP)
    texts = [x.decode("utf-8") for x in want.texts()]
    ref_tok, ref_off = enc.encode_ordinary_batch_packed(texts)
    got = enc.encode_ordinary_jsonl_packed(buf, on_error="skip")
    assert got.n_lines == len(want.status) and (got.status == want.status).all() and (got.line == want.line).all()
    assert (got.tok_off == ref_off).all() and (got.tokens == ref_tok).all()
    got = enc.encode_jsonl_packed(buf, on_error="skip", disallowed_special=())
    assert (got.tok_off == ref_off).all() and (got.tokens == ref_tok).all()


def test_encode_jsonl_special_tokens():
    enc = enc_of()
    buf = b'{"text":"plain"}\n\n{"id":3,"text":"before <|endoftext|> after"}\n'
    with pytest.raises(_tiktoken.DisallowedSpecialError) as e:
        enc.encode_jsonl_packed(buf)
    with pytest.raises(ValueError) as ref:
        enc.encode("before <|endoftext|> after")
    assert str(e.value) == str(ref.value) and e.value.line == 2 and e.value.doc == 1 and e.value.pos == 7
    got = enc.encode_jsonl_packed(buf, allowed_special="all")
    assert enc.eot_token in got.tokens.tolist() and got.line.tolist() == [0, 2]
    ref_tok, ref_off = enc.encode_batch_packed(["plain", "before <|endoftext|> after"], allowed_special="all")
    assert (got.tokens == ref_tok).all() and (got.tok_off == ref_off).all()
    got = enc.encode_jsonl_packed(buf, disallowed_special=())
    ref_tok, ref_off = enc.encode_ordinary_batch_packed(["plain", "before <|endoftext|> after"])
    assert (got.tokens == ref_tok).all() and (got.tok_off == ref_off).all()
