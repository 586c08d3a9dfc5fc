#!/usr/bin/env python3
"""Writes tests/golden/offsets.json.gz: token id lists of the three shaped vocabularies and what the reference's own
Encoding.decode_with_offsets (tiktoken/core.py:312-335) makes of them -- the text and the offset of every token.  Data only.

The reference's core.py is loaded from its source tree and run as it is; its Rust extension is not needed for this method: the one call it
makes into it, CoreBPE.decode_single_token_bytes, is answered from the vocabulary's own table.  The token lists come from this
repository's CPU oracle (prompts) or are written down as ids (byte-level tokens that split characters).

Usage: python tools/gen_golden_offsets.py REFERENCE_DIR   (a source tree of openai/tiktoken: REFERENCE_DIR/tiktoken/core.py)
"""
import gzip
import importlib.util
import json
import os
import random
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import helpers as h  # noqa: E402


class _TableCore:
    """What Encoding.decode_with_offsets asks of the extension class"""

    def __init__(self, ranks, specials):
        self._dec = {r: t for t, r in ranks.items()}
        self._dec.update({i: s.encode() for s, i in specials.items()})

    def decode_single_token_bytes(self, token):
        return self._dec[token]


pkg = types.ModuleType("tiktoken")
pkg.__path__ = [os.path.join(sys.argv[1], "tiktoken")]
ext = types.ModuleType("tiktoken._tiktoken")
ext.CoreBPE = _TableCore
pkg._tiktoken = ext
sys.modules["tiktoken"], sys.modules["tiktoken._tiktoken"] = pkg, ext
spec = importlib.util.spec_from_file_location("tiktoken.core", os.path.join(sys.argv[1], "tiktoken", "core.py"))
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

PROMPTS = [
    # the reference's tests/test_offsets.py
    "hello world", "hello world<|endoftext|> green cow", "我非常渴望与人工智能一起工作", "நடிகர் சூர்யா", " Ġ除",
    # CJK, Tamil, emoji, mixed
    "中文テキスト 한국어 텍스트", "தமிழ் மொழி ஒரு செம்மொழி", "😀😃 👩‍👩‍👧‍👦 🇩🇪 ok 👍🏽", "naïve café — “quotes” … ½ ²", "áé ǅ ſ ​ ",
    "The quick brown fox's 12345 jumps\n\n  over\tthe lazy dog.", "x" * 300, " ", "\n", "é",
    # special tokens
    "<|endoftext|>", "<|endoftext|><|endoftext|>", "a<|endoftext|>中<|endoftext|>😀", "<|endoftext|> tail",
]
UNITS = ["hello", " world", "中", "文", "é", "😀", "ந", "ி", " ", "\n", "1234", "<|endoftext|>", "’", "ǅ", "́", "x'll", "テキスト", "한"]

out = {"source": "Encoding.decode_with_offsets of openai/tiktoken 0.14.0 (tiktoken/core.py:312-335) on token lists of this repository's shaped vocabularies; "
                 "per case: tokens, text, offsets (text null: the reference raises UnicodeDecodeError)", "encodings": {}}
for name in h.ENCODING_NAMES:
    ranks, specials = h.load_vocab(name), h.SPECIALS[name]
    oracle = h.c_oracle_for(name)
    enc = object.__new__(ref.Encoding)
    enc._core_bpe = _TableCore(ranks, specials)
    lists = [[]]  # the empty document
    for p in PROMPTS:
        lists.append(oracle.encode(p.encode(), "all").tolist())
        lists.append(oracle.encode_ordinary(p.encode()).tolist())
    rng = random.Random(0x0FF5E7)
    for _ in range(40):
        text = "".join(rng.choice(UNITS) for _ in range(rng.randrange(1, 30)))
        lists.append(oracle.encode(text.encode(), "all").tolist())
    # byte-level ids: every byte of a char a token of its own, chars split between tokens in every way, with whole tokens around them
    byte_id = {b: ranks[bytes([b])] for b in range(256)}
    for text in ("é", "中", "😀", "aé中😀b", "நடி", "ǅ́"):
        lists.append([byte_id[b] for b in text.encode()])
        lists.append(oracle.encode_ordinary(b"hello") .tolist() + [byte_id[b] for b in text.encode()] + oracle.encode_ordinary(b" world").tolist())
    # ... and lists that are not valid UTF-8: a char cut off, a stray continuation byte, a continuation byte first
    lists += [[byte_id[0xE4], byte_id[0xB8]], [byte_id[0x80]], [byte_id[0x80], byte_id[0xBF], byte_id[0x41]], [byte_id[0x41], byte_id[0xC3]], [byte_id[0xF4], byte_id[0x90], byte_id[0x80], byte_id[0x80]]]
    cases, seen = [], set()
    for toks in lists:
        if tuple(toks) in seen:
            continue
        seen.add(tuple(toks))
        try:
            text, offsets = enc.decode_with_offsets(toks)
        except UnicodeDecodeError:
            text, offsets = None, None
        cases.append({"tokens": toks, "text": text, "offsets": offsets})
    out["encodings"][name] = cases
dst = os.path.join(ROOT, "tests", "golden", "offsets.json.gz")
with gzip.GzipFile(dst, "wb", mtime=0) as f:
    f.write(json.dumps(out, ensure_ascii=False, separators=(",", ":")).encode("utf-8"))
print({k: len(v) for k, v in out["encodings"].items()}, os.path.getsize(dst), "bytes ->", dst)
