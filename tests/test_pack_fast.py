"""Encoding._pack: the batch as UTF-8 back to back.  Byte for byte what the per-text form with a call per text gives (restated here), surrogate repair included (tiktoken/core.py:79,135), and the flag that says whether any text needed that repair."""
import numpy as np

import helpers as h  # noqa: F401  (puts the repository on sys.path)
from tiktoken_amd.core import Encoding


def old_pack(texts):
    """The per-text form: every text encoded on its own, lone surrogates replaced and pairs joined where the encode refuses them."""
    chunks, repaired = [], False
    for t in texts:
        try:
            chunks.append(t.encode("utf-8"))
        except UnicodeEncodeError:
            chunks.append(t.encode("utf-16", "surrogatepass").decode("utf-16", "replace").encode("utf-8"))
            repaired = True
    off = np.zeros(len(chunks) + 1, dtype=np.uint64)
    if chunks:
        np.cumsum(np.fromiter((len(c) for c in chunks), dtype=np.uint64, count=len(chunks)), out=off[1:])
    return np.frombuffer(b"".join(chunks), dtype=np.uint8), off, repaired


CASES = {
    "empty list": [],
    "one empty text": [""],
    "empty texts": ["", "", ""],
    "ascii": ["hello world", "The quick brown fox's 12345 jumps", "x" * 3000, "\x00\x7f"],
    "mixed utf-8": ["héllo", "中文テキスト", "😀 emoji 😀", "plain", "á", "\U0010FFFF߿ࠀ", ""],
    "empty around text": ["", "a", "", "", "é", ""],
    "special tokens are text here": ["<|endoftext|>", "a<|custom_1|>b"],
    "lone high surrogate": ["ok", "bad \ud83d end", "fine"],
    "lone low surrogate": ["\ude00", "x"],
    "surrogate pair as two code units": ["pair \ud83d\ude00 joined", "é"],
    "a pair split over two texts stays two lone ones": ["\ud83d", "\ude00"],
    "surrogates and everything else": ["", "\ud800", "中", "a" * 100, "\udfff\ud800", "\ud83d\ude00", "😀"],
}


def test_pack_equals_the_per_text_form():
    for name, texts in CASES.items():
        for seq in (texts, tuple(texts)):
            blob, off, repaired = Encoding._pack_repaired(seq)
            wb, wo, wr = old_pack(texts)
            assert blob.dtype == np.uint8 and off.dtype == np.uint64, name
            assert blob.tobytes() == wb.tobytes(), name
            assert np.array_equal(off, wo), name
            assert repaired is wr, name
            b2, o2 = Encoding._pack(seq)
            assert b2.tobytes() == wb.tobytes() and np.array_equal(o2, wo), name


def test_repair_flag():
    assert Encoding._pack_repaired(["a", "é", "😀"])[2] is False
    assert Encoding._pack_repaired([])[2] is False
    assert Encoding._pack_repaired(["a", "\ud83d"])[2] is True
    assert Encoding._pack_repaired(["\ud83d\ude00"])[2] is True


def test_pack_random_batches():
    import random

    rng = random.Random(11)
    units = ["a", "Z", " ", "\n", "é", "ß", "中", "文", "😀", "́", "<|endoftext|>", "\ud83d", "\ude00", "\x00", "word " * 9]
    for _ in range(400):
        pool = units if rng.random() < 0.3 else [u for u in units if not 0xD800 <= ord(u[0]) <= 0xDFFF]
        texts = ["".join(rng.choice(pool) for _ in range(rng.choice([0, 1, 3, 20, 200]))) for _ in range(rng.choice([0, 1, 2, 7, 40]))]
        blob, off, repaired = Encoding._pack_repaired(texts)
        wb, wo, wr = old_pack(texts)
        assert blob.tobytes() == wb.tobytes() and np.array_equal(off, wo) and repaired is wr, texts
