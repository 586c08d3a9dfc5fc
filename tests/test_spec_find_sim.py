"""The device scan for a disallowed special token (tk_k_spec_find) on the CPU: tests/hostsim/spec_find_sim.cpp compiles the kernel's
per-thread body (tk_special.h) for the host and runs it lane by lane over packed batches.  The answer -- where in the batch the
first disallowed special token starts -- is compared with the reference's own search (tiktoken/core.py:116-124): the first
document, in order, in which `_special_token_regex(disallowed).search(text)` finds something, and the match's start as a byte offset."""
import ctypes
import random

import numpy as np
import pytest

import helpers as h
from oracle import c_oracle
from tiktoken_amd.core import _special_token_regex

NONE = (1 << 64) - 1
_lib = None


def lib():
    global _lib
    if _lib is None:
        L = h.build_sim("libspec_find_sim.so", ("spec_find_sim.cpp", "tk_tables.cpp", "tk_pattern.cpp", "tk_regex.cpp", "tk_special.h", "tk_device.h", "tk_common.h",
                                                "tk_tables.h", "tk_regex.h", "tk_regex_host.h"), ("-pthread",))
        vp, u64 = ctypes.c_void_p, ctypes.c_uint64
        L.sfs_create.restype = vp
        L.sfs_create.argtypes = [vp, vp, vp, u64, vp, vp, vp, u64, ctypes.c_char_p, ctypes.c_char_p, u64]
        L.sfs_destroy.argtypes = [vp]
        L.sfs_first_bytes.restype = ctypes.c_uint32
        L.sfs_first_bytes.argtypes = [vp]
        L.sfs_find.restype = u64
        L.sfs_find.argtypes = [vp, vp, u64, vp, u64, u64, vp, u64, vp, vp]
        _lib = L
    return _lib


class Sim:
    """The scan over the special tokens `specials` (a vocabulary of the 256 single bytes: the scan never looks at it)."""

    def __init__(self, specials: dict[str, int]):
        self.specials = dict(specials)
        rb, ro, ri = c_oracle._pack([(bytes([b]), b) for b in range(256)])
        sb, so, si = c_oracle._pack([(k.encode(), v) for k, v in specials.items()])
        err = ctypes.create_string_buffer(512)
        self._h = lib().sfs_create(rb.ctypes.data, ro.ctypes.data, ri.ctypes.data, len(ri), sb.ctypes.data, so.ctypes.data, si.ctypes.data, len(si),
                                   h.PAT_STR[2].encode(), err, 512)
        if not self._h:
            raise ValueError(err.value.decode())

    def __del__(self):
        if getattr(self, "_h", None):
            lib().sfs_destroy(self._h)

    def first_bytes(self) -> int:
        return lib().sfs_first_bytes(self._h)

    def find(self, docs: list[bytes], disallowed, order=None, d0=0, d1=None):
        """(doc, pos, id, len) of the first hit in documents [d0, d1) run as ONE chunk of the batch `docs` (document numbers and offsets
        are the batch's), or None."""
        blob, off = h.pack(docs)
        d1 = len(docs) if d1 is None else d1
        base, end = int(off[d0]), int(off[d1])
        text = np.ascontiguousarray(blob[base:end]) if end > base else np.zeros(1, np.uint8)
        sub = np.ascontiguousarray(off[d0:d1 + 1])
        ids = np.asarray([self.specials[s] for s in disallowed] or [0], np.uint32)
        lanes = None
        if order is not None:
            lanes = np.arange((end - base + 15) // 16, dtype=np.uint64)
            random.Random(order).shuffle(lanes)
        out = np.zeros(2, np.uint32)
        r = lib().sfs_find(self._h, text.ctypes.data, end - base, sub.ctypes.data, d1 - d0, base, ids.ctypes.data, len(disallowed),
                           lanes.ctypes.data if lanes is not None else None, out.ctypes.data)
        if r == NONE:
            return None
        assert base <= r < end
        doc = int(np.searchsorted(off, r, side="right")) - 1
        return doc, r - int(off[doc]), int(out[0]), int(out[1])


def expected(specials, docs: list[bytes], disallowed, d0=0, d1=None):
    rx = _special_token_regex(frozenset(disallowed))
    for d in range(d0, len(docs) if d1 is None else d1):
        text = docs[d].decode("utf-8")
        m = rx.search(text)
        if m:
            rest = text[m.start():]
            tok = max((s for s in disallowed if rest.startswith(s)), key=lambda s: len(s.encode()))
            return d, len(text[:m.start()].encode("utf-8")), specials[tok], len(tok.encode())
    return None


def check(sim: Sim, docs, disallowed, **kw):
    docs = [d.encode() if isinstance(d, str) else d for d in docs]
    want = expected(sim.specials, docs, disallowed, kw.get("d0", 0), kw.get("d1"))
    for order in (None, 1, 2):  # (the kernel's threads run in no particular order)
        got = sim.find(docs, disallowed, order=order, **kw)
        assert got == want, (got, want, disallowed, [d[:80] for d in docs][:6])
    return want


@pytest.fixture(scope="module")
def sim8():
    return Sim(h.CUSTOM8)


ALL8 = sorted(h.CUSTOM8)


def test_no_hit_and_decoys(sim8):
    assert check(sim8, ["plain text, nothing special " * 40, "", "a < b <| c |> d"], ALL8) is None
    # helpers.insert_specials' decoys: an unregistered token, truncated tokens, bare delimiters
    decoys = ["<|custom_9|>", "<|endoftext", "<|custom_3|", "<|", "|>", "<|custom_|>", "<|endoftext|", "<<||custom_1||>>", "<|Custom_1|>"]
    assert check(sim8, [" x ".join(decoys) * 7, "".join(decoys), "<"], ALL8) is None
    assert check(sim8, [], ALL8) is None
    assert check(sim8, ["", "", ""], ALL8) is None
    # a registered token that is not in the disallowed set is no hit; the others still are
    assert check(sim8, ["a <|custom_1|> b"], [t for t in ALL8 if t != "<|custom_1|>"]) is None
    assert check(sim8, ["a <|custom_1|> b <|custom_2|>"], ["<|custom_2|>"]) == (0, 17, h.CUSTOM8["<|custom_2|>"], 12)


def test_hit_positions(sim8):
    tok = "<|custom_4|>"
    filler = "The quick brown fox. " * 30
    assert check(sim8, [tok + filler], ALL8)[:2] == (0, 0)  # byte 0
    assert check(sim8, [filler + tok], ALL8)[:2] == (0, len(filler))  # the last possible byte
    assert check(sim8, [filler, filler, filler + tok], ALL8)[:2] == (2, len(filler))  # ... of the batch
    assert check(sim8, [filler[:100] + tok + filler, filler, filler], ALL8)[0] == 0  # first / middle / last document
    assert check(sim8, [filler, filler[:333] + tok + filler, filler], ALL8)[:2] == (1, 333)
    assert check(sim8, [filler, filler, "é中😀" + tok], ALL8)[:2] == (2, 9)
    # two offending documents: the earlier one; two hits in a document: the earlier one
    assert check(sim8, [filler, "x" + tok, filler, tok], ALL8)[:2] == (1, 1)
    assert check(sim8, [filler + "<|endoftext|>" + filler + tok], ALL8)[:2] == (0, len(filler))
    # empty documents around the hit
    assert check(sim8, ["", "", tok, "", ""], ALL8)[:2] == (2, 0)
    assert check(sim8, ["", filler, "", "", "ab" + tok, ""], ALL8)[:2] == (4, 2)


def test_token_split_across_documents_is_no_hit(sim8):
    tok = "<|custom_4|>"
    for cut in range(1, len(tok)):
        assert check(sim8, ["abc" + tok[:cut], tok[cut:] + "def"], ALL8) is None
        assert check(sim8, ["abc" + tok[:cut], "", tok[cut:] + "def"], ALL8) is None
    # ... and a whole one right behind the broken one is found
    assert check(sim8, ["abc<|custom", "_4|>" + tok], ALL8)[:2] == (1, 4)


def test_every_alignment_of_the_lane(sim8):
    tok = "<|custom_7|>"
    for a in range(0, 40):  # (0 .. 15 inside a lane; from 5 on the token crosses into the next lane)
        assert check(sim8, ["." * a + tok + "." * 50], ALL8)[:2] == (0, a)
        assert check(sim8, ["." * 37, "." * a + tok], ALL8)[:2] == (1, a)  # (the document, and so the lanes, start at an odd offset)
    # the first byte is a lane's last: the second byte is the one read behind the sixteen
    assert check(sim8, ["." * 15 + tok], ALL8)[:2] == (0, 15)
    assert check(sim8, ["." * 31 + tok], ALL8)[:2] == (0, 31)


def test_chunks_of_a_batch(sim8):
    """A chunk of a larger batch: offsets are the batch's (`base` is added); the text behind the chunk's end -- the next document --
    is not part of a match."""
    tok = "<|custom_2|>"
    docs = ["a" * 100, "b" * 50 + tok[:5], tok[5:] + "c" * 20, "d" * 10 + tok]
    assert check(sim8, docs, ALL8, d0=0, d1=2) is None  # (the token's halves: end of this chunk's last document / start of the next chunk's first)
    assert check(sim8, docs, ALL8, d0=2, d1=3) is None
    assert check(sim8, docs, ALL8, d0=2, d1=4)[:2] == (3, 10)
    assert check(sim8, docs, ALL8, d0=3, d1=4)[:2] == (3, 10)  # a hit that ends on the chunk's last byte
    assert check(sim8, docs, ALL8)[:2] == (3, 10)


def test_more_than_four_first_bytes_takes_the_bitset():
    specials = {"<|a|>": 1000, "[SEP]": 1001, "{pad}": 1002, "#eos#": 1003, "@@bos": 1004, "«fin»": 1005}
    sim = Sim(specials)
    assert sim.first_bytes() == 0xFF
    assert Sim(h.CUSTOM8).first_bytes() == 1
    every = sorted(specials)
    assert check(sim, ["nothing [SEP here {pad #eos @bos «fin"], every) is None
    for tok in every:
        for a in (0, 3, 15, 16, 29):
            assert check(sim, ["x" * a + tok + " tail"], every)[:2] == (0, a)
            assert check(sim, ["x" * a + tok + " tail"], [t for t in every if t != tok]) is None
    assert check(sim, ["a@@bos", "{pad}[SEP]"], ["[SEP]", "{pad}"])[:2] == (1, 0)


def test_long_special_tokens():
    """Longer than the 32 bytes tk_special_at compares word by word, and 66 bytes and more."""
    specials = {"<|endoftext|>": 1, "<|" + "r" * 40 + "|>": 2, "<|" + "long_" * 14 + "|>": 3, "<|" + "z" * 100 + "|>": 4}
    assert sorted(len(s) for s in specials) == [13, 44, 74, 104]
    sim = Sim(specials)
    every = sorted(specials)
    for tok in every:
        for a in (0, 1, 15, 16, 17, 40):
            assert check(sim, ["pre", "y" * a + tok], every) == (1, a, specials[tok], len(tok))
            assert check(sim, ["y" * a + tok[:-1]], every) is None  # one byte short
            assert check(sim, ["y" * a + tok[:-1] + "x" + tok[-1]], every) is None
            for cut in (1, len(tok) // 2, len(tok) - 1):
                assert check(sim, ["y" * a + tok[:cut], tok[cut:]], every) is None


def test_nested_tokens_report_the_longest():
    specials = {"<|a|>": 10, "<|a|><|b|>": 11, "<|a": 12, "<|a|><|b|>x" + "y" * 30: 13, "|>": 14}
    sim = Sim(specials)
    every = sorted(specials)
    assert check(sim, ["..<|a|>.."], every) == (0, 2, 10, 5)
    assert check(sim, ["..<|a|><|b|>.."], every) == (0, 2, 11, 10)
    assert check(sim, ["..<|a|><|b|>x" + "y" * 30], every) == (0, 2, 13, 41)
    assert check(sim, ["..<|a|><|b|>x" + "y" * 29], every) == (0, 2, 11, 10)
    assert check(sim, ["..<|a|><|b|", ">"], every) == (0, 2, 10, 5)  # (the longer one would cross into the next document)
    assert check(sim, ["..<|a|><|b|>"], ["<|a|><|b|>", "<|a"]) == (0, 2, 11, 10)
    assert check(sim, ["..<|a|><|b|>"], ["<|a"]) == (0, 2, 12, 3)
    assert check(sim, ["..<|a|><|b|>"], ["|>"]) == (0, 5, 14, 2)
    assert check(sim, ["..<|", "a|>"], every) == (1, 1, 14, 2)


def test_fuzzed_batches(sim8):
    rng = random.Random(0xD15A)
    splice = ALL8 + ["<|custom_9|>", "<|endoftext", "<|custom_3|", "<|", "|>"]
    hits = 0
    for seed in range(3000):
        docs = [d.decode() for d in h.fuzz_batch(0xF00D + seed, 4096)]
        for _ in range(rng.choice([0, 0, 1, 1, 2, 5])):
            d = rng.randrange(len(docs))
            at = rng.randrange(len(docs[d]) + 1)
            docs[d] = docs[d][:at] + rng.choice(splice) + docs[d][at:]
        disallowed = ALL8 if rng.random() < 0.5 else rng.sample(ALL8, rng.randrange(1, len(ALL8)))
        docs = [d.encode() for d in docs]
        want = expected(h.CUSTOM8, docs, disallowed)
        got = sim8.find(docs, disallowed, order=seed if seed % 2 else None)
        assert got == want, (seed, got, want, disallowed)
        hits += want is not None
        if len(docs) > 2:  # the same batch as two chunks: the first chunk with a hit holds the batch's first
            cut = rng.randrange(1, len(docs))
            a = sim8.find(docs, disallowed, d0=0, d1=cut)
            assert (a if a is not None else sim8.find(docs, disallowed, d0=cut)) == want, (seed, cut)
    assert 300 < hits < 2700, hits
