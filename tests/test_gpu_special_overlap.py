"""Allowed special tokens that overlap one another, are long, or are a single byte, end to end on the device: encode(...,
allowed_special=...) marks them in two passes (tk_k_spec_cand, tk_k_spec_resolve) whose overlap rule -- the head walk in both its forms,
the greedy walk, "candidate not taken" -- no special token of the form <|...|> ever reaches.  The case list is that of
tests/spec_mark_ref.py, (a) - (g), which tests/test_spec_mark_sim.py runs through the CPU simulation, plus (h): tile and chunk ends.

Every token and every token offset is compared with the oracle (oracle/tk_oracle.c, COracle.encode_batch); under the vocabulary of the 256
single bytes also with a plain walk (at each position the longest allowed special token that matches, else one byte); the decoded tokens
are the text; every token's byte start (encode_batch_spans_packed) is the sum of the decoded lengths before it.  Every check asserts that
the marking passes ran ("spec_mark_launches").

Vocabularies: "bytes" (256 ids, GPT-2 pattern); "edu600" (trained: a special token inside a word cuts it into two haystacks); "generic" (the
256 bytes under a pat_str outside the scanner families: the generic engine takes the marks through TK_RX_CODE_ESC; under this vocabulary
the ids are the bytes whatever the split, so the same oracle holds)."""
import os

import numpy as np
import pytest

import helpers as h
import spec_mark_ref as ref
from test_regex_engine import PATTERNS

pytestmark = pytest.mark.gpu

BYTES = {bytes([b]): b for b in range(256)}
GENERIC_PAT = PATTERNS[5][0]
VOCABS = ("bytes", "edu600", "generic")
TILE = 3840


class Pair:
    """A core and the oracle for the same vocabulary and special tokens."""

    def __init__(self, vocab: str, specials: dict, chunk_bytes: int | None = None):
        from tiktoken_amd import CoreBPE

        ranks = h.golden_vocab("edu600") if vocab == "edu600" else BYTES
        assert max(ranks.values()) < ref.FIRST_ID
        self.plain = vocab != "edu600"
        self.specials = dict(specials)
        self.C = h.c_oracle.COracle(0, ranks, specials)
        old = os.environ.get("TIKTOKEN_AMD_CHUNK_BYTES")
        if chunk_bytes:
            os.environ["TIKTOKEN_AMD_CHUNK_BYTES"] = str(chunk_bytes)
        try:
            self.core = CoreBPE(ranks, specials, GENERIC_PAT if vocab == "generic" else h.PAT_STR[0])
        finally:
            if chunk_bytes:
                if old is None:
                    del os.environ["TIKTOKEN_AMD_CHUNK_BYTES"]
                else:
                    os.environ["TIKTOKEN_AMD_CHUNK_BYTES"] = old
        self.len_of = np.zeros(ref.FIRST_ID + len(specials), np.int64)
        for t, r in ranks.items():
            self.len_of[r] = len(t)
        for s, i in specials.items():
            self.len_of[i] = len(s.encode())

    def close(self):
        self.core.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def marks(self) -> int:
        return self.core.stat("spec_mark_launches")

    def check(self, docs: list[bytes], allowed, what="", plain=None):
        """One batch through encode_batch_packed, decode_batch_packed and encode_batch_spans_packed; returns the ids.
        plain: the plain walk's ids, where the caller has them."""
        blob, off = h.pack(docs)
        allowed = set(allowed)
        before = self.marks()
        toks, toff = self.core.encode_batch_packed(blob, off, allowed)
        assert self.marks() > before, (what, "the marking passes did not run")
        rt, ro = self.C.encode_batch(blob, off, allowed, 8)
        if not (np.array_equal(toff, ro) and np.array_equal(toks, rt)):
            d = next(d for d in range(len(docs)) if toks[int(toff[d]):int(toff[d + 1])].tolist() != rt[int(ro[d]):int(ro[d + 1])].tolist())
            raise AssertionError((what, "document", d, docs[d][:100], "got", toks[int(toff[d]):int(toff[d + 1])].tolist()[:60], "want",
                                  rt[int(ro[d]):int(ro[d + 1])].tolist()[:60]))
        if self.plain:
            walk = plain if plain is not None else [t for d in docs for t in ref.plain_walk(d, self.specials, allowed)]
            assert toks.tolist() == walk, (what, "the oracle and the plain walk disagree")
        data, boff = self.core.decode_batch_packed(toks, toff)
        assert data == blob.tobytes() and np.array_equal(boff, off), (what, "decode")
        before = self.marks()
        st, so, bs, _ = self.core.encode_batch_spans_packed(blob, off, allowed)
        assert self.marks() > before, (what, "the marking passes did not run (spans)")
        assert np.array_equal(st, rt) and np.array_equal(so, ro), (what, "spans: ids")
        lens = self.len_of[toks]
        want_start = np.cumsum(lens) - lens - np.repeat(off[:-1].astype(np.int64), np.diff(toff.astype(np.int64)))
        assert np.array_equal(bs.astype(np.int64), want_start), (what, "spans: byte starts")
        return toks


FORMS = ("", "+65", "+66")  # (c): the core as the case states it; with a 65-byte special token as well; with a 66-byte one


def in_form(c: ref.Case, form: str) -> ref.Case:
    return c if not form else c.also({"+65": ref.NEVER65, "+66": ref.NEVER66}[form], form)


def run_case(vocab: str, c: ref.Case, form: str = ""):
    """One case in one core.  (c): in a core with a 65- or 66-byte special token that occurs nowhere the ids are those of the core
    without it -- asserted against the oracle for the case as it stands, whichever tests ran before."""
    v = in_form(c, form)
    with Pair(vocab, v.specials) as p:
        got = p.check(v.docs, v.allowed, (vocab, v.name))
    if form:
        ranks = h.golden_vocab("edu600") if vocab == "edu600" else BYTES
        want, _ = h.c_oracle.COracle(0, ranks, c.specials).encode_batch(*h.pack(c.docs), set(c.allowed), 8)
        assert np.array_equal(got, want), (vocab, v.name, "the forms of the head walk disagree")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("vocab", VOCABS)
def test_exhaustive_documents(vocab, form):
    """(a), (c): every string over {a, b} of up to 12 bytes as a document, three allowed sets"""
    for c in ref.cases_a():
        run_case(vocab, c, form)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k", range(3))
@pytest.mark.parametrize("vocab", VOCABS)
def test_exhaustive_joined(vocab, k, form):
    """(a), (c): the same strings as ONE document behind 0 .. 70 bytes: every cluster at every alignment to the sixteen-byte lanes and the
    words of the bitmaps, with the head of the cluster below and above position 64"""
    v = in_form(ref.Case("a: joined", ref.S3, ref.S3_ALLOWED[k], []), form)
    walk0 = ref.plain_walk(ref.joined_a(0).encode(), v.specials, v.allowed)
    plain_core = h.c_oracle.COracle(0, h.golden_vocab("edu600") if vocab == "edu600" else BYTES, {s: v.specials[s] for s in ref.S3})
    with Pair(vocab, v.specials) as p:
        for pre in ref.JOINED_PREFIXES:  # ('c' is in no special token: the plain walk of the prefixed document is the prefix, then that of the rest)
            doc = ref.joined_a(pre).encode()
            got = p.check([doc], v.allowed, (vocab, v.name, pre), plain=[ord("c")] * pre + walk0)
            if form:  # (c): the ids of the core without the extra special token
                assert np.array_equal(got, plain_core.encode_batch(*h.pack([doc]), set(ref.S3_ALLOWED[k]), 1)[0]), (vocab, v.name, pre)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k", range(3))
@pytest.mark.parametrize("vocab", VOCABS)
def test_runs(vocab, k, form):
    """(b), (c): runs of one byte, 1 .. 4 096 long (the bound on a cluster in these tests: the head walk is quadratic in it), special tokens
    aa, aaa and both, behind 0, 1, 15, 16, 63 and 64 other bytes"""
    run_case(vocab, ref.cases_b()[k], form)


@pytest.mark.parametrize("k", range(len(ref.cases_d())))
@pytest.mark.parametrize("vocab", VOCABS)
def test_long_special_tokens(vocab, k):
    """(d) long special tokens that overlap themselves: up to 201 bytes, longer than a tile's look-ahead"""
    run_case(vocab, ref.cases_d()[k])


@pytest.mark.parametrize("group", ["e", "f", "g"])
@pytest.mark.parametrize("vocab", VOCABS)
def test_small_cases(vocab, group):
    """(e) document starts; (f) odd bytes; (g) prefixes -- there the reference's own choice depends on hash order: what is
    expected is the oracle's rule, the longest allowed special token"""
    for c in getattr(ref, "cases_" + group)():
        run_case(vocab, c)


def test_encoding_api():
    """The same through Encoding.encode and Encoding.encode_batch."""
    from tiktoken_amd import Encoding

    for c in ref.cases_g() + ref.cases_f():
        enc = Encoding("overlap_test", pat_str=h.PAT_STR[0], mergeable_ranks=BYTES, special_tokens=c.specials)
        core = enc._core_bpe
        texts = [d.decode() for d in c.docs]
        before = core.stat("spec_mark_launches")
        got = enc.encode_batch(texts, allowed_special=set(c.allowed), disallowed_special=())
        assert core.stat("spec_mark_launches") > before
        assert got == [ref.plain_walk(d, c.specials, c.allowed) for d in c.docs], c.name
        for t, d, g in zip(texts, c.docs, got):
            want = ref.plain_walk(d, c.specials, c.allowed)
            if any(i >= ref.FIRST_ID for i in want):
                before = core.stat("spec_mark_launches")
                assert enc.encode(t, allowed_special=set(c.allowed), disallowed_special=()) == want, (c.name, t[:60])
                assert core.stat("spec_mark_launches") > before
            assert enc.decode(g) == t
        core.close()


def edge_docs():
    """(h) each long special token of (d) and a cluster of (a) in a document of its own, placed so that they start 1, 2, len - 1 and len
    bytes before position 3 840 k of the document (a tile's end when the document starts a batch or a chunk), k = 1, 2."""
    toks = [ref.xy(ln) for ln in ref.XY_LENGTHS] + ["b" * 70]
    things = [(t, t) for t in toks] + [("aa", "abaababaabab"), ("bab", "babababaabaa")]
    docs = []
    for tok, text in things:
        for k in (1, 2):
            for back in (1, 2, len(tok) - 1, len(tok)):
                docs.append("." * (TILE * k - back - 7) + " filler" + text + " .")
                assert docs[-1].index(text) == TILE * k - back
    return toks + ref.S3, docs


@pytest.mark.parametrize("vocab", VOCABS)
def test_tile_ends_and_chunk_ends(vocab):
    """(h), device only.  Special tokens across tile ends: all placements as one batch, and that batch with chunks of 4 096 bytes --
    documents are never cut, so each of these documents is a chunk of its own and its special token lies 1, 2, len - 1 and len bytes before
    the chunk's position 3 840 k; then documents that end exactly at and one byte around a chunk's end."""
    specials, docs = edge_docs()
    case = ref.Case("h: tile ends", specials, specials, docs)
    assert sum(len(d) for d in case.docs) < 1 << 20
    with Pair(vocab, case.specials) as p:
        whole = p.check(case.docs, case.allowed, (vocab, case.name))
    with Pair(vocab, case.specials, chunk_bytes=4096) as p:
        assert p.core.stat("chunk_bytes") == 4096
        cut = p.check(case.docs, case.allowed, (vocab, case.name, "chunks"))
        assert p.core.stat("chunks") == len(case.docs)
        assert np.array_equal(cut, whole)
        for delta in (-1, 0, 1):  # documents of 4 096 + delta bytes that end with a cluster, and start with the rest of one
            ends = [("." * (4096 + delta - len(t)) + t) for t in ("abaababaabab", "b" * 70, ref.xy(201), "aa")]
            batch = [d.encode() for pair in zip(ends, ["ababaab" + "." * 50, "b" * 69 + ".", ref.xy(67)[1:], "a"]) for d in pair]
            p.check(batch, case.allowed, (vocab, "chunk end", delta))
            assert p.core.stat("chunks") > 1


def test_named_regressions():
    """Inputs on which the device was found wrong once, by name (the CPU file has the same list)."""
    from test_spec_mark_sim import REGRESSIONS

    for c in REGRESSIONS:
        run_case("bytes", c)
    with Pair("bytes", {"aa": ref.FIRST_ID}) as p:  # (so that this test, too, sees the marking passes run while the list is empty)
        p.check([b"aaa"], ["aa"], "aaa")
