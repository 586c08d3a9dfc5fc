"""The bucketed whole-piece tables (tk_common.h, "bucketed tables") on the device: the o200k- and cl100k-shaped vocabularies and the
collision vocabulary of tests/probe_vocab.py on texts of one, two and three tiles and on one tile of more than 896 pieces (the batched
lists), made of tokens, near-misses of tokens in every length class and strings of the colliding buckets.  Every token and every offset
equals the C oracle's -- as a batch (tk_k_front), as small calls (tk_k_small) and as single documents.  The CPU side:
tests/test_probe_buckets_sim.py."""
import functools
import re

import numpy as np
import pytest

import helpers as h
import probe_vocab as pv
from oracle import c_oracle

pytestmark = pytest.mark.gpu

VOCABS = ("o200k_shaped", "cl100k_shaped", "collision")
PAT_ID = {"o200k_shaped": 2, "cl100k_shaped": 1, "collision": 2}
WORD = re.compile(rb" ?[a-z]+")


@functools.lru_cache(maxsize=None)
def vocab_of(name):
    """(ranks, specials, the tokens the text is made of, strings of the colliding buckets)"""
    if name == "collision":
        ranks, colliding, absent, _ = pv.collision_vocab()
        return ranks, {}, ranks, [t for c in pv.CLASSES for t in colliding[c] + absent[c]]
    g, ranks = h.load_golden(name), h.golden_vocab(name)
    words = {t: r for t, r in ranks.items() if 2 <= len(t) <= 23 and WORD.fullmatch(t)}
    per_class = [[t for t in words if lo <= len(t) <= hi][:400] for lo, hi in pv.CLASSES.values()]
    assert all(len(c) == 400 for c in per_class)
    return ranks, g["special_tokens"], {t: words[t] for c in per_class for t in c}, []


@functools.lru_cache(maxsize=None)
def encoding_of(name):
    from tiktoken_amd import Encoding

    ranks, specials, _, _ = vocab_of(name)
    return Encoding("probe-" + name, pat_str=h.PAT_STR[PAT_ID[name]], mergeable_ranks=ranks, special_tokens=specials)


@functools.lru_cache(maxsize=None)
def docs_of(name):
    """Texts of one, two and three tiles, one tile of short pieces alone (more than 896 of them), one small document"""
    _, _, words, extra = vocab_of(name)
    docs = [pv.text_of(words, extra, k * pv.TILE, 10 + k) for k in (1, 2, 3)]
    docs.append(pv.text_of(words, [t for t in extra if len(t) <= 4], pv.TILE, 20, short_only=True))
    docs.append(pv.text_of(words, extra, 1500, 30))
    assert [-(-len(d) // pv.TILE) for d in docs[:4]] == [1, 2, 3, 1]
    return tuple(docs)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The oracle's (tokens, tok_off) of the packed documents: computed once per vocabulary, never written to"""
    ranks, specials, _, _ = vocab_of(name)
    C = c_oracle.COracle(PAT_ID[name], ranks, specials)
    docs = docs_of(name)
    assert len(C.split(docs[3])) >= 897  # (one tile: the lists of 896 go round more than once)
    for cls, (lo, hi) in pv.CLASSES.items():  # tokens and pieces that are not tokens, in every length class
        pieces = [p for d in docs[:3] for p in (d[a:b] for a, b in zip([0] + C.split(d)[:-1], C.split(d))) if lo <= len(p) <= hi]
        assert sum(p in ranks for p in pieces) >= 20 and sum(p not in ranks for p in pieces) >= 20, (name, cls)
    blob, off = h.pack(list(docs))
    toks, toff = C.encode_batch(blob, off)
    toks, toff = np.asarray(toks), np.asarray(toff)
    toks.setflags(write=False)
    toff.setflags(write=False)
    return blob, off, toks, toff


@pytest.mark.parametrize("name", VOCABS)
def test_batch_equals_the_oracle(name):
    blob, off, toks, toff = reference(name)
    got_toks, got_off = encoding_of(name)._core_bpe.encode_batch_packed(blob, off)
    assert np.array_equal(got_off, toff), np.flatnonzero(np.asarray(got_off) != toff)[:5].tolist()
    assert np.array_equal(got_toks, toks), np.flatnonzero(np.asarray(got_toks)[: len(toks)] != toks[: len(got_toks)])[:5].tolist()


@pytest.mark.parametrize("name", VOCABS)
def test_single_documents_and_a_small_call_equal_the_oracle(name):
    """Each text as a call of its own; the last, of 1500 bytes, is one call of the one-launch path (tk_k_small)"""
    _, _, toks, toff = reference(name)
    core = encoding_of(name)._core_bpe
    docs = docs_of(name)
    for d, doc in enumerate(docs):
        before = core.stat("small_calls")
        assert core.encode_ordinary(doc.decode()) == toks[int(toff[d]):int(toff[d + 1])].tolist(), (name, d)
        if len(doc) <= 2048:  # (the longer ones are cut into segments, which take the same kernel several at a time)
            assert core.stat("small_calls") - before == 1, (name, d)
