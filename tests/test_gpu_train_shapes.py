"""BPE training on the device where only the device can go wrong: the corpora of tests/train_shapes.py (tests/test_train_shapes.py shows
on the CPU what each of them is sensitive to) through train_bpe_packed, on a core with the default chunk size and on one with chunks of
4096 bytes, pairs and counts equal to the restatement's (tests/train_ref.py), step by step.

Paths these tests run on the device that the CPU simulation (tests/test_train_sim.py) runs one lane at a time only:
  - tk_k_train_rehash and the copy of train_blob_reserve: a table and a blob that grow between chunks (`growth`; the launches and the
    "train_table_moves" / "train_blob_moves" figures of tk_stat are asserted), weights and first offsets carried over;
  - tk_train_word_slot's "same length, other bytes: move on" under racing claims: 160 words of 80 bytes with one tk_train_hash, keys
    that name the chunk's text beside keys that name the blob, the chain moved by a rehash (`long_collide`), and the lengths at which
    the hash changes its form or reads a partial word (63 .. 97);
  - gap chars at the first and last byte of documents and chunks, documents and a whole chunk of nothing else (`gaps`);
  - steps decided by the position key between pairs that stand in different chunks (`ties`);
  - the step in "no pair left to merge after K of N merges", the partial result, and the call after the error (`exhaust`);
  - chunk edges (a document of exactly a chunk, a cut behind an empty document), and a seeded sweep over small alphabets under the three
    stock patterns, a pattern with gap chars and the whole-document pattern.
Left uncovered: weights and counts above 2^32 (the CPU simulation has a case), and the grid-stride loops of tk_k_train_words /
tk_k_train_blob / tk_k_train_rehash beyond 65 536 workgroups, which need corpora far above a test's size."""
import os
import re

import numpy as np
import pytest

import train_ref as tr
import train_shapes as ts
from test_gpu_train import pack

pytestmark = pytest.mark.gpu

SMALL = 4096


def make_core(pat_str, chunk_bytes):
    from tiktoken_amd import CoreBPE

    if chunk_bytes is None:
        c = CoreBPE({bytes([b]): b for b in range(256)}, {}, pat_str)
        assert c.stat("chunk_bytes") > 40000  # (every corpus here is one chunk)
        return c
    old = os.environ.get("TIKTOKEN_AMD_CHUNK_BYTES")
    os.environ["TIKTOKEN_AMD_CHUNK_BYTES"] = str(chunk_bytes)
    try:
        c = CoreBPE({bytes([b]): b for b in range(256)}, {}, pat_str)
    finally:
        if old is None:
            del os.environ["TIKTOKEN_AMD_CHUNK_BYTES"]
        else:
            os.environ["TIKTOKEN_AMD_CHUNK_BYTES"] = old
    assert c.stat("chunk_bytes") == chunk_bytes
    return c


@pytest.fixture(scope="module")
def cores():
    """core(pat_str, chunk_bytes or None): one core per pattern and chunk size for the whole module"""
    made = {}

    def core(pat_str, chunk_bytes):
        if (pat_str, chunk_bytes) not in made:
            made[pat_str, chunk_bytes] = make_core(pat_str, chunk_bytes)
        return made[pat_str, chunk_bytes]

    yield core
    for c in made.values():
        c.close()


BOTH = pytest.mark.parametrize("chunk_bytes", [None, SMALL], ids=["one_chunk", "chunks_4096"])


@pytest.fixture(scope="module")
def wanted():
    """the restatement's answer per corpus, computed once: Trained, or the Exhausted it raised"""
    memo = {}

    def want(key, docs, n_merges, pat_str):
        if key not in memo:
            try:
                memo[key] = tr.train_text(docs, 256 + n_merges, pat_str)
            except tr.Exhausted as e:
                memo[key] = e
        return memo[key]

    return want


def check(core, docs, n_merges, want, what=""):
    """train_bpe_packed gives the restatement's pairs and counts, or fails at the restatement's step"""
    if isinstance(want, tr.Exhausted):
        with pytest.raises(ValueError, match=rf"no pair left to merge after {want.done} of {n_merges} merges") as e:
            core.train_bpe_packed(*pack(docs), 256 + n_merges)
        return str(e.value)
    pairs, counts = core.train_bpe_packed(*pack(docs), 256 + n_merges)
    assert pairs.dtype == np.uint32 and pairs.shape == (n_merges, 2) and counts.dtype == np.uint64 and counts.shape == (n_merges,)
    got = [tuple(p) for p in pairs.tolist()]
    bad = next((k for k in range(n_merges) if got[k] != want.pairs[k] or int(counts[k]) != want.counts[k]), None)
    assert bad is None, (what, "step", bad, got[bad], int(counts[bad]), "want", want.pairs[bad], want.counts[bad])
    return None


def run(cores, wanted, c: ts.Corpus, chunk_bytes, docs=None, key=None):
    docs = c.docs if docs is None else docs
    core = cores(c.pat_str, chunk_bytes)
    check(core, docs, c.n_merges, wanted(key or c.name, docs, c.n_merges, c.pat_str), c.name)
    return core


@BOTH
def test_growth(cores, wanted, chunk_bytes):
    """Chunks of 4096 bytes: the table is moved at least twice and the blob at least once, and weights and first offsets survive (lost ones
    change the merges: test_train_shapes.py).  One chunk: nothing moves."""
    c = ts.growth()
    core = cores(c.pat_str, chunk_bytes)
    core.reset_kernel_ms()
    core.set_profiling(True)
    try:
        run(cores, wanted, c, chunk_bytes)
        launches = core.kernel_ms("tk_k_train_rehash")[1]
    finally:
        core.set_profiling(False)
        core.reset_kernel_ms()
    moves = (core.stat("train_table_moves"), core.stat("train_blob_moves"))
    print("growth", chunk_bytes, "rehash launches", launches, "table / blob moves", moves, "by the host's rule", ts.predicted_moves(c.docs, c.pat_str)[:2])
    if chunk_bytes is None:
        assert launches == 0 and moves == (0, 0)
    else:
        assert launches >= 2 and moves[0] == launches and moves[1] >= 1
        core.train_bpe_packed(*pack(["one chunk"]), 257)  # (the figures are the last call's)
        assert (core.stat("train_table_moves"), core.stat("train_blob_moves")) == (0, 0)


@BOTH
@pytest.mark.parametrize("order", ["as_built", "reversed"])
@pytest.mark.parametrize("spread", [False, True], ids=["together", "spread"])
def test_long_collide(cores, wanted, spread, order, chunk_bytes):
    """160 words on one probe chain, in two document orders (another claim order, another table layout)"""
    c = ts.long_collide(spread)
    docs = c.docs if order == "as_built" else c.docs[::-1]
    core = run(cores, wanted, c, chunk_bytes, docs, key=(c.name, order))
    if spread and chunk_bytes:
        assert core.stat("train_table_moves") >= 1 and core.stat("train_blob_moves") >= 1  # (the chain was moved)


@BOTH
@pytest.mark.parametrize("chunked", [False, True], ids=["small", "chunk_sized_documents"])
def test_gaps(cores, wanted, chunked, chunk_bytes):
    c = ts.gaps(chunked)
    core = run(cores, wanted, c, chunk_bytes)
    only = ts.only_gaps_corpus()
    with pytest.raises(ValueError, match="no piece of two bytes"):
        core.train_bpe_packed(*pack(only.docs), 256 + only.n_merges)
    run(cores, wanted, c, chunk_bytes)  # the call after the error


@BOTH
def test_ties(cores, wanted, chunk_bytes):
    """the first six steps are decided by position between pairs of two different chunks (test_train_shapes.py)"""
    run(cores, wanted, ts.ties(), chunk_bytes)


@BOTH
@pytest.mark.parametrize("case", ts.exhaust(), ids=lambda c: c.name)
def test_exhaust(cores, wanted, case, chunk_bytes):
    core = cores(case.pat_str, chunk_bytes)
    want = wanted(case.name, case.docs, case.n_merges, case.pat_str)
    assert isinstance(want, tr.Exhausted) and want.done == case.meta["done"]
    text = check(core, case.docs, case.n_merges, want, case.name)
    assert re.search(rf"after {want.done} of {case.n_merges} merges", text), text
    follow = ts.long_collide(False)  # the call after the error
    run(cores, wanted, follow, chunk_bytes)
    pairs, counts = core.train_bpe_packed(*pack(case.docs), 256 + want.done)  # exactly the merges there are
    assert [tuple(p) for p in pairs.tolist()] == want.partial.pairs and counts.tolist() == want.partial.counts and len(counts) == want.done


def test_chunk_edges(cores, wanted):
    small, whole = cores(ts.GPT2, SMALL), cores(ts.GPT2, None)
    words = " ".join(ts.consonant_word(i)[: 2 + i % 3] for i in range(1500))
    exact = words[:SMALL - 2] + " z"
    assert ts.nbytes(exact) == SMALL
    check(small, [exact], 20, wanted("exact", [exact], 20, ts.GPT2), "a document of exactly one chunk")
    with pytest.raises(ValueError, match="split it into documents"):
        small.train_bpe_packed(*pack([exact + "z"]), 260)
    docs = [exact[:3000], "", exact[2000:], "", ""]  # 3000 + 2096 bytes: the cut falls behind the empty document
    assert ts.chunks_of(docs) == [(0, 2), (2, 5)]
    want = wanted("edge", docs, 20, ts.GPT2)
    check(small, docs, 20, want, "a cut behind an empty document")
    a, b = whole.train_bpe_packed(*pack(docs), 276), small.train_bpe_packed(*pack(docs), 276)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_seeded_sweep(cores):
    """40 seeded samples over small alphabets (runs of one symbol and ties abound), five patterns, both chunk sizes"""
    ran_out = 0
    for i in range(ts.SWEEP_SAMPLES):
        pat, docs, n_merges = ts.sweep_sample(i)
        try:
            want = tr.train_text(docs, 256 + n_merges, ts.PATTERNS[pat])
        except tr.Exhausted as e:
            want = e
            ran_out += 1
        for chunk_bytes in (None, SMALL):
            try:
                check(cores(ts.PATTERNS[pat], chunk_bytes), docs, n_merges, want)
            except BaseException:
                print(f"sweep sample {i} (seed {ts.SWEEP_SEED}), pattern {pat}, chunk_bytes {chunk_bytes}, n_merges {n_merges}, docs {docs!r}")
                raise
    assert ran_out <= ts.SWEEP_SAMPLES // 4
