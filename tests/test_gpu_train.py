"""BPE training on the device (tk_train_bpe, tiktoken_amd.train): the fixtures the reference's own trainer produced are reproduced
exactly, and on shapes the reference was never run on the merges and their counts equal the Python restatement of the rule
(tests/train_ref.py)."""
import os

import numpy as np
import pytest

import helpers as h
import train_ref as tr

pytestmark = pytest.mark.gpu

GPT2 = h.PAT_STR[0]


def case_ids():
    return [c["name"] for c in tr.load_cases()[1]]


@pytest.fixture(scope="module")
def core():
    from tiktoken_amd import CoreBPE

    c = CoreBPE({bytes([b]): b for b in range(256)}, {}, GPT2)
    yield c
    c.close()


WHOLE = r"[\s\S]+"  # a document is one piece (the generic engine)


@pytest.fixture(scope="module")
def whole_core():
    from tiktoken_amd import CoreBPE

    c = CoreBPE({bytes([b]): b for b in range(256)}, {}, WHOLE)
    yield c
    c.close()


def pack(docs):
    raw = [d.encode("utf-8") for d in docs]
    off = np.zeros(len(raw) + 1, dtype=np.uint64)
    np.cumsum([len(b) for b in raw], out=off[1:])
    return np.frombuffer(b"".join(raw) + b"\0", dtype=np.uint8)[:-1], off


def check_against_restatement(core, docs, n_merges, pat=GPT2):
    """pairs and counts of train_bpe_packed == the restatement's, step by step (counts[k] is the restatement's cmax of step k)"""
    want = tr.train_text(docs, 256 + n_merges, pat)
    pairs, counts = core.train_bpe_packed(*pack(docs), 256 + n_merges)
    assert pairs.dtype == np.uint32 and pairs.shape == (n_merges, 2) and counts.dtype == np.uint64 and counts.shape == (n_merges,)
    assert [tuple(p) for p in pairs.tolist()] == want.pairs
    assert counts.tolist() == want.counts
    return pairs, counts


@pytest.mark.parametrize("name", case_ids())
def test_fixtures_are_reproduced(name):
    """`bpe_train` gives the dict the reference's trainer gave: the same tokens with the same ids in the same insertion order."""
    from tiktoken_amd import bpe_train

    texts, cases = tr.load_cases()
    case = next(c for c in cases if c["name"] == name)
    if case.get("exhausted"):
        with pytest.raises(ValueError):
            bpe_train(texts[case["text"]], case["vocab_size"], case["pat_str"])
        return
    got = bpe_train(texts[case["text"]], case["vocab_size"], case["pat_str"])
    assert list(got.items()) == list(tr.case_ranks(case).items())


def filler(n, start=1):
    return "".join(chr(33 + (start + 7 * i) % 90) for i in range(n)).replace("a", "~")


@pytest.mark.parametrize("block", [256])
def test_runs_around_workgroup_boundaries(whole_core, block):
    """Runs of one symbol of lengths 1-9, 63-65 and block +- 1 at the start, at the end and in the middle of words (where the words lie in
    the arrays is the device's choice: every run length comes with several word lengths around the workgroup size)."""
    for k in sorted(set(list(range(1, 10)) + [63, 64, 65, block - 1, block, block + 1])):
        docs = ["a" * k + "," * 3, "." * 2 + "a" * k, "-" * (block - 1) + "a" * k + "!!", "a" * k, "b" * (block - 2 + k % 5)]
        check_against_restatement(whole_core, docs, 9, pat=WHOLE)


def test_long_run_single_bytes_and_sizes(core, whole_core):
    with pytest.raises(ValueError, match="no pair left"):  # words of one byte have no pairs
        core.train_bpe_packed(*pack(["a", "b", "a", "c"]), 257)
    rng = np.random.default_rng(5)
    for total in (256, 255, 257, 2 * 256 + 40):  # total symbols around the workgroup size
        docs, left = [], total
        while left:
            n = min(left, int(rng.choice([1, 2, 3, 5, 8, 60])))
            w = "".join(rng.choice(list("abc"), size=n))
            if w in docs:
                continue
            docs.append(w)
            left -= n
        check_against_restatement(whole_core, docs, 12, pat=WHOLE)
    check_against_restatement(whole_core, ["a" * 5000, "ab", "ab", "ab"], 14, pat=WHOLE)
    check_against_restatement(whole_core, [filler(40, 3), filler(30, 9)[::-1]], 5, pat=WHOLE)  # every pair occurs once: position decides


def test_more_than_1024_workgroups(whole_core):
    """The step's single-workgroup kernels (tk_k_train_carry, tk_k_train_offsets) take the values of 1024 workgroups of 256 symbols at a time:
    distinct words of just over 1024 * 256 symbols run their loops twice.  Most words hold a run of one letter, many of them longer than a
    workgroup, so the first winners have a == b and the largest break mark is carried from workgroup to workgroup, the 1024th included;
    later winners are pairs of the other letters."""
    rng = np.random.default_rng(1024)
    letters, total = list("abcde"), 1024 * 256 + 300
    words, left = set(), total
    while left:
        w = "".join(rng.choice(letters, size=int(rng.integers(1, 120)))) + "z" * int(rng.choice([0, 0, 3, 50, 300, 700])) + "".join(rng.choice(letters, size=int(rng.integers(0, 10))))
        w = w[:left]
        if w in words:
            continue
        words.add(w)
        left -= len(w)
    docs = sorted(words)
    assert sum(map(len, docs)) == total and len(docs) > 500 and len(set(map(len, docs))) > 100
    pairs, _ = check_against_restatement(whole_core, docs, 8, pat=WHOLE)
    assert pairs[0].tolist() == [122, 122] and pairs[1].tolist() == [256, 256] and any(a != b for a, b in pairs.tolist())


def test_large_weight_and_many_words(core):
    rng = np.random.default_rng(11)
    words = ["".join(rng.choice(list("abcdefghijklmnopqrstuvwxyz"), size=int(rng.integers(2, 7)))) for _ in range(3000)]
    text = " ".join(words) + (" again" * 70000)  # a word repeated 70 000 times
    pairs, counts = check_against_restatement(core, [text], 40)
    assert int(counts[0]) >= 70000


def test_documents_are_boundaries(core):
    """Pieces never cross a document boundary; empty documents change nothing."""
    two, _ = core.train_bpe_packed(*pack(["ab", "ab"]), 257)
    one, _ = core.train_bpe_packed(*pack(["abab"]), 258)
    assert two.tolist() == [[97, 98]] and one.tolist() == [[97, 98], [256, 256]]
    with pytest.raises(ValueError):
        core.train_bpe_packed(*pack(["ab", "ab"]), 258)  # "ab" twice is one word "ab": one merge and no more
    docs = ["", "hello world, hello there", "", "", "the world is there", ""]
    check_against_restatement(core, docs, 12)
    a = core.train_bpe_packed(*pack(docs), 268)
    b = core.train_bpe_packed(*pack([d for d in docs if d]), 268)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    p, c = core.train_bpe_packed(*pack(["anything"]), 256)
    assert p.shape == (0, 2) and c.shape == (0,)


def test_chunks(core):
    """A corpus longer than a chunk goes chunk by chunk into one word table, offsets kept global: the merges are those of one chunk."""
    from tiktoken_amd import CoreBPE

    rng = np.random.default_rng(3)
    vocab = ["".join(rng.choice(list("etaoinshr"), size=int(rng.integers(2, 6)))) for _ in range(60)]
    docs = [" ".join(rng.choice(vocab, size=int(rng.integers(60, 200)))) + ".\n" for _ in range(30)]
    assert 15000 < sum(map(len, docs)) < 40000 and max(map(len, docs)) < 4096
    whole = core.train_bpe_packed(*pack(docs), 256 + 120)
    old = os.environ.get("TIKTOKEN_AMD_CHUNK_BYTES")
    os.environ["TIKTOKEN_AMD_CHUNK_BYTES"] = "4096"
    try:
        small = CoreBPE({bytes([b]): b for b in range(256)}, {}, GPT2)
    finally:
        if old is None:
            del os.environ["TIKTOKEN_AMD_CHUNK_BYTES"]
        else:
            os.environ["TIKTOKEN_AMD_CHUNK_BYTES"] = old
    try:
        assert small.stat("chunk_bytes") == 4096
        cut = small.train_bpe_packed(*pack(docs), 256 + 120)
        assert np.array_equal(whole[0], cut[0]) and np.array_equal(whole[1], cut[1])
        assert [tuple(p) for p in cut[0].tolist()] == tr.train_text(docs, 256 + 120, GPT2).pairs
        with pytest.raises(ValueError, match="split it into documents"):
            small.train_bpe_packed(*pack(["x " * 2500]), 260)
    finally:
        small.close()


def test_two_runs_are_identical(core):
    texts, _ = tr.load_cases()
    a = core.train_bpe_packed(*pack([texts["mixed"]]), 400)
    b = core.train_bpe_packed(*pack([texts["mixed"]]), 400)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_train_encoding_round_trips():
    from tiktoken_amd import train_encoding

    texts, _ = tr.load_cases()
    enc = train_encoding("trained_here", texts["mixed"], 400, h.PAT_STR[2], special_tokens={"<|endoftext|>": 400})
    assert enc.n_vocab == 401 and len(enc._mergeable_ranks) == 400
    ids = enc.encode_ordinary(texts["mixed"])
    assert enc.decode(ids) == texts["mixed"] and max(ids) >= 256
    plain = train_encoding("trained_plain", texts["mixed"], 300, h.PAT_STR[2])
    assert plain.n_vocab == 300 and plain.decode(plain.encode_ordinary(texts["mixed"])) == texts["mixed"]
