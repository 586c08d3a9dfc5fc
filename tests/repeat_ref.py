"""The reference of the repetition statistics (tk_repeat.h) -- a Counter of tuples per document and size, the covered tokens as a boolean
array -- and the named batches of the GPU tests, built from the tile T and the class edge C.  Nothing from the code under test."""
from collections import Counter, namedtuple

import numpy as np

Ref = namedtuple("Ref", "n_ngrams n_distinct n_dup n_dup_covered top_count")


def stats(tok, off, sizes) -> Ref:
    out = [np.zeros((len(off) - 1, len(sizes)), np.uint64) for _ in Ref._fields]
    for d in range(len(off) - 1):
        ids = tok[int(off[d]):int(off[d + 1])].tolist()
        for j, k in enumerate(sizes):
            grams = [tuple(ids[i:i + k]) for i in range(len(ids) - k + 1)]
            count = Counter(grams)
            covered = np.zeros(len(ids), bool)
            for i, g in enumerate(grams):
                if count[g] > 1:
                    covered[i:i + k] = True
            row = (len(grams), len(count), sum(c for c in count.values() if c > 1), int(covered.sum()), max(count.values(), default=0))
            for o, v in zip(out, row):
                o[d, j] = v
    return Ref(*out)


def pack(docs):
    docs = [np.asarray(d, dtype=np.uint32) for d in docs]
    off = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.uint64)
    return (np.concatenate(docs) if docs else np.zeros(0, np.uint32)).astype(np.uint32), off


def batches(T: int, C: int, sizes):
    """[(name, tokens, tok_off)], each under 10^5 tokens"""
    rng = np.random.default_rng(T + C + sum(sizes))
    km = max(sizes)
    rand = lambda L, a: rng.integers(0, a, L)  # noqa: E731
    fresh = lambda L: np.arange(1000, 1000 + L)  # noqa: E731  (no n-gram twice)

    def copies(L, src, at):  # distinct ids, the km-gram at `src` copied to every position of `at`
        d = fresh(L)
        for p in at:
            d[p:p + km] = d[src:src + km].copy()
        return d

    run = fresh(200)
    run[40:40 + km + 1] = 7  # two occurrences that overlap
    return [
        ("lengths", *pack([rand(L, 3) for k in sizes for L in (0, 1, k - 1, k, k + 1, 2 * k - 1, 2 * k)])),
        ("one id", *pack([np.full(300, 5)])),
        ("periods", *pack([np.arange(200) % 3, np.arange(500) % 64])),
        ("alphabets", *pack([rand(300, 2), rand(300, 4), rand(C, 2), rand(C, 4)])),
        # a filler of 60, then a document in which one km-gram occurs again abutting, across global bit 64 * 5 and across the tile's edge
        ("one repeat", *pack([fresh(60), run, copies(T + 200, 10, (10 + km, 64 * 5 - 1 - 260, T - 1 - 260))])),
        ("twins", *pack([fresh(50), fresh(50)])),
        ("tiny documents", *pack([rand(1 + i % 2, 2) for i in range(2 * (T + 10) // 3)])),
        ("starts at the tile's last position", *pack([fresh(T - 1), rand(700, 4), rand(5, 2)])),
        ("class edge", *pack([rand(C - 1, 3), rand(C, 3), rand(C + 1, 3)])),
        ("long, repeats in different tiles", *pack([fresh(9), copies(3 * T + 17, 5, (T + 100, 2 * T + 500, 3 * T + 17 - km))])),
        ("long, one id", *pack([np.full(C + 100, 5)])),
        ("interleaved", *pack([rand(100, 2), rand(C + 5, 2), rand(0, 2), rand(C, 3), rand(2 * C + 1, 4), rand(3, 2)])),
        ("extreme ids", *pack([rng.choice([0, 0xFFFFFFFF], 200), rng.choice([0, 0xFFFFFFFF], C + 70)])),
        ("no document", *pack([])),
    ]
