"""Batches for the fingerprint tests (the CPU simulation and the GPU entries share them): packed tokens whose documents sit where a tile
pass can go wrong.  T: the tile, k: the shingle length.  Ids are any uint32 values; 0, 2^31 and 2^32 - 1 are always among them."""
import numpy as np

# (ngram, n_perm, bands, seed): k in {1, 5, 32}; P in {1, 20, 128, 256}; B = 1, B = P and a proper divisor; two seeds
SPECS = [(5, 128, 16, 0), (1, 1, 1, 0x9E3779B97F4A7C15), (32, 256, 256, 0), (5, 20, 4, 0x9E3779B97F4A7C15), (32, 20, 1, 0), (1, 256, 32, 0x9E3779B97F4A7C15),
         (5, 256, 1, 0), (32, 128, 128, 0x9E3779B97F4A7C15), (1, 20, 20, 0)]
REFUSED = [(0, 128, 16), (33, 128, 16), (5, 0, 1), (5, 257, 1), (5, 128, 24), (5, 128, 0), (5, 16, 32)]


def pack(lengths, seed: int):
    off = np.zeros(len(lengths) + 1, np.uint64)
    if len(lengths):
        off[1:] = np.cumsum(np.asarray(lengths, np.uint64))
    n = int(off[-1])
    tok = np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    tok[:3] = np.array([0, 1 << 31, (1 << 32) - 1], np.uint32)[:min(n, 3)]
    if n > 8:
        tok[-3:] = np.array([(1 << 32) - 1, 0, 1 << 31], np.uint32)
    return tok, off


def edge_lengths(T: int, k: int):
    """Documents of 0, 1, k - 1, k, k + 1, T - 1, T, T + 1 and 3T + 5 tokens, each placed (by a filler document in front of it) so that it
    ends exactly at a tile edge, one position before it and one position after it."""
    lengths, cur = [], 0
    for L in (0, 1, k - 1, k, k + 1, T - 1, T, T + 1, 3 * T + 5):
        for delta in (0, -1, 1):
            end = ((cur + L + 1 + T - 1) // T) * T + delta  # (the filler holds at least two tokens)
            while end - L - cur < 2:
                end += T
            lengths += [end - L - cur, L]
            cur = end
    return lengths


def empties_lengths(T: int, run: int):
    """runs of `run` empty documents at the start, across a tile edge and at the end"""
    return [0] * run + [T] + [0] * run + [T // 2 + 3] + [0] * run


def batches(T: int, k: int):
    """(name, tokens, tok_off) of every shape the tests run"""
    out = [("edges", *pack(edge_lengths(T, k), 11))]
    for run in (1, 2, 70):
        out.append((f"empties{run}", *pack(empties_lengths(T, run), 12 + run)))
    out.append(("ones", *pack([1] * 2000, 13)))
    out.append(("one document", *pack([T + T // 2 + 1], 14)))
    out.append(("no documents", *pack([], 15)))
    out.append(("no tokens", *pack([0] * 5, 16)))
    return out


# ---------------------------------------------------------------- the batch of the helper tests
HELPER_SPEC = (5, 128, 16, 0x5EED)
WORDS = ("the of and to in a is that for it as was with be by on not he this are or his from at which but have an had they you were their one all we can her has "
         "there been if more when will would who so no out up into do any your what could time these two may then other some than only new very my over also after "
         "tile wave lane mask store count hash band token shard batch merge rank split chunk row pad stream decode encode").split()


def helper_texts():
    """40 base texts of about 150 words, seeded"""
    import random

    rng = random.Random(0x40)
    return [" ".join(rng.choice(WORDS) for _ in range(rng.randint(120, 180))) + "." for _ in range(40)]


def helper_batch(encode):
    """(tokens, tok_off, pairs): every base text (encode: text -> ids), an identical copy, a copy with about one token in ten replaced, and
    an empty document after every fourth base; pairs: the (i, j) whose Jaccard estimate the tests look at -- base and copy, base and noisy
    copy, base and the next base."""
    rng = np.random.default_rng(0x41)
    docs, base_at = [], []
    for i, t in enumerate(helper_texts()):
        ids = np.asarray(encode(t), np.uint32)
        noisy = ids.copy()
        hit = rng.random(len(ids)) < 0.1
        noisy[hit] = rng.integers(0, 50000, int(hit.sum()), dtype=np.uint64).astype(np.uint32)
        base_at.append(len(docs))
        docs += [ids, ids.copy(), noisy]
        if i % 4 == 3:
            docs.append(np.zeros(0, np.uint32))
    off = np.zeros(len(docs) + 1, np.uint64)
    off[1:] = np.cumsum([len(d) for d in docs])
    pairs = [(b, b + 1) for b in base_at] + [(b, b + 2) for b in base_at] + [(a, b) for a, b in zip(base_at[:-1], base_at[1:])]
    return np.concatenate(docs), off, pairs
