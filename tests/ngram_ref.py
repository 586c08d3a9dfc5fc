"""Token n-gram sets, the reference: a Python set of id tuples and a loop.  It shares no hash with the library, so it is exact, while the
library confuses two n-grams with probability 2^-64 per pair: among the fewer than 10^6 n-grams a test uses, below 10^-7.  Below it, the
batches the tests share (`key`, the library's key, only CHOOSES n-grams that collide in a small table; no expected value comes from it)."""
from typing import NamedTuple

import numpy as np

NONE = M = 2 ** 64 - 1
KS = (1, 2, 13, 32)
Ref = NamedTuple("Ref", [(f, np.ndarray) for f in ("n_hit", "n_covered", "n_ngrams", "first_hit", "length", "mask")])


def ngrams(tok, off, k):
    """(document, start, the n-gram as a tuple) of every n-gram of the batch: none crosses a document, a short document has none"""
    t = tok.tolist()
    for d in range(len(off) - 1):
        for g in range(int(off[d]), int(off[d + 1]) - k + 1):
            yield d, g, tuple(t[g:g + k])


def add(held: set, tok, off, k) -> set:
    held.update(u for _, _, u in ngrams(tok, off, k))
    return held


def overlap(held: set, tok, off, k) -> Ref:
    n = len(off) - 1
    L = np.diff(off).astype(np.uint64)
    r = Ref(np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.where(L >= k, L - np.uint64(k - 1), 0).astype(np.uint64), np.full(n, NONE, np.uint64), L, np.zeros(len(tok), np.uint8))
    for d, g, u in ngrams(tok, off, k):
        if u in held:
            r.n_hit[d] += 1
            r.first_hit[d] = min(int(r.first_hit[d]), g - int(off[d]))
            r.mask[g:g + k] = 1
    for d in range(n):
        r.n_covered[d] = int(r.mask[int(off[d]):int(off[d + 1])].sum())  # (a union: the mask's ones)
    return r


def half(tok, off, k, also=()) -> set:
    """every other of the batch's distinct n-grams, in sorted order, and those that start at `also`"""
    return set(sorted({u for _, _, u in ngrams(tok, off, k)})[::2]) | {tuple(tok[g:g + k].tolist()) for g in also}


# ---------------------------------------------------------------- the batches
def pack(lens, seed, alphabet=3):
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    return np.random.default_rng(seed).integers(0, alphabet, int(off[-1])).astype(np.uint32), off


def as_docs(held, k):
    """a set of n-grams as a packed batch, one document each"""
    return np.array([t for u in sorted(held) for t in u], np.uint32), (np.arange(len(held) + 1) * k).astype(np.uint64)


def batches(T: int, k: int):
    """(name, tokens, tok_off, held) -- documents of 0, 1, k - 1, k, k + 1 and 2k tokens, empty ones first, last and in runs; for every edge P
    (the tile's T - k, T - 1, T, T + 1; the word's 63, 64, 65) a document that ends at P, one that starts there, and one -- of k tokens, and
    a long one -- whose last n-gram starts there, the n-gram at P in the set: at P = T - 1 its coverage lies in the next tile; 2T + 7 tokens,
    so the last tile's halo lies behind the batch; overlapping, adjacent and lone hits; the ids 0 and 2^32 - 1."""
    out = []
    tok, off = pack([0, 0, 1, k - 1, k, 0, 0, 0, k + 1, 2 * k, 2 * k, 0, 3, 0, 0], k)
    out.append(("lengths", tok, off, half(tok, off, k)))
    N = 2 * T + 7
    for P in sorted({T - k, T - 1, T, T + 1, 63, 64, 65} - {0}):
        for cuts in ([P, P + k], [P + k]):
            tok, off = pack(np.diff([0, *cuts, N]), P + len(cuts))
            out.append((f"edge{P}/{len(cuts)}", tok, off, half(tok, off, k, also=[P])))
    tok = np.arange(100, 100 + 6 * k, dtype=np.uint32)
    tok[2 * k:2 * k + 4] = [0, 0xFFFFFFFF, 0xFFFFFFFF, 0]
    off = np.array([0, 0, 5 * k, 6 * k], np.uint64)
    out.append(("union", tok, off, {tuple(tok[g:g + k].tolist()) for g in (0, 1, k + 1, 2 * k, 3 * k + 2, 5 * k)}))
    return out


def mix(z):
    z = (z + 0x9E3779B97F4A7C15) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return z ^ (z >> 31)


def key(u, seed):
    x = mix(seed ^ len(u))
    for t in u:
        x = mix(x ^ t)
    return x or 1


def small_table(k: int, S: int, seed: int = 0):
    """(tokens, tok_off, held) for a set of capacity S / 2, so of S slots: n + 1 different n-grams whose probe starts at the table's last
    slot, one document each, n of them held -- their chain wraps the table's end, and the one that is not held walks it to its end.  n is
    what the add rule admits: an add of n n-grams as n documents carries n k tokens, so n = (S / 2) // k, and none where k > S / 2."""
    n, found, i = (S // 2) // k, [], 0
    while len(found) <= n:
        u = (7,) * (k - 1) + (i,)
        if key(u, seed) & (S - 1) == S - 1:
            found.append(u)
        i += 1
    return *as_docs(found, k), set(found[:n])
