"""The fingerprint rule of include/tiktoken_amd.h, stated once more in plain Python: a loop over documents, Python integers masked to 64
bits.  Written from the header's prose, not from the C++; it is what the CPU simulation and the GPU entries are compared against.  The host
helpers of `Fingerprints` are restated with dicts, and `true_jaccard` gives the Jaccard index of two documents' shingle sets."""
from typing import NamedTuple

import numpy as np

M64 = (1 << 64) - 1
BAND_SALT = 0x42414E4400000000


def mix(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def check_spec(ngram: int, n_perm: int, bands: int) -> None:
    if not 1 <= ngram <= 32:
        raise ValueError("ngram")
    if not 1 <= n_perm <= 256:
        raise ValueError("n_perm")
    if not 1 <= bands <= n_perm or n_perm % bands:
        raise ValueError("bands")


def shingles(ids: list, k: int) -> list:
    """the shingles of a document, as tuples of ids"""
    L = len(ids)
    if L == 0:
        return []
    if L < k:
        return [tuple(ids)]
    return [tuple(ids[i:i + k]) for i in range(L - k + 1)]


def shingle_hash(u: tuple, seed: int) -> int:
    x = mix(seed ^ len(u))
    for t in u:
        x = mix(x ^ (t & 0xFFFFFFFF))
    return x


class Ref(NamedTuple):
    sig: np.ndarray
    band: np.ndarray
    exact: np.ndarray
    n_shingles: np.ndarray
    length: np.ndarray


def fingerprint_plain(tokens, tok_off, ngram: int = 5, n_perm: int = 128, bands: int = 16, seed: int = 0) -> Ref:
    """The rule word for word: Python integers only.  Slow; `fingerprint` is tied to it by tests/test_fingerprint_sim.py."""
    check_spec(ngram, n_perm, bands)
    toks = [int(t) & 0xFFFFFFFF for t in np.asarray(tokens).tolist()]
    off = [int(x) for x in np.asarray(tok_off).tolist()]
    n, r = len(off) - 1, n_perm // bands
    sig = np.full((n, n_perm), 0xFFFFFFFF, np.uint32)
    band, exact = np.zeros((n, bands), np.uint64), np.zeros(n, np.uint64)
    n_sh, length = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    for d in range(n):
        ids = toks[off[d]:off[d + 1]]
        L = len(ids)
        hs = [shingle_hash(u, seed) for u in shingles(ids, ngram)]
        row = [min((perm_value(seed, p, h) for h in hs), default=0xFFFFFFFF) for p in range(n_perm)]
        sig[d] = row
        for j in range(bands):
            x = mix(seed ^ BAND_SALT ^ j)
            for i in range(r):
                x = mix(x ^ row[j * r + i])
            band[d, j] = x
        total = 0
        for i, t in enumerate(ids):
            total = (total + mix(seed ^ (((i + 1) << 32) & M64) ^ t)) & M64
        exact[d] = mix(L ^ total)
        n_sh[d], length[d] = len(hs), L
    return Ref(sig, band, exact, n_sh, length)


def mix_np(z: np.ndarray) -> np.ndarray:
    """mix on a uint64 array: numpy's uint64 arithmetic wraps modulo 2^64, which is the rule's"""
    U = np.uint64
    z = z + U(0x9E3779B97F4A7C15)
    z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
    return z ^ (z >> U(31))


def fingerprint(tokens, tok_off, ngram: int = 5, n_perm: int = 128, bands: int = 16, seed: int = 0) -> Ref:
    """The same rule, document by document, with a document's positions side by side in numpy uint64 arrays."""
    check_spec(ngram, n_perm, bands)
    U = np.uint64
    toks = (np.asarray(tokens).astype(np.int64) & 0xFFFFFFFF).astype(np.uint64)
    off = [int(x) for x in np.asarray(tok_off).tolist()]
    n, r = len(off) - 1, n_perm // bands
    perms = [(mix((seed + 2 * p + 1) & M64) | 1, mix((seed + 2 * p + 2) & M64)) for p in range(n_perm)]
    pa, pb = np.array([a for a, _ in perms], U)[:, None], np.array([b for _, b in perms], U)[:, None]
    sig = np.full((n, n_perm), 0xFFFFFFFF, np.uint32)
    band, exact = np.zeros((n, bands), np.uint64), np.zeros(n, np.uint64)
    n_sh, length = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    with np.errstate(over="ignore"):
        for d in range(n):
            ids = toks[off[d]:off[d + 1]]
            L = len(ids)
            m = min(L, ngram)
            count = 0 if L == 0 else 1 if L < ngram else L - ngram + 1
            if count:
                x = np.full(count, mix(seed ^ m), U)
                for j in range(m):
                    x = mix_np(x ^ ids[j:j + count])
                for p0 in range(0, n_perm, 32):  # (32 permutations at a time: the table stays small)
                    sig[d, p0:p0 + 32] = ((pa[p0:p0 + 32] * x[None, :] + pb[p0:p0 + 32]) >> U(32)).min(axis=1).astype(np.uint32)
            row = sig[d].tolist()
            for j in range(bands):
                y = mix(seed ^ BAND_SALT ^ j)
                for i in range(r):
                    y = mix(y ^ row[j * r + i])
                band[d, j] = y
            pos = (np.arange(1, L + 1, dtype=U) << U(32))
            total = int(mix_np(U(seed) ^ pos ^ ids).sum(dtype=U)) if L else 0
            exact[d] = mix(L ^ total)
            n_sh[d], length[d] = count, L
    return Ref(sig, band, exact, n_sh, length)


def perm_value(seed: int, p: int, h: int) -> int:
    """the value of permutation p at hash h"""
    a, b = mix((seed + 2 * p + 1) & M64) | 1, mix((seed + 2 * p + 2) & M64)
    return (((a * h + b) & M64) >> 32) & 0xFFFFFFFF


def true_jaccard(tokens, tok_off, i: int, j: int, ngram: int) -> float:
    toks, off = np.asarray(tokens).tolist(), [int(x) for x in np.asarray(tok_off).tolist()]
    a, b = set(shingles(toks[off[i]:off[i + 1]], ngram)), set(shingles(toks[off[j]:off[j + 1]], ngram))
    return len(a & b) / len(a | b) if a | b else 1.0


# ---------------------------------------------------------------- the host helpers, with dicts
def jaccard(r: Ref, i: int, j: int) -> float:
    P = r.sig.shape[1]
    return sum(1 for p in range(P) if r.sig[i, p] == r.sig[j, p]) / P


def exact_groups(r: Ref) -> list:
    first: dict = {}
    return [first.setdefault((int(r.exact[d]), int(r.length[d])), d) for d in range(len(r.exact))]


def duplicate_groups(r: Ref, threshold: float = 0.8) -> list:
    n, B = len(r.exact), r.band.shape[1]
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for j in range(B):
        lowest: dict = {}
        for d in range(n):
            if r.n_shingles[d] == 0:
                continue
            rep = lowest.setdefault(int(r.band[d, j]), d)
            if rep != d and jaccard(r, d, rep) >= threshold:
                a, b = find(d), find(rep)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    return [find(d) for d in range(n)]


def keep_mask(r: Ref, threshold: float = 0.8) -> list:
    return [g == d for d, g in enumerate(duplicate_groups(r, threshold))]
