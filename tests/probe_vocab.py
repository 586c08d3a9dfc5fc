"""Vocabularies for the bucketed whole-piece tables (tk_common.h, "bucketed tables"): the tables' hashes and sizing rules restated, a
COLLISION vocabulary whose keys are searched so that three buckets' worth and more of every table's keys share one home bucket -- the
LAST bucket, so that their sequences wrap around --, and text made of its tokens, near-misses and colliding strings that are not
tokens.  Every key is a piece of the stock patterns: lower-case letters behind an optional space.  Seeded, no files.
tests/hostsim/probe_sanitize.cpp counts the same home buckets with the product's own functions."""
from __future__ import annotations

import functools
import random

M32 = 0xFFFFFFFF
SHORT_BW, MID_BW, XL_BW, BUCKET_BOUND = 4, 2, 2, 64  # TK_SHORT_BW, TK_MID_BW, TK_XL_BW, TK_BUCKET_BOUND
SHORT_MUL = 0x9E3779B1
TILE = 3840


def pow2_for(items: int) -> int:
    """Slots of the short / mid table (tk_tables.cpp: load factor <= 0.5, at least 64)"""
    bits = 6
    while (1 << bits) < 2 * items + 2:
        bits += 1
    return 1 << bits


def xl_slots(items: int) -> int:
    cap = 64
    while 2 * cap < 5 * items + 2:
        cap <<= 1
    return cap


def short_slot(key: bytes, slots: int) -> int:
    k = int.from_bytes(key, "little")
    return ((k * SHORT_MUL) & M32) >> (32 - slots.bit_length() + 1)


def mid_slot(key: bytes, slots: int) -> int:
    k = int.from_bytes(key, "little")
    x = ((k & M32) * 0x9E3779B1 + (k >> 32) * 0x85EBCA77) & M32
    x ^= x >> 15
    return ((x * 0xC2B2AE3D) & M32) >> (32 - slots.bit_length() + 1)


def ident(p: bytes):
    """tk_ident of a piece of 9..23 bytes: (w0, w1, w2) = the bytes, each word's left-aligned as tk_keep_bytes leaves them, the length on top"""
    n = len(p)

    def keep(x: bytes, r: int) -> int:
        r = max(0, min(8, r))
        return (int.from_bytes(x[:r], "little") << (8 * (8 - r))) & 0xFFFFFFFFFFFFFFFF if r else 0

    return keep(p[0:8], n), keep(p[8:16], n - 8), (keep(p[16:24], n - 16) >> 8) | (n << 56)


def xl_slot(key: bytes, slots: int) -> int:
    w0, w1, w2 = ident(key)
    a, b, c, d, e, f = w0 & M32, w0 >> 32, w1 & M32, w1 >> 32, w2 & M32, w2 >> 32
    h = (a * 0x9E3779B1 + b * 0x85EBCA77 + c * 0xC2B2AE3D + d * 0x27D4EB2F + e * 0x165667B1 + f * 0xD3A2646D) & M32
    h ^= h >> 15
    h = (h * 0x2C1B3C6D) & M32
    h ^= h >> 12
    return h & (slots - 1)


LETTERS = b"abcdefghijklmnopqrstuvwxyz"
CLASSES = {"short": (2, 4), "mid": (5, 8), "xl": (9, 23)}
N_COLLIDE = {"short": 3 * SHORT_BW + 2, "mid": 3 * MID_BW + 2, "xl": 3 * XL_BW + 2}  # three buckets' worth and two more
N_PLAIN = 40       # tokens per class that go where their hash sends them
N_ABSENT = 6       # per class: strings of the colliding home bucket that are NOT tokens (their search walks the whole sequence)


def _word(rng: random.Random, lo: int, hi: int) -> bytes:
    n = rng.randint(lo, hi)
    lead = b" " if n > 2 and rng.random() < 0.7 else b""
    return lead + bytes(rng.choice(LETTERS) for _ in range(n - len(lead)))


@functools.lru_cache(maxsize=None)
def collision_vocab():
    """(ranks, colliding, absent, slots): `colliding[cls]` = the tokens of the class whose home bucket is the table's last one, `absent[cls]` =
    strings with that home bucket that are not tokens, `slots[cls]` = the table's slots by the builder's rule.  Dense ids in the order of the dictionary (the builder's order)."""
    rng = random.Random(0xB0C4E7)
    n_short = 256 + N_COLLIDE["short"] + N_PLAIN
    slots = {"short": pow2_for(n_short), "mid": pow2_for(N_COLLIDE["mid"] + N_PLAIN), "xl": xl_slots(N_COLLIDE["xl"] + N_PLAIN)}
    slot_of = {"short": short_slot, "mid": mid_slot, "xl": xl_slot}
    bw = {"short": SHORT_BW, "mid": MID_BW, "xl": XL_BW}
    toks, colliding, absent = [], {}, {}
    seen = set()
    for cls, (lo, hi) in CLASSES.items():
        last = slots[cls] // bw[cls] - 1
        hits, plain = [], []
        while len(hits) < N_COLLIDE[cls] + N_ABSENT or len(plain) < N_PLAIN:
            w = _word(rng, lo, hi)
            if w in seen:
                continue
            seen.add(w)
            if slot_of[cls](w, slots[cls]) // bw[cls] == last:
                hits.append(w)
            elif len(plain) < N_PLAIN:
                plain.append(w)
        colliding[cls], absent[cls] = hits[:N_COLLIDE[cls]], hits[N_COLLIDE[cls]:N_COLLIDE[cls] + N_ABSENT]
        toks += colliding[cls] + plain
    rng.shuffle(toks)
    toks = [bytes([b]) for b in range(256)] + toks
    return {t: i for i, t in enumerate(toks)}, colliding, absent, slots


def near_misses(tok: bytes, ranks, rng: random.Random) -> list[bytes]:
    """A proper prefix, an extension by one letter and a one-letter mutation of a token that are not tokens (letters only: still one piece)"""
    out = []
    if len(tok.strip()) > 1:
        out.append(tok[:-1])
    out.append(tok + bytes([rng.choice(LETTERS)]))
    i = rng.randrange(1 if tok[:1] == b" " else 0, len(tok))
    out.append(tok[:i] + bytes([rng.choice(LETTERS)]) + tok[i + 1:])
    return [c for c in out if c not in ranks and c.strip()]


def text_of(ranks, extra: list[bytes], nbytes: int, seed: int, short_only: bool = False) -> bytes:
    """About nbytes (never more) of pieces, each behind its own space or a line break: tokens of more than one byte, their near-misses in every length class, and
    `extra` (the colliding tokens and the colliding strings that are not tokens), all of them more than once"""
    rng = random.Random(seed)
    words = [t for t in ranks if len(t) > 1 and (not short_only or len(t) <= 4)]
    pool = list(extra)
    out = bytearray()
    while True:
        r = rng.random()
        if pool and r < 0.3:
            w = rng.choice(pool)
        elif r < 0.65:
            w = rng.choice(words)
        else:
            w = rng.choice(near_misses(rng.choice(words), ranks, rng) or [b"a"])
        w = w if w[:1] == b" " else b"\n" + w  # (a line break is a piece of its own: the word behind it stays what it is)
        if len(out) + len(w) > nbytes:
            return bytes(out)
        out += w
