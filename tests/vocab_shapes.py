"""Vocabularies of the shapes at which tk_build_tables and tk_create choose other tables and other kernels: a token set crossed with an
id map.  Generated, seeded, no files (the `trained` set is the edu600 fixture the suite already has).  Every vocabulary has at most
3 500 tokens, so a core builds in well under a second -- the ids are wide, not the vocabulary.

    ranks, specials = vocab("untrained", "wide")

Token sets (TOKEN_SETS): bytes_only, untrained, trained.  Id maps (ID_MAPS): see id_map().  Plus the text the GPU tests encode
(shape_docs) and the conditions it has to meet, counted with the oracle's split alone (text_census)."""
from __future__ import annotations

import functools
import os
import random
import re

import helpers as h

# ---------------------------------------------------------------- constants, read from the header
_COMMON = open(os.path.join(h.CSRC, "tk_common.h")).read()


def _define(name: str) -> str:
    return re.search(r"^#define\s+" + name + r"\s+(.+?)\s*(?://.*)?$", _COMMON, re.M).group(1)


TK_PAIR8_ID_BITS = int(_define("TK_PAIR8_ID_BITS"))
assert _define("TK_PAIR8_MAX_ID") == "((1u << TK_PAIR8_ID_BITS) - 2u)"
TK_PAIR8_MAX_ID = (1 << TK_PAIR8_ID_BITS) - 2
TK_SHORT_MAX_RANK = int(_define("TK_SHORT_MAX_RANK").rstrip("uU"), 16)
DEC_TABLE_LIMIT = 1 << 26  # tk_create: a device decode table for ids below this
TOP_ID = 0x7FFFFFFE        # the largest id tk_build_tables accepts

FMT_SHORT, FMT_PAIR_PACKED, FMT_DEC_DENSE = 1, 2, 4  # HostSim.table_format()

# ---------------------------------------------------------------- token sets
LETTERS = b"aeinst"
DIGIT, SPACE = b"7", b" "
CJK = "中".encode()  # three bytes
ALPHABET = LETTERS + DIGIT + SPACE + CJK
LENGTHS = (2, 3, 4, 5, 6, 8, 9, 12, 16, 23, 24, 25, 40, 70)
TOKEN_SETS = ("bytes_only", "untrained", "trained")
N_RANDOM = 3000


def _wordy(rng: random.Random, n: int) -> bytes:
    """n bytes that the r50k pattern takes as one piece: an optional space, then letters and whole CJK chars"""
    out = SPACE if n > 2 and rng.random() < 0.5 else b""
    while len(out) < n:
        out += CJK if n - len(out) >= 3 and rng.random() < 0.15 else bytes([rng.choice(LETTERS)])
    return out


@functools.lru_cache(maxsize=None)
def token_set(name: str) -> tuple[bytes, ...]:
    """The tokens of a set, in a fixed order (the 256 single bytes first)"""
    single = [bytes([b]) for b in range(256)]
    if name == "bytes_only":
        return tuple(single)
    if name == "trained":
        return tuple(sorted(h.golden_vocab("edu600"), key=h.golden_vocab("edu600").get))
    assert name == "untrained"
    rng = random.Random(0x5A17)
    seen = set(single)
    toks = list(single)
    while len(toks) < 256 + N_RANDOM:
        n = rng.choice(LENGTHS)
        # two in three are whole pieces of the pattern (the text is made of them); the others any bytes of the alphabet: digits and spaces
        # inside, CJK chars cut in the middle
        t = _wordy(rng, n) if rng.random() < 0.67 else bytes(rng.choice(ALPHABET) for _ in range(n))
        if t not in seen:
            seen.add(t)
            toks.append(t)
    for n in LENGTHS:
        assert sum(len(t) == n for t in toks) >= 20, n
    assert sum(any(t[:k] not in seen for k in range(1, len(t))) for t in toks) >= 100
    return tuple(toks)


# ---------------------------------------------------------------- id maps
ID_MAPS = ("dense", "packed_edge", "wide_edge", "wide", "dec_edge_lo", "dec_edge_hi", "short_edge", "no_short", "top")
_MAX_OF = {"packed_edge": TK_PAIR8_MAX_ID, "wide": 3_000_017, "dec_edge_lo": DEC_TABLE_LIMIT - 1, "dec_edge_hi": DEC_TABLE_LIMIT,
           "short_edge": TK_SHORT_MAX_RANK, "no_short": TK_SHORT_MAX_RANK + 1, "top": TOP_ID}
# maps whose largest id of all -- special tokens included -- is the edge under test: both special tokens take ids in holes
_NOTHING_ABOVE = ("dec_edge_lo", "short_edge", "top")


def id_map(name: str, n: int) -> list[int]:
    """The ids of n tokens by position, ascending.  dense: 0 .. n - 1.  wide_edge: dense but for the last, TK_PAIR8_MAX_ID + 1.  Every
    other map spreads the ids evenly from 0 to its largest id, which is exactly
      packed_edge  TK_PAIR8_MAX_ID (the last packed pair table)       wide         about 3 M
      dec_edge_lo  2^26 - 1 (the last device decode table)            dec_edge_hi  2^26
      short_edge   TK_SHORT_MAX_RANK (the last short table)           no_short     TK_SHORT_MAX_RANK + 1
      top          0x7FFFFFFE (the largest id there is)"""
    if name == "dense":
        return list(range(n))
    if name == "wide_edge":
        return list(range(n - 1)) + [TK_PAIR8_MAX_ID + 1]
    top = _MAX_OF[name]
    ids = [p * top // (n - 1) for p in range(n)]
    assert ids[-1] == top and len(set(ids)) == n
    return ids


SPECIAL_HI, SPECIAL_LO = "<|shape_hi|>", "<|shape_lo|>"


@functools.lru_cache(maxsize=None)
def vocab(set_name: str, map_name: str):
    """(ranks, specials).  The tokens take the map's ids after a seeded permutation, so that rank order says nothing about length
    (`trained` keeps its order: its merges need it).  Two special tokens: SPECIAL_LO with an id in a hole of the map, SPECIAL_HI with the id
    above the vocabulary's largest -- in a second hole for the maps of _NOTHING_ABOVE; a dense map has no holes: both above."""
    toks = list(token_set(set_name))
    if set_name != "trained":
        random.Random(0xD1CE).shuffle(toks)
    ids = id_map(map_name, len(toks))
    ranks = dict(zip(toks, ids))
    used = set(ids)
    top = ids[-1]
    holes = [i for i in (ids[len(ids) // 3] + 1, ids[len(ids) // 2] + 1, top - 1, top - 2) if i not in used]
    if map_name == "dense":
        specials = {SPECIAL_HI: top + 1, SPECIAL_LO: top + 2}
    elif map_name in _NOTHING_ABOVE:
        specials = {SPECIAL_HI: holes[1], SPECIAL_LO: holes[0]}
    else:
        specials = {SPECIAL_HI: top + 1, SPECIAL_LO: holes[0]}
    assert len(ranks) == len(toks) <= 3500 and not used & set(specials.values()) and len(set(specials.values())) == 2
    return ranks, specials


def expected_format(set_name: str, map_name: str) -> dict:
    """What the tables must look like, from the rules of tk_build_tables and tk_create restated: the short table and the device decode
    table go by the largest id of all, the pair table and the host decoder by the largest rank"""
    ranks, specials = vocab(set_name, map_name)
    top_rank = max(ranks.values())
    top_id = max(top_rank, *specials.values())
    return {"short_table": top_id <= TK_SHORT_MAX_RANK, "pair_table_packed": top_rank <= TK_PAIR8_MAX_ID,
            "dec_dense": top_rank < 4 * len(ranks) + 65536, "decode_table_ids": top_id + 1 if top_id < DEC_TABLE_LIMIT else 0}


# ---------------------------------------------------------------- pieces and text
BOUNDARY_LENGTHS = (4, 5, 8, 9, 23, 24)
BIN_HI = (16, 24, 32, 48, 64, 128, 256, 512, 1024)  # tk_bin_hi (tk_kernels.h); a bin starts one above the bin before it, the first at 2
DELIBERATE = (16, 17, 24, 25, 32, 48, 64, 65, 128, 256, 512, 1024, 1025, 3000)
ONE_PIECE_DOC = 130 << 10  # one document that is one piece: beyond TK_WIDE_MIN (tk_fused.h)
MID_DOCS = (8 << 10, 40 << 10, 100 << 10, 12 << 10)


def bin_of(n: int) -> int:
    """The length bin of a piece of 2 .. 1024 bytes"""
    return sum(n > hi for hi in BIN_HI[:-1])


def pieces(set_name: str, rng: random.Random, count: int, n_long: int = 0) -> list[bytes]:
    """`count` pieces: 1 .. 6 random tokens of the set back to back, cut at a random length of 1 .. 200; then n_long of 200 .. 3000 bytes"""
    toks = token_set(set_name)
    out = []
    for _ in range(count):
        p = b"".join(rng.choice(toks) for _ in range(rng.randint(1, 6)))
        out.append(p[: rng.randint(1, 200)])
    for _ in range(n_long):
        n = rng.randint(200, 3000)
        p = b""
        while len(p) < n:
            p += rng.choice(toks)
        out.append(p[:n])
    return out


def non_tokens(set_name: str, rng: random.Random, count: int) -> list[bytes]:
    """Strings that are not tokens of the set: a token with one byte changed, cut by one, extended by one, random bytes of the boundary lengths"""
    toks = token_set(set_name)
    have = set(toks)
    out = []
    while len(out) < count:
        t = rng.choice(toks)
        k = rng.randrange(4)
        if k == 0:
            i = rng.randrange(len(t))
            c = t[:i] + bytes([rng.choice(ALPHABET) if rng.random() < 0.7 else rng.randrange(256)]) + t[i + 1:]
        elif k == 1:
            c = t[:-1]
        elif k == 2:
            c = t + bytes([rng.choice(ALPHABET)])
        else:
            c = bytes(rng.choice(ALPHABET) for _ in range(rng.choice(BOUNDARY_LENGTHS)))
        if c and c not in have:
            out.append(c)
    return out


def _word(rng: random.Random, n: int) -> bytes:
    """A run of n bytes of letters and CJK chars: one piece behind a separator"""
    out = b""
    while len(out) < n:
        out += CJK if n - len(out) >= 3 and rng.random() < 0.1 else bytes([rng.choice(LETTERS)])
    return out


@functools.lru_cache(maxsize=None)
def shape_docs(seed: int = 0x7E47) -> tuple[bytes, ...]:
    """The documents every shape encodes, valid UTF-8 over untrained's alphabet: letter runs -- tokens, tokens with a byte changed, tokens
    back to back, words of every length bin -- with a space, a line break or a number between them; single pieces of the DELIBERATE
    lengths; three documents of MID_DOCS bytes whose pieces are tokens or short; one of ONE_PIECE_DOC bytes that is a single piece."""
    rng = random.Random(seed)
    wordy = [t for t in token_set("untrained") if len(t) > 1 and t.lstrip(b" ").replace(CJK, b"a").isalpha() and b" " not in t[1:]]
    long_wordy = [t for t in wordy if len(t) > 23]

    def unit(short: bool = False) -> bytes:
        r = rng.random()
        if short:  # pieces of at most 24 bytes (TK_SMALL_PIECE, tk_fused.h) unless they are tokens: what a segment of a mid-size call takes
            if r < 0.5 and short != "words":  # (a long token behind a line break: the piece is the token itself, with its own space or without one)
                t = rng.choice(wordy)
                return b"\n" + t if len(t) > 23 else t
            if r < 0.6:
                return DIGIT * rng.randint(1, 4)
            return _word(rng, rng.randint(1, 23))
        if r < 0.30:
            return rng.choice(wordy)
        if r < 0.36:
            return rng.choice(long_wordy)
        if r < 0.50:  # one byte changed
            t = bytearray(rng.choice(wordy))
            i = rng.randrange(1, len(t))
            if t[i] < 0x80:  # (a CJK char stays whole)
                t[i] = rng.choice(LETTERS)
            return bytes(t)
        if r < 0.70:  # tokens back to back
            return b"".join(rng.choice(wordy).lstrip(b" ") for _ in range(rng.randint(2, 5)))
        if r < 0.74:
            return DIGIT * rng.randint(1, 4)
        b = rng.randrange(len(BIN_HI))  # a word of a length bin, the long bins as likely as the short ones
        return _word(rng, rng.randint(2 if b == 0 else BIN_HI[b - 1] + 1, BIN_HI[b]))

    def doc(target: int, short: bool = False) -> bytes:
        parts, size = [], 0
        while size < target:
            u = unit(short) + rng.choice([b" ", b" ", b"\n", b"\n", b"  ", b" \n"])
            parts.append(u)
            size += len(u)
        cut = b"".join(parts)[:target].decode("utf-8", "ignore").encode()  # (a CJK char cut in the middle goes)
        return cut + b"a" * (target - len(cut))

    docs = [doc(rng.choice([40, 200, 700, 1500, 2048, 3000])) for _ in range(300)]
    docs += [b"", b"a", CJK]
    for n in DELIBERATE:  # a document that is one piece, and the same piece inside a document
        w = _word(rng, n)
        docs += [w, doc(100) + b"\n" + w + b" " + doc(60)]
    for n in (1100, 1500, 2000, 2500):
        docs.append(b" " + _word(rng, n))
    docs += [doc(n, short=True) for n in MID_DOCS[:3]] + [doc(MID_DOCS[3], short="words")]  # (the last: no piece that only untrained has as a token)
    docs.append(_word(rng, ONE_PIECE_DOC))
    assert sum(map(len, docs)) <= 1 << 20
    for d in docs:
        d.decode("utf-8")
    return tuple(docs)


def text_census(C, docs, ranks) -> dict:
    """What the text holds, counted with the oracle's split: per length bin the pieces that are not tokens, the pieces of more than
    1 KiB, the pieces that are tokens of more than 23 bytes"""
    census = {"bins": [0] * len(BIN_HI), "over_1k": 0, "long_tokens": 0}
    for d in docs:
        a = 0
        for e in C.split(d):
            p, a = d[a:e], e
            if len(p) > 1024:
                census["over_1k"] += 1
            elif p in ranks:
                census["long_tokens"] += len(p) > 23
            elif len(p) >= 2:
                census["bins"][bin_of(len(p))] += 1
    return census
