"""Decode restated from the reference's rule (CoreBPE::decode_bytes, src/lib.rs:345-358: concatenate decoder[token] for every token, the
special tokens' decoder behind the ordinary one; KeyError for the first id without bytes) -- not from the kernels: bytes are a join over a
Python table, byte offsets are cumulative sums, the bad position is the first offending index.  Plus edge_vocab(), the vocabulary the
decode tests share (tests/test_decode_sim.py on the CPU, tests/test_gpu_decode.py on the device)."""
from __future__ import annotations

import functools

import numpy as np

SPEC_BIT = 0x80000000  # entry.x bit of the id -> {offset, length} table: the bytes live in the special-token blob
PAD = 16               # bytes the table builder leaves behind each blob (tk_tables.cpp)

LONG_LENGTHS = list(range(2, 41)) + [47, 48, 49, 63, 64, 65, 127, 128, 129, 255, 256, 300]
SPECIAL_LENGTHS = [1, 7, 8, 9, 16, 17, 40]


def token_bytes(k: int, n: int) -> bytes:
    """Byte j of token k depends on k and on j: a byte that is shifted, duplicated or taken from the wrong token shows."""
    return bytes((k * 31 + j * 7 + 1) & 0xFF for j in range(n))


def special_text(k: int, n: int, last: bool) -> str:
    """The same for a special token (ASCII, since it is text); `last`: sorts behind every other special token."""
    return ("~" if last else "<") + "".join(chr(0x30 + (k * 31 + j * 7 + 1) % 64) for j in range(1, n))


@functools.lru_cache(maxsize=None)
def edge_vocab():
    """(ranks, specials): the 256 single bytes; one token of every length in LONG_LENGTHS, ranks with holes in them (every third rank
    above 255 is left out), in rank order -- the last-ranked token, of 300 bytes, is the last in the blob; special tokens of the lengths
    in SPECIAL_LENGTHS, ids directly above the largest rank and the last one after a gap of 50 ids without entry -- it starts with '~', so
    that it is the last in its blob too (the builder sorts the special tokens by their bytes)."""
    ranks = {bytes([b]): b for b in range(256)}
    r = 256
    for i, n in enumerate(LONG_LENGTHS):
        ranks[token_bytes(r, n)] = r
        r += 2 if i % 3 == 2 and i + 1 < len(LONG_LENGTHS) else 1
    top = max(ranks.values())
    specials = {}
    for i, n in enumerate(SPECIAL_LENGTHS):
        last = i + 1 == len(SPECIAL_LENGTHS)
        k = top + 1 + i + (50 if last else 0)
        specials[special_text(k, n, last)] = k
    assert len(ranks) == 256 + len(LONG_LENGTHS) and len(specials) == len(SPECIAL_LENGTHS)
    return ranks, specials


class Table:
    """id -> bytes as the reference holds it (decoder first, then special_tokens_decoder), and the same as the device holds it: dec
    uint32[n_ids, 2] = {offset | SPEC_BIT, length} (length 0: no entry), the ordinary tokens' bytes back to back in the order given, the
    special tokens' sorted by their bytes, PAD zero bytes behind each."""

    def __init__(self, ranks: dict[bytes, int], specials: dict[str, int]):
        self.by_id = {v: k.encode() for k, v in specials.items()}
        self.by_id.update({r: t for t, r in ranks.items()})  # (an id both have: the ordinary token's bytes, lib.rs:347-351)
        self.special_ids = set(specials.values()) - set(ranks.values())
        self.n_ids = max(self.by_id) + 1
        self.dec = np.zeros((self.n_ids, 2), np.uint32)
        at = 0
        for t, r in ranks.items():
            self.dec[r] = (at, len(t))
            at += len(t)
        self.tok_blob = np.frombuffer(b"".join(ranks) + bytes(PAD), np.uint8)
        at, parts = 0, []
        for s in sorted(k.encode() for k in specials):
            i = specials[s.decode()]
            if i in self.special_ids:
                self.dec[i] = (at | SPEC_BIT, len(s))
            at += len(s)
            parts.append(s)
        self.spec_blob = np.frombuffer(b"".join(parts) + bytes(PAD), np.uint8)
        self.holes = [i for i in range(self.n_ids) if i not in self.by_id]
        self.len_of = {i: len(b) for i, b in self.by_id.items()}

    def id_of_len(self, n: int, special: bool = False) -> int:
        return next(i for i, b in self.by_id.items() if len(b) == n and (i in self.special_ids) == special and (n > 1 or special))

    def last_of_blob(self, special: bool) -> int:
        """The id whose bytes end its blob"""
        best = max((i for i in self.by_id if (i in self.special_ids) == special), key=lambda i: int(self.dec[i][0] & ~np.uint32(SPEC_BIT)))
        return best


@functools.lru_cache(maxsize=None)
def edge_table() -> Table:
    return Table(*edge_vocab())


def decode_ref(table: Table, tokens):
    """(bytes, byte offsets uint64[n + 1], None), or (None, None, position of the first id without bytes)"""
    tokens = [int(t) for t in tokens]
    for i, t in enumerate(tokens):
        if t not in table.by_id:
            return None, None, i
    off = np.zeros(len(tokens) + 1, np.uint64)
    if tokens:
        off[1:] = np.cumsum([len(table.by_id[t]) for t in tokens])
    return b"".join(table.by_id[t] for t in tokens), off, None


def doc_offsets_ref(byte_off, tok_off):
    """Byte offset of every document of a packed batch: that of its first token (byte_off: n + 1 entries, the last one the total)"""
    return np.asarray(byte_off, np.uint64)[np.asarray(tok_off, np.int64)]


# ---------------------------------------------------------------- batches both test files use
def alignment_sweep(table: Table, fill_id: int | None = None):
    """For every token length L of the vocabulary (ordinary and special), every destination alignment s in 0 .. 7 and every lane slot j in
    0 .. 7: a stretch that begins at a lane's first slot on a word boundary -- j filler tokens of 8 bytes, then s single bytes, then the
    token of length L, then single bytes up to the end of a lane of eight and one more lane of 8-byte tokens, so that the next stretch
    starts aligned again.  (Slots j + s > 7 wrap into the next lane: the token then sits at slot (j + s) % 8.)  Returns the ids."""
    eight = table.id_of_len(8) if fill_id is None else fill_id
    ids = sorted(i for i in table.by_id if table.len_of[i] > 1 or i in table.special_ids)
    out = []
    for t in ids:
        for s in range(8):
            for j in range(8):
                unit = [eight] * j + [(t * 7 + s + k) & 0xFF for k in range(s)] + [t]
                tail = (-len(unit)) % 8
                unit += [(t + j + k) & 0xFF for k in range(tail)]
                # back to a word boundary: single bytes up to a multiple of 8 bytes, in whole lanes
                nbytes = 8 * j + s + table.len_of[t] + tail
                pad = (-nbytes) % 8
                unit += [(t * 3 + k) & 0xFF for k in range(pad)] + [eight] * (8 - pad)
                assert len(unit) % 8 == 0 and (nbytes + pad) % 8 == 0
                out += unit
    return np.array(out, np.uint32)


def random_batch(table: Table, rng, n: int, long_share: float = 0.35, special_share: float = 0.15):
    """n ids, weighted towards long tokens and special tokens"""
    long_ids = [i for i in table.by_id if table.len_of[i] > 1 and i not in table.special_ids]
    spec_ids = sorted(table.special_ids)
    u = rng.random(n)
    out = rng.integers(0, 256, size=n)
    pick_long = u < long_share
    pick_spec = (u >= long_share) & (u < long_share + special_share)
    out[pick_long] = rng.choice(long_ids, size=int(pick_long.sum()))
    out[pick_spec] = rng.choice(spec_ids, size=int(pick_spec.sum()))
    return out.astype(np.uint32)
