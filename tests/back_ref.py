"""The back end's rule, restated from its description (not from the kernels): a chunk is a list of pieces in text order, each with the
tokens it encodes to (none for a gap char); the chunk's tokens are every piece's tokens in order, and tok_off[d] is the number of tokens
before the piece that starts at doc_off[d] -- the chunk's token count for a document at or behind the end of the text -- plus the tokens of
the chunks before.  Beside it, the builder of the synthetic device state the simulation reads (tests/test_back_sim.py)."""
from dataclasses import dataclass

import numpy as np

TILE, CAP = 3840, 4096
FLAG, GAP, NONE = 0x80000000, 0x7FFFFFFF, 0xFFFFFFFF
INLINE, INLINE_BIT = 13, 0x40000000


@dataclass
class Piece:
    start: int                  # byte offset in the chunk
    tokens: list                # [] for a gap char
    kind: str = "auto"          # token | gap | table | ovf | noentry (a missed piece the front kernel had no entry for: the token 0)


def rule(pieces, doc_off, n, tok_base=0):
    """(tokens, tok_off) of the chunk"""
    flat, before = [], {}
    for p in pieces:
        before[p.start] = len(flat)
        flat.extend(p.tokens)
    tok_off = [tok_base + (len(flat) if pos >= n else before[pos]) for pos in doc_off]
    return np.array(flat, np.uint32), np.array(tok_off, np.uint64)


@dataclass
class Device:
    """What the front stage and the merge kernels leave for the back end"""
    n: int
    ntiles: int
    tile_np: np.ndarray
    res: np.ndarray
    tab: np.ndarray
    ovf: np.ndarray
    cnt8: np.ndarray
    staging: np.ndarray
    starts: np.ndarray
    doc_off: np.ndarray
    doc_first: np.ndarray
    ovf_base: int


def build(pieces, doc_off, n, res_words, starts_words, ovf_base=64, rng=None):
    """Result words with their tails, the entries (a table of ovf_base slots, overflow entries behind it), the start bitmap, doc_first.
    kind "auto": one token -> a token word, none -> a gap char, else a table slot while there are free ones (tokens inline up to INLINE,
    in the staging area beyond), then overflow entries."""
    rng = rng or np.random.default_rng(1)
    ntiles = max(1, -(-n // TILE))
    res = np.full(res_words, 0xDEADBEEF, np.uint32)
    starts = np.zeros(starts_words, np.uint32)
    tile_np = np.zeros(ntiles, np.uint32)
    tab = np.full((max(ovf_base, 1), 16), 0xABABABAB, np.uint32)
    cnt8 = np.full(ovf_base + 16, 77, np.uint8)
    ovf, staging = [[0, 0, 0, 0]], []  # (overflow entry 0 is what a lane without an entry reads, so the first real one is entry 1 here)
    free = list(rng.permutation(ovf_base)) if ovf_base else []
    tails, words = [[] for _ in range(ntiles)], [[] for _ in range(ntiles)]
    ngap = [0] * ntiles
    last = -1
    for p in pieces:
        assert last < p.start < n, "pieces in text order, inside the text"
        last = p.start
        t = p.start // TILE
        tile_np[t] += 1
        starts[p.start >> 5] |= np.uint32(1 << (p.start & 31))
        cnt = len(p.tokens)
        kind = p.kind
        if kind == "auto":
            kind = "gap" if cnt == 0 else "token" if cnt == 1 else "table" if free else "ovf"
        if kind == "token":
            assert cnt == 1 and p.tokens[0] < GAP
            word = p.tokens[0]
        elif kind == "gap":
            assert cnt == 0
            word = GAP
            ngap[t] += 1
        elif kind == "noentry":
            assert p.tokens == [0]
            word = 0
            tails[t].append(NONE)
        else:
            assert cnt >= 1
            if kind == "table" and free:  # (a table without free slots: an overflow entry)
                e = int(free.pop())
                tab[e, :3] = (p.start, 2, cnt)
                if cnt == 1:
                    tab[e, 3] = p.tokens[0]
                elif cnt <= INLINE:
                    tab[e, 2] |= INLINE_BIT
                    tab[e, 3:3 + cnt] = p.tokens
                else:
                    tab[e, 3] = len(staging)
                    staging.extend(p.tokens)
                cnt8[e] = min(cnt, 255)
            else:
                e = ovf_base + len(ovf)
                ovf.append([p.start, 2, cnt, p.tokens[0] if cnt == 1 else len(staging)])
                if cnt > 1:
                    staging.extend(p.tokens)
            word = FLAG | e
            tails[t].append(e)
        words[t].append(word)
    for t in range(ntiles):
        assert tile_np[t] + len(tails[t]) + 2 <= CAP, "the tail fits behind the pieces"
        order = rng.permutation(len(tails[t]))  # (in no particular order)
        for q, i in enumerate(order):
            res[t * CAP + CAP - 3 - q] = tails[t][i]
        if tile_np[t]:
            res[t * CAP + CAP - 2] = ngap[t]
            res[t * CAP + CAP - 1] = len(tails[t])
        res[t * CAP: t * CAP + len(words[t])] = words[t]
    doc_first = np.full(ntiles + 1, NONE, np.uint32)
    for d, pos in enumerate(doc_off[:-1]):
        t = pos // TILE if pos < n else ntiles
        doc_first[t] = min(int(doc_first[t]), d)
    return Device(n, ntiles, tile_np, res, tab.reshape(-1), np.array(ovf, np.uint32).reshape(-1), cnt8, np.array(staging + [0], np.uint32), starts,
                  np.array(doc_off, np.uint64), doc_first, ovf_base)

