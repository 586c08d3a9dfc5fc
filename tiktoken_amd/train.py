"""Training BPE vocabularies on the GPU: the merges the reference's educational trainer makes (tiktoken/_educational.py: `bpe_train`), the
same pairs in the same order, so the returned dict has the reference's ids and insertion order.

The pre-tokeniser cuts the text into pieces under `pat_str`; the distinct pieces become weighted words; every merge counts the adjacent
pairs, picks the most frequent one -- ties go to the pair that occurs first in the text -- and rewrites the words (tk_train_bpe; the rule
is written out in include/tiktoken_amd.h).  This module packs the text, calls the core and assembles the byte strings.

Not built: a merge whose bytes spell a token that exists already (two different pairs with the same concatenation).  The reference
overwrites the dict entry there and runs one step more, which leaves ids with holes; `merges_to_ranks` refuses such a list loudly.
"""
from __future__ import annotations

from typing import Iterable, Sequence

import numpy as np

from . import _tiktoken


def merges_to_ranks(pairs: Iterable[Sequence[int]]) -> dict[bytes, int]:
    """The vocabulary a list of merges stands for: the 256 bytes, ids 0..255, then merge k -- the pair (left, right) of earlier ids -- as
    id 256 + k with the bytes of its two parts joined.  ValueError for a pair that names an id that does not exist yet; RuntimeError,
    naming the two pairs, for a merge that spells an existing token."""
    tokens = [bytes([b]) for b in range(256)]
    ranks = {t: i for i, t in enumerate(tokens)}
    made_by: dict[bytes, tuple[int, int]] = {}
    for k, pair in enumerate(pairs):
        left, right = int(pair[0]), int(pair[1])
        if not (0 <= left < len(tokens) and 0 <= right < len(tokens)):
            raise ValueError(f"merge {k} joins ({left}, {right}), but only ids below {len(tokens)} exist by then")
        spelled = tokens[left] + tokens[right]
        if spelled in ranks:
            other = made_by.get(spelled)
            what = f"merge {ranks[spelled] - 256} = {other}" if other is not None else f"byte {ranks[spelled]}"
            raise RuntimeError(f"merge {k} = ({left}, {right}) spells {spelled!r}, which {what} spells already: duplicate spellings are not built")
        ranks[spelled] = len(tokens)
        made_by[spelled] = (left, right)
        tokens.append(spelled)
    return ranks


def _pack(data: "str | Sequence[str]") -> tuple[np.ndarray, np.ndarray]:
    docs = [data] if isinstance(data, str) else list(data)
    raw = [d.encode("utf-8") for d in docs]  # strict: a lone surrogate raises UnicodeEncodeError, as in the reference
    off = np.zeros(len(raw) + 1, dtype=np.uint64)
    if raw:
        np.cumsum(np.fromiter((len(b) for b in raw), dtype=np.uint64, count=len(raw)), out=off[1:])
    blob = np.frombuffer(b"".join(raw), dtype=np.uint8)
    return blob, off


def bpe_train(data: "str | Sequence[str]", vocab_size: int, pat_str: str, *, device: int | None = None) -> dict[bytes, int]:
    """`tiktoken._educational.bpe_train(data, vocab_size, pat_str, visualise=None)` on the GPU.  `data`: one text or several documents
    (pieces never cross a document boundary; several documents train as the reference trains on each document's pieces in turn)."""
    if vocab_size < 2**8:
        raise ValueError("vocab_size must be at least 256, so we can encode all bytes")
    blob, off = _pack(data)
    core = _tiktoken.CoreBPE({bytes([b]): b for b in range(256)}, {}, pat_str, devices=[device if device is not None else _tiktoken.default_devices()[0]])
    try:
        pairs, _ = core.train_bpe_packed(blob, off, vocab_size)
    finally:
        core.close()
    return merges_to_ranks(pairs.tolist())


def train_encoding(name: str, data: "str | Sequence[str]", vocab_size: int, pat_str: str, *, special_tokens: dict[str, int] | None = None):
    """An `Encoding` over a freshly trained vocabulary of `vocab_size` mergeable tokens."""
    from .core import Encoding

    return Encoding(name, pat_str=pat_str, mergeable_ranks=bpe_train(data, vocab_size, pat_str), special_tokens=dict(special_tokens or {}))
