"""A Python restatement of the training rule (include/tiktoken_amd.h, tk_train_bpe), written from that description -- not from the kernels,
and not from the reference's trainer.  Words are the distinct pieces with a weight and the corpus offset of their first occurrence; a
symbol keeps the offset of its first byte; a step counts the adjacent pairs inside words, weighted, the winner is the pair at the
smallest position among the pairs with the largest count, and every word is rewritten from left to right."""
from __future__ import annotations

from typing import NamedTuple, Sequence

import base64
import functools
import gzip
import json
import os

import regex


class Word(NamedTuple):
    data: bytes
    weight: int
    first: int  # corpus offset of the first occurrence


class Trained(NamedTuple):
    pairs: list  # [(left, right)] per merge
    counts: list  # cmax of each step
    symbols: list  # [(position, symbol)] of the distinct words after the last step, ascending positions


class Exhausted(ValueError):
    """A step found no pair (the reference's max() over an empty Counter).  `done`: the merges made before; `partial`: their Trained."""

    def __init__(self, done: int, partial: "Trained"):
        super().__init__(f"no pair left after {done} merges")
        self.done, self.partial = done, partial


def pieces_of(docs: Sequence[str], pat_str: str):
    """(bytes, corpus byte offset) of every piece regex.findall yields, document by document; unmatched chars are no pieces."""
    out, base = [], 0
    pat = regex.compile(pat_str)
    for doc in docs:
        at_char, at_byte = 0, 0
        for m in pat.finditer(doc):
            at_byte += len(doc[at_char:m.start()].encode("utf-8"))
            at_char = m.start()
            out.append((m.group(0).encode("utf-8"), base + at_byte))
        base += len(doc.encode("utf-8"))
    return out


def distinct_words(pieces) -> list[Word]:
    """Equal pieces are one word: weight = occurrences, first = the smallest offset."""
    seen: dict[bytes, list] = {}
    for data, off in pieces:
        if not data:
            continue
        w = seen.setdefault(data, [0, off])
        w[0] += 1
        w[1] = min(w[1], off)
    return [Word(d, w, f) for d, (w, f) in seen.items()]


def train_words(words: Sequence[Word], n_merges: int) -> Trained:
    syms = [list(w.data) for w in words]
    offs = [list(range(len(w.data))) for w in words]  # offset of every symbol's first byte inside its word
    pairs, counts = [], []
    for k in range(n_merges):
        cnt: dict[tuple, int] = {}
        for w, s in zip(words, syms):
            for p in zip(s[:-1], s[1:]):
                cnt[p] = cnt.get(p, 0) + w.weight
        if not cnt:
            raise Exhausted(k, Trained(pairs, counts, _symbols(words, syms, offs)))
        cmax = max(cnt.values())
        best = None
        for w, s, o in zip(words, syms, offs):
            for i in range(len(s) - 1):
                if cnt[(s[i], s[i + 1])] == cmax and (best is None or w.first + o[i] < best[0]):
                    best = (w.first + o[i], (s[i], s[i + 1]))
        a, b = best[1]
        pairs.append((a, b))
        counts.append(cmax)
        new = 256 + k
        for wi, (s, o) in enumerate(zip(syms, offs)):
            ns, no, i = [], [], 0
            while i < len(s):
                if i + 1 < len(s) and s[i] == a and s[i + 1] == b:
                    ns.append(new)
                    no.append(o[i])  # (a merged symbol keeps the offset of its left part)
                    i += 2
                else:
                    ns.append(s[i])
                    no.append(o[i])
                    i += 1
            syms[wi], offs[wi] = ns, no
    return Trained(pairs, counts, _symbols(words, syms, offs))


def _symbols(words, syms, offs):
    return sorted((w.first + off, sym) for w, s, o in zip(words, syms, offs) for sym, off in zip(s, o))


def ranks_of(pairs) -> dict[bytes, int]:
    tokens = [bytes([b]) for b in range(256)]
    for a, b in pairs:
        tokens.append(tokens[a] + tokens[b])
    return {t: i for i, t in enumerate(tokens)}


def train_text(data, vocab_size: int, pat_str: str) -> Trained:
    if vocab_size < 256:
        raise ValueError("vocab_size must be at least 256")
    docs = [data] if isinstance(data, str) else list(data)
    return train_words(distinct_words(pieces_of(docs, pat_str)), vocab_size - 256)


@functools.lru_cache(maxsize=None)
def load_cases():
    """(texts by name, cases) of tests/golden/train_cases.json.gz: what the reference's own trainer returned (tools/gen_golden_train.py)"""
    with gzip.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_cases.json.gz")) as f:
        g = json.loads(f.read().decode("utf-8"))
    return g["texts"], g["cases"]


def case_ranks(case) -> dict[bytes, int]:
    return {base64.b64decode(t): i for i, t in enumerate(case["tokens"])}
