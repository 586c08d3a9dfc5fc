"""Corpora for the training tests: inputs on which a wrong word table, a wrong position key or a wrong "no pair left" step changes the
merges.  Every builder returns Corpus(name, docs, pat_str, n_merges, meta) objects; tests/test_train_shapes.py shows with the restatement
alone (tests/train_ref.py) that each corpus meets the condition it was built for, tests/test_gpu_train_shapes.py runs them on the device.
Plain Python: nothing here touches the GPU or reads anything outside tests/.

The host's rules restated here (tiktoken_amd/csrc/tk_api.hip, train_words / train_tab_reserve / train_blob_reserve / ensure): a chunk is
the longest run of documents of at most `limit` bytes; before a chunk of P piece starts goes in, the word table has
pow2_at_least(1024, 2 * (NWORDS + P)) slots, and the blob has room for need = used + n + 64 bytes -- a new one is made for
need + need / 2, which the allocator rounds up by an eighth and 256 bytes."""
from __future__ import annotations

import random
from typing import NamedTuple

import regex

import helpers as h
import train_ref as tr

GPT2 = h.PAT_STR[0]
WHOLE = r"[\s\S]+"  # a document is one piece
GAPS = r"\p{L}+|\p{N}{1,3}|[^\s\p{L}\p{N}]+"  # white space is matched by nothing: gap chars
CHUNK = 4096  # the smallest TIKTOKEN_AMD_CHUNK_BYTES


class Corpus(NamedTuple):
    name: str
    docs: list
    pat_str: str
    n_merges: int
    meta: dict  # what the builder intends (test_train_shapes.py asserts it)


def nbytes(s: str) -> int:
    return len(s.encode("utf-8"))


# ---------------------------------------------------------------- the host's rules
def chunks_of(docs, limit=CHUNK):
    """[(d0, d1)]: the document ranges train_words cuts (a document above `limit` bytes is refused there: ValueError here)"""
    out, d0 = [], 0
    size = [nbytes(d) for d in docs]
    while d0 < len(docs):
        d1, total = d0, 0
        while d1 < len(docs) and total + size[d1] <= limit:
            total += size[d1]
            d1 += 1
        if d1 == d0:
            raise ValueError(f"document {d0} is longer than a chunk")
        out.append((d0, d1))
        d0 = d1
    return out


def piece_starts(doc: str, pat_str: str) -> int:
    """P of a chunk's document: the pieces and the gap chars (every char no piece covers is listed with bit 31 set)"""
    covered, n = 0, 0
    for m in regex.finditer(pat_str, doc):
        n += 1
        covered += m.end() - m.start()
    return n + len(doc) - covered


def pow2_at_least(floor, x):
    while floor < x:
        floor <<= 1
    return floor


def chunk_of_position(docs, limit=CHUNK):
    """corpus byte offset -> index of the chunk it lies in"""
    ends, at = [], 0
    size = [nbytes(d) for d in docs]
    for d0, d1 in chunks_of(docs, limit):
        at += sum(size[d0:d1])
        ends.append(at)
    return lambda pos: next(i for i, e in enumerate(ends) if pos < e)


def words_by_chunk(docs, pat_str, limit=CHUNK):
    """{word bytes: (first offset, [occurrences per chunk])} and the number of chunks"""
    where = chunk_of_position(docs, limit)
    n_chunks = len(chunks_of(docs, limit))
    out = {}
    for data, off in tr.pieces_of(docs, pat_str):
        e = out.setdefault(data, [off, [0] * n_chunks])
        e[0] = min(e[0], off)
        e[1][where(off)] += 1
    return {d: (f, c) for d, (f, c) in out.items()}, n_chunks


def predicted_moves(docs, pat_str, limit=CHUNK):
    """(table moves, blob moves) of a run in chunks of `limit` bytes by the host's sizing rules, and the chunks that have pieces"""
    slots = cap = words = used = table_moves = blob_moves = with_pieces = 0
    seen = set()
    for d0, d1 in chunks_of(docs, limit):
        n = sum(nbytes(d) for d in docs[d0:d1])
        P = sum(piece_starts(d, pat_str) for d in docs[d0:d1])
        if not n or not P:
            continue
        with_pieces += 1
        need = used + n + 64
        if need > cap:
            blob_moves += 1 if used else 0
            want = need + need // 2
            cap = want + want // 8 + 256
        want = pow2_at_least(1024, 2 * (words + P))
        if want > slots:
            table_moves += 1 if slots else 0
            slots = want
        for data, _ in tr.pieces_of(docs[d0:d1], pat_str):
            if data not in seen:
                seen.add(data)
                used += len(data)
        words = len(seen)
    return table_moves, blob_moves, with_pieces


# ---------------------------------------------------------------- growth
CONSONANTS = "bcdfghjklmnpqrstvwxz"


def consonant_word(i: int) -> str:
    """four consonants, word i of 160 000: consecutive i differ in every letter"""
    v = (i * 7919) % 160000
    return "".join(CONSONANTS[(v // 20 ** k) % 20] for k in range(4))


def growth() -> Corpus:
    """20 documents of 200 distinct words each under the GPT-2 pattern: the table and the blob outgrow what the first 4096-byte chunk got
    them.  " ae" and " io" come often, with different counts in the first chunk and behind it: the first steps depend on the sum."""
    docs = []
    for d in range(20):
        words = [consonant_word(200 * d + i) for i in range(200)]
        random.Random(d).shuffle(words)  # (which first letter a document meets first differs from document to document)
        docs.append(" ".join(words))
    docs[0] += " ae" * 130 + " io" * 60
    docs[6] += " ae" * 90
    docs[12] += " io" * 170
    return Corpus("growth", docs, GPT2, 24, {"repeated": [b" ae", b" io"]})


# ---------------------------------------------------------------- long words of one hash
CHAIN_LEN = 80  # 32 + 16 + 32
CHAIN_HEAD, CHAIN_TAIL = "x" * 32, "y" * 32


def chain_words(n=160, seed=80):
    """n words of CHAIN_LEN bytes that differ in bytes 32 .. 47 only: tk_train_hash reads the length, the first 32 and the last 32 bytes"""
    rng, out = random.Random(seed), []
    while len(out) < n:
        w = CHAIN_HEAD + "".join(rng.choice("abcd") for _ in range(CHAIN_LEN - 64)) + CHAIN_TAIL
        if w not in out:
            out.append(w)
    return out


def edge_words():
    """words at the lengths where the hash changes its form (64 / 65) and where tk_train_word8 reads a partial word (len - 32 no multiple
    of 8: 71, 95, 97; a multiple: 72, 96), and two of 64 and 65 bytes that agree on their first 64"""
    out = ["".join("pqrstuvw"[(7 * k + j * j) % 8] for j in range(k)) for k in (63, 64, 65, 71, 72, 95, 96, 97)]
    same64 = "mn" * 32
    return out + [same64, same64 + "m"]


def long_collide(spread: bool) -> Corpus:
    """One document = one word.  spread=False: the chain, the edge words, then some chain words again (one chunk by default).
    spread=True: the same words dealt over the corpus, short filler words between them, so that with 4096-byte chunks every chunk
    claims new slots on the chain with keys that name its text while the earlier ones name the blob, a later chunk repeats words of an
    earlier one, and the table (more than 512 words) is moved while it holds the chain."""
    chain, edges = chain_words(), edge_words()
    rng = random.Random(5)
    again = [chain[i] for i in rng.sample(range(len(chain)), 40)] + [chain[3]] * 4 + [edges[1], edges[8]]
    if not spread:
        return Corpus("long_collide", chain + edges + again, WHOLE, 48, {"chain": chain, "edges": edges})
    filler = ["".join("EFGHJKLM"[(i >> (3 * k)) & 7] for k in range(3)) + "Z" for i in range(512)]  # 512 distinct words of 4 bytes
    docs = []
    for i, w in enumerate(chain):
        docs.append(w)
        docs += filler[3 * i: 3 * i + 3]
        if i % 16 == 15:
            docs.append(edges[(i // 16) % len(edges)])
        if i >= 60 and i % 4 == 0:
            docs.append(again[(i - 60) // 4])  # a word of an earlier chunk again
    docs += edges + filler[3 * len(chain):] + again
    return Corpus("long_collide_spread", docs, WHOLE, 48, {"chain": chain, "edges": edges})


def merged_pair_changes(words, chain, n_merges):
    """For every ordered pair (i, j) of `chain` (bytes): does the restatement's result change when word j is taken for word i (its weight
    goes to i, its bytes are gone)?  Returns (decided, undecided): the number of pairs for which a step's largest count provably differs,
    and the list of pairs for which that argument does not decide (the caller runs the restatement on those).

    The argument: follow the true run step by step.  While a damaged run has made the true merges, every word stands as in the true run, so
    its pair counts are the true ones plus weight[j] * (pairs of i - pairs of j); if the largest of them is not the true cmax of that
    step, `counts` differ.  If it has not made the true merges before, `pairs` differ already."""
    import numpy as np

    index = {w.data: k for k, w in enumerate(words)}
    ids = [index[c] for c in chain]
    weight = np.array([w.weight for w in words], np.int64)
    syms = [list(w.data) for w in words]
    true = tr.train_words(words, n_merges)
    changed = np.zeros((len(ids), len(ids)), bool)
    for k in range(n_merges):
        cols = {}
        for s in syms:
            for p in zip(s[:-1], s[1:]):
                cols.setdefault(p, len(cols))
        N = np.zeros((len(words), len(cols)), np.int64)
        for wi, s in enumerate(syms):
            for p in zip(s[:-1], s[1:]):
                N[wi, cols[p]] += 1
        c = weight @ N
        assert int(c.max()) == true.counts[k]
        C = N[ids]
        for x, i in enumerate(ids):
            damaged = c[None, :] + weight[ids][:, None] * (C[x][None, :] - C)  # row y: word ids[y] taken for word i
            changed[x] |= damaged.max(axis=1) != true.counts[k]
        a, b = true.pairs[k]
        for wi, s in enumerate(syms):
            ns, i = [], 0
            while i < len(s):
                if i + 1 < len(s) and s[i] == a and s[i + 1] == b:
                    ns.append(256 + k)
                    i += 2
                else:
                    ns.append(s[i])
                    i += 1
            syms[wi] = ns
    np.fill_diagonal(changed, True)
    undecided = [(chain[x], chain[y]) for x, y in zip(*np.nonzero(~changed))]
    return int(changed.sum()) - len(ids), undecided


def with_word_taken_for(words, keep: bytes, gone: bytes):
    """the words as a table leaves them that took `gone` for `keep`: one word, the weights added, the smaller offset"""
    k = next(w for w in words if w.data == keep)
    g = next(w for w in words if w.data == gone)
    return [tr.Word(keep, k.weight + g.weight, min(k.first, g.first)) if w.data == keep else w for w in words if w.data != gone]


# ---------------------------------------------------------------- gap chars
def gap_words(rng, n):
    vocab = ["the", "of", "and", "tokens", "merge", "rule", "étude", "naïve", "中文", "2024", "7", "99", "1234567", "...", "!", "(", ");", "->", "don't"]
    return [rng.choice(vocab) for _ in range(n)]


def gaps(chunked: bool) -> Corpus:
    """Documents that begin with a gap char, end with one, hold nothing else, are empty, and hold gap chars of two and three bytes
    (U+00A0, U+3000).  chunked=False: about 1 KB, one chunk whatever the core.  chunked=True: documents of up to 4096 bytes, so that with
    4096-byte chunks every document edge below is a chunk edge as well, and the chunk in the middle is gap chars only."""
    rng = random.Random(31)
    if not chunked:
        docs = [" begins with a gap", "ends with a gap\n", " \t\n　  ", "", "　wide　gaps inside ", " ",
                "no gap", " ".join(gap_words(rng, 120)), "", "\n\n" + "　".join(gap_words(rng, 60)) + "　"]
        return Corpus("gaps", docs, GAPS, 24, {})

    def text(size, sep):
        out = ""
        while True:
            more = out + rng.choice(sep) + rng.choice(gap_words(rng, 1))
            if nbytes(more) > size:
                return out
            out = more

    first = text(4000, [" ", "\n", "　"]) + " 　"  # begins with a gap (a separator), ends with a three-byte one
    only_gaps = "".join(rng.choice([" ", "\n", "\t", "　", " "]) for _ in range(2300))
    while nbytes(only_gaps) > CHUNK:
        only_gaps = only_gaps[:-1]
    last = " " + text(3800, [" ", " ", "\r\n"]).lstrip() + "\n"  # begins with a two-byte gap char
    middle = text(4090, [" "])[1:]  # begins and ends with a piece
    docs = [first, only_gaps, "", middle, "", last, " "]
    return Corpus("gaps_chunked", docs, GAPS, 24, {"gap_chunk": 1})


def only_gaps_corpus() -> Corpus:
    return Corpus("gaps_only", [" \n", "", "　　\t", " "], GAPS, 3, {})


# ---------------------------------------------------------------- ties across chunks
TIE_TARGETS = [0, 2, 3, 1, 3, 0]  # the chunk in which the winner of step s stands
TIE_COUNTS = [120, 116, 112, 108, 104, 100]


def ties() -> Corpus:
    """Four chunks of one document each (4096-byte chunks), empty documents between them.  Step s is decided between two pairs of one
    count, TIE_COUNTS[s]: (a, b) of the words "ab" and "abc" and (b, c) of "abc" and "bc", half the count from each word; merging (a, b)
    halves (b, c), so the next step is the next group's.  "ab" is first seen late in chunk TIE_TARGETS[s], "abc" and "bc" early in the
    next chunk (in the last chunk: behind it): the winner is (a, b) by its position alone, and positions kept relative to the chunk
    would make (b, c) win.  The other occurrences lie in the chunks behind, the rest is words of capital letters whose pairs stay rare."""
    rng = random.Random(17)
    letters = "abcdefghijklmnopqr"
    n_chunks = 4
    early = [[] for _ in range(n_chunks)]
    late = [[] for _ in range(n_chunks)]
    tail = []  # behind the late words of the last chunk
    reps = [[] for _ in range(n_chunks)]
    groups = []
    for s, (t, cnt) in enumerate(zip(TIE_TARGETS, TIE_COUNTS)):
        a, b, c = letters[3 * s: 3 * s + 3]
        groups.append((a, b, c))
        half = cnt // 2
        late[t].append(a + b)
        rival = min(t + 1, n_chunks - 1)
        (early[rival] if rival != t else tail).extend([b + c, a + b + c])
        for w, first_chunk in ((a + b, t), (a + b + c, rival), (b + c, rival)):
            left = half - 1
            if first_chunk == n_chunks - 1:
                tail.extend([w] * left)
                continue
            behind = list(range(first_chunk + 1, n_chunks))
            for i in range(left):
                reps[behind[i % len(behind)]].append(w)
    docs = []
    for j in range(n_chunks):
        rng.shuffle(reps[j])
        fixed = early[j] + reps[j] + late[j] + (tail if j == n_chunks - 1 else [])
        room = 3600 - sum(len(w) + 1 for w in fixed)
        assert room > 400, (j, room)
        filler = []
        while room > 0:
            filler.append("".join(rng.choice("ABCDEFGHIJKLMNOPQRSTUVWXYZ") for _ in range(rng.randrange(4, 9))))
            room -= len(filler[-1]) + 1
        docs += [" ".join(early[j] + reps[j] + filler + late[j] + (tail if j == n_chunks - 1 else [])), ""]
        if j == 1:
            docs.append("")
    return Corpus("ties", docs, GAPS, 12, {"groups": groups, "targets": TIE_TARGETS, "counts": TIE_COUNTS})


# ---------------------------------------------------------------- running out of pairs
def exhaust():
    """meta["done"]: the step that finds no pair, by hand.  One document = one word."""
    return [
        Corpus("exhaust_step0_three_bytes", ["a", "b", "c"], WHOLE, 3, {"done": 0}),  # N = 3 symbols and no pair
        Corpus("exhaust_step0_repeats", ["a", "", "b", "a", "\n", "b"], WHOLE, 1, {"done": 0}),
        # abab cd: (a, b) twice; then XX and cd once each, XX stands first; then cd; then nothing
        Corpus("exhaust_middle", ["abab", "cd", "abab"], WHOLE, 8, {"done": 3}),
        # aaaa b: (a, a) three times -> XX; (X, X) -> one symbol; step 2 of 4 finds nothing
        Corpus("exhaust_last_but_one", ["aaaa", "b"], WHOLE, 4, {"done": 2}),
        # hello help: he, hel, then (hel, l) / (l, o) / (hel, p) once each: three more steps, one symbol each after five merges
        Corpus("exhaust_last_but_one_words", ["hello", "help", "x", "help"], WHOLE, 7, {"done": 5}),
    ]


# ---------------------------------------------------------------- the seeded sweep
SWEEP_SEED = 2  # (7 of its 40 samples run out of pairs, under four of the five patterns: test_train_shapes.py)
SWEEP_SAMPLES = 40
PATTERNS = {"gpt2": h.PAT_STR[0], "cl100k": h.PAT_STR[1], "o200k": h.PAT_STR[2], "gaps": GAPS, "whole": WHOLE}
SWEEP_PATTERNS = tuple(PATTERNS)


def sweep_sample(i: int, seed: int = SWEEP_SEED):
    """(pattern name, docs, n_merges) of sample i: 0 .. 12 documents of 0 .. 1500 bytes (short ones far more often than long ones) over
    2 .. 5 letters, a space, a digit, an apostrophe, é, 中 and 🙂; 1 .. 48 merges"""
    rng = random.Random(f"train sweep {seed} {i}")
    alphabet = rng.sample("abcde", rng.randrange(2, 6)) + [" ", "7", "'", "é", "中", "🙂"]
    weights = [8] * (len(alphabet) - 6) + [5, 2, 1, 1, 1, 1]
    docs = []
    for _ in range(rng.randrange(0, 13)):
        size = int(1500 * rng.random() ** 3) if rng.random() < 0.85 else 0
        chars, total = [], 0
        while True:
            ch = rng.choices(alphabet, weights)[0]
            if total + nbytes(ch) > size:
                break
            chars.append(ch)
            total += nbytes(ch)
        docs.append("".join(chars))
    return SWEEP_PATTERNS[i % len(SWEEP_PATTERNS)], docs, rng.randrange(1, 49)
