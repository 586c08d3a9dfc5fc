"""The corpora of tests/train_shapes.py can expose a wrong kernel: each meets the condition it was built for, shown with the restatement
(tests/train_ref.py) and the host's sizing rules alone.  No GPU here; tests/test_gpu_train_shapes.py runs the same corpora on the device."""
import ctypes

import pytest

import test_train_sim as sim
import train_ref as tr
import train_shapes as ts

FAR = 1 << 40  # added to a damaged `first`: behind every true position


def result(c: ts.Corpus, words=None):
    return tr.train_words(words if words is not None else tr.distinct_words(tr.pieces_of(c.docs, c.pat_str)), c.n_merges)


def all_corpora():
    return [ts.growth(), ts.long_collide(False), ts.long_collide(True), ts.gaps(False), ts.gaps(True), ts.only_gaps_corpus(), ts.ties()] + ts.exhaust()


def test_sizes():
    """under 40 KB, at most 64 merges, no document above a 4096-byte chunk"""
    names = set()
    for c in all_corpora():
        assert sum(map(ts.nbytes, c.docs)) < 40000 and 1 <= c.n_merges <= 64, c.name
        ts.chunks_of(c.docs)
        names.add(c.name)
    assert len(names) == len(all_corpora())


def damaged_first(c: ts.Corpus):
    """the words after a move that lost `first` of the words it moved: those first seen in the first chunk"""
    by_chunk, _ = ts.words_by_chunk(c.docs, c.pat_str)
    where = ts.chunk_of_position(c.docs)
    return [tr.Word(w.data, w.weight, w.first + FAR if where(by_chunk[w.data][0]) == 0 else w.first) for w in tr.distinct_words(tr.pieces_of(c.docs, c.pat_str))]


def test_growth_moves_table_and_blob():
    c = ts.growth()
    table, blob, chunks = ts.predicted_moves(c.docs, c.pat_str)
    assert table >= 2 and blob >= 1 and chunks >= 5
    assert ts.predicted_moves(c.docs, c.pat_str, limit=512 << 20) == (0, 0, 1)  # (one chunk: nothing moves)
    by_chunk, n_chunks = ts.words_by_chunk(c.docs, c.pat_str)
    assert len(by_chunk) > 3900  # most words are distinct
    for w in c.meta["repeated"]:  # different counts in the first chunk and behind it
        per = by_chunk[w][1]
        assert per[0] > 0 and sum(per[1:]) > 0 and per[0] != sum(per[1:])


@pytest.mark.parametrize("name", ["growth", "ties"])
def test_a_lost_first_changes_the_merges(name):
    c = ts.growth() if name == "growth" else ts.ties()
    true, bad = result(c), result(c, damaged_first(c))
    assert true.counts == bad.counts  # (positions decide among equal counts, nothing else)
    assert true.pairs != bad.pairs
    print(name, "first step that differs:", next(k for k in range(c.n_merges) if true.pairs[k] != bad.pairs[k]))


def test_growth_a_lost_weight_changes_the_merges():
    """a move that lost the weights: the words of the first chunk count from the second chunk on"""
    c = ts.growth()
    by_chunk, _ = ts.words_by_chunk(c.docs, c.pat_str)
    words = tr.distinct_words(tr.pieces_of(c.docs, c.pat_str))
    bad = [tr.Word(w.data, sum(by_chunk[w.data][1][1:]), w.first) if by_chunk[w.data][1][0] else w for w in words]
    assert any(b.weight for b, w in zip(bad, words) if b.weight != w.weight)
    true, lost = result(c), result(c, bad)
    assert true.pairs[:10] != lost.pairs[:10] and true.counts[:10] != lost.counts[:10]  # a step among the first ten depends on them
    rep = {tuple(w[i:i + 2]) for w in c.meta["repeated"] for i in range(len(w) - 1)}
    assert any(p in rep for p in true.pairs[:10])


def train_hash(word: bytes, seed=sim.SEED):
    L = sim.lib()
    L.train_sim_hash.restype = ctypes.c_uint64
    L.train_sim_hash.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint64]
    return L.train_sim_hash(word, len(word), seed)


@pytest.mark.parametrize("spread", [False, True])
def test_long_words_share_a_hash(spread):
    """the production seed: one hash for the whole chain, and different hashes around the lengths where the hash changes its form"""
    c = ts.long_collide(spread)
    chain = [w.encode() for w in c.meta["chain"]]
    assert len(set(chain)) == len(chain) >= 150 and {len(w) for w in chain} == {ts.CHAIN_LEN} and ts.CHAIN_LEN > 64
    assert len({w[:32] for w in chain}) == 1 and len({w[-32:] for w in chain}) == 1
    assert len({train_hash(w) for w in chain}) == 1
    edges = [w.encode() for w in c.meta["edges"]]
    assert [len(w) for w in edges] == [63, 64, 65, 71, 72, 95, 96, 97, 64, 65] and edges[9][:64] == edges[8]
    assert len({train_hash(w) for w in edges + chain[:1]}) == len(edges) + 1
    assert train_hash(b"ab", 0) == train_hash(b"ac", 0) and train_hash(b"ab") != train_hash(b"ac")  # (the test seed collides, this one does not)
    by_chunk, n_chunks = ts.words_by_chunk(c.docs, c.pat_str)
    assert set(chain + edges) <= set(by_chunk)
    repeated = [w for w in chain if sum(by_chunk[w][1]) > 1]
    assert len(repeated) >= 20 and max(sum(by_chunk[w][1]) for w in chain) >= 4  # weights matter
    first_chunks = {ts.chunk_of_position(c.docs)(by_chunk[w][0]) for w in chain}
    assert len(first_chunks) >= 3  # with 4096-byte chunks: chain words claimed in at least three chunks
    if spread:
        table, blob, _ = ts.predicted_moves(c.docs, c.pat_str)
        assert table >= 1 and blob >= 1
        later = [w for w in chain if sum(1 for n in by_chunk[w][1] if n) > 1]
        assert len(later) >= 20  # words that meet their own key in the blob


@pytest.mark.parametrize("spread", [False, True])
def test_taking_one_chain_word_for_another_changes_the_merges(spread):
    c = ts.long_collide(spread)
    words = tr.distinct_words(tr.pieces_of(c.docs, c.pat_str))
    chain = [w.encode() for w in c.meta["chain"]]
    decided, undecided = ts.merged_pair_changes(words, chain, c.n_merges)
    assert decided + len(undecided) == len(chain) * (len(chain) - 1) and len(undecided) < 60, len(undecided)
    true = result(c, words)
    for keep, gone in undecided:  # the argument about counts does not decide these: run them
        bad = result(c, ts.with_word_taken_for(words, keep, gone))
        assert (bad.pairs, bad.counts) != (true.pairs, true.counts), (keep, gone)
    # the argument itself, on a sample: what it calls changed is changed
    open_pairs = set(undecided)
    sample = [(chain[i], chain[j]) for i, j in ((0, 1), (1, 0), (5, 150), (77, 12), (159, 158))]
    for keep, gone in sample:
        if (keep, gone) not in open_pairs:
            bad = result(c, ts.with_word_taken_for(words, keep, gone))
            assert bad.counts != true.counts or bad.pairs != true.pairs


def step_pairs(words, k):
    """{pair: [weighted count, smallest position]} as step k of the restatement finds them: the symbols after k merges, word by word"""
    symbols = tr.train_words(words, k).symbols
    spans = sorted((w.first, w.first + len(w.data), w.weight) for w in words)
    out, si = {}, 0
    for (p0, s0), (p1, s1) in zip(symbols[:-1], symbols[1:]):
        while spans[si][1] <= p0:
            si += 1
        lo, hi, weight = spans[si]
        assert lo <= p0 < hi
        if p1 < hi:
            e = out.setdefault((s0, s1), [0, p0])
            e[0] += weight
            e[1] = min(e[1], p0)
    return out


def test_ties_winners_move_between_chunks():
    c = ts.ties()
    assert len(ts.chunks_of(c.docs)) == 4 and c.docs.count("") >= 4
    assert {0, 3} < set(c.meta["targets"]) and set(c.meta["targets"]) & {1, 2}  # the first, a middle one, the last
    words = tr.distinct_words(tr.pieces_of(c.docs, c.pat_str))
    where = ts.chunk_of_position(c.docs)
    true = result(c, words)
    for k, (target, count, (a, b, cc)) in enumerate(zip(c.meta["targets"], c.meta["counts"], c.meta["groups"])):
        found = step_pairs(words, k)
        cmax = max(n for n, _ in found.values())
        tied = {p: pos for p, (n, pos) in found.items() if n == cmax}
        assert cmax == count == true.counts[k] and len(tied) >= 2, (k, cmax, tied)
        winner = min(tied, key=tied.get)
        assert winner == true.pairs[k] == (ord(a), ord(b)) and where(tied[winner]) == target, (k, winner, tied)
        rivals = {where(pos) for p, pos in tied.items() if p != winner}
        assert rivals == ({target + 1} if target < 3 else {3})  # the loser stands in the next chunk (the last chunk: behind the winner)


def test_gap_documents():
    pat = ts.regex.compile(ts.GAPS)

    def is_gap(ch):
        return not pat.match(ch)

    for c in (ts.gaps(False), ts.gaps(True)):
        docs = c.docs
        assert any(d and is_gap(d[0]) for d in docs) and any(d and is_gap(d[-1]) for d in docs) and "" in docs
        assert any(d and all(map(is_gap, d)) for d in docs)
        assert any("　" in d for d in docs) and any(" " in d for d in docs)
        result(c)  # (no Exhausted)
    one, cut = ts.gaps(False), ts.gaps(True)
    assert sum(map(ts.nbytes, one.docs)) < ts.CHUNK
    chunks = ts.chunks_of(cut.docs)
    pieces = [len(tr.pieces_of(cut.docs[d0:d1], cut.pat_str)) for d0, d1 in chunks]
    assert len(chunks) == 4 and pieces[cut.meta["gap_chunk"]] == 0 and all(n > 0 for i, n in enumerate(pieces) if i != cut.meta["gap_chunk"])
    firsts, lasts = [cut.docs[d0][0] for d0, _ in chunks], [[d for d in cut.docs[d0:d1] if d][-1][-1] for d0, d1 in chunks]
    assert any(map(is_gap, firsts)) and not all(map(is_gap, firsts)) and "　" in lasts and " " in firsts  # gaps on chunk edges, of several bytes too
    with pytest.raises(tr.Exhausted) as e:
        result(ts.only_gaps_corpus())
    assert e.value.done == 0 and not tr.pieces_of(ts.only_gaps_corpus().docs, ts.GAPS)


def test_exhaust_steps():
    cases = ts.exhaust()
    for c in cases:
        with pytest.raises(tr.Exhausted) as e:
            result(c)
        assert e.value.done == c.meta["done"] < c.n_merges, c.name
        part = tr.train_text(c.docs, 256 + c.meta["done"], c.pat_str)  # exactly that many merges are there
        assert part.pairs == e.value.partial.pairs and len(part.pairs) == c.meta["done"]
    zero = [c for c in cases if c.meta["done"] == 0]
    assert zero and all(sum(len(w.data) for w in tr.distinct_words(tr.pieces_of(c.docs, c.pat_str))) >= 2 for c in zero)  # N >= 2 and no pair
    assert any(0 < c.meta["done"] < c.n_merges - 2 for c in cases) and any(c.meta["done"] == c.n_merges - 2 for c in cases)


def test_sweep_samples():
    """the generator keeps its ranges, and at most a quarter of its samples run out of pairs"""
    out, pats, sizes, merges = 0, set(), [], []
    for i in range(ts.SWEEP_SAMPLES):
        pat, docs, n = ts.sweep_sample(i)
        assert (pat, docs, n) == ts.sweep_sample(i)
        assert 0 <= len(docs) <= 12 and all(ts.nbytes(d) <= 1500 for d in docs) and 1 <= n <= 48
        pats.add(pat)
        sizes += [ts.nbytes(d) for d in docs]
        merges.append(n)
        try:
            tr.train_text(docs, 256 + n, ts.PATTERNS[pat])
        except tr.Exhausted:
            out += 1
    assert ts.SWEEP_SAMPLES <= 40 and 1 <= out <= ts.SWEEP_SAMPLES // 4, out
    assert pats == set(ts.PATTERNS) and 0 in sizes and max(sizes) > 1000 and min(merges) <= 4 and max(merges) >= 40
