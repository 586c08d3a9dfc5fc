"""Streaming decode on the GPU (tk_stream.h) at the figures its interface promises and test_gpu_decode_stream.py does not reach: steps of
64 columns (every lane of the row's wavefront), rows that emit more than 1024 bytes in one call (the emit loop's later turns), tails of
65 and 66 bytes (the tail copies' second round), the largest row buffer and scratch slot (w_max = 64 over tokens of 248 bytes), a pack
pass of several workgroups with rows of over 256 bytes in the later ones, and 65536 rows.  Every expected value is stream_ref.Stream's,
and at the end the one-shot decode_rows_until's on the assembled matrix; the helpers are the sibling module's."""
import functools

import numpy as np
import pytest

import decode_rows_ref as D
import helpers as h
import stream_ref as R
import tiktoken_amd as tiktoken
from test_gpu_decode_stream import KERNELS, MODES, PACK_WG, enc, feed, finish, o200k, pair, same, totals

pytestmark = pytest.mark.gpu
HOLE = R.HOLE


# ---------------------------------------------------------------- every lane of the row's wavefront
@pytest.mark.parametrize("keep_stop", (False, True))
@pytest.mark.parametrize("mode", MODES)
def test_full_width_columns(mode, keep_stop):
    kw, steps = R.full_width_steps()
    stops = kw.pop("stops")
    seen = R.coverage(R.Stream(9, stops, token_bytes=R.token_bytes, special=lambda t: t in R.SPECIALS, keep_stop=keep_stop, mode=mode, **kw), steps)
    assert seen["begins"] >= set(R.EDGES) and seen["ends"] >= set(R.EDGES) and seen["stop_cols"] >= {31, 32, 63} and seen["skipped"] == {False, True}, seen
    for how in ("int64", "uint32", "int32", "int64 slice", "uint32 slice"):
        gpu, ref = pair(9, stops, mode=mode, keep_stop=keep_stop, **kw)
        for k, (ids, begin, end) in enumerate(steps):
            given = D.held(ids, np.dtype(how.split()[0]), ld_extra=7, shift=3) if how.endswith("slice") else ids.astype(how)
            assert not how.endswith("slice") or given.strides[0] == (ids.shape[1] + 7) * given.itemsize
            same(gpu.step_packed(given, begin, end), ref.step(ids, begin, end), ref, (how, k))
        assert len(set(ref.emitted)) == 9 and ref.state == seen["state"]  # (no two rows alike: a lane taken for another shows)
        finish(gpu, ref, how)


# ---------------------------------------------------------------- the emit loop beyond its first turn
@pytest.mark.parametrize("mode", MODES)
def test_emit_beyond_one_turn(mode):
    stops, steps = R.long_emit_steps()
    gpu, ref = pair(5, stops, mode=mode, stop=[300], w_max=64)  # (five rows: the row kernel's second workgroup has one)
    feed(gpu, ref, steps[:1])
    raw = [ref.tail[r] + b"".join(R.token_bytes(t) for t in steps[1][0][r].tolist()) for r in range(5)]
    assert all(len(b) > 2048 for b in raw) and all(R.straddles(raw[r], 1024) and R.straddles(raw[r], 2048) for r in (3, 4))
    want = ref.step(*steps[1])
    assert want == [{R.REPLACE: R.U.FFFD * 2560, R.IGNORE: b"", R.BYTES: raw[2]}[mode] if r == 2 else raw[r] for r in range(5)]
    same(gpu.step_packed(*steps[1]), want, ref)
    totals(gpu, ref)
    want = ref.step(*steps[2])
    assert len(want[0]) == 1023 + len({R.REPLACE: R.U.FFFD, R.IGNORE: b"", R.BYTES: b"\xf0"}[mode]) and ref.state[:2] == [R.STOP_ID, R.STOP_ID]
    same(gpu.step_packed(*steps[2]), want, ref)
    finish(gpu, ref)


# ---------------------------------------------------------------- tails of 63 .. 66 bytes
def rows_as_steps(cases):
    """the cases of stream_ref.hold_cases as the rows of one stream: step k gives row r the k-th item of its case, through end[r]"""
    items = [ids for ids, _, _ in cases]
    steps = []
    for k in range(max(map(len, items))):
        part = [(list(it[k]) if isinstance(it[k], tuple) else [it[k]]) if k < len(it) else [] for it in items]
        m = np.full((len(items), max(map(len, part))), HOLE, np.int64)
        for r, p in enumerate(part):
            m[r, :len(p)] = p
        steps.append((m, None, [len(p) for p in part]))
    return steps


@pytest.mark.parametrize("keep", (False, True))
@pytest.mark.parametrize("mode", MODES)
def test_tail_at_the_hold_limit(mode, keep):
    cases = list(R.hold_cases().values())
    steps = rows_as_steps(cases)
    gpu, ref = pair(len(cases), [R.STOP64, b"\n\n"], mode=mode, keep_stop_text=keep, w_max=max(s[0].shape[1] for s in steps))
    most = [0] * len(cases)
    for k, s in enumerate(steps):
        feed(gpu, ref, [s], k)
        most = [max(a, len(t)) for a, t in zip(most, ref.tail)]
    assert most == [held if mode != R.BYTES else 63 for _, held, _ in cases]  # (void unless the rule's own tails get there)
    assert ref.state == [R.STOP_TEXT if hit else R.LIVE for _, _, hit in cases]
    finish(gpu, ref)


@pytest.mark.parametrize("mode", (R.REPLACE, R.IGNORE))
def test_reset_and_refusals_on_rows_that_hold_66_bytes(mode):
    gpu, ref = pair(3, [R.STOP64], mode=mode, w_max=64)
    lead = list(b"\xf0\x9f\x98")
    first = np.array([lead + list(R.STOP64[:61]), lead[:2] + list(R.STOP64[:62]), list(b"q" * 64)], np.int64)
    feed(gpu, ref, [(first, None, None), ([list(R.STOP64[61:63]), [R.STOP64[62], HOLE], [0x71, 0xC3]], None, [2, 1, 2])])
    assert [len(t) for t in ref.tail] == [R.HOLD, 65, 1]
    for ids, begin, end, exc in (([[65, 66], [67, 68], [0xA9, HOLE]], None, None, KeyError), ([[65, 66], [67, 68], [0xA9, 69]], [0, 2, 0], [2, 1, 2], ValueError)):
        with pytest.raises(exc):
            gpu.step_packed(np.array(ids, np.int64), begin, end)
        totals(gpu, ref)  # (state and totals as they were ...)
    gpu.reset([0]), ref.reset([0])
    totals(gpu, ref)
    feed(gpu, ref, [([[65, 66], [R.STOP64[63], 68], [0xA9, 69]], None, None)])  # (... and the tails: the next step is the rule's)
    assert ref.emitted[0] == b"AB" and ref.state == [R.LIVE, R.STOP_TEXT, R.LIVE] and ref.emitted[2].endswith("qé".encode() + b"E")
    finish(gpu, ref)


# ---------------------------------------------------------------- the largest row buffer: 64 columns of tokens of 248 bytes
LONG = {256: b"y" * 248, 257: b"\x80" * 248, 258: "é".encode() * 124}


@functools.lru_cache(maxsize=None)
def long_enc(longest=248):
    ranks = {bytes([b]): b for b in range(256)}
    ranks.update({v[:longest] if k != 256 else b"y" * longest: k for k, v in LONG.items()})
    return tiktoken.Encoding(f"long{longest}", pat_str=h.PAT_STR[1], mergeable_ranks=ranks, special_tokens={})


def long_bytes(t):
    return bytes([t]) if 0 <= t < 256 else LONG.get(t)


@pytest.mark.parametrize("mode", MODES)
def test_largest_row_buffer(mode):
    assert R.HOLD + 64 * 248 <= R.ROW_LDS < R.HOLD + 64 * 249
    with pytest.raises(ValueError, match="decode_rows_until"):
        long_enc(249).decode_stream(1, w_max=64, errors=None)
    rng = np.random.default_rng(248)
    stops = [b"y" * 10 + b"Z", b"\x80" * 5 + b"!", "éé!".encode(), b"\n\n"]
    gpu, ref = pair(6, stops, mode=mode, e=long_enc(), token_bytes=long_bytes, special=lambda t: False, w_max=64)

    def step(top, ends):  # rows 0 .. 2 as given, three rows of byte-level tokens
        m = rng.choice(list(b"abc \n.") + [0xC3, 0xA9, 0xE4, 0xB8, 0xAD, 0xF0, 0x9F, 0x98, 0x80], size=(6, 64)).astype(np.int64)
        for r, ids in enumerate(top):
            m[r, :len(ids)] = ids
        return m, None, ends + [64, 64, 64]

    # a full buffer each; row 2 only a lead, so that every é of its next step lies across two lanes' sixteen bytes
    feed(gpu, ref, [step([[256] * 64, [257] * 64, [0xC3]], [64, 64, 1])])
    assert [len(t) for t in ref.tail[:3]] == [10, 5, 1]  # (the lead is the first byte of a stop string as well)
    assert ref.n_text[1] == {R.REPLACE: 3, R.IGNORE: 0, R.BYTES: 1}[mode] * (64 * 248 - 5)
    # the same behind the held tails: the search runs over all of the 15882, 15877 and 15873 bytes
    feed(gpu, ref, [step([[256] * 64, [257] * 64, [258] * 64], [64, 64, 64])])
    assert ref.state[:3] == [R.LIVE] * 3
    if mode == R.REPLACE:
        assert ref.n_text[1] == 3 * (2 * 64 * 248 - 5) and ref.emitted[2].startswith(R.U.FFFD + "é".encode())
    # the stop strings complete: at the front of the buffer, and at the very end of 15000 bytes
    feed(gpu, ref, [step([list(b"yyyZ"), [0x21], [258] * 60 + [0x21]], [4, 1, 61])])
    assert ref.state[:3] == [R.STOP_TEXT] * 3 and ref.hit[:3] == [0, 1, 2]
    finish(gpu, ref, e=long_enc())


# ---------------------------------------------------------------- the pack pass over several workgroups
@pytest.mark.parametrize("mode", MODES)
def test_many_pack_workgroups(mode):
    n_rows = 3 * PACK_WG + 1
    rng = np.random.default_rng(769)
    gpu, ref = pair(n_rows, ["\n\n", "ab"], mode=mode, stop=[300], skip=[R.PAD], w_max=64)
    share = rng.choice([0.0, 0.1, 0.6, 1.0], size=n_rows)  # of the 40-byte tokens in a row
    share[::8] = share[-1] = 1.0
    over_256 = set()

    def step():
        m = rng.choice([32, 46, 97, 98, 99, 0xC3, 0xA9, 0xF0, 0x9F, 0x98, 260, 261, 264, R.PAD], size=(n_rows, 64)).astype(np.int64)
        m[rng.random((n_rows, 64)) < share[:, None]] = R.X40
        m[rng.random((n_rows, 64)) < 0.002] = 300
        end = rng.integers(0, 65, size=n_rows)
        end[::8] = end[-1] = 64
        m[-1] = R.X40
        want = ref.step(m, None, end)
        over_256.update((r // PACK_WG, len(w) > 1024) for r, w in enumerate(want) if len(w) > 256)
        same(gpu.step_packed(m, None, end), want, ref)

    step(), step()
    some = rng.choice(n_rows, size=100, replace=False).tolist()
    same(gpu.flush_packed(some), ref.flush(some), ref)
    gpu.reset(some[:30]), ref.reset(some[:30])
    step(), step()
    assert {w for w, _ in over_256} == {0, 1, 2, 3} and {(2, True), (3, True)} <= over_256  # rows of over 256, and of over 1024 bytes, in the later workgroups
    assert {R.LIVE, R.STOP_ID, R.STOP_TEXT, R.FLUSHED} == set(ref.state) and min(ref.n_text) == 0
    totals(gpu, ref)
    core = enc()._core_bpe  # the launch count at this size: still one of each kernel
    core.set_profiling(True)
    core.reset_kernel_ms()
    try:
        step()
        assert [core.kernel_ms(k)[1] for k in KERNELS] == [1, 1]
    finally:
        core.set_profiling(False)
    finish(gpu, ref)


# ---------------------------------------------------------------- the most rows a stream takes
class Tiled:
    """a stream of `times` copies of the rows of `ref`, one behind the other: rows are independent, so the rule's outputs repeat"""

    def __init__(self, ref, times):
        self.ref, self.times, self.R = ref, times, ref.R * times
        self.mode, self.stops, self.keep_text, self.rule = ref.mode, ref.stops, ref.keep_text, ref.rule

    def __getattr__(self, name):  # state, hit, n_kept, n_text, n_chars, fed, emitted
        return getattr(self.ref, name) * self.times

    def step(self, ids, begin=None, end=None):
        return self.ref.step(ids[:self.ref.R], begin, end) * self.times

    def flush(self):
        return self.ref.flush() * self.times


def test_row_limit():
    import torch

    n_rows, rng = 65536, np.random.default_rng(65536)
    with pytest.raises(ValueError, match="65536"):
        enc().decode_stream(n_rows + 1, ["\n\n"])
    rows = rng.choice([10, 32, 97, 98, 0xC3, 0xA9, 0xF0, 0x9F, 256, 258, 260, 261, R.X40, R.BAD40, R.LEAD3], size=(64, 2))
    rows[:7] = [[97, 10], [0xF0, 0x9F], [300, HOLE], [97, 300], [10, 10], [R.LEAD3, 0x80], [10, 99]]  # a held prefix, an unfinished char, stop ids, a stop string, ...
    free = torch.cuda.mem_get_info()[0]
    gpu, _ = pair(n_rows, ["\n\n", "ab"], stop=[300])  # (the rule is run on 64 rows and tiled)
    cap = R.HOLD + max(len(R.token_bytes(t)) for t in range(R.N_IDS) if R.token_bytes(t))
    print(f"\na stream of {n_rows} rows took {free - torch.cuda.mem_get_info()[0]} bytes of device memory; its two copies of the slots, its scratch and its text: {2 * n_rows * (112 + ((3 * cap + 15) & ~15))}")
    ref = Tiled(R.Stream(64, [b"\n\n", b"ab"], token_bytes=R.token_bytes, special=lambda t: t in R.SPECIALS, stop=[300]), n_rows // 64)
    for c in range(2):
        ids = np.tile(rows[:, c:c + 1], (n_rows // 64, 1)).astype(np.int64)
        same(gpu.step_packed(ids), ref.step(ids), ref, c)
    assert {R.LIVE, R.STOP_ID, R.STOP_TEXT} == set(ref.ref.state) and ref.ref.tail[:2] == [b"\n", b"\xf0\x9f"] and ref.ref.emitted[6] == b"\nc", (ref.ref.state, ref.ref.tail[:7])
    finish(gpu, ref)


# ---------------------------------------------------------------- random rows from the shaped o200k vocabulary, in steps as wide as it allows
@functools.lru_cache(maxsize=None)
def wide_rows():
    """(rows of ids, stop strings, widths per step, id -> bytes, the stop id, the widest step): 64 rows over the shaped o200k vocabulary as
    test_gpu_decode_stream.random_rows makes them, in steps of 1 .. the widest the vocabulary's longest token allows, every other one from
    the upper half of that range.  Steps this wide cut few chars and stop strings by chance, so the generator knows where the steps end:
    where a word would reach the end of a step it first spells a char of several bytes, a byte per id, across it; of eight rows two end
    by a stop string spelled across the end of a step, three by one whose last byte is at column 16 or more of its step, one by a stop
    string where it falls, one by a stop id at column 16 or more, one not at all."""
    e = o200k()
    ranks = h.load_vocab("o200k_shaped")
    by_id = {v: k for k, v in ranks.items()}
    longest = max(max(map(len, ranks)), max(len(s.encode()) for s in e._special_tokens))
    widest = min((R.ROW_LDS - R.HOLD) // longest, 64)
    rng = np.random.default_rng(0x0200 + widest)
    byte_id = [ranks[bytes([b])] for b in range(256)]
    longest_rank = max(map(len, ranks))
    widths = np.where(rng.random(96) < 0.5, rng.integers(widest // 2 + 1, widest + 1, size=96), rng.integers(1, widest + 1, size=96))
    widths[:2] = 1, widest
    bounds = np.cumsum(widths).tolist()

    def greedy(data: bytes):
        out, i = [], 0
        while i < len(data):
            n = next(n for n in range(min(longest_rank, len(data) - i), 0, -1) if data[i:i + n] in ranks)
            out.append(ranks[data[i:i + n]])
            i += n
        return out

    def spelled(data: bytes):
        return [byte_id[b] for b in data]

    def column(i):  # of id i of a row, in its step
        return i - max([0] + [b for b in bounds if b <= i])

    def across(at, n):  # a step ends inside the n ids from `at`
        return any(at < b < at + n for b in bounds)

    stops = ["\n\nQuestion:", "</answer>", "###", "STOP", "\n\n\n", "<|user|>", "终止", "Ende."] + [f"<stop{i}>" for i in range(8)]
    words = ["The quick brown fox", " jumps over", " the lazy dog.", " naïve café", " 中文", " 😀", " déjà vu", "\n", " 1234", " x = y + z;", " 日本語", " 🙂🙃"]
    space, rows = byte_id[0x20], []
    for r in range(64):
        ids = []
        for _ in range(int(rng.integers(4, 16))):
            w = words[int(rng.integers(0, len(words)))].encode()
            w = spelled(w) if rng.random() < 0.6 else greedy(w)
            edge = next(b for b in bounds if b > len(ids))
            if len(ids) + len(w) >= edge and rng.random() < 0.9:
                ch = ["é", "中", "😀"][int(rng.integers(0, 3))].encode()
                k = min(int(rng.integers(1, len(ch))), edge - len(ids))  # bytes of it in front of the step's end
                ids += [space] * (edge - k - len(ids)) + spelled(ch)
            ids += w
        kind, stop = r % 8, spelled(stops[r % 16].encode())
        if kind in (1, 2):
            while not across(len(ids), len(stop)):
                ids.append(space)
        if kind in (3, 4, 5):
            while column(len(ids) + len(stop) - 1) < 16:
                ids.append(space)
        if kind == 0:
            while column(len(ids)) < 16:
                ids.append(space)
            ids += [e.eot_token] + greedy(b" and what follows")
        elif kind != 6:
            ids += stop + greedy(b" and what follows")
        rows.append(ids)
    n_steps = next(k for k, b in enumerate(bounds) if b >= max(map(len, rows))) + 1
    return rows, stops, widths[:n_steps].tolist(), by_id, e.eot_token, widest


def wide_shares(rows, stops, widths, token_bytes, stop_id):
    """by the rule alone: (rows that end by a stop string, hits that straddle a step, chars of several bytes, those that straddle a step,
    rows that end by a stop id or a stop string, those that end at a column of 16 or more of their step)"""
    bounds = np.cumsum(widths).tolist()
    ended = straddling_hits = chars = straddling_chars = ends = late_ends = 0
    for ids in rows:
        live = ids[:ids.index(stop_id)] if stop_id in ids else ids
        starts = np.concatenate([[0], np.cumsum([len(token_bytes(t)) for t in live])]).tolist()
        doc = b"".join(token_bytes(t) for t in live)
        step_edges = {starts[b] for b in bounds if b < len(live)}  # byte positions where a step ends
        cut, k = R.S.cut_doc(doc, [s.encode() for s in stops], False)
        last = None  # the column of the row's matrix at which it ends
        if k != R.NO_HIT:
            ended += 1
            hit_end = cut + len(stops[k].encode())
            straddling_hits += any(cut < x < hit_end for x in step_edges)
            last = next(i for i in range(len(live)) if starts[i + 1] >= hit_end)
        elif stop_id in ids:
            last = len(live)
        if last is not None:
            ends += 1
            late_ends += last - max([0] + [b for b in bounds if b <= last]) >= 16
        units, _ = R.unit_starts(doc[:cut])
        for a, b in zip(units[:-1], units[1:]):
            if b - a > 1:
                chars += 1
                straddling_chars += any(a < x < b for x in step_edges)
    return ended, straddling_hits, chars, straddling_chars, ends, late_ends


@pytest.mark.parametrize("mode", MODES)
def test_random_wide_rows(mode):
    e = o200k()
    rows, stops, widths, by_id, stop_id, widest = wide_rows()
    n_rows, pad, token_bytes = len(rows), 1 << 25, by_id.get
    assert n_rows == 64 and 16 < widest < 64 and max(widths) == widest and min(widths) == 1
    with pytest.raises(ValueError, match="decode_rows_until"):
        e.decode_stream(1, w_max=widest + 1)
    gpu, ref = pair(n_rows, stops, mode=mode, e=e, token_bytes=token_bytes, special=lambda t: False, stop=[stop_id], skip=[pad], w_max=widest)
    ended, straddling_hits, chars, straddling_chars, ends, late_ends = shares = wide_shares(rows, stops, widths, token_bytes, stop_id)
    assert ended * 2 >= n_rows and straddling_hits * 4 >= ended and straddling_chars * 4 >= chars and chars >= 32 and late_ends * 4 >= ends and ends > ended, shares
    at = 0
    for w in widths:
        ids = np.full((n_rows, w), pad, np.int64)
        for r, row in enumerate(rows):
            part = row[at:at + w]
            ids[r, :len(part)] = part
        at += w
        same(gpu.step_packed(ids), ref.step(ids), ref, at)
    assert sum(1 for s in ref.state if s == R.STOP_TEXT) == ended and sum(1 for s in ref.state if s != R.LIVE) == ends
    finish(gpu, ref, e=e)
