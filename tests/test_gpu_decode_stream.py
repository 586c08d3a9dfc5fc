"""Streaming decode on the GPU (tk_stream.h) through Encoding.decode_stream: every step's output against the rule of
include/tiktoken_amd.h restated in tests/stream_ref.py, and everything a row emitted, concatenated, against the existing one-shot
decode_rows_until / decode_rows_until_bytes on the matrix assembled from the columns the row was fed."""
import functools

import numpy as np
import pytest

import helpers as h
import stream_ref as R
import tiktoken_amd as tiktoken

pytestmark = pytest.mark.gpu
ERRORS = {R.REPLACE: "replace", R.IGNORE: "ignore", R.BYTES: None}
MODES = (R.REPLACE, R.IGNORE, R.BYTES)
ROWS_WG, PACK_WG = 4, 256  # rows of a workgroup of the row kernel, of the pack pass
KERNELS = ("tk_k_stream_row", "tk_k_stream_pack")


@functools.lru_cache(maxsize=None)
def enc():
    ranks = {bytes([b]): b for b in range(256)}
    ranks.update({v: k for k, v in R.TOKENS.items()})
    return tiktoken.Encoding("stream", pat_str=h.PAT_STR[1], mergeable_ranks=ranks, special_tokens={v.decode(): k for k, v in R.SPECIALS.items()})


def pair(n_rows, stops=(), *, mode=R.REPLACE, e=None, token_bytes=R.token_bytes, special=lambda t: t in R.SPECIALS, **kw):
    stops = [s.encode() if isinstance(s, str) else s for s in stops]
    gpu = (e or enc()).decode_stream(n_rows, stops, errors=ERRORS[mode], **kw)
    ids_of = {v.decode(): k for k, v in R.SPECIALS.items()}  # (stop and skip take special-token strings; the reference takes ids)
    for name in ("stop", "skip"):
        if name in kw:
            kw[name] = [ids_of.get(t, t) for t in kw[name]]
    return gpu, R.Stream(n_rows, stops, token_bytes=token_bytes, special=special, mode=mode, **kw)


def pieces(p):
    data, off = bytes(p.text), p.text_off.tolist()
    return [data[a:b] for a, b in zip(off[:-1], off[1:])]


def same(p, want, ref, ctx=None):
    """a call's packed output against what the reference's rows emitted and hold now"""
    assert pieces(p) == want, (ctx, pieces(p), want)
    assert p.state.tolist() == ref.state and p.hit.tolist() == ref.hit, ctx
    if ref.mode == R.BYTES:
        assert p.char_off is None
    else:
        assert p.char_off.tolist() == [0] + np.cumsum([len(w.decode()) for w in want]).tolist(), ctx


def feed(gpu, ref, steps, ctx=None):
    for k, (ids, begin, end) in enumerate(steps):
        ids = np.asarray(ids, np.int64)
        same(gpu.step_packed(ids, begin, end), ref.step(ids, begin, end), ref, (ctx, k))


def totals(gpu, ref, ctx=None):
    assert gpu.state.tolist() == ref.state and gpu.hit.tolist() == ref.hit, ctx
    assert (gpu.n_kept.tolist(), gpu.n_text.tolist(), gpu.n_chars.tolist()) == (ref.n_kept, ref.n_text, ref.n_chars), ctx


def finish(gpu, ref, ctx=None, e=None, flush=True):
    """flush, the totals, and the concatenation against the one-shot entries on the assembled matrix"""
    if flush:
        same(gpu.flush_packed(), ref.flush(), ref, ctx)
    totals(gpu, ref, ctx)
    width = max([len(f) for f in ref.fed] + [1])
    m = np.zeros((ref.R, width), np.int64)
    for r, f in enumerate(ref.fed):
        m[r, :len(f)] = f
    kw = dict(end=np.array([len(f) for f in ref.fed], np.uint32), keep_stop_text=ref.keep_text, **ref.rule)
    one = (e or enc()).decode_rows_until_packed(m, ref.stops, errors=ERRORS[ref.mode], **kw)
    data, off = bytes(one.data), one.byte_off.tolist()
    assert [data[a:b] for a, b in zip(off[:-1], off[1:])] == ref.emitted, ctx
    assert one.hit.tolist() == ref.hit, ctx
    gpu.close()


def one_per_step(ids):
    return [(np.array([[t]]), None, None) for t in ids]


# ---------------------------------------------------------------- chars spelled by byte-level tokens
@pytest.mark.parametrize("mode", MODES)
def test_a_char_spelled_by_four_byte_tokens(mode):
    smile = list("😀".encode())
    gpu, ref = pair(1, mode=mode)
    got = [gpu.step(np.array([t], np.int64)).text[0] for t in smile]  # (1-D ids: [R, 1])
    assert got == {R.REPLACE: ["", "", "", "😀"], R.IGNORE: ["", "", "", "😀"], R.BYTES: [bytes([t]) for t in smile]}[mode]
    gpu.close()
    gpu, ref = pair(1, mode=mode)  # broken by an ASCII byte after two bytes
    feed(gpu, ref, one_per_step(smile[:2] + [0x41]))
    assert ref.emitted[0] == {R.REPLACE: "�A".encode(), R.IGNORE: b"A", R.BYTES: bytes(smile[:2]) + b"A"}[mode]
    finish(gpu, ref)
    gpu, ref = pair(1, mode=mode)  # left unfinished at the flush
    feed(gpu, ref, one_per_step(smile[:3]))
    out = gpu.flush()
    assert out.text == [{R.REPLACE: "�", R.IGNORE: "", R.BYTES: b""}[mode]] and out.finished.tolist() == [True] and out.state.tolist() == [R.FLUSHED]
    ref.flush()
    finish(gpu, ref, flush=False)


# ---------------------------------------------------------------- stop strings across steps
@pytest.mark.parametrize("keep", (False, True))
@pytest.mark.parametrize("mode", MODES)
def test_stop_strings_across_steps(mode, keep):
    for name, (stops, ids) in R.stop_cases().items():
        gpu, ref = pair(1, stops, keep_stop_text=keep, mode=mode)
        feed(gpu, ref, one_per_step(ids), name)
        finish(gpu, ref, name)
        if name == "the hit beats a lower, longer candidate":
            assert ref.hit == [0] and ref.emitted[0] == (b"xabc" if keep else b"xa")
        if name == "a prefix that breaks":
            assert ref.state == [R.FLUSHED] and ref.emitted[0] == b"a\n\nQuest! more"
        if name == "the tail of a token":
            assert ref.state == [R.STOP_TEXT] and ref.emitted[0] == (b"ab.\n\n" if keep else b"ab.")


def test_held_bytes_appear_in_the_next_step():
    with enc().decode_stream(1, ["\n\nQuestion:"]) as s:
        got = [s.step(np.array([[t]], np.int64)).text[0] for t in list(b"a\n\nQu!")]
        assert got == ["a", "", "", "", "", "\n\nQu!"]


# ---------------------------------------------------------------- stop ids, skipped ids, rows that have ended
@pytest.mark.parametrize("keep_stop", (False, True))
@pytest.mark.parametrize("mode", MODES)
def test_stop_ids_skips_and_ended_rows(mode, keep_stop):
    HOLE, PAD = R.HOLE, R.PAD
    gpu, ref = pair(3, ["\n\n"], stop=["<|eot|>"], skip=[PAD, 7], keep_stop=keep_stop, mode=mode, w_max=3)
    feed(gpu, ref, [
        ([[300, PAD, PAD], [97, 10, 7], [0xE4, 0xB8, 98]], None, None),  # a stop id in column 0 with pad behind it; a stop string spelled across a skipped id ...
        ([[HOLE, HOLE, HOLE], [10, 99, 100], [99, 100, 300]], None, None),  # ... completes; an ended row's ids without tokens are not judged; a stop id in the last column
        ([[HOLE, -1, 2**40], [HOLE, HOLE, HOLE], [PAD, HOLE, -5]], None, None),  # every row has ended: silent, nothing raises
    ])
    assert ref.state == [R.STOP_ID, R.STOP_TEXT, R.STOP_ID]
    assert ref.emitted[0] == (b"<|eot|>" if keep_stop else b"")
    finish(gpu, ref)
    gpu, ref = pair(2, [], skip_special=True, w_max=2)
    feed(gpu, ref, [([[104, 301], [300, 105]], None, None)])
    assert ref.emitted == [b"h", b"i"]
    finish(gpu, ref)


def test_begin_and_end_per_row():
    HOLE = R.HOLE
    gpu, ref = pair(3, ["\n\n"], w_max=3)
    feed(gpu, ref, [([[HOLE, HOLE, HOLE], [97, HOLE, HOLE], [98, 10, 99]], None, [0, 1, 3]), ([[99, 10, 100], [10, 10, 7], [1, 2, 3]], [1, 0, 3], [2, 2, 3])])
    assert ref.fed == [[10], [97, 10, 10], [98, 10, 99]]
    finish(gpu, ref)


@pytest.mark.parametrize("n_rows", (ROWS_WG + 1, PACK_WG + 1))
def test_one_row_more_than_a_workgroup(n_rows):
    rng = np.random.default_rng(n_rows)
    gpu, ref = pair(n_rows, ["\n\n", "ab"], w_max=2)
    alphabet = [10, 97, 98, 99, 0xC3, 0xA9, 256, 260, 261, 262]
    feed(gpu, ref, [(rng.choice(alphabet, size=(n_rows, 2)), None, None) for _ in range(4)])
    assert len(set(ref.state)) > 1  # (rows that have ended beside rows that go on, in the last workgroup too)
    finish(gpu, ref)


def test_reset_and_partial_flush():
    gpu, ref = pair(3, ["\n\nQuestion:"])
    feed(gpu, ref, [([[0xF0], [10], [104]], None, None), ([[0x9F], [10], [105]], None, None)])
    assert ref.tail == [b"\xf0\x9f", b"\n\n", b""]  # in mid-char; with a held stop prefix
    gpu.reset([0, 1]), ref.reset([0, 1])
    totals(gpu, ref)
    feed(gpu, ref, [([[0x98], [81], [33]], None, None)])  # nothing of the old requests leaks into the new ones
    assert ref.emitted == ["�".encode(), b"Q", b"hi!"]
    same(gpu.flush_packed([2]), ref.flush([2]), ref)
    assert ref.state == [R.LIVE, R.LIVE, R.FLUSHED]
    feed(gpu, ref, [([[65], [66], [67]], None, None)])
    with pytest.raises(ValueError):
        gpu.flush([3])
    finish(gpu, ref)


def test_refusals_change_nothing():
    HOLE = R.HOLE
    gpu, ref = pair(2, ["\n\n"], w_max=2)
    first = gpu.step_packed(np.array([[97, 10], [0xC3, 0xA9]], np.int64))
    same(first, ref.step(np.array([[97, 10], [0xC3, 0xA9]], np.int64)), ref)
    before = (gpu.state.tolist(), gpu.hit.tolist(), gpu.n_kept.tolist(), gpu.n_text.tolist(), gpu.n_chars.tolist())
    for ids, begin, end, exc, text in (([[98, HOLE], [99, 100]], None, None, KeyError, "row 0, column 1"), ([[98, 99], [99, 100]], [2, 0], [1, 2], ValueError, "row 0"),
                                       ([[98, 99], [99, 100]], None, [2, 3], ValueError, "row 1"), ([[98, 99, 100], [99, 100, 101]], None, None, ValueError, "w_max")):
        with pytest.raises(exc, match=text):
            gpu.step_packed(np.array(ids, np.int64), begin, end)
        assert (gpu.state.tolist(), gpu.hit.tolist(), gpu.n_kept.tolist(), gpu.n_text.tolist(), gpu.n_chars.tolist()) == before
    with pytest.raises(KeyError) as theirs:
        enc().decode_rows_until_packed(np.array([[98, HOLE], [99, 100]], np.int64), ["\n\n"])
    with pytest.raises(KeyError) as ours:
        gpu.step_packed(np.array([[98, HOLE], [99, 100]], np.int64))
    assert str(ours.value) == str(theirs.value)  # the reference's message, the row and the column
    feed(gpu, ref, [([[98, 10], [99, 100]], None, None)])  # the same step with the fault removed
    finish(gpu, ref)
    for bad in (dict(w_max=0), dict(w_max=65), dict(stop_text=["x" * 65]), dict(stop=list(range(17))), dict(errors="strict")):
        with pytest.raises(ValueError):
            enc().decode_stream(2, **{"stop_text": ["\n\n"], **bad})
    wide = tiktoken.Encoding("wide", pat_str=h.PAT_STR[1], mergeable_ranks={**{bytes([b]): b for b in range(256)}, b"y" * 400: 256}, special_tokens={})
    with pytest.raises(ValueError, match="decode_rows_until"):
        wide.decode_stream(1, w_max=64)
    wide.decode_stream(1, w_max=39).close()


def test_the_previous_outputs_survive_a_refused_step():
    from tiktoken_amd import _lib
    import ctypes

    gpu, ref = pair(2, ["\n\n"], w_max=2)
    gpu.step_packed(np.array([[97, 98], [99, 100]], np.int64))
    with pytest.raises(KeyError):
        gpu.step_packed(np.array([[R.HOLE, 98], [99, 100]], np.int64))
    n = gpu._native
    out, refs = n._outs()
    _lib.raise_for(_lib.lib().tk_stream_fetch(n._h, *refs))
    assert pieces(n._packed(out)) == [b"ab", b"cd"]
    assert isinstance(out[0], ctypes.c_void_p)
    gpu.close()


# ---------------------------------------------------------------- dtypes, strides, degenerate sizes
@pytest.mark.parametrize("where", ("numpy int64 slice", "numpy uint32", "torch int32", "torch int64 slice"))
def test_dtypes_and_strides(where):
    import torch

    rng = np.random.default_rng(7)
    R_, T, W = 5, 12, 3
    wide = rng.choice([10, 97, 98, 0xC3, 0xA9, 256, 261, 262, 46], size=(R_, T)).astype(np.int64)
    gpu, ref = pair(R_, ["\n\n", "ab"], w_max=W)
    dev = torch.from_numpy(wide).cuda() if where.startswith("torch") else None
    for t in range(0, T, W):
        if where == "numpy int64 slice":
            ids = wide[:, t:t + W]
        elif where == "numpy uint32":
            ids = np.ascontiguousarray(wide[:, t:t + W]).astype(np.uint32)
        elif where == "torch int32":
            ids = dev[:, t:t + W].to(torch.int32).contiguous()
        else:
            ids = dev[:, t:t + W]
        same(gpu.step_packed(ids), ref.step(wide[:, t:t + W]), ref, (where, t))
    finish(gpu, ref)


def test_degenerate_sizes():
    gpu, ref = pair(0, ["\n\n"])
    p = gpu.step_packed(np.zeros((0, 1), np.int64))
    assert len(p.text) == 0 and p.text_off.tolist() == [0] and len(p.state) == 0
    assert gpu.flush().text == [] and len(gpu.n_kept) == 0
    gpu.close()
    gpu, ref = pair(3, ["\n\n"], w_max=2)
    feed(gpu, ref, [(np.zeros((3, 0), np.int64), None, None), ([[97, 98]] * 3, None, None), (np.zeros((3, 0), np.int64), None, None)])
    finish(gpu, ref)


# ---------------------------------------------------------------- the launch count does not depend on R, W or the data
def test_launch_invariance():
    core = enc()._core_bpe
    counts = []
    for n_rows, W in ((3, 1), (300, 4)):
        with enc().decode_stream(n_rows, ["\n\n"], w_max=4) as s:
            ids = np.full((n_rows, W), 97, np.int64)
            s.step_packed(ids)
            core.set_profiling(True)
            core.reset_kernel_ms()
            s.step_packed(ids)
            counts.append([core.kernel_ms(k)[1] for k in KERNELS])
            core.set_profiling(False)
    assert counts[0] == counts[1] == [1, 1]


# ---------------------------------------------------------------- random rows from the shaped o200k vocabulary
@functools.lru_cache(maxsize=None)
def o200k():
    return tiktoken.get_encoding("o200k_shaped")


@functools.lru_cache(maxsize=None)
def random_rows():
    """(rows of ids, stop strings, widths per step, id -> bytes): 64 rows over the shaped o200k vocabulary -- words cut into its tokens by
    the longest match, or spelled by its byte-level tokens, so that multi-byte chars arrive a byte per id -- and 16 stop strings; the
    generator plants a stop string, spelled a byte per id, into two rows of three, so it crosses whatever step boundary falls into it."""
    ranks = h.load_vocab("o200k_shaped")
    by_id = {v: k for k, v in ranks.items()}
    rng = np.random.default_rng(0x0200)
    byte_id = [ranks[bytes([b])] for b in range(256)]
    longest = max(map(len, ranks))

    def greedy(data: bytes):
        out, i = [], 0
        while i < len(data):
            n = next(n for n in range(min(longest, len(data) - i), 0, -1) if data[i:i + n] in ranks)
            out.append(ranks[data[i:i + n]])
            i += n
        return out

    stops = ["\n\nQuestion:", "</answer>", "###", "STOP", "\n\n\n", "<|user|>", "终止", "Ende."] + [f"<stop{i}>" for i in range(8)]
    words = ["The quick brown fox", " jumps over", " the lazy dog.", " naïve café", " 中文", " 😀", " déjà vu", "\n", " 1234", " x = y + z;", " 日本語", " 🙂🙃"]
    rows = []
    for r in range(64):
        ids = []
        for _ in range(int(rng.integers(2, 9))):
            w = words[int(rng.integers(0, len(words)))].encode()
            ids += [byte_id[b] for b in w] if rng.random() < 0.6 else greedy(w)
        if r % 3:
            ids += [byte_id[b] for b in stops[r % 16].encode()] + greedy(b" and what follows")
        rows.append(ids)
    widths = rng.integers(1, 5, size=max(map(len, rows))).tolist()
    return rows, stops, widths, by_id


@pytest.mark.parametrize("mode", MODES)
def test_random_rows(mode):
    e = o200k()
    rows, stops, widths, by_id = random_rows()
    n_rows, pad, token_bytes = len(rows), 1 << 25, by_id.get

    gpu, ref = pair(n_rows, stops, mode=mode, e=e, token_bytes=token_bytes, special=lambda t: False, skip=[pad], w_max=4)
    # the shares, from the reference alone, before the GPU is asked: rows that end by a stop string, hits and chars that straddle a step
    bounds, at = [], 0
    for w in widths:
        at += w
        bounds.append(at)
    ended = straddling_hits = chars = straddling_chars = 0
    for ids in rows:
        lens = [len(token_bytes(t)) for t in ids]
        starts = np.concatenate([[0], np.cumsum(lens)]).tolist()
        doc = b"".join(token_bytes(t) for t in ids)
        step_edges = {starts[b] for b in bounds if b < len(ids)}  # byte positions where a step ends
        cut, k = R.S.cut_doc(doc, [s.encode() for s in stops], False)
        if k != R.NO_HIT:
            ended += 1
            straddling_hits += any(cut < x < cut + len(stops[k].encode()) for x in step_edges)
        units, _ = R.unit_starts(doc[:cut])
        for a, b in zip(units[:-1], units[1:]):
            if b - a > 1:
                chars += 1
                straddling_chars += any(a < x < b for x in step_edges)
    assert ended * 2 >= n_rows and straddling_hits * 4 >= ended and straddling_chars * 4 >= chars and chars >= 32, (ended, straddling_hits, chars, straddling_chars)
    at = 0
    for w in widths:
        ids = np.full((n_rows, w), pad, np.int64)
        for r, row in enumerate(rows):
            part = row[at:at + w]
            ids[r, :len(part)] = part
        at += w
        same(gpu.step_packed(ids), ref.step(ids), ref, at)
    assert sum(1 for s in ref.state if s == R.STOP_TEXT) == ended
    finish(gpu, ref, e=e)
