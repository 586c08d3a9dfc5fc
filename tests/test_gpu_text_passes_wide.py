"""UTF-8 repair and stop strings on the GPU (tk_utf8_repair.h, tk_stop_text.h) at the sizes where the code AROUND their lanes can be wrong:
more than 1024 documents (a second workgroup of tk_k_stops_rows), more than 2^20 (the carrying trip of tk_scan_blocks, the second
grid-stride trip of the per-document kernels), a workgroup whose output is as large as the count pass's 16-bit scan allows, and an output
of no bytes at all.  The lanes' own rules are covered by tests/test_gpu_utf8_repair.py and tests/test_gpu_stop_text.py.

The many documents are drawn from a pool of a few dozen (tests/utf8_repair_ref.py, tests/stop_text_ref.py): the rule restated in Python
runs once per pool entry and numpy spreads it over the batch; tests/test_utf8_repair_sim.py and tests/test_stop_text_sim.py compare that
with the per-document reference, and with CPython's decoder, on the CPU.  One batch of 2^20 + 1030 documents goes to the device once; every
smaller size is a prefix of it, whose reference is a slice.  Nothing in a reference comes from a GPU call."""
import functools

import numpy as np
import pytest

import decode_ref as dr
import decode_rows_ref as rows_ref
import helpers as h
import stop_text_ref as S
import tiktoken_amd as tiktoken
import utf8_repair_ref as R

pytestmark = pytest.mark.gpu
MODES = ("replace", "ignore")
MODE_OF = {"replace": R.REPLACE, "ignore": R.IGNORE}
LANE, WAVE, BLOCK = 16, 1024, 4096  # the kernels' geometry in bytes
M = 1 << 20  # the items of a per-document grid at its cap: 4096 workgroups of 256


@functools.lru_cache(maxsize=None)
def enc():
    ranks, specials = dr.edge_vocab()  # the 256 single bytes (id == byte), tokens of 2 .. 300 bytes, special tokens, ids without a token
    return tiktoken.Encoding("edge", pat_str=h.PAT_STR[1], mergeable_ranks=dict(ranks), special_tokens=dict(specials))


def core():
    return enc()._core_bpe


def dev_u8(ptr, n):
    import torch

    return torch.as_tensor(h._DevArray(ptr, n, "|u1"), device="cuda").cpu().numpy() if n else np.zeros(0, np.uint8)


class OnDevice:
    """packed text on the device: 16 readable bytes behind it that are not zero; a call may take the first n_docs documents alone, which
    have the documents behind them in their readable bytes"""

    def __init__(self, docs):
        import torch

        blob, self.n, off = R.pack(docs)
        self.n_docs, self.host_off = len(docs), off
        self.held = torch.from_numpy(blob.copy()).cuda()
        self.off = torch.from_numpy(off.view(np.int64).copy()).cuda()
        torch.cuda.synchronize()
        self.ptr, self.off_ptr = self.held.data_ptr(), self.off.data_ptr()

    def stop(self, stops, keep=False, n_docs=None):
        n_docs = self.n_docs if n_docs is None else n_docs
        return core().stop_text_device(self.ptr, int(self.host_off[n_docs]), self.off_ptr, n_docs, stops, keep)

    def repair(self, errors, n_docs=None):
        n_docs = self.n_docs if n_docs is None else n_docs
        return core().utf8_repair_device(self.ptr, int(self.host_off[n_docs]), self.off_ptr, n_docs, errors)


class Pooled:
    """who is who in a pooled batch, for the message of a mismatch"""

    def __init__(self, pool, idx):
        self.pool, self.idx = pool, idx

    def doc(self, d):
        d = min(max(int(d), 0), len(self.idx) - 1)
        return f"document {d} (pool entry {int(self.idx[d])}: {self.pool[int(self.idx[d])]!r})"

    def same(self, what, got, want, offsets=False):
        """whole arrays: one figure per document, or n + 1 running totals (the figure before document d: document d - 1 made it)"""
        assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
        if not np.array_equal(got, want):
            d = int(np.flatnonzero(got != want)[0])
            pytest.fail(f"{what}[{d}] is {got[d]}, not {want[d]}: the first that differs, at {self.doc(d - 1 if offsets else d)}; {int((got != want).sum())} differ")

    def same_text(self, got, want, want_off):
        if len(got) != len(want) or not np.array_equal(got, want):
            n = min(len(got), len(want))
            diff = np.flatnonzero(got[:n] != want[:n])
            b = int(diff[0]) if len(diff) else n
            d = int(np.searchsorted(want_off, b, side="right")) - 1
            pytest.fail(f"text: {len(got)} bytes for {len(want)}; byte {b} is the first that differs, in {self.doc(d)}: {bytes(got[b:b + 16])!r}, not {bytes(want[b:b + 16])!r}")


# ---------------------------------------------------------------- stop strings over many documents
@functools.lru_cache(maxsize=None)
def stop_batch():
    pool, idx = S.wide_batch()
    return Pooled(pool, idx), OnDevice(S.pooled_docs(pool, idx))


@functools.lru_cache(maxsize=None)
def stop_reference(keep):
    who, _ = stop_batch()
    return S.pooled_cut(who.pool, who.idx, S.WIDE_STOPS, keep)


@pytest.mark.parametrize("keep", (False, True))
@pytest.mark.parametrize("n_docs", S.WIDE_PREFIXES)
def test_stop_strings_over_many_documents(n_docs, keep):
    """1024: the last size of one workgroup of tk_k_stops_rows; 1025 and 2051: a second and a third, their bases, their hit counts added;
    2^20 - 1 and 2^20: one trip of everything, the closing offset alone in the per-document kernels' second; all: tk_scan_blocks carries"""
    who, d = stop_batch()
    text, text_off, hit = stop_reference(keep)
    r = d.stop(S.WIDE_STOPS, keep, n_docs)
    who.same("hit", h.dev_u32(r.hit, n_docs), hit[:n_docs])
    who.same("text_off", h.dev_u64(r.text_off, n_docs + 1), text_off[:n_docs + 1], offsets=True)
    n_hit = int((hit[:n_docs] != S.NO_HIT).sum())
    assert (r.n_bytes, r.n_hit) == (int(text_off[n_docs]), n_hit) and n_docs // 4 < n_hit < 3 * n_docs // 4
    assert r.data != d.ptr and r.text_off != d.off_ptr
    who.same_text(dev_u8(r.data, r.n_bytes), text[:int(text_off[n_docs])], text_off[:n_docs + 1])


@pytest.mark.parametrize("keep", (False, True))
def test_no_hit_in_many_documents_hands_back_the_callers_pointers(keep):
    who, d = stop_batch()
    n_docs = 2051
    assert not any(S.cut_doc(p, S.NO_STOPS, keep)[1] != S.NO_HIT for p in who.pool)
    r = d.stop(S.NO_STOPS, keep, n_docs)
    assert r.n_hit == 0 and r.data == d.ptr and r.text_off == d.off_ptr and r.n_bytes == int(d.host_off[n_docs])
    who.same("hit", h.dev_u32(r.hit, n_docs), np.full(n_docs, S.NO_HIT, np.uint32))


# ---------------------------------------------------------------- repair over many documents
@functools.lru_cache(maxsize=None)
def repair_batch():
    pool, idx = R.wide_batch()
    return Pooled(pool, idx), OnDevice(R.pooled_docs(pool, idx))


@functools.lru_cache(maxsize=None)
def repair_reference(errors):
    who, _ = repair_batch()
    return R.pooled_repair(who.pool, who.idx, MODE_OF[errors])


@pytest.mark.parametrize("errors", MODES)
@pytest.mark.parametrize("n_docs", R.WIDE_PREFIXES)
def test_repair_over_many_documents(n_docs, errors):
    """from 2^20 documents on tk_k_u8r_check, tk_k_span_mark and tk_k_u8r_docs take a second grid-stride trip: the closing offset alone at
    2^20, documents with ill-formed units behind it"""
    who, d = repair_batch()
    text, *offs = repair_reference(errors)
    r = d.repair(errors, n_docs)
    for got, want, what in zip((r.text_off, r.char_off, r.repl_off), offs, ("text_off", "char_off", "repl_off")):
        who.same(what, h.dev_u64(got, n_docs + 1), want[:n_docs + 1], offsets=True)
    assert (r.n_bytes, r.n_replaced) == (int(offs[0][n_docs]), int(offs[2][n_docs])) and r.n_replaced > n_docs // 4
    assert r.data != d.ptr and r.text_off != d.off_ptr
    who.same_text(dev_u8(r.data, r.n_bytes), text[:int(offs[0][n_docs])], offs[0][:n_docs + 1])


# ---------------------------------------------------------------- the extremes of the output
def against_cpython(docs, errors):
    """(text, text_off, char_off) from CPython per document, repl_off from the restatement, as tests/test_gpu_utf8_repair.py"""
    strs = [d.decode("utf-8", errors) for d in docs]
    parts = [s.encode("utf-8") for s in strs]
    text_off = np.zeros(len(docs) + 1, np.uint64)
    char_off = np.zeros(len(docs) + 1, np.uint64)
    if docs:
        text_off[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
        char_off[1:] = np.cumsum([len(s) for s in strs], dtype=np.uint64)
    return b"".join(parts), text_off, char_off, np.array(R.repair_batch(docs, MODE_OF[errors])[3], np.uint64)


def check_repair(docs, errors, ctx=None):
    d = OnDevice(docs)
    want = against_cpython(docs, errors)
    r = d.repair(errors)
    assert (r.n_bytes, r.n_replaced) == (len(want[0]), int(want[3][-1])), ctx
    assert (r.data == d.ptr and r.text_off == d.off_ptr) == (r.n_replaced == 0), ctx  # nothing replaced: the input is the output
    assert bytes(dev_u8(r.data, r.n_bytes)) == want[0], ctx
    for got, w, what in zip((r.text_off, r.char_off, r.repl_off), want[1:], ("text_off", "char_off", "repl_off")):
        assert np.array_equal(h.dev_u64(got, len(docs) + 1), w), (what, ctx)
    return r


@pytest.mark.parametrize("errors", MODES)
def test_repair_at_maximum_growth(errors):
    """R.growth in one batch, every case from a workgroup's first byte on: workgroups that leave 3 x 4096 bytes and, with the replacement of
    a lead from the workgroup before charged to their first byte, 3 x 4096 + 3 -- the bound that tk_k_u8r_count states for its scan of
    bytes and chars in 16 bits each, and reachable (tests/test_utf8_repair_sim.py shows it with CPython's incremental decoder); 'ignore'
    leaves nothing of the same workgroups"""
    docs = []
    for case in R.growth(BLOCK):
        assert sum(map(len, docs)) % BLOCK == 0
        docs += case
        docs.append(b"." * ((-sum(map(len, case))) % BLOCK))
    per_wg = R.charged(docs, BLOCK)
    assert max(per_wg) == 3 * BLOCK + 3 and per_wg.count(3 * BLOCK + 3) >= 6 and per_wg.count(3 * BLOCK) >= 4
    check_repair(docs, errors)


def test_repair_that_leaves_no_byte():
    docs = [b"\x80" * 5000, b"\xff", b"", b"\xe4\xb8"]
    d = OnDevice(docs)
    r = d.repair("ignore")
    assert (r.n_bytes, r.n_replaced) == (0, 5002)
    assert r.data != d.ptr and r.text_off != d.off_ptr and r.data and r.text_off
    assert h.dev_u64(r.text_off, 5).tolist() == [0] * 5 and h.dev_u64(r.char_off, 5).tolist() == [0] * 5
    assert h.dev_u64(r.repl_off, 5).tolist() == [0, 5000, 5001, 5001, 5002]
    check_repair(docs, "ignore")
    d = OnDevice(docs + [b"k"])
    r = d.repair("ignore")
    assert (r.n_bytes, r.n_replaced) == (1, 5002) and r.data != d.ptr and bytes(dev_u8(r.data, 1)) == b"k"
    assert h.dev_u64(r.text_off, 6).tolist() == [0] * 5 + [1] and h.dev_u64(r.char_off, 6).tolist() == [0] * 5 + [1]
    assert h.dev_u64(r.repl_off, 6).tolist() == [0, 5000, 5001, 5001, 5002, 5002]
    check_repair(docs + [b"k"], "replace")


def test_stop_strings_that_leave_no_byte():
    s4, s9, one = S.stop_of(4), S.stop_of(9, 0x54), b"\xfe"
    stops = [s4, s9, one]
    docs = [s4, s9 + b"x" * (BLOCK + 100), one, s4 + s4 + s9, one + b"y" * (3 * BLOCK) + s4, s9, s4 + b"tail", one * 40]
    d = OnDevice(docs)
    r = d.stop(stops, False)
    assert (r.n_bytes, r.n_hit) == (0, len(docs))
    assert r.data != d.ptr and r.text_off != d.off_ptr and r.data and r.text_off
    assert h.dev_u64(r.text_off, len(docs) + 1).tolist() == [0] * (len(docs) + 1)
    want_hit = [0, 1, 2, 0, 2, 1, 0, 2]
    assert h.dev_u32(r.hit, len(docs)).tolist() == want_hit == S.cut_batch(docs, stops, False)[2]
    r = d.stop(stops, True)
    want = [stops[k] for k in want_hit]
    assert (r.n_bytes, r.n_hit) == (sum(map(len, want)), len(docs)) and bytes(dev_u8(r.data, r.n_bytes)) == b"".join(want)
    assert h.dev_u64(r.text_off, len(docs) + 1).tolist() == [0] + np.cumsum([len(w) for w in want]).tolist() == S.cut_batch(docs, stops, True)[1]
    assert h.dev_u32(r.hit, len(docs)).tolist() == want_hit


@pytest.mark.parametrize("errors", MODES)
def test_runs_of_empty_documents_and_random_batches_on_the_device(errors):
    """the inputs that the CPU simulation alone ran: runs of 1, 2 and 70 empty documents at the text's start, middle and end (tk_span_first_at,
    the extra lane at p0 == n), and random batches; a call per batch"""
    batches = R.empties() + R.random_batches(0xE3D, 60)
    assert len(batches) == 15 + 60
    replaced = 0
    for k, docs in enumerate(batches):
        replaced += check_repair(docs, errors, k).n_replaced
    assert replaced > 1000


# ---------------------------------------------------------------- id matrices of many rows
N_ROWS, WIDTH, LD = M + 300, 6, 8
ROW_PREFIXES = (1025, M, N_ROWS)
ROW_FORCED = (1023, 1024, M - 1, M, N_ROWS - 1)
PAD_ID = 100000  # outside the vocabulary
SKIPPED = 0x07  # a skipped id inside the text


@functools.lru_cache(maxsize=None)
def row_batch():
    """(pool rows int64[P, WIDTH], idx, call arguments, stop strings, the 3-byte token's id): rows over the edge vocabulary's byte ids, its
    3-byte token, a stop id, a skipped id and the pad id; the rows of ROW_FORCED have their hit inside the 3-byte token"""
    table = dr.edge_table()
    t3 = table.id_of_len(3)
    S_ID, K, P, T = sorted(table.special_ids)[0], SKIPPED, PAD_ID, t3
    inside = table.by_id[t3][1:]  # the token's second and third byte
    stops = [b"\n\n", inside, "é".encode()]
    a, b, c, e, f, g, nl = (*b"abcefg", 10)
    assert b"\n" not in table.by_id[t3] and not set(table.by_id[t3]) & set(b"abcefg")
    pool = [
        [a, b, c, e, f, g], [a, nl, nl, b, c, e], [nl, nl, a, b, c, e], [a, b, c, e, nl, nl], [a, b, c, e, f, nl], [nl, a, b, c, e, f],  # "\n\n" at each place, and halved
        [a, b, T, c, e, f], [T, a, b, c, e, f], [T, T, T, T, T, T], [a, 0xC3, 0xA9, T, b, c], [a, b, c, e, f, T], [P, a, K, T, P, b], [a, T, T, b, c, e],  # a hit inside the 3-byte token
        [a, nl, K, nl, b, c], [a, b, S_ID, nl, nl, c], [S_ID, a, b, c, e, f], [a, b, c, T, S_ID, T],  # across a skipped id; behind a stop id: never searched
        [P, P, P, P, P, P], [K, K, K, K, K, K], [a, b, c, e, P, P], [P, P, a, P, P, P],  # rows without text, short rows
        [0xE4, 0xB8, 0xAD, a, T, P], [0xE4, 0xB8, S_ID, a, b, c], [0x80, a, b, nl, nl, c], [a, b, c, e, f, 0xC3], [0xF0, 0x9F, K, 0x80, a, b],  # for the repair behind the cut
        [a, 0xC3, 0xA9, b, c, e], [0xC3, 0xA9, nl, nl, a, b], [0xF0, 0x9F, 0x98, 0x80, nl, nl],
    ]
    pool = np.array(pool, np.int64)
    assert pool.shape[1] == WIDTH and len(pool) <= 64
    kw = dict(stop=[S_ID], skip=[PAD_ID, SKIPPED])
    per = [row_rule(row, kw, stops) for row in pool]
    in_token = [i for i, p in enumerate(per) if p["hit"] == 1 and p["n_tok"] != p["n_kept"]]
    assert len(in_token) >= 5
    idx = R.draw(len(pool), in_token, 0xD0C5, N_ROWS, ROW_FORCED)
    return pool, idx, kw, stops, tuple(per)


def row_rule(row, kw, stops):
    """one row by the rules restated in Python: decode_rows_ref.rows_rule, the edge table's bytes, S.cut_doc and S.n_tok_ref, CPython"""
    table = dr.edge_table()
    rows = rows_ref.rows_rule(np.array([row], np.int64), stop=kw["stop"], skip=kw["skip"], valid=lambda t: t in table.by_id, special=lambda t: t in table.special_ids)
    tokens = rows.tokens.tolist()
    kept, hit = S.cut_doc(b"".join(table.by_id[t] for t in tokens), stops, False)
    cut = b"".join(table.by_id[t] for t in tokens)[:kept]
    text = cut.decode("utf-8", "replace")
    return dict(tokens=tokens, n_kept=int(rows.n_kept[0]), stop_col=int(rows.stop_col[0]), hit=hit, n_tok=S.n_tok_ref([table.len_of[t] for t in tokens], kept), cut=cut,
                text=text.encode(), chars=len(text), repl=R.repair(cut, R.REPLACE)[2])


@functools.lru_cache(maxsize=None)
def row_matrix(dtype):
    pool, idx, *_ = row_batch()
    n = N_ROWS if dtype is np.int32 else ROW_PREFIXES[0]
    wide = np.full((n, LD), -7, dtype)  # (columns 6 and 7 belong to the wider matrix: never read)
    wide[:, :WIDTH] = pool[idx[:n]]
    return wide


@functools.lru_cache(maxsize=None)
def row_reference():
    pool, idx, _, _, per = row_batch()
    ref = {}
    ref["tokens"], ref["tok_off"] = R.spread([p["tokens"] for p in per], idx, np.uint32)
    for name in ("n_kept", "stop_col", "hit", "n_tok"):
        ref[name] = np.array([p[name] for p in per], np.uint32)[idx]
    ref["cut"], ref["cut_off"] = R.spread([p["cut"] for p in per], idx)
    ref["text"], ref["text_off"] = R.spread([p["text"] for p in per], idx)
    ref["char_off"], ref["repl_off"] = R.running([p["chars"] for p in per], idx), R.running([p["repl"] for p in per], idx)
    return ref


@pytest.mark.parametrize("errors", (None, "replace"))
@pytest.mark.parametrize("n_rows,dtype", [(n, np.int32) for n in ROW_PREFIXES] + [(ROW_PREFIXES[0], np.int64)])
def test_decode_rows_until_packed_over_many_rows(n_rows, dtype, errors):
    """more than 2^20 rows: the stop-string and repair passes as above behind the rows passes, and the second grid-stride trip of
    tk_k_stops_ntok; on both sides of its edge rows whose n_tok is not their n_kept"""
    pool, idx, kw, stops, per = row_batch()
    who = Pooled([row.tolist() for row in pool], idx)
    ref = row_reference()
    m = row_matrix(dtype)[:n_rows, :WIDTH]
    assert m.strides == (LD * m.itemsize, m.itemsize)
    for r in ROW_FORCED:
        assert ref["hit"][r] == 1 and ref["n_tok"][r] < ref["n_kept"][r]
    got = enc().decode_rows_until_packed(m, stops, keep_stop_text=False, errors=errors, **kw)
    for name in ("n_kept", "stop_col", "hit", "n_tok"):
        who.same(name, getattr(got, name), ref[name][:n_rows])
    who.same("tok_off", got.tok_off, ref["tok_off"][:n_rows + 1], offsets=True)
    n_tokens = int(ref["tok_off"][n_rows])
    assert len(got.tokens) == n_tokens and np.array_equal(got.tokens, ref["tokens"][:n_tokens]), "tokens"
    text, off = ("cut", "cut_off") if errors is None else ("text", "text_off")
    who.same("byte_off", got.byte_off, ref[off][:n_rows + 1], offsets=True)
    who.same_text(np.asarray(got.data), ref[text][:int(ref[off][n_rows])], ref[off][:n_rows + 1])
    if errors is None:
        assert got.char_off is None and got.repl_off is None
    else:
        who.same("char_off", got.char_off, ref["char_off"][:n_rows + 1], offsets=True)
        who.same("repl_off", got.repl_off, ref["repl_off"][:n_rows + 1], offsets=True)
        assert int(ref["repl_off"][n_rows]) > n_rows // 16
