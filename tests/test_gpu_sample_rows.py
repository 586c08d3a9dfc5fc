"""Packed sample rows on the GPU (tk_sample_rows.h): tk_pack_samples_device and tk_encode_batch_sample_rows through CoreBPE and Encoding,
against the restatement of the rule as Python loops in tests/sample_rows_ref.py (written from the rule's description in
include/tiktoken_amd.h, not from the kernels).  The device entry runs on synthetic ids: it needs no vocabulary."""
import ctypes

import numpy as np
import pytest

import helpers as h
import sample_rows_ref as rr
import samples_ref as sr
import tiktoken_amd as tiktoken
from tiktoken_amd import _lib
from test_gpu_samples import body, core_of, dev, golden_texts, to_device

pytestmark = pytest.mark.gpu
BLOCK = 2048  # TK_DEC_BLOCK: positions per workgroup
NONE = rr.NONE


def shim_args(kw):
    """sample_rows_ref's keywords as pack_samples_device's"""
    out = dict(keep="tail" if kw.get("keep_tail") else "head", skip_long=bool(kw.get("skip_long")), ignore_first=bool(kw.get("ignore_first")))
    if kw.get("left"):
        out["padding_side"] = "left"
    if kw.get("width_multiple"):
        out["pad_to_multiple_of"] = kw["width_multiple"]
    return out


def read(r, n_samples: int, L: int) -> rr.SampleRows:
    R, n = r.n_rows, n_samples
    grid = [h.dev_u32(p, R * L).reshape(R, L) for p in (r.input_ids, r.segment_ids, r.position_ids)]
    return rr.SampleRows(grid[0], dev(r.labels, R * L, "<i4", np.int32).reshape(R, L), grid[1], grid[2], h.dev_u32(r.cu_seqlens, r.n_segs + 1), h.dev_u32(r.row_seg, R + 1),
                         h.dev_u32(r.row_sample, R + 1), h.dev_u32(r.length, n), h.dev_u64(r.full_length, n) if n else np.zeros(0, np.uint64), h.dev_u32(r.n_trained, n),
                         h.dev_u32(r.sample_row, n), h.dev_u32(r.sample_col, n))


def call(core, arrays, held, roles, L, bos=None, eos=None, pad=0, ignore=sr.IGNORE, **kw):
    tokens, tok_off, part_role, sample_off = arrays
    d_tok, d_off, d_role, d_so = held
    return core.pack_samples_device(d_tok.data_ptr(), len(tokens), d_off.data_ptr(), len(tok_off) - 1, d_role.data_ptr(), d_so.data_ptr(), len(sample_off) - 1, roles,
                                    max_length=L, bos=bos, eos=eos, pad=pad, ignore_index=ignore, **shim_args(kw))


def check(core, samples, L, kws, roles=sr.CHAT, pad=7, ignore=sr.IGNORE, ctx="", arrays=None):
    arrays = sr.pack(samples) if arrays is None else arrays
    held = to_device(*arrays)
    n = len(arrays[3]) - 1
    for kw in kws:
        kw = dict(kw)
        bos, eos = kw.pop("bos", None), kw.pop("eos", None)
        want = rr.rows_rule(*arrays, roles, L, bos=bos, eos=eos, pad=pad, ignore=ignore, **kw)
        got = read(call(core, arrays, held, roles, L, bos, eos, pad, ignore, **kw), n, L)
        rr.same(got, want, (ctx, L, bos, eos, kw))
        if ignore == sr.IGNORE:
            rr.invariants(got, L)  # pos == 0 exactly at cu_seqlens[:-1], full rows without a padding segment, n_trained = a count of the labels


CASES = rr.cases(np.random.default_rng(BLOCK))


# ---------------------------------------------------------------- the device entry against the restatement
@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0].replace(" ", "_")[:60] for c in CASES])
def test_device_entry_case_list(i):
    """Chains of 0 .. 17, 2049 and 4097 rows (the rounds of pointer doubling, across workgroups and scan blocks); 1023 .. 2049 samples of
    mixed lengths; 2047, 2048, 2049 and 4101 positions, rows that are no multiple of 8 and rows narrower than a lane; fills that end at L
    and one past it; a sample of L alone; samples of one element; runs of 0, 1 and 3000 unplaced samples at the start, in the middle and at
    the end; only empty samples and none; skip_long and the cut at L - 1, L, L + 1; the tail kept; ignore_first on a bos, a before id, a
    trained body token and a one-element sample; every bos / eos combination."""
    name, samples, L, kws = CASES[i]
    check(core_of(), samples, L, kws, ctx=name)


@pytest.mark.parametrize("ignore", [-100, 0, -1])
def test_training_flags_and_ignore_index(ignore):
    core = core_of()
    rng = np.random.default_rng(3)
    samples = [[(int(rng.integers(0, 6)), body(rng, int(k))) for k in rng.integers(0, 12, size=3)] for _ in range(20)]
    for roles in (sr.ALL_TRAINED, sr.NONE_TRAINED):
        check(core, samples, 24, [dict(bos=1, eos=2, ignore_first=True), dict(keep_tail=True, ignore_first=True), dict(eos=2)], roles=roles, ignore=ignore)
    arrays = sr.pack(samples)
    got = read(call(core, arrays, to_device(*arrays), sr.NONE_TRAINED, 24, 1, 2, ignore=ignore), len(samples), 24)
    assert (got.labels == ignore).all() and not got.n_trained.any()


def test_ignore_first_by_hand():
    """n_trained against a count of the labels, and the masked label itself: a bos first (nothing changes), a before id first (nothing
    changes), a trained body token first (one less), a one-element trained sample (none left)."""
    core = core_of()
    roles = (sr.Role((61,), (62,), True), sr.Role((), (), True))
    arrays = sr.pack([[(0, [10, 11])], [(1, [20, 21, 22])], [(1, [30])]])
    held = to_device(*arrays)
    I = sr.IGNORE
    got = read(call(core, arrays, held, roles, 16, bos=1, ignore_first=True), 3, 16)
    assert got.labels[0].tolist() == [I, I, 10, 11, 62, I, 20, 21, 22, I, 30] + [I] * 5 and got.n_trained.tolist() == [3, 3, 1]
    got = read(call(core, arrays, held, roles, 16, ignore_first=True), 3, 16)
    assert got.labels[0].tolist() == [I, 10, 11, 62, I, 21, 22, I] + [I] * 8 and got.n_trained.tolist() == [3, 2, 0]
    got = read(call(core, arrays, held, roles, 16), 3, 16)
    assert got.labels[0].tolist() == [I, 10, 11, 62, 20, 21, 22, 30] + [I] * 8 and got.n_trained.tolist() == [3, 3, 1]
    got = read(call(core, arrays, held, roles, 3, keep_tail=True, ignore_first=True), 3, 3)  # the tail cut drops the before id: 10 11 62 | 20 21 22 | 30
    assert got.labels.tolist() == [[I, 11, 62], [I, 21, 22], [I, I, I]] and got.n_trained.tolist() == [2, 2, 0] and got.sample_row.tolist() == [0, 1, 2]
    assert np.array_equal(np.bincount(got.seg[got.labels != I].astype(np.int64), minlength=3), got.n_trained)


@pytest.mark.parametrize("bos,eos", sr.SPECIALS[::3])
def test_token_pointer_that_is_not_16_byte_aligned(bos, eos):
    """A lane loads eight body tokens as two 16-byte words where their address allows it: shifting the array moves the lanes that can"""
    import torch

    core = core_of()
    rng = np.random.default_rng(5)
    arrays = sr.pack([[(2, body(rng, 700)), (0, [])], [(3, body(rng, 1500)), (1, body(rng, 9))], [(3, body(rng, 300))]])
    tokens = arrays[0]
    held = to_device(*arrays)
    buf = torch.zeros(len(tokens) + 8, dtype=torch.int32, device="cuda")
    modes = [(1024, dict()), (2000, dict(keep_tail=True)), (64, dict(ignore_first=True))]
    wants = [rr.rows_rule(*arrays, sr.CHAT, L, bos=bos, eos=eos, pad=7, **kw) for L, kw in modes]
    for shift in (0, 1, 2, 3):
        buf[shift: shift + len(tokens)] = held[0]
        torch.cuda.synchronize()
        for (L, kw), want in zip(modes, wants):
            rr.same(read(call(core, arrays, (buf[shift:],) + held[1:], sr.CHAT, L, bos, eos, 7, **kw), 3, L), want, (shift, L, kw))


def test_last_lane_stores_three_elements_and_nothing_behind_them():
    """2048 + 3 positions: two workgroups, whose last lane writes three elements one by one where every other lane writes eight at once.
    The library's arrays hold a multiple of 8 elements each, so the five behind the result exist: they are painted between two calls of
    the same shape and must come through the second one untouched."""
    import torch

    core = core_of()
    rng = np.random.default_rng(2051)
    n, n8 = BLOCK + 3, BLOCK + 8
    arrays = sr.pack([[(3, body(rng, k))] for k in (293, 200, 300, 150, 140, 294, 292, 1, 293)])  # 7 rows of 293
    held = to_device(*arrays)
    want = rr.rows_rule(*arrays, sr.CHAT, 293, pad=7)
    assert want.ids.shape == (7, 293)
    seen = None
    for round_ in range(2):
        r = call(core, arrays, held, sr.CHAT, 293, pad=7)
        ptrs = (r.input_ids, r.labels, r.segment_ids, r.position_ids)
        assert r.n_rows == 7 and seen in (None, ptrs)
        seen = ptrs
        for ptr in ptrs:
            t = torch.as_tensor(h._DevArray(ptr + n * 4, n8 - n, "<i4"), device="cuda")
            if round_ == 0:
                t.fill_(0x5A5A5A5A)
                torch.cuda.synchronize()
            else:
                assert (t.cpu().numpy() == 0x5A5A5A5A).all()
        rr.same(read(r, 9, 293), want, round_)


def test_invariants_on_a_random_batch():
    core = core_of("cl100k_shaped")
    rng = np.random.default_rng(0x20000)
    samples = [[(int(rng.integers(0, 6)), body(rng, 0 if rng.random() < 0.15 else int(rng.integers(1, 60)))) for _ in range(int(rng.integers(0, 6)))] for _ in range(400)]
    check(core, samples, 256, [dict(eos=100257), dict(bos=100258, eos=100257, skip_long=True, ignore_first=True), dict(keep_tail=True, ignore_first=True)], pad=100276)


# ---------------------------------------------------------------- refusals
def test_refusals_leave_the_previous_result_and_the_encode_result_whole():
    """Refusals, not faults: the count pass checks every entry of the three arrays before anything is indexed with them, every later pass
    does nothing once an entry offends, and all of them work in scratch arrays: nothing is written into the buffers of the previous
    result, and nothing into the encode call's."""
    import torch

    enc = tiktoken.get_encoding("gpt2_shaped")
    core = enc._core_bpe
    texts = golden_texts("gpt2_shaped", enc)[100:140]
    blob, off = enc._pack(texts)
    tokens, tok_off = enc.encode_ordinary_batch_packed(texts)
    d_text = torch.zeros(len(blob) + 256, dtype=torch.uint8, device="cuda")
    d_text[: len(blob)] = torch.from_numpy(blob.copy()).cuda()
    d_doc = torch.from_numpy(off.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    dt, nt, dof = core.encode_batch_device(d_text.data_ptr(), len(blob), d_doc.data_ptr(), off, len(texts))
    n_parts = len(texts)
    part_role = (np.arange(n_parts) % 3).astype(np.uint8)
    sample_off = np.array(list(range(0, n_parts, 4)) + [n_parts], np.uint64)
    n = len(sample_off) - 1
    _, _, d_role, d_so = to_device([], [0], part_role, sample_off)
    args = dict(max_length=64, eos=1, pad=0, ignore_first=True)

    def run(off=None, n_tok=nt, role=d_role, so=d_so, n_p=n_parts, n_s=n, roles=sr.CHAT, **kw):  # (off: a tensor that lives as long as the caller holds it)
        return core.pack_samples_device(dt, n_tok, dof if off is None else off.data_ptr(), n_p, role.data_ptr(), so.data_ptr(), n_s, roles, **{**args, **kw})

    good = run()
    want = rr.rows_rule(tokens, tok_off, part_role, sample_off, sr.CHAT, 64, eos=1, pad=0, ignore_first=True)
    rr.same(read(good, n, 64), want, "before")

    def bad_u64(a, i, v):
        b = np.array(a, np.uint64)
        b[i] = v
        return torch.from_numpy(b.view(np.int64).copy()).cuda()

    # R * L reaches 2^32 by shape arithmetic only: two samples of 2^30 + 1 tokens cannot share a row of 2^31 (nothing is read at those indices)
    two_off = torch.from_numpy(np.array([0, (1 << 30) + 1, (1 << 31) + 2], np.uint64).view(np.int64).copy()).cuda()
    two_so = torch.from_numpy(np.array([0, 1, 2], np.int64)).cuda()
    refused = [
        (dict(pad_to_multiple_of=8), "width_multiple"),
        (dict(padding_side="left"), "TK_SMP_LEFT"),
        (dict(max_length=0), "max_len"),
        (dict(roles=()), "n_roles"),
        (dict(roles=sr.CHAT * 43), "256 roles"),
        (dict(role=torch.from_numpy(np.where(np.arange(n_parts) == 5, 200, part_role).astype(np.uint8)).cuda()), r"part 5\b"),
        (dict(off=bad_u64(tok_off, 3, int(tok_off[4]) + 1)), r"document 3\b"),
        (dict(off=bad_u64(tok_off, 9, 1 << 40)), r"document 9\b"),
        (dict(off=bad_u64(tok_off, n_parts, nt + 1)), rf"document {n_parts - 1}\b"),
        (dict(so=bad_u64(sample_off, 0, 1)), r"sample 0\b"),
        (dict(so=bad_u64(sample_off, 3, 1 << 50)), r"sample 3\b"),
        (dict(so=bad_u64(sample_off, n, n_parts + 1)), rf"sample {n - 1}\b"),
        (dict(n_tok=1 << 32), "32-bit"),
        (dict(n_s=(1 << 32) - 1), "32-bit"),
        (dict(off=two_off, so=two_so, role=torch.zeros(4, dtype=torch.uint8, device="cuda"), n_tok=(1 << 31) + 2, n_p=2, n_s=2, max_length=1 << 31, roles=(sr.Role(),)),
         "rows times width"),
    ]
    for kw, what in refused:
        with pytest.raises(ValueError, match=what):
            run(**kw)
        rr.same(read(good, n, 64), want, ("after", what))
        assert np.array_equal(h.dev_u32(dt, nt), tokens) and np.array_equal(h.dev_u64(dof, n_parts + 1), tok_off)
    rr.same(read(run(), n, 64), want, "after the refusals")
    # the one-row-per-sample entry refuses the two flags that mean something here only
    n_roles, ids_t, off_t, train_t = core._role_table(sr.CHAT)
    for flag in (4, 8):
        spec = core._smp_spec(64, "head", "right", None, None, 1, 0, -100)
        out, cnt, refs = core._outs(6, 2)
        table = (n_roles, ids_t.ctypes.data, off_t.ctypes.data, train_t.ctypes.data)
        assert core._L.tk_assemble_samples_device(core._h, dt, nt, dof, n_parts, d_role.data_ptr(), d_so.data_ptr(), n, *table, ctypes.byref(spec), None, *refs) == _lib.TK_OK
        spec.flags |= flag
        assert core._L.tk_assemble_samples_device(core._h, dt, nt, dof, n_parts, d_role.data_ptr(), d_so.data_ptr(), n, *table, ctypes.byref(spec), None,
                                                  *refs) == _lib.TK_VALUE_ERROR and "unknown flag" in _lib.last_error()
    several = tiktoken.CoreBPE(enc._mergeable_ranks, enc._special_tokens, enc._pat_str, devices=[0, 0])
    with pytest.raises(ValueError, match="one device"):
        several.pack_samples_device(dt, nt, dof, n_parts, d_role.data_ptr(), d_so.data_ptr(), n, sr.CHAT, max_length=8)
    with pytest.raises(ValueError, match="one device"):
        several.encode_batch_sample_rows_packed(np.frombuffer(b"ab", np.uint8), np.array([0, 2], np.uint64), part_role=[0], sample_off=[0, 1], roles=sr.CHAT, max_length=2)


# ---------------------------------------------------------------- end to end
@pytest.mark.parametrize("name", h.ENCODING_NAMES)
def test_end_to_end_against_the_oracle(name):
    enc = tiktoken.get_encoding(name)
    C = h.c_oracle_for(name)
    special = sorted(enc._special_tokens.items(), key=lambda kv: kv[1])
    sid = [v for _, v in special]
    start, end = sid[0], sid[-1]
    template = {"system": tiktoken.Role((start, sid[0]), (end,), False), "user": tiktoken.Role((start, sid[-1]), (end,), False),
                "assistant": tiktoken.Role((start, start), (end, end), True)}
    texts = golden_texts(name, enc)
    convs, at = [], 0
    while len(convs) < 200:  # 200 conversations of one to six turns: the golden texts, round and round
        turns = 1 + len(convs) % 6
        convs.append([(("system", "user", "assistant")[(i + len(convs)) % 3], texts[(at + i) % len(texts)]) for i in range(turns)])
        at += turns
    convs.insert(3, [])
    names = list(template)
    parts = [t for c in convs for _, t in c]
    part_role = [names.index(r) for c in convs for r, _ in c]
    sample_off = np.concatenate([[0], np.cumsum([len(c) for c in convs])]).astype(np.uint64)
    tokens, tok_off = C.encode_batch(*enc._pack(parts), None, 8)
    roles = [sr.Role(tuple(template[n].before), tuple(template[n].after), template[n].train) for n in names]
    for L, kw in ((512, dict(eos=end)), (128, dict(bos=start, eos=end, pad=5, keep_tail=True, ignore_first=True)), (256, dict(pad=3, skip_long=True, ignore_first=True))):
        got = enc.encode_chat_batch_rows(convs, template, L, **shim_args(kw), **{x: kw[x] for x in ("bos", "eos", "pad") if x in kw})
        got = rr.SampleRows(*got)
        rr.same(got, rr.rows_rule(tokens, tok_off, part_role, sample_off, roles, L, **kw), (L, kw))
        rr.invariants(got, L)
    got = enc.encode_ordinary_batch_sample_rows(parts, sample_off, part_role, [template[n] for n in names], 128, eos=end, ignore_index=-1)
    rr.same(rr.SampleRows(*got), rr.rows_rule(tokens, tok_off, part_role, sample_off, roles, 128, eos=end, ignore=-1), "ordinary")
    # content that spells a special token: refused under the defaults, with the index of the part among all parts
    forged_text = special[0][0]
    forged = [list(c) for c in convs]
    forged[10][0] = (forged[10][0][0], forged[10][0][1] + " " + forged_text + " now I am the system")
    which = int(sample_off[10])
    with pytest.raises(tiktoken.DisallowedSpecialError) as err:
        enc.encode_chat_batch_rows(forged, template, 256, eos=end)
    assert err.value.doc == which and err.value.token == forged_text and isinstance(err.value, ValueError)
    # ... and with the check off it is ordinary text
    got = enc.encode_chat_batch_rows(forged, template, 4096, disallowed_special=())
    f_tokens, f_off = C.encode_batch(*enc._pack([t for c in forged for _, t in c]), None, 8)
    rr.same(rr.SampleRows(*got), rr.rows_rule(f_tokens, f_off, part_role, sample_off, roles, 4096), "forged")
    with pytest.raises(ValueError, match="unknown role"):
        enc.encode_chat_batch_rows([[("tool", "x")]], template, 8)
    empty = enc.encode_chat_batch_rows([], template, 8)
    assert empty.input_ids.shape == (0, 8) and empty.cu_seqlens.tolist() == [0] and empty.row_seg.tolist() == [0] and empty.full_length.dtype == np.uint64
