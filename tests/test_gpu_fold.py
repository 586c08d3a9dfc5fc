"""What the rows, padded and samples families share on the host side (tk_api.hip): the refusal of an offsets array that does not describe the
batch -- one function, six texts -- and the carving of their result buffers into arrays that start at multiples of 16 bytes."""
import numpy as np
import pytest

import helpers as h
import padded_ref as pr
import rows_ref as rr
import samples_ref as sr
import test_gpu_padded as gp
import test_gpu_rows as gr
import test_gpu_samples as gs

pytestmark = pytest.mark.gpu

# the texts of tok_off_refusal and of smp_run's sample_off switch as they stood before the two became one (commit 3220802), {} = the entry
TOK_OFF_TEXTS = ("tok_off[0] must be 0 (document {})", "tok_off must be non-decreasing: document {} ends before it starts",
                 "tok_off must end at n_tokens: document {} ends elsewhere")
SAMPLE_OFF_TEXTS = ("sample_off[0] must be 0 (sample {})", "sample_off must be non-decreasing: sample {} ends before it starts",
                    "sample_off must end at n_parts: sample {} ends elsewhere")


def u64_on_device(a, i=None, v=None):
    import torch

    b = np.array(a, np.uint64)
    if i is not None:
        b[i] = v
    return torch.from_numpy(b.view(np.int64).copy()).cuda()


def test_refusal_texts_are_the_parents():
    """Ten parts of 0 .. 9 tokens in three samples.  Each of the three things that can be wrong with tok_off, through pack_rows_device,
    pad_batch_device and assemble_samples_device, and each of the three with sample_off: the message is, character for character, the
    one of the two functions that offsets_refusal replaces.  After every refusal the previous result of every family is read again through
    the pointers it was returned with: a refused call writes into none of the padded and the samples buffers, and no family touches
    another's.  Only the rows family promises its buffers until the next rows call and no longer (a refused one included): after a refusal
    by pack_rows_device the good call is repeated, compared, and its pointers are the ones read from then on."""
    core = gr.core_of()
    rng = np.random.default_rng(10)
    parts = [(int(r), gs.body(rng, n)) for r, n in zip(rng.integers(0, 6, size=10), (3, 0, 9, 1, 7, 2, 8, 4, 6, 5))]
    arrays = sr.pack([parts[:4], parts[4:5], parts[5:]])
    tokens, tok_off, part_role, sample_off = arrays
    T, n = len(tokens), 10
    assert sorted(np.diff(tok_off.astype(np.int64)).tolist()) == list(range(10)) and sample_off.tolist() == [0, 4, 5, 10]
    d_tok, d_off, d_role, d_so = gs.to_device(*arrays)

    def rows(off=d_off):
        return core.pack_rows_device(d_tok.data_ptr(), T, off.data_ptr(), n, seq_len=16, eos=1)

    def padded(off=d_off):
        return core.pad_batch_device(d_tok.data_ptr(), T, off.data_ptr(), n, max_length=16, eos=1)

    def samples(off=d_off, so=d_so):
        return core.assemble_samples_device(d_tok.data_ptr(), T, off.data_ptr(), n, d_role.data_ptr(), so.data_ptr(), 3, sr.CHAT, max_length=16, eos=1)

    def read_padded(r):
        R, W = r.n_rows, r.width
        return pr.Padded(h.dev_u32(r.input_ids, R * W).reshape(R, W), gp.dev(r.attention_mask, R * W, "|u1", np.uint8).reshape(R, W), h.dev_u32(r.lengths, R),
                         h.dev_u32(r.row_doc, R), h.dev_u32(r.row_tok, R), h.dev_u32(r.doc_row, n + 1))

    want_rows = rr.rows_rule(tokens, tok_off, 16, eos=1, pad=1)
    want_padded = pr.padded_rule(tokens, tok_off, 16, eos=1, pad=1)
    want_samples = sr.samples_rule(*arrays, sr.CHAT, 16, eos=1, pad=0)

    def read_rows(r):
        m = r.n_rows * 16 + r.n_tail
        return rr.Rows(h.dev_u32(r.ids, m), h.dev_u32(r.doc, m), h.dev_u32(r.pos, m), h.dev_u32(r.cu_seqlens, r.n_segs + 1), h.dev_u32(r.row_seg, r.n_rows + 1), r.n_rows,
                       r.n_segs, r.n_stream, r.n_tail)

    good_padded, good_samples, good_rows = padded(), samples(), [rows()]
    gr.same(read_rows(good_rows[0]), want_rows, "before")
    pr.same(read_padded(good_padded), want_padded, "before")
    sr.same(gs.read(good_samples), want_samples, "before")

    def after(name, ctx):
        pr.same(read_padded(good_padded), want_padded, ctx)
        sr.same(gs.read(good_samples), want_samples, ctx)
        if name == "rows":
            good_rows[0] = rows()
        gr.same(read_rows(good_rows[0]), want_rows, ctx)

    # tok_off[0] != 0; document 5 ends before it starts; the last entry is not n_tokens (it speaks for the last document)
    bad_tok_off = ((u64_on_device(tok_off, 0, 1), 0), (u64_on_device(tok_off, 5, int(tok_off[6]) + 1), 5), (u64_on_device(tok_off, n, T + 1), n - 1))
    for text, (off, entry) in zip(TOK_OFF_TEXTS, bad_tok_off):
        for name, entry_point in (("rows", rows), ("padded", padded), ("samples", samples)):
            with pytest.raises(ValueError) as err:
                entry_point(off)
            assert str(err.value) == text.format(entry), (name, str(err.value))
            after(name, (name, text))
    bad_sample_off = ((u64_on_device(sample_off, 0, 1), 0), (u64_on_device(sample_off, 1, 6), 1), (u64_on_device(sample_off, 3, n - 1), 2))
    for text, (so, entry) in zip(SAMPLE_OFF_TEXTS, bad_sample_off):
        with pytest.raises(ValueError) as err:
            samples(so=so)
        assert str(err.value) == text.format(entry), str(err.value)
        after("samples", text)


def test_every_result_array_starts_at_16_bytes():
    """Sizes at which no array of a result ends at a multiple of 16 bytes: every pointer a call returns is one all the same (the write
    passes store 16 bytes at a time), and the arrays hold what the rule says -- none overlaps the next.  Then a call of 40 documents, which
    makes the buffers grow, and the small call again."""
    core = gr.core_of()
    rng = np.random.default_rng(16)
    docs = [gs.body(rng, 1), [], gs.body(rng, 9)]
    many = [gs.body(rng, int(m)) for m in rng.integers(0, 30, size=40)]
    small, large = rr.pack_docs(docs), rr.pack_docs(many)
    held = {id(small): gr.to_device(*small), id(large): gr.to_device(*large)}

    def aligned(r, fields):
        for f in fields:
            assert getattr(r, f) % 16 == 0, (f, hex(getattr(r, f)))

    # rows
    def rows(batch, dtype, drop_last, eos):
        (tokens, tok_off), (d_tok, d_off) = batch, held[id(batch)]
        aligned(core.pack_rows_device(d_tok.data_ptr(), len(tokens), d_off.data_ptr(), len(tok_off) - 1, seq_len=5, eos=eos, pad=7, drop_last=drop_last, dtype=dtype),
                ("ids", "doc", "pos", "cu_seqlens", "row_seg"))
        gr.same(gr.pack_device(core, tokens, tok_off, 5, eos=eos, pad=7, drop_last=drop_last, dtype=dtype, held=(d_tok, d_off)),
                rr.rows_rule(tokens, tok_off, 5, eos=eos, pad=7, drop_last=drop_last), ("rows", dtype, drop_last, eos))

    for dtype in (np.uint32, np.uint16):
        for drop_last in (False, True):
            for eos in (None, 1):  # (a stream of 10 and of 13 positions)
                rows(small, dtype, drop_last, eos)
                rows(large, dtype, drop_last, eos)
                rows(small, dtype, drop_last, eos)

    # padded
    def padded(batch, dtype, **kw):
        (tokens, tok_off), (d_tok, d_off) = batch, held[id(batch)]
        aligned(core.pad_batch_device(d_tok.data_ptr(), len(tokens), d_off.data_ptr(), len(tok_off) - 1, max_length=5, eos=1, pad=7, dtype=dtype, **gp.shim_args(kw)),
                ("input_ids", "attention_mask", "lengths", "row_doc", "row_tok", "doc_row"))
        pr.same(gp.pad_device(core, tokens, tok_off, 5, eos=1, pad=7, dtype=dtype, held=(d_tok, d_off), **kw), pr.padded_rule(tokens, tok_off, 5, eos=1, pad=7, **kw),
                ("padded", dtype, kw))

    for dtype in (np.uint32, np.uint16):
        for kw in (dict(), dict(width_multiple=1), dict(windows=True, stride=1)):
            padded(small, dtype, **kw)
            padded(large, dtype, **kw)
            padded(small, dtype, **kw)

    # samples: 7 parts in 3 samples, 3 roles with 5 role ids in all
    roles = (sr.Role((90001, 90002), (90003,), False), sr.Role((), (), True), sr.Role((90004,), (90005,), True))
    few = sr.pack([[(0, gs.body(rng, 1)), (2, gs.body(rng, 3))], [(1, [])], [(2, gs.body(rng, 2)), (0, []), (1, gs.body(rng, 9)), (2, gs.body(rng, 1))]])
    lots = sr.pack([[(int(rng.integers(0, 3)), body)] for body in many])
    assert len(few[2]) == 7 and len(few[3]) == 4
    for kw in (dict(), dict(width_multiple=1, left=True), dict(keep_tail=True)):
        for arrays in (few, lots, few):
            on_device = gs.to_device(*arrays)
            r = gs.call(core, arrays, on_device, roles, 5, eos=1, pad=7, **kw)
            aligned(r, ("input_ids", "attention_mask", "labels", "length", "full_length", "n_trained"))
            sr.same(gs.read(r), sr.samples_rule(*arrays, roles, 5, eos=1, pad=7, **kw), ("samples", kw, len(arrays[2])))
