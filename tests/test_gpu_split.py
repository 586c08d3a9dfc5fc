"""Text chunks on the GPU (tk_split.h): tk_split_device and tk_encode_batch_split through CoreBPE and Encoding, bit-exact against the
restatement of the rule in tests/split_ref.py (a loop per document, written from the rule's description in include/tiktoken_amd.h, not from
the kernels) on the ids and the text of the same call.  The shapes are the smallest at which each mechanism can go wrong: windows at the
edges of a 64-bit plane word, chars cut by tokens, blocks of K = 64 with steps that jump them, separators at a document's edges."""
import ctypes

import numpy as np
import pytest

import helpers as h
import split_ref as sr
import tiktoken_amd as tiktoken
from tiktoken_amd import _lib, _tiktoken

pytestmark = pytest.mark.gpu


def enc_of(name="gpt2_shaped"):
    return tiktoken.get_encoding(name)


def want_of(enc, ch, texts, N, M, O, separators):
    docs = [t if isinstance(t, bytes) else t.encode("utf-8") for t in texts]
    return sr.split_rule(docs, sr.token_lens(enc, ch.tokens, ch.tok_off), N, M, O, separators)


def check(enc, texts, N, M=None, O=0, separators=sr.DEFAULT, ctx="", **kw):
    """split_ordinary_batch_packed against the restatement; returns (result, reference)"""
    ch = enc.split_ordinary_batch_packed(texts, N, min_tokens=M, overlap=O, separators=separators, **kw)
    M = max(O + 1, N // 2) if M is None else M
    want = want_of(enc, ch, texts, N, M, O, separators)
    sr.same(ch, want, (ctx, N, M, O, kw))
    return ch, want


def single_token_words(enc, n):
    """n different words " w" that are one token each, none a prefix of another"""
    found = []
    for w in (" the", " of", " and", " in", " to", " is", " for", " on", " with", " as", " at", " by", " it", " be", " or"):
        if len(enc.encode_ordinary(w)) == 1:
            found.append(w)
    assert len(found) >= n, found
    return found[:n]


# ---------------------------------------------------------------- windows at the edges of a plane word
@pytest.mark.parametrize("O", (0, 1))
def test_window_at_the_edges_of_a_plane_word(O):
    """One document of 200 one-token words per call, so that a token's index in the document is its bit in the planes; N = 7, M = 2: the
    only level-0 boundary before token 63, 64, 65, 127, 128 in turn (bits 63, 0, 1, 63, 0 of a plane word), a level-1 boundary one and
    two tokens later -- in the same window for some chains -- which must lose.  Then the same documents behind one of 64 tokens, which
    moves every boundary into the next word."""
    enc = enc_of()
    plain, zero, one = single_token_words(enc, 3)
    seps = [[("", zero)], [("", one)]]
    seen = 0
    for lead in (0, 64):
        for k in (63, 64, 65, 127, 128):
            for later in (1, 2):
                words = [plain] * 200
                words[k], words[k + later] = zero, one
                texts = ([plain * lead] if lead else []) + ["".join(words)]
                ch, want = check(enc, texts, 7, 2, O, seps, ctx=(lead, k, later))
                d = len(texts) - 1
                assert ch.tok_off.tolist() == ([0, 64, 264] if lead else [0, 200])
                assert (int(ch.tok_off[d]) + k) % 64 == k % 64 and k % 64 in (63, 0, 1)  # (the boundary's bit in its plane word)
                for i in range(int(ch.doc_chunk[d]), int(ch.doc_chunk[d + 1])):  # a chunk whose window [s + 2, s + 7] holds the level-0 boundary ends there
                    s = int(ch.tok_begin[i])
                    if s + 2 <= k <= s + 7 and 200 - s > 7:
                        assert int(ch.tok_end[i]) == k and int(ch.cut[i]) == 0, (lead, k, later, i)
                        seen += 1
    assert seen >= 10  # (a chain may step over the boundary: it may lie at s + 1)


# ---------------------------------------------------------------- char boundaries
@pytest.mark.parametrize("O", (0, 2))
def test_chunks_begin_and_end_at_chars(O):
    """4-byte emoji and 3-byte CJK under the shaped o200k vocabulary, where a char is several tokens; N - M = 3, the least the rule allows."""
    enc = enc_of("o200k_shaped")
    rng = np.random.default_rng(3)
    chars = list("😀🦊🧪日本語漢字テキスト") + [" ", "a", "\n"]
    texts = ["".join(rng.choice(chars, size=n)) for n in (1, 17, 400, 900)]
    ch, _ = check(enc, texts, 6, 3, O)
    assert int(np.diff(ch.tok_off).max()) > max(len(t) for t in texts)  # (chars do split into tokens)
    blob = [t.encode() for t in texts]
    for i in range(len(ch)):
        b = blob[int(ch.doc[i])]
        assert not sr.is_cont(b[int(ch.byte_begin[i])]) and sr.FORCED != int(ch.cut[i])
        assert ch.text_bytes(i).decode("utf-8") == texts[int(ch.doc[i])][int(ch.char_begin[i]):int(ch.char_end[i])]
    if O == 0:
        assert ["".join(p) for p in enc.split_batch(texts, 6, min_tokens=3, disallowed_special=())] == texts


# ---------------------------------------------------------------- segments
def paragraphs(rng, n_words):
    words = ["alpha", "beta", "gamma", "of", "the", "3.14", "naïve"]
    out = []
    for _ in range(n_words):
        out.append(words[int(rng.integers(len(words)))])
        r = rng.random()
        out.append("\n\n" if r < 0.04 else "\n" if r < 0.1 else ". " if r < 0.25 else " ")
    return "".join(out)


def text_of_tokens(enc, rng, n):
    """prose that encodes to exactly n tokens: a prefix of an encoding, decoded; cutting may change the count at the cut, so prefixes are tried"""
    ids = enc.encode_ordinary(paragraphs(rng, n + 50))
    for k in sorted(range(max(n - 8, 1), n + 9), key=lambda k: abs(k - n)):
        t = enc.decode(ids[:k])
        if len(enc.encode_ordinary(t)) == n:
            return t
    raise AssertionError(f"no prefix encodes to {n} tokens")


def test_blocks_of_64_with_documents_around_their_edges():
    """K = 64; documents of 1, 63, 64, 65, 300 and 5 000 tokens with empty ones between them, first and last; N = 200 > K, so steps jump
    whole blocks, and N = 16 < K."""
    enc = enc_of()
    rng = np.random.default_rng(64)
    body = [text_of_tokens(enc, rng, n) for n in (1, 63, 64, 65, 300, 5000)]
    texts = [""] + [x for t in body for x in (t, "")]
    for N, M, O in ((200, 100, 0), (200, 150, 37), (16, 8, 0), (16, 8, 7)):
        ch, _ = check(enc, texts, N, M, O, seg_tokens=64, ctx="K=64")
        assert np.diff(ch.tok_off.astype(np.int64)).tolist() == [0, 1, 0, 63, 0, 64, 0, 65, 0, 300, 0, 5000, 0]
        assert ch.doc_chunk[0] == 0 and ch.doc_chunk[1] == 0 and ch.doc_chunk[-1] == len(ch)


def test_segments_join_on_paragraphs_and_not_on_separator_free_text():
    """With K = 64 the true chain meets the speculative walks in prose (tk_stat "split_joined" > 0).  In "x" * n and in digit runs no
    boundary has a level and every one is legal, so every cut is hard: the true chain stands on the multiples of N, the speculative walk of
    block b on 64 b + (N - M) + j N, and with N = 16, M = 8 the two never meet (64 b + 8 is no multiple of 16): joined == 0, and the result
    is exact all the same -- the stitch pass has walked everything."""
    enc = enc_of()
    core = enc._core_bpe
    rng = np.random.default_rng(5)
    check(enc, [paragraphs(rng, 3000)], 16, 8, seg_tokens=64)
    assert core.stat("split_joined") > 0 and core.stat("split_segments") > 1 and core.stat("split_spec_steps") > 0
    for flat in ("x" * 6000, "7" * 6000):
        ch, _ = check(enc, [flat], 16, 8, seg_tokens=64)
        assert set(ch.cut.tolist()) <= {sr.HARD, sr.END} and len(ch.tokens) > 64 * 3
        assert core.stat("split_joined") == 0 and core.stat("split_stitch_steps") >= len(ch) - 8


def test_k_does_not_change_the_answer():
    enc = enc_of("cl100k_shaped")
    rng = np.random.default_rng(300)
    texts = [paragraphs(rng, int(n)) if i % 7 else "9" * int(n) for i, n in enumerate(rng.integers(0, 500, size=300))]
    first, _ = check(enc, texts, 64, 32, 5, seg_tokens=64)
    for K in (1024, 0):
        other = enc.split_ordinary_batch_packed(texts, 64, min_tokens=32, overlap=5, seg_tokens=K)
        sr.same(other, first, K)


# ---------------------------------------------------------------- separators
def test_separators_tail_head_both_long_and_at_document_edges():
    enc = enc_of()
    s16 = "0123456789abcdef"
    rng = np.random.default_rng(16)
    parts = ["x", " yy", s16, "ab", "cd", "\n", " the"]
    body = "".join(parts[int(i)] for i in rng.integers(len(parts), size=900))
    texts = [s16 + body + s16, "cd" + body[:80] + "ab", "\n" * 40, "\n\n" + body[:300] + "\n\n"]
    seps = [[(s16, "")], [("", s16)], [("ab", "cd")], [("\n", ""), ("", "\n")]]  # tail only, head only, both, parts of 16 bytes
    ch, _ = check(enc, texts, 9, 3, 0, seps)
    assert {0, 1, 2, 3} <= set(ch.cut.tolist())
    check(enc, texts, 9, 3, 2, seps)
    # two levels that match one boundary: the lower wins
    ch, _ = check(enc, texts, 9, 3, 0, [[("\n", "")], [("\n", "")]])
    assert 1 not in ch.cut.tolist() and 0 in ch.cut.tolist()
    # a bare str is (x, ""); L = 0: hard cuts only
    ch, _ = check(enc, texts, 9, 3, 0, [["\n"], [b"ab"]])
    ch, _ = check(enc, texts, 9, 3, 0, [])
    assert set(ch.cut.tolist()) <= {sr.HARD, sr.END}
    # L = 4 with four separators in each level
    four = [[(c + str(i), "") for i in range(4)] for c in ("x", "y", "\n", "d")]
    check(enc, texts, 9, 3, 0, four)
    # the default separators on prose: every level occurs
    ch, _ = check(enc, [paragraphs(rng, 2000)], 24)
    assert {0, 1, 2, 3} <= set(ch.cut.tolist())


def test_separators_do_not_match_across_a_document_edge():
    """A tail that would need the previous document's last byte, a head that would need the next document's first: neither matches.
    N = 4, M = 1, so boundary 1 of a document lies in its first window and the last boundary in the last one."""
    enc = enc_of()
    tok = lambda t: [enc.decode_single_token_bytes(i) for i in enc.encode_ordinary(t)]  # noqa: E731
    # tail ("ab", ""): document 0 ends with "a", document 1 is "b" and then " cd" tokens; its boundary 1 has "b" before it, "ab" across the edge
    texts = [" x" * 20 + "a", "b" + " cd" * 30]
    assert tok(texts[1])[0] == b"b" and texts[0].endswith("a")
    ch, _ = check(enc, texts, 4, 1, 0, [[("ab", "")]])
    assert 0 not in ch.cut.tolist()
    ch, _ = check(enc, [texts[0] + texts[1]], 4, 1, 0, [[("ab", "")]])  # (in one document it does match)
    assert 0 in ch.cut.tolist()
    # head = document 0's last token and then "d": document 1 starts with "d"; n_0 = 4 j + 1, so the hard cuts of 4 tokens leave a last
    # window that holds the boundary before that token
    reps = next(r for r in range(30, 40) if len(tok(" x" * r + " c")) % 4 == 1)
    texts = [" x" * reps + " c", "d" + " x" * 30]
    head = tok(texts[0])[-1] + b"d"
    assert len(tok(texts[0])) > 8 and head in (b" cd", b"cd")
    ch, _ = check(enc, texts, 4, 1, 0, [[(b"", head)]])
    assert 0 not in ch.cut.tolist()
    ch, _ = check(enc, [texts[0] + texts[1]], 4, 1, 0, [[(b"", head)]])
    assert 0 in ch.cut.tolist()


def test_overlap_up_to_min_tokens_less_one():
    enc = enc_of("o200k_shaped")
    rng = np.random.default_rng(9)
    texts = [paragraphs(rng, 800), "😀日本" * 200, ""]
    for N, M in ((6, 3), (9, 4)):
        ch, want = check(enc, texts, N, M, M - 1)
        assert len(ch) == len(want.doc)
        blob = [t.encode() for t in texts]
        for d in range(len(texts)):
            mine = slice(int(ch.doc_chunk[d]), int(ch.doc_chunk[d + 1]))
            assert (np.diff(ch.tok_begin[mine].astype(np.int64)) > 0).all()
            assert not any(sr.is_cont(blob[d][int(b)]) for b in ch.byte_begin[mine])


# ---------------------------------------------------------------- refusals
def device_batch(enc, texts):
    """(blob, off, d_text, d_off, d_tok pointer, n_tokens, d_tok_off pointer) of a batch encoded on the device"""
    import torch

    blob, off = enc._pack(texts)
    d_text = torch.zeros(len(blob) + 256, dtype=torch.uint8, device="cuda")
    d_text[: len(blob)] = torch.from_numpy(blob.copy()).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    dt, nt, dof = enc._core_bpe.encode_batch_device(d_text.data_ptr(), len(blob), d_off.data_ptr(), off, len(texts))
    return blob, off, d_text, d_off, dt, nt, dof


def fetch(r, n_docs):
    C = r.n_chunks
    u8 = h.dev_u32(r.cut, (C + 3) // 4).view(np.uint8)[:C] if C else np.zeros(0, np.uint8)
    return sr.Chunks(*[h.dev_u32(p, C) for p in r[:7]], u8, h.dev_u32(r.doc_chunk, n_docs + 1))


def test_spec_refusals_name_their_argument():
    enc = enc_of()
    texts = ["some text to split. " * 30]
    for kw, name in ((dict(min_tokens=0), "min_tokens"), (dict(max_tokens=5, min_tokens=3), "max_tokens"), (dict(min_tokens=4, overlap=4), "overlap"),
                     (dict(separators=[[("x" * 17, "")]]), "separators"), (dict(separators=[[("", "y" * 17)]]), "separators"), (dict(separators=[[("", "")]]), "separators"),
                     (dict(separators=[["a"]] * 5), "n_levels"), (dict(separators=[["a", "b", "c", "d", "e"]]), "n_seps"), (dict(seg_tokens=96), "seg_tokens"),
                     (dict(seg_tokens=1), "seg_tokens")):
        args = {"max_tokens": 16, **kw}
        with pytest.raises(ValueError, match=name):
            enc.split_ordinary_batch_packed(texts, args.pop("max_tokens"), **args)
    # ... by the library itself, not only by the wrapper: a structure the wrapper would not build
    core = enc._core_bpe
    spec = core._split_spec(16, 8, 0, [["a"]], 0)
    blob, off, d_text, d_off, dt, nt, dof = device_batch(enc, texts)
    for field, value, name in (("n_levels", 5, "n_levels"), ("flags", 1, "flag")):
        bad = type(spec).from_buffer_copy(spec)
        setattr(bad, field, value)
        outs = [ctypes.c_void_p() for _ in range(9)]
        rc = core._L.tk_split_device(core._h, dt, nt, dof, 1, d_text.data_ptr(), d_off.data_ptr(), ctypes.byref(bad), None, *[ctypes.byref(x) for x in outs],
                                     ctypes.byref(ctypes.c_uint64()))
        assert rc == _lib.TK_VALUE_ERROR and name in _lib.last_error()
    bad = type(spec).from_buffer_copy(spec)
    bad.n_seps[0] = 5
    bad.sep[0][0].tail_len = 17
    rc = core._L.tk_split_device(core._h, dt, nt, dof, 1, d_text.data_ptr(), d_off.data_ptr(), ctypes.byref(bad), None, *[ctypes.byref(ctypes.c_void_p()) for _ in range(9)],
                                 ctypes.byref(ctypes.c_uint64()))
    assert rc == _lib.TK_VALUE_ERROR and "n_seps" in _lib.last_error()
    for tail_len, head_len, words in ((17, 0, "at most 16 bytes"), (0, 17, "at most 16 bytes"), (0, 0, "both empty")):
        bad = type(spec).from_buffer_copy(spec)
        bad.sep[0][0].tail_len, bad.sep[0][0].head_len = tail_len, head_len
        rc = core._L.tk_split_device(core._h, dt, nt, dof, 1, d_text.data_ptr(), d_off.data_ptr(), ctypes.byref(bad), None,
                                     *[ctypes.byref(ctypes.c_void_p()) for _ in range(9)], ctypes.byref(ctypes.c_uint64()))
        assert rc == _lib.TK_VALUE_ERROR and "separators" in _lib.last_error() and words in _lib.last_error(), _lib.last_error()
    with pytest.raises(ValueError, match="n_tokens"):  # (refused from the figures alone: nothing is read)
        core.split_device(dt, 1 << 32, dof, 1, d_text.data_ptr(), d_off.data_ptr(), max_tokens=16)
    with pytest.raises(ValueError, match="n_docs"):
        core.split_device(dt, nt, dof, (1 << 32) - 1, d_text.data_ptr(), d_off.data_ptr(), max_tokens=16)


def test_bad_tok_off_names_the_document_and_leaves_the_previous_result():
    import torch

    enc = enc_of()
    core = enc._core_bpe
    rng = np.random.default_rng(2)
    texts = [paragraphs(rng, 200), "a short one", paragraphs(rng, 50)]
    blob, off, d_text, d_off, dt, nt, dof = device_batch(enc, texts)
    good = core.split_device(dt, nt, dof, 3, d_text.data_ptr(), d_off.data_ptr(), max_tokens=16)
    before = fetch(good, 3)
    tok_off = torch.as_tensor(h._DevArray(dof, 4 * 2, "<i4"), device="cuda").cpu().numpy().view(np.uint64).copy()
    for bad, msg in ((tok_off + np.uint64(1), r"tok_off\[0\] must be 0 \(document 0\)"), (tok_off[[0, 2, 1, 3]], "document 1 ends before it starts"),
                     (np.concatenate([tok_off[:3], [tok_off[3] + np.uint64(7)]]).astype(np.uint64), "document 2 ends elsewhere")):
        d_bad = torch.from_numpy(bad.view(np.int64).copy()).cuda()
        torch.cuda.synchronize()
        with pytest.raises(ValueError, match=msg):
            core.split_device(dt, nt, d_bad.data_ptr(), 3, d_text.data_ptr(), d_off.data_ptr(), max_tokens=16)
        sr.same(fetch(good, 3), before, "the previous result after a refusal")
    with pytest.raises(ValueError, match="overlap"):
        core.split_device(dt, nt, dof, 3, d_text.data_ptr(), d_off.data_ptr(), max_tokens=16, min_tokens=8, overlap=8)
    sr.same(fetch(good, 3), before, "the previous result after a refused spec")


# ---------------------------------------------------------------- the other entries
def test_special_tokens_inside_chunks_and_at_cuts():
    enc = enc_of("o200k_shaped")
    eot = "<|endoftext|>"
    rng = np.random.default_rng(8)
    texts = [(paragraphs(rng, 30) + eot) * 20, eot * 40, "no specials here. " * 40]
    seps = [[("", eot)], [(eot, "")], [("", " ")]]
    ch = enc.split_batch_packed(texts, 12, min_tokens=4, separators=seps, allowed_special={eot})
    assert int((ch.tokens == enc.eot_token).sum()) == 60
    want = want_of(enc, ch, texts, 12, 4, 0, seps)
    sr.same(ch, want, "allowed_special")
    assert 0 in ch.cut.tolist() and any(enc.eot_token in ch.ids(i)[1:-1].tolist() for i in range(len(ch)))
    with pytest.raises(_tiktoken.DisallowedSpecialError):
        enc._core_bpe.encode_batch_split_packed(*enc._pack(texts), None, disallowed_special=frozenset({eot}), max_tokens=12)
    with pytest.raises(ValueError):
        enc.split_batch_packed(texts, 12)
    pieces = enc.split_batch(texts, 12, disallowed_special=())
    assert ["".join(p) for p in pieces] == texts


def test_split_device_agrees_with_the_host_text_entry():
    enc = enc_of("cl100k_shaped")
    rng = np.random.default_rng(4)
    texts = [paragraphs(rng, int(n)) for n in (0, 5, 700, 0, 64, 2000)]
    blob, off, d_text, d_off, dt, nt, dof = device_batch(enc, texts)
    for kw in (dict(max_tokens=48), dict(max_tokens=48, min_tokens=20, overlap=6, seg_tokens=128)):
        got = fetch(enc._core_bpe.split_device(dt, nt, dof, len(texts), d_text.data_ptr(), d_off.data_ptr(), **kw), len(texts))
        host = enc.split_ordinary_batch_packed(texts, kw.pop("max_tokens"), **kw)
        sr.same(got, host, kw)
        assert len(host.tokens) == nt and [host.text(i) for i in range(3)] == [host.text_bytes(i).decode() for i in range(3)]


def test_ill_formed_text_forces_cuts():
    """A run of 40 continuation bytes through the packed entry (a str cannot hold them): no boundary inside the run is legal."""
    enc = enc_of()
    doc = b"ab " + b"\x80" * 40 + b" cd" * 10
    blob, off = np.frombuffer(doc, np.uint8), np.array([0, len(doc)], np.uint64)
    ch = enc._core_bpe.encode_batch_split_packed(blob, off, None, max_tokens=7, min_tokens=2)
    want = sr.split_rule([doc], sr.token_lens(enc, ch.tokens, ch.tok_off), 7, 2, 0, sr.DEFAULT)
    sr.same(ch, want, "forced")
    assert sr.FORCED in ch.cut.tolist()


def test_one_larger_run_on_the_test_corpus():
    """About 2 000 documents of the corpus generator at N = 512 with the default separators."""
    enc = enc_of("o200k_shaped")
    blob, off = h.gen_corpus(0x5911, 0, 2 << 20)
    keep = min(len(off) - 1, 2000)
    blob, off = blob[: int(off[keep])], off[: keep + 1]
    ch = enc._core_bpe.encode_batch_split_packed(blob, off, None, max_tokens=512)
    docs = [blob[int(a):int(b)].tobytes() for a, b in zip(off[:-1], off[1:])]
    want = sr.split_rule(docs, sr.token_lens(enc, ch.tokens, ch.tok_off), 512, 256, 0, sr.DEFAULT)
    sr.same(ch, want, "corpus")
    assert len(ch) > keep // 2
