"""Token n-gram sets on the GPU (tk_ngram.h): the set's entries through CoreBPE and Encoding, value for value against tests/ngram_ref.py --
a Python set of tuples --, never against another run of the code under test.  Every batch goes through the host entries and through the
device entries on a side stream.  The shapes are ngram_ref.batches' (lengths, tile and word edges, unions, extreme ids) and, here, the
contended table, persistence, the refusals and the one-call entries.
Tables of 4 and 8 slots: an add of n n-grams carries at least n k tokens and is refused past the capacity, so such a set takes
(S / 2) // k n-grams -- chains that wrap for k = 1 and 2, none at k = 13 and 32, where the table is asked empty and the add is refused."""
import functools

import numpy as np
import pytest
import torch

import ngram_ref as nr
import tiktoken_amd as tiktoken
from tiktoken_amd import DisallowedSpecialError
from tiktoken_amd._lib import last_error as lib_error

pytestmark = pytest.mark.gpu
POISON = 0x55


def enc_of(name="gpt2_shaped"):
    return tiktoken.get_encoding(name)


@functools.lru_cache(maxsize=None)
def cases(T: int, k: int):
    """(name, tokens, tok_off, held, the reference's result), computed once"""
    return [(*c, nr.overlap(c[3], c[1], c[2], k)) for c in nr.batches(T, k)]


def on_device(enc, arr, stream):
    with torch.cuda.stream(stream):
        return torch.from_numpy(arr.view({4: np.int32, 8: np.int64}[arr.itemsize]).copy()).to(torch.device("cuda", enc._core_bpe.device), non_blocking=True)


def device_overlap(enc, ngs, tok, off, skip=()):
    """tk_ngram_overlap_device on a side stream: uploads, poison, the call and the copies back are queued there and nothing else is waited for"""
    dev = torch.device("cuda", enc._core_bpe.device)
    stream = torch.cuda.Stream(dev)
    t_tok, t_off = on_device(enc, tok, stream), on_device(enc, off, stream)
    with torch.cuda.stream(stream):
        outs = [torch.full((len(off) - 1,), POISON, dtype=torch.int64, device=dev) for _ in range(4)] + [torch.full((len(tok),), POISON, dtype=torch.uint8, device=dev)]
        names = ("n_hit", "n_covered", "n_ngrams", "first_hit", "mask")
        enc._core_bpe.ngram_overlap_device(ngs._native, t_tok, t_off, **{n: o for n, o in zip(names, outs) if n not in skip})
        pinned = [torch.empty(o.shape, dtype=o.dtype, pin_memory=True) for o in outs]
        for h, o in zip(pinned, outs):
            h.copy_(o, non_blocking=True)
    stream.synchronize()
    return nr.Ref(*[h.numpy().view(np.uint64) for h in pinned[:4]], np.diff(off), pinned[4].numpy())


def same(got, want, what, skip=()):
    for f in nr.Ref._fields:
        a, b = getattr(got, f), getattr(want, f)
        if f in skip:
            assert (a == POISON).all(), (what, f, "written though not asked for")
        else:
            assert a.shape == b.shape and (a == b).all(), (what, f, np.flatnonzero(a != b)[:8])


def filled(enc, k, held, capacity=None, device=False):
    """a set of `held`, added through the host entry or through the device entry on a side stream"""
    ngs = enc.ngram_set(k, capacity=capacity or max(len(held) * k, 1), seed=9)
    tok, off = nr.as_docs(held, k)
    if device:
        stream = torch.cuda.Stream(torch.device("cuda", enc._core_bpe.device))
        t = on_device(enc, tok, stream), on_device(enc, off, stream)
        enc._core_bpe.ngram_add_device(ngs._native, *t, stream=stream.cuda_stream)  # (len() waits for it; t lives until then)
        assert len(ngs) == len(held)
    else:
        ngs.add_tokens_packed(tok, off)
    return ngs


@pytest.mark.parametrize("k", nr.KS)
def test_every_shape_through_host_and_device_entries(k):
    enc = enc_of()
    T = int(enc._core_bpe.stat("ngram_tile"))
    small = [(f"S{S}", *nr.small_table(k, S, seed=9)) for S in (4, 8)]
    for i, (name, tok, off, held, *want) in enumerate(cases(T, k) + small):
        want = want[0] if want else nr.overlap(held, tok, off, k)
        with filled(enc, k, held, int(name[1:]) // 2 if name[0] == "S" else None, device=i % 2 == 1) as ngs:
            assert len(ngs) == len(held), name
            same(ngs.overlap_tokens_packed(tok, off, mask=True), want, (name, "host"))
            same(device_overlap(enc, ngs, tok, off), want, (name, "device"))
            if name[0] == "S" and not held:  # (k > S / 2: one n-gram is more tokens than the capacity)
                with pytest.raises(ValueError):
                    ngs.add_tokens_packed(tok[:k], off[:2])
                assert len(ngs) == 0


@pytest.mark.parametrize("k", nr.KS)
def test_contended_table(k):
    """One n-gram 5000 times in one call; 20 000 random documents over 4 ids against half their n-grams, added from the documents themselves."""
    enc = enc_of()
    one = (3,) * k
    with enc.ngram_set(k, capacity=5000 * k) as ngs:
        ngs.add_tokens_packed(np.full(5000 * k, 3, np.uint32), (np.arange(5001) * k).astype(np.uint64))
        assert len(ngs) == 1
        same(ngs.overlap_tokens_packed(*nr.as_docs({one, (4,) * k}, k), mask=True), nr.overlap({one}, *nr.as_docs({one, (4,) * k}, k), k), "one key")
    tok, off = nr.pack(np.random.default_rng(k).integers(0, 2 * k + 1, 20000), 77 + k, alphabet=4)
    held = nr.half(tok, off, k)
    want = nr.overlap(held, tok, off, k)
    share = want.n_hit.sum() / want.n_ngrams.sum()
    assert 0 < share < 1 and want.n_ngrams.sum() < 10 ** 6, share
    a_tok, a_off = nr.as_docs(held, k)
    with enc.ngram_set(k, capacity=2 * len(a_tok)) as ngs:
        ngs.add_tokens_packed(np.tile(a_tok, 2), np.concatenate([a_off, a_off[1:] + a_off[-1]]))  # (every key twice in one call)
        assert len(ngs) == len(held)
        same(ngs.overlap_tokens_packed(tok, off, mask=True), want, "host")
        same(device_overlap(enc, ngs, tok, off), want, "device")


def test_persistence_null_outputs_clear_and_refusals():
    enc, k = enc_of(), 2
    _, tok, off, held, want = cases(int(enc._core_bpe.stat("ngram_tile")), k)[0]
    parts = [set(sorted(held)[::2]), set(sorted(held)[1::2])]
    with enc.ngram_set(k, capacity=len(held) * k, seed=3) as ngs:
        for p in parts:  # two adds, then an overlap: the reference's result for the union
            ngs.add_tokens_packed(*nr.as_docs(p, k))
        same(ngs.overlap_tokens_packed(tok, off, mask=True), want, "two adds")
        for skip in [(f,) for f in nr.Ref._fields[:4] + ("mask",)] + [nr.Ref._fields[:4]]:  # each output null in turn, then the mask alone
            same(device_overlap(enc, ngs, tok, off, skip=skip), want, ("without", skip), skip=skip)
        assert ngs.overlap_tokens_packed(tok, off).mask is None
        with pytest.raises(ValueError):  # the bound is full: an add past it is refused, and nothing has changed
            ngs.add_tokens_packed(*nr.as_docs({(9, 9)}, k))
        assert "capacity" in lib_error()
        assert len(ngs) == len(held)
        same(device_overlap(enc, ngs, tok, off), want, "after the refused add")
        other = enc_of("cl100k_shaped")
        dev = torch.device("cuda", enc._core_bpe.device)
        n_hit = torch.full((len(off) - 1,), POISON, dtype=torch.int64, device=dev)
        with pytest.raises(ValueError):  # a set of another core
            other._core_bpe.ngram_overlap_device(ngs._native, on_device(enc, tok, torch.cuda.default_stream(dev)), on_device(enc, off, torch.cuda.default_stream(dev)), n_hit=n_hit)
        assert "another core" in lib_error()
        torch.cuda.synchronize(dev)
        assert (n_hit.cpu().numpy() == POISON).all(), "a refused call has written"
        ngs.clear()
        assert len(ngs) == 0
        same(ngs.overlap_tokens_packed(tok, off, mask=True), nr.overlap(set(), tok, off, k), "cleared")
    for ngram, cap in ((0, 8), (33, 8), (13, 0), (13, 2 ** 30 + 1)):
        with pytest.raises(ValueError):
            enc.ngram_set(ngram, capacity=cap)
        assert "ngram" in lib_error() or "capacity" in lib_error(), lib_error()  # (the library's refusal, not Python's)


def test_one_call_entries_and_keep_mask():
    enc, k = enc_of(), 3
    held_texts = ["the quick brown fox jumps over the lazy dog", "", "a tile <|endoftext|> a wave and a lane"]
    texts = ["", "he said the quick brown fox jumps over it", "nothing in common here at all", "over the lazy dog " * 700, "x", "a tile <|endoftext|> a wave"]
    allow = {"<|endoftext|>"}
    with enc.ngram_set(k, capacity=1 << 12) as ngs:
        n_tok = ngs.add_ordinary_batch(held_texts[:2]) + ngs.add_batch(held_texts[2:], allowed_special=allow)
        held = nr.add(nr.add(set(), *enc.encode_ordinary_batch_packed(held_texts[:2]), k), *enc.encode_batch_packed(held_texts[2:], allowed_special=allow), k)
        assert len(ngs) == len(held) and n_tok == len(enc.encode_batch_packed(held_texts, allowed_special=allow)[0])
        for special in (False, True):
            tok, off = enc.encode_batch_packed(texts, allowed_special=allow) if special else enc.encode_ordinary_batch_packed(texts)
            want = nr.overlap(held, tok, off, k)
            got = ngs.overlap_batch(texts, mask=True, allowed_special=allow) if special else ngs.overlap_ordinary_batch(texts, mask=True)
            same(got, want, ("one call", special))
            same(ngs.overlap_tokens_packed(tok, off, mask=True), want, ("packed", special))
        assert int(np.diff(off).max()) > 2 * int(enc._core_bpe.stat("ngram_tile")) and want.n_hit[1] > 0 and want.n_hit[5] > 0
        assert got.keep_mask().tolist() == (want.n_hit == 0).tolist()
        assert got.keep_mask(max_hits=10 ** 6, max_covered_ratio=0.5).tolist() == [int(c) * 2 <= int(n) for c, n in zip(want.n_covered, want.length)]
        with pytest.raises(DisallowedSpecialError) as e:
            ngs.overlap_batch(texts)
        assert e.value.doc == 5
        with pytest.raises(DisallowedSpecialError):
            ngs.add_batch(texts)
        assert len(ngs) == len(held)
