"""Near-duplicate fingerprints on the GPU (tk_fingerprint.h): tk_fingerprint_device, tk_fingerprint and tk_encode_batch_fingerprint through
CoreBPE and Encoding, value for value against tests/fingerprint_ref.py -- the rule in Python --, never against another run of the code
under test.  The shapes (tests/fingerprint_cases.py): documents of 0, 1, k - 1, k, k + 1, T - 1, T, T + 1 and 3T + 5 tokens that end at a
tile's edge, one before and one behind it; runs of empty documents at the start, across an edge and at the end; more documents than a tile
has positions; one document, none, documents without tokens; ids all over uint32."""
import functools

import numpy as np
import pytest
import torch

import fingerprint_cases as fc
import fingerprint_ref as fr
import tiktoken_amd as tiktoken
from tiktoken_amd import DisallowedSpecialError, Fingerprints
from tiktoken_amd._lib import last_error as lib_error

pytestmark = pytest.mark.gpu
SPEC_IDS = [f"k{s[0]}-P{s[1]}-B{s[2]}-{s[3] & 0xFF:x}" for s in fc.SPECS]


def enc_of(name="gpt2_shaped"):
    return tiktoken.get_encoding(name)


def tile_of(enc) -> int:
    return int(enc._core_bpe.stat("fingerprint_tile"))


def kw(spec):
    return dict(ngram=spec[0], n_perm=spec[1], bands=spec[2], seed=spec[3])


@functools.lru_cache(maxsize=None)
def cases(T: int, k: int):
    return fc.batches(T, k)


@functools.lru_cache(maxsize=None)
def wanted(T: int, spec, i: int):
    """the reference's result for batch i of cases(T, k), computed once"""
    _, tok, off = cases(T, spec[0])[i]
    return fr.fingerprint(tok, off, *spec)


def same(got, want, what):
    for name in fr.Ref._fields:
        a, b = np.asarray(getattr(got, name)), getattr(want, name)
        assert a.shape == b.shape and a.dtype == b.dtype and (a == b).all(), (what, name, np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))[:8])


def device_run(enc, tok, off, spec, skip=None, side=False):
    """tk_fingerprint_device on torch tensors; output `skip` (0 .. 3) is not asked for.  Everything -- the uploads, the poison every array is
    filled with first, the call, the copies back -- is queued on one stream, torch's default stream or (`side`) a stream of its own, and
    nothing but that stream is waited for: the call has to order itself there."""
    dev = torch.device("cuda", enc._core_bpe.device)
    n, P, B = len(off) - 1, spec[1], spec[2]
    stream = torch.cuda.Stream(dev) if side else torch.cuda.default_stream(dev)
    with torch.cuda.stream(stream):
        t_tok = torch.from_numpy(tok.view(np.int32).copy()).to(dev, non_blocking=True)
        t_off = torch.from_numpy(off.view(np.int64).copy()).to(dev, non_blocking=True)
        outs = [torch.full((n * P,), 0x55, dtype=torch.int32, device=dev), *[torch.full((m,), 0x55, dtype=torch.int64, device=dev) for m in (n * B, n, n)]]
        given = [None if i == skip else o for i, o in enumerate(outs)]
        enc._core_bpe.fingerprint_device(t_tok, t_off, **kw(spec), sig=given[0], band=given[1], exact=given[2], n_shingles=given[3])
        pinned = [torch.empty(o.shape, dtype=o.dtype, pin_memory=True) for o in outs]
        for h, o in zip(pinned, outs):
            h.copy_(o, non_blocking=True)
    stream.synchronize()
    host = [h.numpy() for h in pinned]
    return [host[0].view(np.uint32).reshape(n, P), host[1].view(np.uint64).reshape(n, B), host[2].view(np.uint64), host[3].view(np.uint64)]


@pytest.mark.parametrize("spec", fc.SPECS, ids=SPEC_IDS)
def test_token_entries_on_every_shape(spec):
    """Every shape through the host entry and through the device entry, on torch's default stream and on a side stream."""
    enc = enc_of()
    T = tile_of(enc)
    assert T % 4 == 0
    for i, (name, tok, off) in enumerate(cases(T, spec[0])):
        want = wanted(T, spec, i)
        same(enc.fingerprint_tokens_packed(tok, off, **kw(spec)), want, (name, "host"))
        for side in (False, True):
            got = device_run(enc, tok, off, spec, side=side)
            same(Fingerprints(*got, np.diff(off)), want, (name, "device", side))


def test_device_entry_with_each_output_left_out():
    """Every spec, every shape, each of the four outputs null in turn (the streams alternating): the others are right, and the array that
    was not handed over keeps its poison."""
    enc = enc_of()
    T = tile_of(enc)
    for spec in fc.SPECS:
        for i, (name, tok, off) in enumerate(cases(T, spec[0])):
            want = wanted(T, spec, i)
            for skip in range(4):
                got = device_run(enc, tok, off, spec, skip, side=skip % 2 == 1)
                for j, field in enumerate(("sig", "band", "exact", "n_shingles")):
                    if j == skip:
                        assert (got[j] == 0x55).all(), (spec, name, field, "written though not asked for")
                    else:
                        assert (got[j] == getattr(want, field)).all(), (spec, name, field, skip)


DELAY = 40_000_000  # cycles of torch.cuda._sleep: some tens of milliseconds on the stream, far longer than a call takes to return


def test_device_entry_is_ordered_on_its_stream():
    """The stream is held up (torch.cuda._sleep) before the inputs are made on it -- copies of tensors uploaded earlier -- and before the
    outputs are poisoned: a call that ran on another stream than the caller's would read the inputs before they exist, be overwritten by
    the poison, or be read back before it is done.  On torch's default stream and on a side stream; only that stream is waited for."""
    enc = enc_of()
    spec = fc.SPECS[0]
    T = tile_of(enc)
    _, tok, off = cases(T, spec[0])[0]
    want = wanted(T, spec, 0)
    dev = torch.device("cuda", enc._core_bpe.device)
    n, P, B = len(off) - 1, spec[1], spec[2]
    up_tok, up_off = torch.from_numpy(tok.view(np.int32).copy()).to(dev), torch.from_numpy(off.view(np.int64).copy()).to(dev)
    torch.cuda.synchronize(dev)
    for side in (False, True):
        stream = torch.cuda.Stream(dev) if side else torch.cuda.default_stream(dev)
        with torch.cuda.stream(stream):
            t_tok, t_off = torch.zeros_like(up_tok), torch.zeros_like(up_off)
            torch.cuda._sleep(DELAY)
            t_tok.copy_(up_tok)
            t_off.copy_(up_off)
            outs = [torch.full((n * P,), 0x55, dtype=torch.int32, device=dev), *[torch.full((m,), 0x55, dtype=torch.int64, device=dev) for m in (n * B, n, n)]]
            enc._core_bpe.fingerprint_device(t_tok, t_off, **kw(spec), sig=outs[0], band=outs[1], exact=outs[2], n_shingles=outs[3])
            pinned = [torch.empty(o.shape, dtype=o.dtype, pin_memory=True) for o in outs]
            for h, o in zip(pinned, outs):
                h.copy_(o, non_blocking=True)
        stream.synchronize()
        got = [pinned[0].numpy().view(np.uint32).reshape(n, P), pinned[1].numpy().view(np.uint64).reshape(n, B), pinned[2].numpy().view(np.uint64),
               pinned[3].numpy().view(np.uint64)]
        same(Fingerprints(*got, np.diff(off)), want, ("held up", side))


def test_band_keys_without_signatures_on_two_streams():
    """Band keys without signatures pass the signatures through a buffer of the core, which the library orders among the calls that use it.
    Two such calls on two streams, the first held up, then a host call (which uses the buffer too) before either is waited for: all
    three results are right.  (The interleaving that would corrupt an unordered buffer cannot be forced from here; this checks that the
    ordering neither deadlocks nor loses a result.)"""
    enc = enc_of()
    spec = fc.SPECS[0]
    T = tile_of(enc)
    _, tok, off = cases(T, spec[0])[0]
    tok2 = (tok ^ np.uint32(0x5A5A5A5A)).astype(np.uint32)
    want, want2 = wanted(T, spec, 0), fr.fingerprint(tok2, off, *spec)
    dev = torch.device("cuda", enc._core_bpe.device)
    runs = []
    for t, delay in ((tok, True), (tok2, False)):
        stream = torch.cuda.Stream(dev)
        d_tok, d_off = torch.from_numpy(t.view(np.int32).copy()).to(dev), torch.from_numpy(off.view(np.int64).copy()).to(dev)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(stream):
            if delay:
                torch.cuda._sleep(DELAY)
            band = torch.full(((len(off) - 1) * spec[2],), 0x55, dtype=torch.int64, device=dev)
            enc._core_bpe.fingerprint_device(d_tok, d_off, **kw(spec), band=band)
        runs.append((stream, band, d_tok, d_off))
    same(enc.fingerprint_tokens_packed(tok2, off, **kw(spec)), want2, "host call in between")
    for (stream, band, _, _), w in zip(runs, (want, want2)):
        stream.synchronize()
        assert (band.cpu().numpy().view(np.uint64).reshape(w.band.shape) == w.band).all()


def text_batch(T: int):
    import random

    rng = random.Random(0x7E)
    words = fc.WORDS
    lens = [0, 1, 3, 7, 0, 0, 40, 300, T, 3 * T + 5, 2, 0]
    return [" ".join(rng.choice(words) for _ in range(n)) for n in lens] + ["", "\n\n", "x" * (T + 1), "héllo wörld 中文 😀 " * 9]


@pytest.mark.parametrize("spec", [fc.SPECS[0], fc.SPECS[2], fc.SPECS[5]], ids=[SPEC_IDS[0], SPEC_IDS[2], SPEC_IDS[5]])
def test_encode_entry_against_the_rule_on_the_encoders_tokens(spec):
    enc = enc_of()
    texts = text_batch(tile_of(enc))
    tok, off = enc.encode_ordinary_batch_packed(texts)
    assert int(np.diff(off).max()) > 3 * tile_of(enc) and int(np.diff(off).min()) == 0
    want = fr.fingerprint(tok, off, *spec)
    same(enc.fingerprint_ordinary_batch(texts, **kw(spec)), want, "ordinary")
    same(enc.fingerprint_batch(texts, **kw(spec)), want, "checked, nothing to find")
    same(enc.fingerprint_batch([], **kw(spec)), fr.fingerprint(tok[:0], off[:1], *spec), "no texts")


def test_refused_specs_raise_and_leave_the_next_call_correct():
    enc = enc_of()
    tok, off = fc.pack([3, 0, 40, 9], 5)
    dev = torch.device("cuda", enc._core_bpe.device)
    good = fc.SPECS[0]
    want = fr.fingerprint(tok, off, *good)
    for k, P, B in fc.REFUSED:
        with pytest.raises(ValueError):
            enc.fingerprint_tokens_packed(tok, off, ngram=k, n_perm=P, bands=B)
        with pytest.raises(ValueError):
            enc.fingerprint_ordinary_batch(["a b c", ""], ngram=k, n_perm=P, bands=B)
        exact = torch.full((4,), 0x55, dtype=torch.int64, device=dev)  # (no sig or band: their sizes follow P and B, and Python's size check would refuse first)
        with pytest.raises(ValueError):
            enc._core_bpe.fingerprint_device(torch.from_numpy(tok.view(np.int32).copy()).to(dev), torch.from_numpy(off.view(np.int64).copy()).to(dev), ngram=k, n_perm=P,
                                             bands=B, exact=exact)
        assert "ngram" in lib_error() or "n_perm" in lib_error() or "bands" in lib_error(), lib_error()  # (the library's refusal, not Python's)
        torch.cuda.synchronize(dev)
        assert (exact.cpu().numpy() == 0x55).all(), "a refused call has written"
        same(enc.fingerprint_tokens_packed(tok, off, **kw(good)), want, ("after", k, P, B))
    with pytest.raises(ValueError):
        enc.fingerprint_tokens_packed(tok, np.array([0, 5, 3, 52, 52], np.uint64))


def test_special_tokens_allowed_and_disallowed():
    enc = enc_of()
    texts = ["one two three four five six seven", "", "a tile <|endoftext|> a wave and a lane and a mask", "three four five"]
    spec = fc.SPECS[0]
    tok, off = enc.encode_batch_packed(texts, allowed_special={"<|endoftext|>"})
    assert enc.eot_token in tok.tolist()
    want = fr.fingerprint(tok, off, *spec)
    got = enc.fingerprint_batch(texts, allowed_special={"<|endoftext|>"}, **kw(spec))
    same(got, want, "allowed")
    plain = fr.fingerprint(*enc.encode_ordinary_batch_packed(texts), *spec)
    same(enc.fingerprint_batch(texts, disallowed_special=(), **kw(spec)), plain, "as plain text")
    assert plain.exact[2] != want.exact[2] and (plain.sig[2] != want.sig[2]).any() and (plain.sig[0] == want.sig[0]).all()
    with pytest.raises(DisallowedSpecialError) as e:
        enc.fingerprint_batch(texts, **kw(spec))
    assert e.value.doc == 2 and e.value.token == "<|endoftext|>"
    same(enc.fingerprint_batch(texts, allowed_special={"<|endoftext|>"}, **kw(spec)), want, "after the refusal")


def test_helpers_on_copies_and_noisy_copies():
    enc = enc_of()
    base = fc.helper_texts()
    packed = enc.encode_ordinary_batch_packed(base)
    ids = [packed[0][int(a):int(b)] for a, b in zip(packed[1][:-1], packed[1][1:])]
    by_text = dict(zip(base, ids))
    tok, off, pairs = fc.helper_batch(lambda t: by_text[t])
    k, P, B, seed = fc.HELPER_SPEC
    for bands in (B, P):
        want = fr.fingerprint(tok, off, k, P, bands, seed)
        got = enc.fingerprint_tokens_packed(tok, off, ngram=k, n_perm=P, bands=bands, seed=seed)
        same(got, want, bands)
        assert got.exact_groups().tolist() == fr.exact_groups(want)
        for th in (0.8, 0.3):
            assert got.duplicate_groups(th).tolist() == fr.duplicate_groups(want, th)
            assert got.keep_mask(th).tolist() == fr.keep_mask(want, th)
    assert not got.keep_mask(0.8).all() and got.keep_mask(0.8)[0]
    for i, j in pairs:
        J = fr.true_jaccard(tok, off, i, j, k)
        est = got.jaccard(i, j)
        assert abs(est - J) <= 4 * (J * (1 - J) / P) ** 0.5, (i, j, J, est)
