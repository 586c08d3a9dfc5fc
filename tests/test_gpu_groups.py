"""Near-duplicate groups and the selection of kept documents on the GPU (tk_groups.h): tk_fingerprint_groups through the host entry,
tk_fingerprint_groups_device and tk_select_docs_device on a side stream, and the dedup entries of Encoding -- against the host code that
was there before: Fingerprints.duplicate_groups / keep_mask, and numpy indexing; never against another run of the code under test."""
import numpy as np
import pytest
import torch

import tiktoken_amd as tiktoken
from tiktoken_amd import DisallowedSpecialError, Fingerprints
from tiktoken_amd._tiktoken import min_match

pytestmark = pytest.mark.gpu
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)


def enc_of():
    return tiktoken.get_encoding("gpt2_shaped")


def fp_of(sig, band, nsh):
    return Fingerprints(sig, band, np.zeros(len(nsh), np.uint64), nsh, np.zeros(len(nsh), np.uint64))


def to_dev(dev, a, as_type):
    return torch.from_numpy(a.view(as_type).copy()).to(dev, non_blocking=True)


def device_groups(enc, sig, band, nsh, th, skip=None):
    """tk_fingerprint_groups_device on a side stream: uploads, the poison the outputs are filled with, the call and the copies back are
    queued there, and only that stream is waited for.  Output `skip` (0 .. 2) is not asked for."""
    dev, n = torch.device("cuda", enc._core_bpe.device), len(nsh)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        ins = [to_dev(dev, sig, np.int32), to_dev(dev, band, np.int64), to_dev(dev, nsh, np.int64)]
        outs = [torch.full((n,), 0x55555555, dtype=torch.int32, device=dev), torch.full((n,), 0x55, dtype=torch.uint8, device=dev), torch.full((1,), 0x55, dtype=torch.int64, device=dev)]
        given = [None if i == skip else o for i, o in enumerate(outs)]
        enc._core_bpe.fingerprint_groups_device(*ins, th, group=given[0], keep=given[1], n_kept=given[2])
        pinned = [torch.empty(o.shape, dtype=o.dtype, pin_memory=True) for o in outs]
        for h, o in zip(pinned, outs):
            h.copy_(o, non_blocking=True)
    stream.synchronize()
    return pinned[0].numpy().view(np.uint32), pinned[1].numpy(), int(pinned[2].numpy()[0])


def check_groups(enc, sig, band, nsh, th, what, nulls=False):
    want = fp_of(sig, band, nsh).duplicate_groups(th)
    keep = want == np.arange(len(want))
    g, k = enc._core_bpe.fingerprint_groups_packed(fp_of(sig, band, nsh), th)
    assert g.dtype == np.int64 and k.dtype == bool and np.array_equal(g, want) and np.array_equal(k, keep), (what, "host entry", np.flatnonzero(g != want)[:8])
    for skip in (None, 0, 1, 2) if nulls else (None,):
        got = device_groups(enc, sig, band, nsh, th, skip)
        for i, (a, b, poison) in enumerate(zip(got, (want, keep, int(keep.sum())), (0x55555555, 0x55, 0x55))):
            assert (np.asarray(a) == poison).all() if i == skip else np.array_equal(a, b), (what, "device entry", i, skip)
    return want


def random_batch(n, P, B, th, seed):
    """Keys from about n / 20 values that include 0 and 2^64 - 1; one document in twenty not live; every signature a copy of one of four
    base rows whose first P - t positions are overwritten, t in {min_match - 1, min_match, min_match + 1}: two documents of one base agree
    in min(t, t') positions, right at the threshold."""
    rng = np.random.default_rng(seed)
    keys = np.concatenate([np.array([0, U64_MAX], np.uint64), rng.integers(1, 1 << 63, max(n // 20, 1), dtype=np.uint64)])
    band = keys[rng.integers(0, len(keys), (n, B))]
    nsh = np.where(rng.random(n) < 0.05, 0, rng.integers(1, 1000, n)).astype(np.uint64)
    base = rng.integers(0, 1 << 32, (4, P), dtype=np.uint32)
    sig = base[rng.integers(0, 4, n)]
    t = np.clip(min_match(th, P) + rng.integers(-1, 2, n), 0, P)
    over = np.arange(P)[None, :] < (P - t)[:, None]
    sig[over] = rng.integers(0, 1 << 32, int(over.sum()), dtype=np.uint32)
    return np.ascontiguousarray(sig), np.ascontiguousarray(band), nsh


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 20000])
@pytest.mark.parametrize("P,B", [(128, 16), (6, 3), (1, 1), (256, 1)])
def test_groups_on_random_batches(P, B, n):
    enc = enc_of()
    for th in (0.0, 0.8, 1.0, 1.5):
        want = check_groups(enc, *random_batch(n, P, B, th, n * 1000 + P + B), th, (P, B, n, th), nulls=n == 65)
        if n == 20000 and th in (0.8, 1.0) and P > 1:
            assert 1 < len(np.unique(want)) < n, "the batch joins nothing or everything: it tests little"


@pytest.mark.parametrize("P,B", [(128, 16), (6, 3), (256, 1)])
def test_groups_chain_is_one_group(P, B):
    """Document i and i + 1 share a key in band i mod B only, all signatures are equal: one group, through 4999 edges in a row."""
    n = 5000
    band = (np.arange(n * B, dtype=np.uint64) + np.uint64(1)).reshape(n, B)
    for i in range(n - 1):
        band[i + 1, i % B] = band[i, i % B]
    sig = np.tile(np.arange(P, dtype=np.uint32), (n, 1))
    want = check_groups(enc_of(), sig, band, np.ones(n, np.uint64), 1.0, ("chain", P, B))
    assert not want.any()


@pytest.mark.parametrize("live", [True, False])
def test_groups_of_identical_documents(live):
    """5000 documents with one signature and one set of keys: every claim meets the same B slots.  Live: one group, one kept; not live:
    every document its own."""
    n, P, B = 5000, 128, 16
    sig, band = np.full((n, P), 7, np.uint32), np.tile(np.arange(B, dtype=np.uint64) * U64_MAX, (n, 1))
    nsh = np.full(n, 3 if live else 0, np.uint64)
    want = check_groups(enc_of(), sig, band, nsh, 0.8, ("identical", live))
    assert np.array_equal(want, np.zeros(n, np.int64) if live else np.arange(n))
    assert device_groups(enc_of(), sig, band, nsh, 0.8)[2] == (1 if live else n)


def test_groups_refusals_write_nothing():
    enc, n = enc_of(), 8
    sig, band, nsh = np.zeros((n, 6), np.uint32), np.zeros((n, 4), np.uint64), np.ones(n, np.uint64)
    with pytest.raises(ValueError, match="bands"):  # P % B != 0: the library's refusal
        device_groups(enc, sig, band, nsh, 0.8)
    with pytest.raises(ValueError, match="bands"):
        enc._core_bpe.fingerprint_groups_packed(fp_of(sig, band, nsh), 0.8)
    dev = torch.device("cuda", enc._core_bpe.device)
    group = torch.full((n,), 0x55555555, dtype=torch.int32, device=dev)
    for bad in ((sig, band[:, :3], nsh[:-1]), (sig, band[:-1, :3], nsh), (sig, band, nsh)):
        with pytest.raises(ValueError):
            enc._core_bpe.fingerprint_groups_device(to_dev(dev, np.ascontiguousarray(bad[0]), np.int32), to_dev(dev, np.ascontiguousarray(bad[1]), np.int64),
                                                    to_dev(dev, bad[2], np.int64), 0.8, group=group)
    torch.cuda.synchronize(dev)
    assert (group.cpu().numpy() == 0x55555555).all(), "a refused call has written"


def select_lens(name, T):
    return {"shapes": [0, 1, T - 1, T, T + 1, 3 * T + 5, 0, 0, 7, 0], "no documents": [], "no tokens": [0, 0, 0], "many": [3] * 700 + [0] * 300 + [T + 3]}[name]


@pytest.mark.parametrize("pattern", ["none", "all", "alternating", "first and last"])
@pytest.mark.parametrize("shape", ["shapes", "no documents", "no tokens", "many"])
def test_select_against_numpy(shape, pattern):
    enc = enc_of()
    lens = np.array(select_lens(shape, int(enc._core_bpe.stat("select_tile"))), np.uint64)
    n, rng = len(lens), np.random.default_rng(5)
    off = np.concatenate([np.zeros(1, np.uint64), np.cumsum(lens, dtype=np.uint64)])
    T = int(off[-1])
    tok = rng.integers(0, 1 << 32, T, dtype=np.uint32)
    keep = {"none": np.zeros(n, np.uint8), "all": np.full(n, 0xFF, np.uint8), "alternating": (np.arange(n) % 2 == 1).astype(np.uint8) * 2,
            "first and last": np.isin(np.arange(n), (0, n - 1)).astype(np.uint8)}[pattern]
    kept = np.flatnonzero(keep)
    want_tok = np.concatenate([tok[int(off[d]):int(off[d + 1])] for d in kept] + [tok[:0]])
    want_off = np.concatenate([np.zeros(1, np.uint64), np.cumsum(lens[kept], dtype=np.uint64)])
    dev = torch.device("cuda", enc._core_bpe.device)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        ins = [to_dev(dev, tok, np.int32), to_dev(dev, off, np.int64), to_dev(dev, keep, np.uint8)]
        outs = [torch.full((T,), 0x55555555, dtype=torch.int32, device=dev), torch.full((n + 1,), 0x55, dtype=torch.int64, device=dev),
                torch.full((n,), 0x55555555, dtype=torch.int32, device=dev), torch.full((2,), 0x55, dtype=torch.int64, device=dev)]
        enc._core_bpe.select_docs_device(*ins, tokens_out=outs[0], tok_off_out=outs[1], doc_out=outs[2], counts_out=outs[3])
        pinned = [torch.empty(o.shape, dtype=o.dtype, pin_memory=True) for o in outs]
        for h, o in zip(pinned, outs):
            h.copy_(o, non_blocking=True)
    stream.synchronize()
    g_tok, g_off, g_doc, g_cnt = (h.numpy() for h in pinned)
    assert g_cnt.tolist() == [len(kept), len(want_tok)]
    assert np.array_equal(g_tok.view(np.uint32)[:len(want_tok)], want_tok) and (g_tok[len(want_tok):] == 0x55555555).all()
    assert np.array_equal(g_off.view(np.uint64)[:len(kept) + 1], want_off) and (g_off[len(kept) + 1:] == 0x55).all()
    assert np.array_equal(g_doc[:len(kept)], kept) and (g_doc[len(kept):] == 0x55555555).all()
    if T:
        with pytest.raises(ValueError, match="in place"):
            enc._core_bpe.select_docs_device(*ins, tokens_out=ins[0], tok_off_out=outs[1], doc_out=outs[2], counts_out=outs[3])


def dedup_texts():
    rng = np.random.default_rng(11)
    words = "a tile of lanes walks the wave and a mask keeps what the scan has left behind in shared memory".split()
    long = [" ".join(rng.choice(words, 60 + 7 * i)) for i in range(40)]
    near = [t.replace(" ", " one ", 1) for t in long[:20]] + [t + " tail" for t in long[20:30]]
    return long + ["", "x"] + long[::3] + near + ["", "x", "y z"] + [long[5]] * 30 + [" ".join(rng.choice(words, 9)) for _ in range(120)]


@pytest.mark.parametrize("th", [0.8, 0.5])
def test_dedup_entries_end_to_end(th):
    enc, texts = enc_of(), dedup_texts()
    tok, off = enc.encode_batch_packed(texts)
    fp = enc.fingerprint_batch(texts)
    keep = fp.keep_mask(th)
    assert 1 < keep.sum() <= len(texts) - 45  # (14 + 30 exact copies of long texts and the second "x" go at any threshold)
    kept = np.flatnonzero(keep)
    want_tok = np.concatenate([tok[int(off[d]):int(off[d + 1])] for d in kept])
    for got in (enc.dedup_ordinary_batch(texts, threshold=th), enc.dedup_batch(texts, threshold=th), enc.dedup_tokens_packed(tok, off, th)):
        assert np.array_equal(got.group, fp.duplicate_groups(th)) and np.array_equal(got.doc, kept)
        assert np.array_equal(got.tokens, want_tok) and np.array_equal(np.diff(got.tok_off), np.diff(off)[kept]) and got.tok_off[0] == 0
    empty = enc.dedup_ordinary_batch([])
    assert len(empty.tokens) == len(empty.doc) == len(empty.group) == 0 and empty.tok_off.tolist() == [0]
    with pytest.raises(DisallowedSpecialError) as e:
        enc.dedup_batch(texts[:3] + ["a <|endoftext|> b"] + texts[3:], threshold=th)
    assert e.value.doc == 3 and e.value.token == "<|endoftext|>"
