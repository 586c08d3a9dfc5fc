#!/usr/bin/env python3
"""What the check against a token n-gram set costs on one GPU, beside the encode step it follows, beside the fingerprint pass -- which
stages and hashes the same ids -- and beside the host route, a Python set of id tuples on the copied-out ids.

    python tools/ngram_path.py [MiB] [label]    (default: 256 MiB of the bench corpus, o200k-shaped; k = 13)

The set holds the 13-grams of a held-out slice: 8 MiB of the same generator under another seed.  Two batches are asked: the corpus as
it is, and the corpus with a passage of 200 held-out tokens copied into every fifth document that is long enough.  Reported: the
encode step (tk_encode_batch_device, wall clock); the add of the held-out slice; tk_ngram_overlap_device on either batch, with and
without the token mask (wall clock around the call and a synchronise of its stream) and its kernels from HIP events;
tk_fingerprint_device on the same ids at the same k, hash step alone (exact hash and shingle count) and whole (P = 128); the host
route on the leading documents that hold about 1/64 of the ids, timed once and SCALED to the batch.  The device result on those
documents is compared with the host route's before anything is timed.  Every device figure is the median of 10 calls after 2 warm-up
calls.  `label` names the build in every line (the filter was measured on and off with two builds of the library)."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (first: its HIP runtime has to be the one that is loaded)

import ngram_ref as nr  # noqa: E402
from bench import gen_corpus  # noqa: E402
from tiktoken_amd import Encoding  # noqa: E402
from tiktoken_ext import amd_shaped  # noqa: E402

mib = int(sys.argv[1]) if len(sys.argv) > 1 else 256
label = sys.argv[2] if len(sys.argv) > 2 else "shipped"
WARMUP, REPS, K, HELD_MIB, PASSAGE = 2, 10, 13, 8, 200
KERNELS = ("tk_k_ng_fill", "tk_k_ng_overlap")

spec = amd_shaped.ENCODING_CONSTRUCTORS["o200k_shaped"]()
enc = Encoding("o200k_shaped_ngram_path", pat_str=spec["pat_str"], mergeable_ranks=spec["mergeable_ranks"], special_tokens=spec["special_tokens"])
core = enc._core_bpe
dev = torch.device("cuda", core.device)
tag = f"ngram_path {mib} MiB [{label}]"


def med(f, reps=REPS):
    for _ in range(WARMUP):
        f()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def ms(t):
    return f"median {t[0] * 1e3:.3f} ms (min {t[1] * 1e3:.3f}, max {t[2] * 1e3:.3f})"


def corpus(seed, n_bytes):
    blob, off = gen_corpus(seed, 1, n_bytes, 16)
    return np.ascontiguousarray(blob[:int(off[-1])]), np.ascontiguousarray(off, dtype=np.uint64)


def to_dev(a):
    return torch.from_numpy(a.view({1: np.uint8, 4: np.int32, 8: np.int64}[a.itemsize]).copy()).to(dev)


blob, off = corpus(0x5EED0003, mib << 20)  # (the bench's corpus)
n_docs = len(off) - 1
d_text, d_doc_off = to_dev(blob), to_dev(off)
torch.cuda.synchronize()
t_enc = med(lambda: core.encode_batch_device(d_text.data_ptr(), len(blob), d_doc_off.data_ptr(), off, n_docs))
tok, tok_off = core.encode_batch_packed(blob, off, None)
held_tok, held_off = core.encode_batch_packed(*corpus(0x5EED0004, HELD_MIB << 20), None)
T = len(tok)
print(f"{tag}: {n_docs} documents, {T} ids; k = {K}; tile {core.stat('ngram_tile')} positions; held-out slice: {len(held_off) - 1} documents, {len(held_tok)} ids", flush=True)
print(f"{tag}: encode step (tk_encode_batch_device, wall clock): {ms(t_enc)}", flush=True)

copied = np.array(tok)  # every fifth document that has room gets a held-out passage
rng = np.random.default_rng(5)
n_copied = 0
for d in range(0, n_docs, 5):
    s, e = int(tok_off[d]), int(tok_off[d + 1])
    if e - s >= 2 * PASSAGE:
        at, src = s + int(rng.integers(0, e - s - PASSAGE)), int(rng.integers(0, len(held_tok) - PASSAGE))
        copied[at:at + PASSAGE] = held_tok[src:src + PASSAGE]
        n_copied += 1

ngs = enc.ngram_set(K, capacity=len(held_tok))
set_bytes = (1 << (2 * len(held_tok) - 1).bit_length()) * 17 // 2  # 8 S bytes of table, S / 2 of filter
d_held = to_dev(held_tok), to_dev(held_off)
d_off = to_dev(tok_off)


def add():
    ngs.clear()
    core.ngram_add_device(ngs._native, *d_held)


t_add = med(add)
print(f"{tag}: clear and tk_ngram_add_device of the held-out slice: {ms(t_add)}; {len(ngs)} distinct {K}-grams in {set_bytes >> 20} MiB of table and filter",
      flush=True)
outs = [torch.empty(n_docs, dtype=torch.int64, device=dev) for _ in range(4)]
d_mask = torch.empty(T, dtype=torch.uint8, device=dev)
sub = int(np.searchsorted(tok_off, T // 64, side="right"))  # the leading documents with about 1/64 of the ids
held = nr.add(set(), held_tok, held_off, K)
for name, ids in (("corpus as it is", tok), (f"a passage of {PASSAGE} held-out ids in {n_copied} documents", copied)):
    d_tok = to_dev(ids)

    def overlap(mask=None):
        core.ngram_overlap_device(ngs._native, d_tok, d_off, n_hit=outs[0], n_covered=outs[1], n_ngrams=outs[2], first_hit=outs[3], mask=mask)

    overlap(d_mask)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want = nr.overlap(held, ids[:int(tok_off[sub])], tok_off[:sub + 1], K)
    t_host = time.perf_counter() - t0
    got = [o.cpu().numpy().view(np.uint64) for o in outs]
    for g, w in zip(got, want[:4]):
        assert np.array_equal(g[:sub], w)
    assert np.array_equal(d_mask.cpu().numpy()[:int(tok_off[sub])], want.mask)
    share = int(tok_off[sub]) / T
    print(f"{tag}: {name}: {int((got[0] > 0).sum())} documents with a hit, {int(got[0].sum())} of {int(got[2].sum())} n-grams hit, {int(got[1].sum())} ids covered; "
          f"the first {sub} documents equal the host route's", flush=True)
    t_ov, t_ovm = med(overlap), med(lambda: overlap(d_mask))
    print(f"{tag}: {name}: tk_ngram_overlap_device (wall clock, call and synchronise): {ms(t_ov)} = {T / t_ov[0] / 1e9:.2f} G ids/s; with the mask: {ms(t_ovm)}", flush=True)
    core.set_profiling(True)
    per = {k: [] for k in KERNELS}
    for i in range(WARMUP + REPS):
        core.reset_kernel_ms()
        overlap()
        if i >= WARMUP:
            for k in KERNELS:
                per[k].append(core.kernel_ms(k)[0])
    core.set_profiling(False)
    print(f"{tag}: {name}: " + ", ".join(f"{k} median {statistics.median(v):.4f} ms" for k, v in per.items()), flush=True)
    print(f"{tag}: {name}: host route (a Python set of tuples) on {share:.4f} of the ids: {t_host:.2f} s, SCALED to the batch {t_host / share:.1f} s = "
          f"{t_host / share / t_ov[0]:.0f}x the device pass; overlap / encode step = {t_ov[0] / t_enc[0]:.3f}", flush=True)

d_tok = to_dev(tok)
exact, nsh = outs[0], outs[1]
sig, band = torch.empty(n_docs * 128, dtype=torch.int32, device=dev), torch.empty(n_docs * 16, dtype=torch.int64, device=dev)
t_fh = med(lambda: core.fingerprint_device(d_tok, d_off, ngram=K, n_perm=128, bands=16, exact=exact, n_shingles=nsh))
t_fp = med(lambda: core.fingerprint_device(d_tok, d_off, ngram=K, n_perm=128, bands=16, sig=sig, band=band, exact=exact, n_shingles=nsh))
print(f"{tag}: tk_fingerprint_device on the same ids, k = {K}: hash step alone (exact, n_shingles) {ms(t_fh)}; whole (P = 128, B = 16) {ms(t_fp)}", flush=True)
