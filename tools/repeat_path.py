#!/usr/bin/env python3
"""What the repetition statistics cost on one GPU, beside the encode step they follow, beside tk_ngram_overlap_device at k = 13 -- which
stages and hashes the same ids -- and beside the host route, a Counter of id tuples per document and size on the copied-out ids.

    python tools/repeat_path.py [MiB] [label]    (default: 256 MiB of the bench corpus, o200k-shaped)

tk_repetition_device runs for the nine default sizes (as 8 + 1 calls), for (13,) alone and for (2, 3, 4): wall clock around the calls and
a synchronise, and the LDS class (tk_k_rp_fill, tk_k_rp_lds) and the long class (tk_k_rp_long_*) apart, from HIP events.  Then a batch
in which every document is long: the first 64 MiB of the text as one document.  The host route runs on the leading documents that hold
about 1/64 of the ids, timed once and SCALED to the batch; the device result on those documents is compared with it before anything is
timed.  Every device figure is the median of 10 calls after 2 warm-up calls.  `label` names the build in every line."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (first: its HIP runtime has to be the one that is loaded)

import repeat_ref as rr  # noqa: E402
from bench import gen_corpus  # noqa: E402
from tiktoken_amd import Encoding  # noqa: E402
from tiktoken_ext import amd_shaped  # noqa: E402

mib = int(sys.argv[1]) if len(sys.argv) > 1 else 256
label = sys.argv[2] if len(sys.argv) > 2 else "shipped"
WARMUP, REPS, ONE_DOC_MIB = 2, 10, 64
DEFAULT = (2, 3, 4, 5, 6, 7, 8, 9, 10)
LDS, LONG = ("tk_k_rp_fill", "tk_k_rp_lds"), ("tk_k_rp_long_clear", "tk_k_rp_long_insert", "tk_k_rp_long_count")

spec = amd_shaped.ENCODING_CONSTRUCTORS["o200k_shaped"]()
enc = Encoding("o200k_shaped_repeat_path", pat_str=spec["pat_str"], mergeable_ranks=spec["mergeable_ranks"], special_tokens=spec["special_tokens"])
core = enc._core_bpe
dev = torch.device("cuda", core.device)
tag = f"repeat_path {mib} MiB [{label}]"


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


def to_dev(a):
    return torch.from_numpy(a.view({1: np.uint8, 4: np.int32, 8: np.int64}[a.itemsize]).copy()).to(dev)


def classes(call):
    """the medians of the two classes' kernels over REPS profiled calls, in ms"""
    core.set_profiling(True)
    per = {"LDS class": [], "long class": []}
    for i in range(WARMUP + REPS):
        core.reset_kernel_ms()
        call()
        if i >= WARMUP:
            per["LDS class"].append(sum(core.kernel_ms(k)[0] for k in LDS))
            per["long class"].append(sum(core.kernel_ms(k)[0] for k in LONG))
    core.set_profiling(False)
    return ", ".join(f"{k} median {statistics.median(v):.3f} ms" for k, v in per.items())


def measure(name, d_tok, d_off, n_docs, T):
    for sizes in (DEFAULT, (13,), (2, 3, 4)):
        parts = [sizes[i:i + 8] for i in range(0, len(sizes), 8)]
        outs = [[torch.empty(n_docs * len(p), dtype=torch.int64, device=dev) for _ in range(5)] for p in parts]

        def call():
            for p, o in zip(parts, outs):
                core.repetition_device(d_tok, d_off, p, n_ngrams=o[0], n_distinct=o[1], n_dup=o[2], n_dup_covered=o[3], top_count=o[4])

        t = med(call)
        print(f"{tag}: {name}: sizes {sizes}: tk_repetition_device (wall clock, call and synchronise): {ms(t)} = {T / t[0] / 1e9:.2f} G ids/s; {classes(call)}", flush=True)
    return t


blob, off = gen_corpus(0x5EED0003, 1, mib << 20, 16)  # (the bench's corpus)
blob, off = np.ascontiguousarray(blob[:int(off[-1])]), np.ascontiguousarray(off, dtype=np.uint64)
n_docs = len(off) - 1
d_text, d_doc_off = to_dev(blob), to_dev(off)
torch.cuda.synchronize()
t_enc = med(lambda: core.encode_batch_device(d_text.data_ptr(), len(blob), d_doc_off.data_ptr(), off, n_docs))
tok, tok_off = core.encode_batch_packed(blob, off, None)
T, C = len(tok), core.stat("repeat_lds_tokens")
lengths = np.diff(tok_off)
print(f"{tag}: {n_docs} documents, {T} ids; tile {core.stat('repeat_tile')} positions, LDS class up to {C} tokens; {int((lengths > C).sum())} long documents "
      f"with {int(lengths[lengths > C].sum())} ids", flush=True)
print(f"{tag}: encode step (tk_encode_batch_device, wall clock): {ms(t_enc)}", flush=True)

d_tok, d_off = to_dev(tok), to_dev(tok_off)
sub = int(np.searchsorted(tok_off, T // 64, side="right"))  # the leading documents with about 1/64 of the ids
t0 = time.perf_counter()
want = rr.stats(tok[:int(tok_off[sub])], tok_off[:sub + 1], DEFAULT[:8])
t_host = (time.perf_counter() - t0) * 9 / 8
outs = [torch.empty(n_docs * 8, dtype=torch.int64, device=dev) for _ in range(5)]
core.repetition_device(d_tok, d_off, DEFAULT[:8], n_ngrams=outs[0], n_distinct=outs[1], n_dup=outs[2], n_dup_covered=outs[3], top_count=outs[4])
for o, w in zip(outs, want):
    assert np.array_equal(o.cpu().numpy().view(np.uint64).reshape(n_docs, 8)[:sub], w)
print(f"{tag}: corpus: the first {sub} documents equal the host route's", flush=True)
t_dev = measure("corpus", d_tok, d_off, n_docs, T)
share = int(tok_off[sub]) / T
print(f"{tag}: corpus: host route (a Counter of tuples per document and size, nine sizes) on {share:.4f} of the ids: {t_host:.1f} s, SCALED to the batch "
      f"{t_host / share:.0f} s", flush=True)

ngs = enc.ngram_set(13, capacity=1 << 20)
ngs.add_tokens_packed(tok[:1 << 19], np.array([0, 1 << 19], np.uint64))
o4 = [torch.empty(n_docs, dtype=torch.int64, device=dev) for _ in range(4)]
t_ng = med(lambda: core.ngram_overlap_device(ngs._native, d_tok, d_off, n_hit=o4[0], n_covered=o4[1], n_ngrams=o4[2], first_hit=o4[3]))
print(f"{tag}: tk_ngram_overlap_device on the same ids, k = 13: {ms(t_ng)}", flush=True)

one_off = np.array([0, min(ONE_DOC_MIB << 20, len(blob))], np.uint64)
one_tok, one_tok_off = core.encode_batch_packed(blob[:int(one_off[1])], one_off, None)
measure(f"one document of {ONE_DOC_MIB} MiB", to_dev(one_tok), to_dev(one_tok_off), 1, len(one_tok))
