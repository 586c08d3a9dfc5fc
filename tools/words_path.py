#!/usr/bin/env python3
"""What the word statistics cost on one GPU, beside the line statistics and the encode step of the same text and beside the host route,
str.split, str.isalpha and bytes.count per document on the copied-out text.

    python tools/words_path.py [MiB] [label]    (default: 256 MiB of the bench corpus, o200k-shaped)

tk_word_stats_device runs on the corpus and on a batch that is one document without white space, the first 64 MiB of the text with every
ASCII white-space byte replaced: wall clock around the call and a synchronise (the call itself waits for nothing), and its kernels apart,
from HIP events; tk_line_stats_device on the same buffers in the same session.  The host route runs on the leading documents that hold
about 1/64 of the bytes, timed once and SCALED to the batch; the device result on those documents is compared with it before anything is
timed.  Every device figure is the median of 10 calls after 2 warm-up calls.  `label` names the build in every line: $TIKTOKEN_AMD_LIB
selects another one, such as the form without the ASCII path (tools/build_variant.sh no_ascii_path -DTK_WD_ASCII_PATH=0)."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (first: its HIP runtime has to be the one that is loaded)

import words_ref as wr  # noqa: E402
from bench import gen_corpus  # noqa: E402
from tiktoken_amd import Encoding  # noqa: E402
from tiktoken_ext import amd_shaped  # noqa: E402

mib = int(sys.argv[1]) if len(sys.argv) > 1 else 256
label = sys.argv[2] if len(sys.argv) > 2 else "shipped"
WARMUP, REPS, ONE_DOC_MIB = 2, 10, 64
WD_KERNELS = ("tk_k_wd_clear", "tk_k_wd_sum", "tk_k_wd_carry", "tk_k_wd_count", "tk_k_wd_final")
LN_KERNELS = ("tk_k_ln_clear", "tk_k_ln_sum", "tk_k_ln_carry", "tk_k_ln_count", "tk_k_ln_final")

spec = amd_shaped.ENCODING_CONSTRUCTORS["o200k_shaped"]()
enc = Encoding("o200k_shaped_words_path", pat_str=spec["pat_str"], mergeable_ranks=spec["mergeable_ranks"], special_tokens=spec["special_tokens"])
core = enc._core_bpe
dev = torch.device("cuda", core.device)
tag = f"words_path {mib} MiB [{label}]"


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
    return torch.from_numpy(a.view({1: np.uint8, 8: np.int64}[a.itemsize]).copy()).to(dev)


def kernels(call, names):
    """the median of every kernel's time per call over REPS profiled calls, in ms"""
    core.set_profiling(True)
    per = {k: [] for k in names}
    for i in range(WARMUP + REPS):
        core.reset_kernel_ms()
        call()
        if i >= WARMUP:
            for k in names:
                per[k].append(core.kernel_ms(k)[0])
    core.set_profiling(False)
    return ", ".join(f"{k} {statistics.median(v):.3f}" for k, v in per.items())


def measure(name, d_text, d_off, n_docs, n_bytes):
    outs = {m: torch.empty(n_docs, dtype=torch.int64, device=dev) for m in wr.Ref._fields}
    call = lambda: core.word_stats_device(d_text, d_off, **outs)  # noqa: E731
    t = med(call)
    print(f"{tag}: {name}: tk_word_stats_device (wall clock, call and synchronise): {ms(t)} = {n_bytes / t[0] / 1e9:.1f} GB/s; kernels, ms: {kernels(call, WD_KERNELS)}", flush=True)
    lines = {m: torch.empty(n_docs, dtype=torch.int64, device=dev) for m in core.LINE_OUTS}
    call = lambda: core.line_stats_device(d_text, d_off, **lines)  # noqa: E731
    t = med(call)
    print(f"{tag}: {name}: tk_line_stats_device, same buffers (wall clock, call with its one wait and synchronise): {ms(t)}; kernels, ms: {kernels(call, LN_KERNELS)}", flush=True)
    return outs


blob, off = gen_corpus(0x5EED0003, 1, mib << 20, 16)  # (the bench's corpus)
blob, off = np.ascontiguousarray(blob[:int(off[-1])]), np.ascontiguousarray(off, dtype=np.uint64)
n_docs, N = len(off) - 1, len(blob)
d_text, d_off = to_dev(blob), to_dev(off)
torch.cuda.synchronize()
t_enc = med(lambda: core.encode_batch_device(d_text.data_ptr(), N, d_off.data_ptr(), off, n_docs))
print(f"{tag}: {n_docs} documents, {N} bytes, {int((blob >= 0x80).sum())} of them >= 0x80; tile {core.stat('words_tile')} bytes, {core.stat('words_docs')} documents of a tile "
      f"gathered in LDS", flush=True)
print(f"{tag}: encode step (tk_encode_batch_device, wall clock): {ms(t_enc)}", flush=True)

sub = int(np.searchsorted(off, N // 64, side="right"))  # the leading documents with about 1/64 of the bytes
data = blob.tobytes()
t0 = time.perf_counter()
want = wr.stats([data[int(a):int(b)] for a, b in zip(off[:sub], off[1:sub + 1])])
t_host = time.perf_counter() - t0
outs = measure("corpus", d_text, d_off, n_docs, N)
for m, w in zip(wr.Ref._fields, want):
    assert np.array_equal(outs[m].cpu().numpy().view(np.uint64)[:sub], w), m
got = wr.Ref(*[outs[m].cpu().numpy().view(np.uint64) for m in wr.Ref._fields])
print(f"{tag}: corpus: the first {sub} documents equal the host route's; {int(got.n_words.sum())} words, {int(got.n_alpha_words.sum())} of them with a letter, "
      f"{int(got.n_lines.sum())} lines, {int(got.n_punct_lines.sum())} of them punctuated", flush=True)
share = int(off[sub]) / N
print(f"{tag}: corpus: host route (split, isalpha, count and split on newlines per document) on {share:.4f} of the bytes: {t_host:.1f} s, SCALED to the batch "
      f"{t_host / share:.0f} s", flush=True)

one = blob[:min(ONE_DOC_MIB << 20, N)].copy()
one[((one >= 9) & (one <= 13)) | ((one >= 28) & (one <= 32))] = ord("_")
one_off = np.array([0, len(one)], np.uint64)
o1 = measure(f"one document of {len(one) >> 20} MiB without ASCII white space", to_dev(one), to_dev(one_off), 1, len(one))
print(f"{tag}: one document: {int(o1['n_words'].item())} words (white space of several bytes remains), {int(o1['word_chars'].item())} chars in them", flush=True)
