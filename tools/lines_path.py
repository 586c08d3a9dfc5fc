#!/usr/bin/env python3
"""What the line statistics cost on one GPU, beside the encode step of the same text and beside the host route, re.split and a Counter per
document on the copied-out text.

    python tools/lines_path.py [MiB] [label]    (default: 256 MiB of the bench corpus, o200k-shaped)

tk_line_stats_device runs on the corpus and on a batch that is one document without a newline, the first 64 MiB of the text with every
newline replaced: wall clock around the call and a synchronise (the call itself waits once, for the table's size), and its kernels apart,
from HIP events.  The host route runs on the leading documents that hold about 1/64 of the bytes, timed once and SCALED to the batch; the
device result on those documents is compared with it before anything is timed.  Every device figure is the median of 10 calls after 2
warm-up calls.  `label` names the build in every line.  (Per kernel from the profiler: run this file under rocprofv3 --kernel-trace
--stats, in a run of its own.)"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (first: its HIP runtime has to be the one that is loaded)

import lines_ref as lr  # noqa: E402
from bench import gen_corpus  # noqa: E402
from tiktoken_amd import Encoding  # noqa: E402
from tiktoken_ext import amd_shaped  # noqa: E402

mib = int(sys.argv[1]) if len(sys.argv) > 1 else 256
label = sys.argv[2] if len(sys.argv) > 2 else "shipped"
WARMUP, REPS, ONE_DOC_MIB = 2, 10, 64
KERNELS = ("tk_k_ln_clear", "tk_k_ln_sum", "tk_k_ln_carry", "tk_k_ln_count", "tk_k_ln_final")

spec = amd_shaped.ENCODING_CONSTRUCTORS["o200k_shaped"]()
enc = Encoding("o200k_shaped_lines_path", pat_str=spec["pat_str"], mergeable_ranks=spec["mergeable_ranks"], special_tokens=spec["special_tokens"])
core = enc._core_bpe
dev = torch.device("cuda", core.device)
tag = f"lines_path {mib} MiB [{label}]"


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


def kernels(call):
    """the median of every kernel's time per call over REPS profiled calls, in ms"""
    core.set_profiling(True)
    per = {k: [] for k in KERNELS}
    for i in range(WARMUP + REPS):
        core.reset_kernel_ms()
        call()
        if i >= WARMUP:
            for k in KERNELS:
                per[k].append(core.kernel_ms(k)[0])
    core.set_profiling(False)
    return ", ".join(f"{k} {statistics.median(v):.3f}" for k, v in per.items())


def measure(name, d_text, d_off, n_docs, n_bytes):
    outs = {m: torch.empty(n_docs, dtype=torch.int64, device=dev) for m in lr.Ref._fields}
    call = lambda: core.line_stats_device(d_text, d_off, **outs)  # noqa: E731
    t = med(call)
    print(f"{tag}: {name}: tk_line_stats_device (wall clock, call and synchronise): {ms(t)} = {n_bytes / t[0] / 1e9:.1f} GB/s; kernels, ms: {kernels(call)}", flush=True)
    return outs


blob, off = gen_corpus(0x5EED0003, 1, mib << 20, 16)  # (the bench's corpus)
blob, off = np.ascontiguousarray(blob[:int(off[-1])]), np.ascontiguousarray(off, dtype=np.uint64)
n_docs, N = len(off) - 1, len(blob)
d_text, d_off = to_dev(blob), to_dev(off)
torch.cuda.synchronize()
t_enc = med(lambda: core.encode_batch_device(d_text.data_ptr(), N, d_off.data_ptr(), off, n_docs))
print(f"{tag}: {n_docs} documents, {N} bytes; tile {core.stat('lines_tile')} bytes, {core.stat('lines_docs')} documents of a tile gathered in LDS", flush=True)
print(f"{tag}: encode step (tk_encode_batch_device, wall clock): {ms(t_enc)}", flush=True)

sub = int(np.searchsorted(off, N // 64, side="right"))  # the leading documents with about 1/64 of the bytes
data = blob.tobytes()
t0 = time.perf_counter()
want = lr.stats([data[int(a):int(b)] for a, b in zip(off[:sub], off[1:sub + 1])])
t_host = time.perf_counter() - t0
outs = measure("corpus", d_text, d_off, n_docs, N)
for m, w in zip(lr.Ref._fields, want):
    assert np.array_equal(outs[m].cpu().numpy().view(np.uint64)[:sub], w), m
got = lr.Ref(*[outs[m].cpu().numpy().view(np.uint64) for m in lr.Ref._fields])
print(f"{tag}: corpus: the first {sub} documents equal the host route's; {int(got.n_lines.sum())} lines, {int(got.n_dup_lines.sum())} of them duplicates, "
      f"{int(got.n_paragraphs.sum())} paragraphs", flush=True)
share = int(off[sub]) / N
print(f"{tag}: corpus: host route (re.split, Counter and a char count per document) on {share:.4f} of the bytes: {t_host:.1f} s, SCALED to the batch "
      f"{t_host / share:.0f} s", flush=True)

one = blob[:min(ONE_DOC_MIB << 20, N)].copy()
one[one == 10] = 32
one_off = np.array([0, len(one)], np.uint64)
o1 = measure(f"one document of {len(one) >> 20} MiB without a newline", to_dev(one), to_dev(one_off), 1, len(one))
assert int(o1["n_lines"].item()) == 1 and int(o1["n_chars"].item()) == lr.chars(one.tobytes()[:1 << 20]) + int(((one[1 << 20:] & 0xC0) != 0x80).sum())
