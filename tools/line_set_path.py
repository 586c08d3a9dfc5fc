#!/usr/bin/env python3
"""What a line set's dedup call costs on one GPU, beside the line statistics of the same text and beside the host route, a loop over the
pieces of every document against a Python set.

    python tools/line_set_path.py [MiB] [label] [normalize]    (default: 256 MiB of the bench corpus, a plain set)

tk_line_dedup_device runs on the corpus written as one batch -- a first add=True call on an empty set, a second one on the same text, in
which every line is dropped, and an add=False call against the filled set -- and on a batch that is one document without a newline, the
first 64 MiB of the text with every newline replaced: wall clock around the call and a synchronise (the call itself waits once, for the
number of lines), and its kernels apart, from HIP events.  Clearing and counting the set between calls is outside the clock.
tk_line_stats_device runs on the same buffers in the same session.  The host route runs on the leading documents that hold about 1/64 of
the bytes, timed once and SCALED to the batch; the device result on those documents is compared with it before anything is timed.  Every
device figure is the median of 10 calls after 2 warm-up calls.  `label` names the build in every line.  `normalize`: the set's mask of
NORM_* bits; the host route is then tests/line_norm_ref.py's, the normal form in Python and a set of normal forms."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (first: its HIP runtime has to be the one that is loaded)

import line_norm_ref as ref  # noqa: E402
import lines_ref as lr  # noqa: E402
from bench import gen_corpus  # noqa: E402
from tiktoken_amd import Encoding  # noqa: E402
from tiktoken_ext import amd_shaped  # noqa: E402

mib = int(sys.argv[1]) if len(sys.argv) > 1 else 256
label = sys.argv[2] if len(sys.argv) > 2 else "shipped"
normalize = int(sys.argv[3], 0) if len(sys.argv) > 3 else 0
WARMUP, REPS, ONE_DOC_MIB = 2, 10, 64
HASHING = ("tk_k_ln_sum", "tk_k_ln_carry", "tk_k_ls_mark", "tk_k_ls_decide")  # the kernels a normalising set launches in their other instantiation
LS_KERNELS = ("tk_k_ln_clear", *[k + "_norm" * bool(normalize) for k in HASHING], "tk_k_ls_keep", "tk_k_ls_scan", "tk_k_ls_write")
LN_KERNELS = ("tk_k_ln_clear", "tk_k_ln_sum", "tk_k_ln_carry", "tk_k_ln_count", "tk_k_ln_final")

spec = amd_shaped.ENCODING_CONSTRUCTORS["o200k_shaped"]()
enc = Encoding("o200k_shaped_line_set_path", pat_str=spec["pat_str"], mergeable_ranks=spec["mergeable_ranks"], special_tokens=spec["special_tokens"])
core = enc._core_bpe
dev = torch.device("cuda", core.device)
tag = f"line_set_path {mib} MiB [{label}]" + f" normalize={normalize}" * bool(normalize)


def timed(call, before, names):
    """wall clock of call() -- before() outside it -- as (median, min, max), then every kernel's median time per call from HIP events"""
    ts, per = [], {k: [] for k in names}
    for profiled in (False, True):
        core.set_profiling(profiled)
        for i in range(WARMUP + REPS):
            before()
            core.reset_kernel_ms()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            if i >= WARMUP and not profiled:
                ts.append(time.perf_counter() - t0)
            if i >= WARMUP and profiled:
                for k in names:
                    per[k].append(core.kernel_ms(k)[0])
    core.set_profiling(False)
    return f"median {statistics.median(ts) * 1e3:.3f} ms (min {min(ts) * 1e3:.3f}, max {max(ts) * 1e3:.3f}); kernels, ms: " + ", ".join(
        f"{k} {statistics.median(v):.3f}" for k, v in per.items())


def to_dev(a):
    return torch.from_numpy(a.view({1: np.uint8, 8: np.int64}[a.itemsize]).copy()).to(dev)


def measure(name, ls, d_text, d_off, n_docs):
    new = lambda n, dtype=torch.int64: torch.empty(n, dtype=dtype, device=dev)  # noqa: E731
    outs = dict(text_out=new(d_text.numel(), torch.uint8), doc_off_out=new(n_docs + 1), n_lines=new(n_docs), n_dropped=new(n_docs), counts=new(2))
    stats = {m: new(n_docs) for m in lr.Ref._fields}
    dedup = lambda add: core.line_dedup_device(ls._native, d_text, d_off, add, **outs)  # noqa: E731
    counts = lambda: "kept %d bytes, dropped %d lines" % tuple(outs["counts"].cpu().tolist())  # noqa: E731
    print(f"{tag}: {name}: tk_line_stats_device: {timed(lambda: core.line_stats_device(d_text, d_off, **stats), lambda: None, LN_KERNELS)}", flush=True)
    print(f"{tag}: {name}: tk_line_dedup_device, add=True on an empty set: {timed(lambda: dedup(True), ls.clear, LS_KERNELS)}; {counts()}; {len(ls)} keys", flush=True)
    print(f"{tag}: {name}: tk_line_dedup_device, add=True on the same text again: {timed(lambda: dedup(True), lambda: len(ls), LS_KERNELS)}; {counts()}", flush=True)
    ls.clear()
    dedup(True)  # (a set that holds the batch's lines, and outputs that say what the first call gives)
    first = {k: v.cpu().numpy() for k, v in outs.items()}
    print(f"{tag}: {name}: tk_line_dedup_device, add=False against the filled set: {timed(lambda: dedup(False), lambda: None, LS_KERNELS)}; {counts()}", flush=True)
    return first


blob, off = gen_corpus(0x5EED0003, 1, mib << 20, 16)  # (the bench's corpus)
blob, off = np.ascontiguousarray(blob[:int(off[-1])]), np.ascontiguousarray(off, dtype=np.uint64)
n_docs, N = len(off) - 1, len(blob)
print(f"{tag}: {n_docs} documents, {N} bytes; tile {core.stat('lines_tile')} bytes", flush=True)

sub = int(np.searchsorted(off, N // 64, side="right"))  # the leading documents with about 1/64 of the bytes
data = blob.tobytes()
t0 = time.perf_counter()
want = ref.dedup(set(), [data[int(a):int(b)] for a, b in zip(off[:sub], off[1:sub + 1])], normalize=normalize)
t_host = time.perf_counter() - t0
with enc.line_set(1 << 21, normalize=normalize) as ls:
    first = measure("corpus", ls, to_dev(blob), to_dev(off), n_docs)
    w_text, w_off = lr.pack(want[0])
    assert np.array_equal(first["doc_off_out"].view(np.uint64)[:sub + 1], w_off) and first["text_out"][:len(w_text)].tobytes() == w_text.tobytes()
    assert np.array_equal(first["n_lines"].view(np.uint64)[:sub], want[1]) and np.array_equal(first["n_dropped"].view(np.uint64)[:sub], want[2])
    share = int(off[sub]) / N
    print(f"{tag}: corpus: the first {sub} documents equal the host route's (re.findall, the normal form and a set of bytes) on {share:.4f} of the bytes: {t_host:.2f} s, "
          f"SCALED to the batch {t_host / share:.0f} s", flush=True)
    one = blob[:min(ONE_DOC_MIB << 20, N)].copy()
    one[one == 10] = 32
    measure(f"one document of {len(one) >> 20} MiB without a newline", ls, to_dev(one), to_dev(np.array([0, len(one)], np.uint64)), 1)
