#!/usr/bin/env python3
"""What the line cleaning costs on one GPU under C4's defaults, beside the two existing passes whose work it combines -- the word
statistics' classification and the line sets' write -- and beside the host route, a loop over the pieces of every document.

    python tools/clean_path.py [MiB]    (default: 256 MiB of the bench corpus, o200k-shaped)

tk_line_clean_device runs in its counting form (no text out) and in its text-out form on the corpus, and on a batch that is one
document without a newline, the first 64 MiB of the text with every '\\n' replaced: wall clock around the call and a synchronise (the
call itself waits for nothing), and its kernels apart, from HIP events.  tk_word_stats_device and tk_line_dedup_device(add=False), on an
empty set, run on the same buffers in the same session: their sum is the yardstick.  The host route (tests/clean_ref.py) runs on the
leading documents that hold about 1/64 of the bytes, timed once and SCALED to the batch; the device result on those documents is
compared with it before anything is timed.  Every device figure is the median of 10 calls after 2 warm-up calls."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (first: its HIP runtime has to be the one that is loaded)

import clean_ref as cr  # noqa: E402
from bench import gen_corpus  # noqa: E402
from tiktoken_amd import Encoding  # noqa: E402
from tiktoken_ext import amd_shaped  # noqa: E402

mib = int(sys.argv[1]) if len(sys.argv) > 1 else 256
WARMUP, REPS, ONE_DOC_MIB = 2, 10, 64
CL_COUNT = ("tk_k_cl_clear", "tk_k_cl_sum", "tk_k_cl_carry", "tk_k_cl_decide", "tk_k_cl_final", "tk_k_cl_report")
CL_TEXT = CL_COUNT[:-1] + ("tk_k_cl_keep", "tk_k_cl_scan", "tk_k_cl_write")
WD_KERNELS = ("tk_k_wd_clear", "tk_k_wd_sum", "tk_k_wd_carry", "tk_k_wd_count", "tk_k_wd_final")
LS_KERNELS = ("tk_k_ln_clear", "tk_k_ln_sum", "tk_k_ln_carry", "tk_k_ls_decide", "tk_k_ls_keep", "tk_k_ls_scan", "tk_k_ls_write")

spec = amd_shaped.ENCODING_CONSTRUCTORS["o200k_shaped"]()
enc = Encoding("o200k_shaped_clean_path", pat_str=spec["pat_str"], mergeable_ranks=spec["mergeable_ranks"], special_tokens=spec["special_tokens"])
core = enc._core_bpe
dev = torch.device("cuda", core.device)
tag = f"clean_path {mib} MiB"


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
    """the median of every kernel's time per call over REPS profiled calls, in ms (a kernel launched several times per call: their sum)"""
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
    new = lambda n, dtype=torch.int64: torch.empty(n, dtype=dtype, device=dev)  # noqa: E731
    outs = dict(text_out=new(n_bytes, torch.uint8), doc_off_out=new(n_docs + 1), counts=new(2), **{m: new(n_docs) for m in core.CLEAN_OUTS})
    count_only = {k: v for k, v in outs.items() if k not in ("text_out", "doc_off_out")}
    call = lambda: core.line_clean_device(d_text, d_off, **count_only)  # noqa: E731
    t = med(call)
    print(f"{tag}: {name}: tk_line_clean_device, counting (wall clock, call and synchronise): {ms(t)} = {n_bytes / t[0] / 1e9:.1f} GB/s; kernels, ms: {kernels(call, CL_COUNT)}", flush=True)
    call = lambda: core.line_clean_device(d_text, d_off, **outs)  # noqa: E731
    t_text = med(call)
    print(f"{tag}: {name}: tk_line_clean_device, text out (wall clock, call and synchronise): {ms(t_text)} = {n_bytes / t_text[0] / 1e9:.1f} GB/s; kernels, ms: {kernels(call, CL_TEXT)}",
          flush=True)
    words = {m: new(n_docs) for m in core.WORD_OUTS}
    call = lambda: core.word_stats_device(d_text, d_off, **words)  # noqa: E731
    t_wd = med(call)
    print(f"{tag}: {name}: tk_word_stats_device, same buffers: {ms(t_wd)}; kernels, ms: {kernels(call, WD_KERNELS)}", flush=True)
    ls = core.line_set_create(1024)
    dedup = dict(text_out=outs["text_out"], doc_off_out=outs["doc_off_out"], n_lines=new(n_docs), n_dropped=new(n_docs), counts=new(2))
    call = lambda: core.line_dedup_device(ls, d_text, d_off, False, **dedup)  # noqa: E731
    t_ls = med(call)
    print(f"{tag}: {name}: tk_line_dedup_device(add=False) on an empty set, same buffers (its one wait included): {ms(t_ls)}; kernels, ms: {kernels(call, LS_KERNELS)}", flush=True)
    ls.close()
    print(f"{tag}: {name}: text out {t_text[0] * 1e3:.3f} ms beside the yardstick, word statistics + line dedup = {(t_wd[0] + t_ls[0]) * 1e3:.3f} ms", flush=True)
    core.line_clean_device(d_text, d_off, **outs)
    return {k: v.cpu().numpy().view(np.uint8 if k == "text_out" else np.uint64) for k, v in outs.items()}


blob, off = gen_corpus(0x5EED0003, 1, mib << 20, 16)  # (the bench's corpus)
blob, off = np.ascontiguousarray(blob[:int(off[-1])]), np.ascontiguousarray(off, dtype=np.uint64)
n_docs, N = len(off) - 1, len(blob)
d_text, d_off = to_dev(blob), to_dev(off)
torch.cuda.synchronize()
print(f"{tag}: {n_docs} documents, {N} bytes; tile {core.stat('clean_tile')} bytes, {core.stat('clean_docs')} documents of a tile gathered in LDS; C4's defaults", flush=True)

sub = int(np.searchsorted(off, N // 64, side="right"))  # the leading documents with about 1/64 of the bytes
data = blob.tobytes()
t0 = time.perf_counter()
want = cr.clean([data[int(a):int(b)] for a, b in zip(off[:sub], off[1:sub + 1])])
t_host = time.perf_counter() - t0
got = measure("corpus", d_text, d_off, n_docs, N)
for m in cr.FIELDS:
    assert np.array_equal(got[m][:sub], getattr(want, m)), m
assert np.array_equal(got["doc_off_out"][:sub + 1], want.doc_off) and bytes(got["text_out"][:len(want.text)]) == bytes(want.text)
kept, gone = (int(v) for v in got["counts"])
print(f"{tag}: corpus: the first {sub} documents equal the host route's, text and counts; {int(got['n_lines'].sum())} lines, {gone} not written ({int(got['n_short'].sum())} short, "
      f"{int(got['n_long'].sum())} long word, {int(got['n_no_end'].sum())} no end, {int(got['n_ellipsis'].sum())} ellipsis, {int(got['n_phrase'].sum())} phrase); "
      f"{int((got['doc_hit'] != 0).sum())} of {n_docs} documents dropped; {kept} of {N} bytes kept", flush=True)
share = int(off[sub]) / N
print(f"{tag}: corpus: host route (finditer, split, rstrip, lower and `in` per line) on {share:.4f} of the bytes: {t_host:.1f} s, SCALED to the batch {t_host / share:.0f} s", flush=True)

one = blob[:min(ONE_DOC_MIB << 20, N)].copy()
one[one == ord("\n")] = ord(" ")
o1 = measure(f"one document of {len(one) >> 20} MiB without a newline", to_dev(one), to_dev(np.array([0, len(one)], np.uint64)), 1, len(one))
print(f"{tag}: one document: {int(o1['n_lines'][0])} line, {int(o1['n_kept'][0])} kept, doc_hit {int(o1['doc_hit'][0]):#x}, {int(o1['counts'][0])} bytes kept", flush=True)
