#!/usr/bin/env python3
"""What masking e-mail and IPv4 addresses costs on one GPU, beside the nearest existing pass that reads text and writes text -- the line
cleaning with text out -- and beside the host route, re.sub per document.

    python tools/pii_path.py [MiB]    (default: 256 MiB of the bench corpus, o200k-shaped)

tk_pii_mask_device runs in its counting form (no text out) and in its text-out form on the corpus as it is (its natural density of
addresses), on the corpus with one address planted in every document (an e-mail and an IPv4 address in turn, written over the
document's first bytes), and on one document of the first 64 MiB: wall clock around the call and a synchronise (the call itself waits
for nothing), and its kernels apart, from HIP events.  tk_line_clean_device with text out runs on the same buffers in the same session.
The host route (tests/pii_ref.py) runs on the leading documents that hold about 1/64 of the bytes, timed once and SCALED to the batch;
the device result on those documents is compared with it before anything is timed.  Every device figure is the median of 10 calls
after 2 warm-up calls."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (first: its HIP runtime has to be the one that is loaded)

import pii_ref as ref  # noqa: E402
from bench import gen_corpus  # noqa: E402
from tiktoken_amd import Encoding  # noqa: E402
from tiktoken_ext import amd_shaped  # noqa: E402

mib = int(sys.argv[1]) if len(sys.argv) > 1 else 256
WARMUP, REPS, ONE_DOC_MIB = 2, 10, 64
PII_COUNT = ("tk_k_pii_clear", "tk_k_pii_find", "tk_k_pii_scan")
PII_TEXT = PII_COUNT + ("tk_k_pii_write",)
CL_TEXT = ("tk_k_cl_clear", "tk_k_cl_sum", "tk_k_cl_carry", "tk_k_cl_decide", "tk_k_cl_final", "tk_k_cl_keep", "tk_k_cl_scan", "tk_k_cl_write")

spec = amd_shaped.ENCODING_CONSTRUCTORS["o200k_shaped"]()
enc = Encoding("o200k_shaped_pii_path", pat_str=spec["pat_str"], mergeable_ranks=spec["mergeable_ranks"], special_tokens=spec["special_tokens"])
core = enc._core_bpe
dev = torch.device("cuda", core.device)
tag = f"pii_path {mib} MiB"


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


def measure(name, blob, off):
    """the masking call in both forms and the line cleaning with text out on (blob, off); the masking's outputs on the host"""
    n_docs, n_bytes = len(off) - 1, len(blob)
    d_text, d_off = to_dev(blob), to_dev(off)
    new = lambda n, dtype=torch.int64: torch.empty(n, dtype=dtype, device=dev)  # noqa: E731
    outs = dict(doc_off_out=new(n_docs + 1), n_email=new(n_docs), n_ip=new(n_docs), counts=new(4))
    count_only = {k: v for k, v in outs.items() if k != "doc_off_out"}
    call = lambda: core.pii_mask_device(d_text, d_off, **count_only)  # noqa: E731
    t = med(call)
    print(f"{tag}: {name}: tk_pii_mask_device, counting (wall clock, call and synchronise): {ms(t)} = {n_bytes / t[0] / 1e9:.1f} GB/s; kernels, ms: {kernels(call, PII_COUNT)}", flush=True)
    need = int(outs["counts"][0].item())
    outs["text_out"] = new(need, torch.uint8)
    call = lambda: core.pii_mask_device(d_text, d_off, **outs)  # noqa: E731
    t_text = med(call)
    print(f"{tag}: {name}: tk_pii_mask_device, text out (wall clock, call and synchronise): {ms(t_text)} = {n_bytes / t_text[0] / 1e9:.1f} GB/s; kernels, ms: {kernels(call, PII_TEXT)}",
          flush=True)
    clean = dict(text_out=new(n_bytes, torch.uint8), doc_off_out=new(n_docs + 1), counts=new(2), **{m: new(n_docs) for m in core.CLEAN_OUTS})
    call = lambda: core.line_clean_device(d_text, d_off, **clean)  # noqa: E731
    t_cl = med(call)
    print(f"{tag}: {name}: tk_line_clean_device, text out, same buffers: {ms(t_cl)}; kernels, ms: {kernels(call, CL_TEXT)}", flush=True)
    got = {k: v.cpu().numpy().view(np.uint8 if k == "text_out" else np.uint64) for k, v in outs.items()}
    print(f"{tag}: {name}: {n_docs} documents, {n_bytes} bytes in, {need} out; {int(got['counts'][1])} e-mails, {int(got['counts'][2])} addresses replaced; masking with text out "
          f"{t_text[0] * 1e3:.3f} ms beside the line cleaning's {t_cl[0] * 1e3:.3f} ms", flush=True)
    return got


def check(got, blob, off, sub):
    """the first `sub` documents against the host route; its seconds"""
    data = blob.tobytes()
    t0 = time.perf_counter()
    want = ref.mask([data[int(a):int(b)] for a, b in zip(off[:sub], off[1:sub + 1])])
    t_host = time.perf_counter() - t0
    assert np.array_equal(got["n_email"][:sub], want.n_email) and np.array_equal(got["n_ip"][:sub], want.n_ip)
    assert np.array_equal(got["doc_off_out"][:sub + 1], want.doc_off) and bytes(got["text_out"][:len(want.text)]) == bytes(want.text)
    return t_host


blob, off = gen_corpus(0x5EED0003, 1, mib << 20, 16)  # (the bench's corpus)
blob, off = np.ascontiguousarray(blob[:int(off[-1])]), np.ascontiguousarray(off, dtype=np.uint64)
n_docs, N = len(off) - 1, len(blob)
print(f"{tag}: {n_docs} documents, {N} bytes; tile {core.stat('pii_tile')} bytes, halo {core.stat('pii_halo')}; the default placeholders, public addresses only", flush=True)
sub = int(np.searchsorted(off, N // 64, side="right"))  # the leading documents with about 1/64 of the bytes
share = int(off[sub]) / N

t_host = check(measure("corpus", blob, off), blob, off, sub)
print(f"{tag}: corpus: the first {sub} documents equal the host route's, text and counts; host route (re.sub per document) on {share:.4f} of the bytes: {t_host:.2f} s, SCALED to the "
      f"batch {t_host / share:.1f} s", flush=True)

planted = blob.copy()
for d in range(n_docs):  # one address over the first bytes of every document that is long enough
    m = (b" bob.x+y@mail.site.org ", b" 93.184.216.34 ")[d & 1]
    if int(off[d + 1]) - int(off[d]) >= len(m):
        planted[int(off[d]):int(off[d]) + len(m)] = np.frombuffer(m, np.uint8)
t_host = check(measure("an address planted in every document", planted, off), planted, off, sub)
print(f"{tag}: planted: the first {sub} documents equal the host route's; host route on {share:.4f} of the bytes: {t_host:.2f} s, SCALED {t_host / share:.1f} s", flush=True)

one = np.ascontiguousarray(blob[:min(ONE_DOC_MIB << 20, N)])
measure(f"one document of {len(one) >> 20} MiB", one, np.array([0, len(one)], np.uint64))
