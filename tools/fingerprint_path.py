#!/usr/bin/env python3
"""What near-duplicate fingerprints cost on one GPU, beside the encode step they follow and beside the host route, the same rule in numpy
on the copied-out ids.

    python tools/fingerprint_path.py [MiB]      (default: 256 MiB of the bench corpus, o200k-shaped; k = 5, P = 128, B = 16)

Reported: the encode step (tk_encode_batch_device on text that is on the device, wall clock); tk_fingerprint_device on the ids (wall clock
around the call and a synchronise of its stream) and each of its kernels from HIP events (tk_get_kernel_ms); the host route
(tests/fingerprint_ref.py's numpy form, document by document) on the leading documents that hold about 1/32 of the ids, timed once and
scaled to the batch; the two ratios.  The device result on those documents is compared with the host route's before anything is timed.
Every device figure is the median of 10 calls after 2 warm-up calls."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (first: its HIP runtime has to be the one that is loaded)

import fingerprint_ref as fr  # noqa: E402
from bench import gen_corpus  # noqa: E402
from tiktoken_amd import Encoding  # noqa: E402
from tiktoken_ext import amd_shaped  # noqa: E402

mib = int(sys.argv[1]) if len(sys.argv) > 1 else 256
WARMUP, REPS = 2, 10
K, P, B, SEED = 5, 128, 16, 0
KERNELS = ("tk_k_fp_fill", "tk_k_fp_tile", "tk_k_fp_finish")

spec = amd_shaped.ENCODING_CONSTRUCTORS["o200k_shaped"]()
enc = Encoding("o200k_shaped_fingerprint_path", pat_str=spec["pat_str"], mergeable_ranks=spec["mergeable_ranks"], special_tokens=spec["special_tokens"])
core = enc._core_bpe
dev = torch.device("cuda", core.device)


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


n = mib << 20
blob, off = gen_corpus(0x5EED0003, 1, n, 16)  # (the bench's corpus)
blob, off = np.ascontiguousarray(blob[:int(off[-1])]), np.ascontiguousarray(off, dtype=np.uint64)
n_docs = len(off) - 1
tag = f"fingerprint_path {mib} MiB"
d_text = torch.from_numpy(blob).to(dev)
d_doc_off = torch.from_numpy(off.view(np.int64)).to(dev)
torch.cuda.synchronize()


def encode():
    return core.encode_batch_device(d_text.data_ptr(), len(blob), d_doc_off.data_ptr(), off, n_docs)


t_enc = med(encode)
tok, tok_off = core.encode_batch_packed(blob, off, None)
T = len(tok)
print(f"{tag}: {n_docs} documents, {T} ids; k = {K}, P = {P}, B = {B}; tile {core.stat('fingerprint_tile')} positions", flush=True)
print(f"{tag}: encode step (tk_encode_batch_device, wall clock): median {t_enc[0] * 1e3:.3f} ms (min {t_enc[1] * 1e3:.3f}, max {t_enc[2] * 1e3:.3f})", flush=True)
d_tok = torch.from_numpy(tok.view(np.int32).copy()).to(dev)  # (the library's arrays are read-only: torch wants a writable one)
d_off = torch.from_numpy(tok_off.view(np.int64).copy()).to(dev)
sig = torch.empty(n_docs * P, dtype=torch.int32, device=dev)
band = torch.empty(n_docs * B, dtype=torch.int64, device=dev)
exact, nsh = torch.empty(n_docs, dtype=torch.int64, device=dev), torch.empty(n_docs, dtype=torch.int64, device=dev)


def fingerprint():
    core.fingerprint_device(d_tok, d_off, ngram=K, n_perm=P, bands=B, seed=SEED, sig=sig, band=band, exact=exact, n_shingles=nsh)


fingerprint()
torch.cuda.synchronize()
sub = int(np.searchsorted(tok_off, T // 32, side="right"))  # the leading documents with about 1/32 of the ids
t0 = time.perf_counter()
want = fr.fingerprint(tok[:int(tok_off[sub])], tok_off[:sub + 1], K, P, B, SEED)
t_host = time.perf_counter() - t0
share = int(tok_off[sub]) / T
assert np.array_equal(sig.cpu().numpy().view(np.uint32).reshape(n_docs, P)[:sub], want.sig) and np.array_equal(band.cpu().numpy().view(np.uint64).reshape(n_docs, B)[:sub], want.band)
assert np.array_equal(exact.cpu().numpy().view(np.uint64)[:sub], want.exact) and np.array_equal(nsh.cpu().numpy().view(np.uint64)[:sub], want.n_shingles)
print(f"{tag}: the device result on the first {sub} documents ({int(tok_off[sub])} ids) equals the host route's", flush=True)
t_fp = med(fingerprint)
print(f"{tag}: tk_fingerprint_device (wall clock, call and synchronise): median {t_fp[0] * 1e3:.3f} ms (min {t_fp[1] * 1e3:.3f}, max {t_fp[2] * 1e3:.3f}) = "
      f"{T / t_fp[0] / 1e9:.2f} G ids/s, {T * P / t_fp[0] / 1e12:.3f} T permutation values/s", flush=True)
core.set_profiling(True)
for _ in range(WARMUP):
    fingerprint()
per = {name: [] for name in KERNELS}
for _ in range(REPS):
    core.reset_kernel_ms()
    fingerprint()
    for name in KERNELS:
        per[name].append(core.kernel_ms(name)[0])
core.set_profiling(False)
for name in KERNELS:
    print(f"{tag}: {name}: median {statistics.median(per[name]):.4f} ms per call", flush=True)
print(f"{tag}: kernels, summed (HIP events, {REPS} calls): median {sum(statistics.median(v) for v in per.values()):.4f} ms", flush=True)
print(f"{tag}: host route (numpy, document by document) on {share:.4f} of the ids: {t_host:.2f} s, scaled to the batch {t_host / share:.1f} s", flush=True)
print(f"{tag}: fingerprint / encode step = {t_fp[0] / t_enc[0]:.3f}; host route / fingerprint = {t_host / share / t_fp[0]:.0f}x", flush=True)
