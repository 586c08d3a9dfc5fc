#!/usr/bin/env python3
"""Token spans on the bench's 1 GiB corpus (profiles/offsets_path.txt): device-resident spans (tk_token_spans_device), the device-resident
decode (tk_decode_batch_device) on the same ids, both one after the other, the kernels' own times, and one decode_with_offsets call on a
million tokens against the per-token host path.  $TIKTOKEN_AMD_LIB selects another build of the library for a comparison in
the same session.
Usage: python tools/offsets_path.py [MiB of text, default 1024] [single]"""
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from bench import gen_corpus
import tiktoken_amd

mib = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
enc = tiktoken_amd.get_encoding("o200k_shaped")
core = enc._core_bpe
print("library:", os.environ.get("TIKTOKEN_AMD_LIB", "the shipped build"), flush=True)
blob, off = gen_corpus(0x5EED0003, 1, mib << 20, 16)
n = int(off[-1])
n_docs = len(off) - 1
d_text = torch.zeros(n + 256, dtype=torch.uint8, device="cuda")
d_text[:n] = torch.from_numpy(blob[:n]).cuda()
d_off = torch.from_numpy(off.view(np.int64)).cuda()
torch.cuda.synchronize()
dt, nt, dof = core.encode_batch_device(d_text.data_ptr(), n, d_off.data_ptr(), off, n_docs)
print(f"{n} bytes of text, {n_docs} documents, {nt} tokens", flush=True)


def timed(name, f, warm=2, runs=7):
    for _ in range(warm):
        f()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    med = statistics.median(ts)
    print(f"{name}: median {med:.3f} ms (min {min(ts):.3f}, max {max(ts):.3f}, {runs} runs after {warm}) = {n / med / 1e6:.1f} GB/s of decoded text", flush=True)
    return med


spans = lambda: core.token_spans_device(dt, nt, dof, n_docs)
spans_checked = lambda: core.token_spans_device(dt, nt, dof, n_docs, d_off.data_ptr())
decode = lambda: core.decode_batch_device(dt, nt, dof, n_docs)
for rep in range(2):  # (the three alternate, twice)
    timed("spans only (tk_token_spans_device)", spans)
    timed("decode (tk_decode_batch_device, unchanged from the parent commit)", decode)
    timed("spans, then bytes (both calls)", lambda: (spans(), decode()))
timed("spans only, token bytes checked against the text's offsets", spans_checked)
core.set_profiling(True)
core.reset_kernel_ms()
spans(); decode()
for k in ("tk_k_span_mark", "tk_k_span_len", "tk_k_span_scan", "tk_k_span_write", "tk_k_span_docs", "tk_k_dec_len", "tk_k_dec_copy"):
    ms, launches = core.kernel_ms(k)
    print(f"  kernel {k}: {ms:.3f} ms in {launches} launch(es)", flush=True)
core.set_profiling(False)

# host buffers in and out, 256 MiB of the text: tk_decode_batch_spans (spans and bytes, validated) beside tk_decode_batch
sub_docs = int(np.searchsorted(off, min(n, 256 << 20), side="right")) - 1
h_tok, h_off = core.encode_batch_packed(blob[: int(off[sub_docs])], off[: sub_docs + 1])
n_all, n = n, int(off[sub_docs])
print(f"host path: {n} bytes of text, {len(h_tok)} tokens", flush=True)
for rep in range(2):
    timed("host path, decode (tk_decode_batch)", lambda: core.decode_batch_packed(h_tok, h_off, as_array=True), warm=1, runs=4)
    timed("host path, spans + bytes, validated (tk_decode_batch_spans)", lambda: core.decode_batch_spans_packed(h_tok, h_off), warm=1, runs=4)
    timed("host path, spans only, not validated (tk_decode_batch_spans)", lambda: core.decode_batch_spans_packed(h_tok, h_off, want_bytes=False, validate=False), warm=1, runs=4)
n = n_all

if "single" in sys.argv:
    sub_docs = int(np.searchsorted(off, min(n, 8 << 20), side="right")) - 1
    tokens, tok_off = core.encode_batch_packed(blob[: int(off[sub_docs])], off[: sub_docs + 1])
    k = int(np.searchsorted(tok_off, 1_000_000))
    one = tokens[: int(tok_off[k])].tolist()
    print(f"single call: {len(one)} tokens", flush=True)
    ts = []
    for _ in range(4):
        t0 = time.perf_counter()
        text, offsets = enc.decode_with_offsets(one)
        ts.append(time.perf_counter() - t0)
    print(f"decode_with_offsets, one call: {min(ts) * 1e3:.1f} ms best of 4 (all: {', '.join(f'{t * 1e3:.1f}' for t in ts)})", flush=True)
    t0 = time.perf_counter()
    pieces = [enc.decode_single_token_bytes(t) for t in one]  # the parent commit's decode_with_offsets, statement by statement
    offs, n_chars = [], 0
    for piece in pieces:
        offs.append(max(0, n_chars - (1 if 0x80 <= piece[0] < 0xC0 else 0)))
        n_chars += sum(1 for b in piece if not 0x80 <= b < 0xC0)
    text2 = b"".join(pieces).decode("utf-8", errors="strict")
    t_host = time.perf_counter() - t0
    print(f"the parent commit's per-token path on the same tokens: {t_host * 1e3:.1f} ms (one run), identical {text2 == text and offs == offsets}", flush=True)
