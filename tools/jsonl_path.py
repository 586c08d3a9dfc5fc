#!/usr/bin/env python3
"""What reading a JSON Lines buffer costs on one GPU, beside the encode step it precedes and beside the host route,
`[json.loads(l)["text"] for l in f]` followed by `encode_ordinary_batch_packed`.

    python tools/jsonl_path.py [MiB]      (default: 256 MiB of the bench corpus, o200k-shaped)

The documents of the bench corpus are written as JSON Lines by json.dumps with a `text` field and a small `meta` object, once with
ensure_ascii=True and once with False, until the buffer holds the asked size.  Reported per buffer: the extract kernels from HIP events
(tk_get_kernel_ms), per kernel and summed; the wall clock of tk_jsonl_extract_device alone (buffer already on the device); tk_encode_jsonl
(host bytes in, ids out) beside tk_encode_batch_device on the same text already extracted; the host route, timed once; the ratios of the
extract to the encode step and to the host route's json.loads loop.  The extracted text is compared with the host route's before anything is
timed.  Every device figure is the median of 10 calls after 2 warm-up calls."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (first: its HIP runtime has to be the one that is loaded)

from bench import gen_corpus  # noqa: E402
from tiktoken_amd import Encoding  # noqa: E402
from tiktoken_ext import amd_shaped  # noqa: E402

mib = int(sys.argv[1]) if len(sys.argv) > 1 else 256
WARMUP, REPS = 2, 10
KERNELS = ("tk_k_jsonl_sum", "tk_k_jsonl_carry", "tk_k_jsonl_select", "tk_k_jsonl_count", "tk_k_jsonl_tile_scan", "tk_k_jsonl_lines", "tk_k_jsonl_line_scan",
           "tk_k_jsonl_docs", "tk_k_jsonl_write")

spec = amd_shaped.ENCODING_CONSTRUCTORS["o200k_shaped"]()
enc = Encoding("o200k_shaped_jsonl_path", pat_str=spec["pat_str"], mergeable_ranks=spec["mergeable_ranks"], special_tokens=spec["special_tokens"])
core = enc._core_bpe
dev = torch.device("cuda")


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


def kernel_ms(f, names):
    core.set_profiling(True)
    for _ in range(WARMUP):
        f()
    per = {name: [] for name in names}
    for _ in range(REPS):
        core.reset_kernel_ms()
        f()
        for name in names:
            per[name].append(core.kernel_ms(name)[0])
    core.set_profiling(False)
    return {name: statistics.median(v) for name, v in per.items()}


def run(tag, buf: bytes):
    n = len(buf)
    t0 = time.perf_counter()
    texts = [json.loads(line)["text"] for line in buf.splitlines()]
    t_loads = time.perf_counter() - t0
    t0 = time.perf_counter()
    ref_tok, ref_off = enc.encode_ordinary_batch_packed(texts)
    t_host_enc = time.perf_counter() - t0
    got = enc.extract_jsonl(buf)
    assert got.texts() == texts, tag
    print(f"{tag}: {n / 2**20:.1f} MiB, {got.n_lines} lines -> {len(got.text) / 2**20:.1f} MiB of text; the extracted text equals json.loads's", flush=True)
    d_buf = torch.frombuffer(bytearray(buf), dtype=torch.uint8).to(dev)
    torch.cuda.synchronize()

    def extract():
        return core.jsonl_extract_device(d_buf.data_ptr(), n)

    t_ext = med(extract)
    print(f"{tag}: tk_jsonl_extract_device (wall clock, the call waits for the text): median {t_ext[0] * 1e3:.3f} ms (min {t_ext[1] * 1e3:.3f}, max {t_ext[2] * 1e3:.3f}) = "
          f"{n / t_ext[0] / 1e9:.1f} GB/s of JSON Lines", flush=True)
    per = kernel_ms(extract, KERNELS)
    for k in KERNELS:
        print(f"{tag}: {k}: median {per[k]:.4f} ms per call", flush=True)
    print(f"{tag}: extract kernels, summed (HIP events, {REPS} calls): median {sum(per.values()):.4f} ms", flush=True)
    v = extract()
    doc_off = np.asarray(got.doc_off)

    def encode():
        return core.encode_batch_device(v.text, v.n_text, v.doc_off, doc_off, v.n_docs)

    t_enc = med(encode)
    print(f"{tag}: encode step on the extracted text (tk_encode_batch_device, wall clock): median {t_enc[0] * 1e3:.3f} ms (min {t_enc[1] * 1e3:.3f}, max {t_enc[2] * 1e3:.3f})",
          flush=True)
    out = enc.encode_ordinary_jsonl_packed(buf)
    assert np.array_equal(out.tokens, ref_tok) and np.array_equal(out.tok_off, ref_off), tag
    t_all = med(lambda: enc.encode_ordinary_jsonl_packed(buf), reps=5)
    print(f"{tag}: tk_encode_jsonl (host bytes in, ids out, wall clock): median {t_all[0] * 1e3:.1f} ms (min {t_all[1] * 1e3:.1f}, max {t_all[2] * 1e3:.1f}); ids equal the host route's",
          flush=True)
    print(f"{tag}: host route: json.loads loop {t_loads * 1e3:.0f} ms ({n / t_loads / 1e6:.0f} MB/s), then encode_ordinary_batch_packed {t_host_enc * 1e3:.0f} ms", flush=True)
    print(f"{tag}: extract / encode step = {t_ext[0] / t_enc[0]:.3f}; json.loads loop / extract = {t_loads / t_ext[0]:.0f}x; host route / tk_encode_jsonl = "
          f"{(t_loads + t_host_enc) / t_all[0]:.1f}x", flush=True)
    assert t_loads > t_ext[0], f"{tag}: the device pass is slower than json.loads"


n = mib << 20
blob, off = gen_corpus(0x5EED0003, 1, n, 16)  # (the bench's corpus)
data = bytes(blob[:int(off[-1])])
docs = [data[int(a):int(b)].decode("utf-8", "replace") for a, b in zip(off[:-1], off[1:])]
for ascii_only in (True, False):
    lines, size = [], 0
    for i, t in enumerate(docs):
        line = json.dumps({"id": i, "text": t, "meta": {"source": "bench", "lang": "mixed", "n": len(t)}}, ensure_ascii=ascii_only).encode("utf-8") + b"\n"
        if size + len(line) > n:
            break
        lines.append(line)
        size += len(line)
    run(f"jsonl_path {mib} MiB, ensure_ascii={ascii_only}", b"".join(lines))
