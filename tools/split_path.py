#!/usr/bin/env python3
"""What cutting an encoded batch into text chunks costs on one GPU, beside the encode step it follows and beside the host route: ids' offsets
and spans copied out and the rule walked per document with numpy.

    python tools/split_path.py [MiB]      (default: 256 MiB of the bench corpus, o200k-shaped)

The batch is encoded device-resident (tk_encode_batch_device), then split (tk_split_device) at max_tokens 512 with the default separators,
overlap 0 and overlap 64.  Reported per configuration: the time of the split kernels from HIP events (tk_get_kernel_ms), per kernel and
summed, and of the span kernels the entry runs before them; the wall clock of the call; the tk_stat counters (segments, joined, stitch steps,
speculative steps); the bytes the split kernels move -- 4 T of byte_start and the text's bytes read, (L + 1) T / 8 of planes written and read
by the walks, 4 T / 8 for the cut and spec planes, 29 C + 4 (n_docs + 1) written, 8 (n_docs + 1) read -- beside the HBM copy rate recorded in
profiles/rows_path.txt; the encode step's wall clock in the same process; and the host route: tok_off, byte_start, char_start and the
documents' totals copied to the host, the classes of all boundaries computed with numpy at once and the chain walked chunk by chunk (numpy
cannot vectorise a chain).  The two results are compared array for array before anything is timed, and the host route must be no faster.
Two adverse cases follow, one document of 64 MiB each: the head of the corpus as one document (paragraphs), and a run of one digit (no
separator anywhere, so no speculative walk is ever joined and one wavefront walks the document).  Every device figure is the median of 10 calls after 2
warm-up calls; the host route is timed once."""
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
HBM_COPY = 6.29e12  # measured with a float4 copy kernel (profiles/rows_path.txt)
SPLIT = ("tk_k_split_check", "tk_k_split_class", "tk_k_split_walk", "tk_k_split_stitch", "tk_k_split_count", "tk_k_split_scan", "tk_k_split_write", "tk_k_split_docs")
SPANS = ("tk_k_span_mark", "tk_k_span_len", "tk_k_span_scan", "tk_k_span_write", "tk_k_span_docs")
STATS = ("split_segments", "split_joined", "split_stitch_steps", "split_spec_steps")
N, HARD, FORCED, END = 512, 0xFD, 0xFE, 0xFF

spec = amd_shaped.ENCODING_CONSTRUCTORS["o200k_shaped"]()
enc = Encoding("o200k_shaped_split_path", pat_str=spec["pat_str"], mergeable_ranks=spec["mergeable_ranks"], special_tokens=spec["special_tokens"])
core = enc._core_bpe
dev = torch.device("cuda")


class _Dev:
    def __init__(self, ptr, count, typestr):
        self.__cuda_array_interface__ = {"shape": (count,), "typestr": typestr, "data": (ptr, False), "version": 2}


def host(ptr, count, typestr="<i4", dtype=np.uint32):
    if not count:
        return np.zeros(0, dtype)
    return torch.as_tensor(_Dev(ptr, count, typestr), device=dev).cpu().numpy().view(dtype)


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


def host_route(blob, off, tok_off, bs, cs, byte_len, char_len, M, O):
    """The rule on the host: the class of every boundary with numpy at once, then the chain chunk by chunk"""
    T = len(bs)
    n_tok = np.diff(tok_off.astype(np.int64))
    doc_of = np.repeat(np.arange(len(n_tok)), n_tok)
    p = off.astype(np.int64)[doc_of] + bs
    text = np.concatenate([blob, np.zeros(2, np.uint8)])
    here, b1, b2 = text[p], text[p - 1], text[p - 2]  # (a document's first token is never asked: its class is set below)
    in2 = bs >= 2
    cls = np.full(T, 4, np.uint8)  # legal, no level
    cls[here == 0x20] = 3
    cls[((b1 == 0x2E) | (b1 == 0x3F) | (b1 == 0x21)) & (here == 0x20)] = 2
    cls[b1 == 0x0A] = 1
    cls[(b1 == 0x0A) & (b2 == 0x0A) & in2] = 0
    cls[(here & 0xC0) == 0x80] = 5
    cls[tok_off[:-1][n_tok > 0].astype(np.int64)] = 5
    cols = [[] for _ in range(8)]
    doc_chunk = [0]
    for d in range(len(n_tok)):
        g0, n, s = int(tok_off[d]), int(n_tok[d]), 0
        while n:
            if n - s <= N:
                e, cut = n, END
            else:
                w = cls[g0 + s + M:g0 + s + N + 1]
                m = int(w.min())
                if m <= 4:
                    e, cut = s + M + len(w) - 1 - int(np.argmax(w[::-1] == m)), m if m < 4 else HARD
                else:
                    e, cut = s + N, FORCED
            last = e == n
            for c, v in zip(cols, (d, s, e, bs[g0 + s], byte_len[d] if last else bs[g0 + e], cs[g0 + s], char_len[d] if last else cs[g0 + e], cut)):
                c.append(v)
            if last:
                break
            s = e
            if O:
                legal = cls[g0 + e - O:g0 + e + 1] != 5
                if legal.any():
                    s = e - O + int(np.argmax(legal))
        doc_chunk.append(len(cols[0]))
    return [np.array(c, np.uint32) for c in cols[:7]] + [np.array(cols[7], np.uint8), np.array(doc_chunk, np.uint32)]


def run(tag, blob, off, overlaps, t_enc_out=None):
    n, n_docs = len(blob), len(off) - 1
    d_text = torch.zeros(n + 256, dtype=torch.uint8, device=dev)
    d_text[:n] = torch.from_numpy(blob).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    torch.cuda.synchronize()

    def encode():
        out = core.encode_batch_device(d_text.data_ptr(), n, d_off.data_ptr(), off, n_docs)
        torch.cuda.synchronize()
        return out

    t_enc = med(encode)
    print(f"{tag}: encode step (tk_encode_batch_device, wall clock): median {t_enc[0] * 1e3:.3f} ms (min {t_enc[1] * 1e3:.3f}, max {t_enc[2] * 1e3:.3f})", flush=True)
    dt, nt, dof = encode()
    slower = []
    for O in overlaps:
        cfg = dict(max_tokens=N, overlap=O)
        M = max(O + 1, N // 2)
        name = f"{tag}, overlap {O}"

        def split():
            return core.split_device(dt, nt, dof, n_docs, d_text.data_ptr(), d_off.data_ptr(), **cfg)

        r = split()
        C = r.n_chunks
        stats = {k: core.stat(k) for k in STATS}
        print(f"{name}: {nt} tokens in {n_docs} documents -> {C} chunks; " + ", ".join(f"{k} {v}" for k, v in stats.items()) +
              (f"; join rate {stats['split_joined'] / max(stats['split_segments'] - n_docs, 1):.3f} of the segments that do not start a document" if nt else ""), flush=True)
        got = [host(p, C) for p in r[:7]] + [host(r.cut, (C + 3) // 4).view(np.uint8)[:C], host(r.doc_chunk, n_docs + 1)]
        # the host route: what it copies out, then the loop
        t0 = time.perf_counter()
        sp = core._L.tk_token_spans_device  # (the spans as a caller without the split entry gets them)
        import ctypes
        outs = [ctypes.c_void_p() for _ in range(4)]
        rc = sp(core._h, dt, nt, dof, n_docs, d_off.data_ptr(), None, *[ctypes.byref(x) for x in outs])
        assert rc == 0
        bs, cs = host(outs[0].value, nt), host(outs[1].value, nt)
        byte_off, char_off = host(outs[2].value, n_docs + 1, "<i8", np.uint64), host(outs[3].value, n_docs + 1, "<i8", np.uint64)
        tok_off = host(dof, n_docs + 1, "<i8", np.uint64)
        t_copy = time.perf_counter() - t0
        want = host_route(blob, off, tok_off, bs, cs, np.diff(byte_off), np.diff(char_off), M, O)
        t_host = time.perf_counter() - t0
        for what, g, w in zip(("doc", "tok_begin", "tok_end", "byte_begin", "byte_end", "char_begin", "char_end", "cut", "doc_chunk"), got, want):
            assert g.shape == w.shape and np.array_equal(g, w), (name, what)
        print(f"{name}: the device result and the host route give equal doc, tok_begin, tok_end, byte_begin, byte_end, char_begin, char_end, cut and doc_chunk", flush=True)
        split()  # (the spans call above has used the span buffers)
        t_split = med(split)
        print(f"{name}: tk_split_device (wall clock, spans included, the call waits for the chunks): median {t_split[0] * 1e3:.3f} ms (min {t_split[1] * 1e3:.3f}, "
              f"max {t_split[2] * 1e3:.3f})", flush=True)
        per = kernel_ms(split, SPLIT + SPANS)
        for k in SPLIT:
            print(f"{name}: {k}: median {per[k]:.4f} ms per call", flush=True)
        total, spans = sum(per[k] for k in SPLIT), sum(per[k] for k in SPANS)
        moved = 4 * nt + n + 2 * 5 * nt // 8 + 4 * nt // 8 + 29 * C + 12 * (n_docs + 1)
        rate = moved / (total * 1e-3) if total else 0.0
        print(f"{name}: split kernels, summed (HIP events, {REPS} calls): median {total:.4f} ms; the span kernels before them {spans:.4f} ms; bytes moved {moved / 1e6:.1f} MB -> "
              f"{rate / 1e9:.0f} GB/s = {rate / HBM_COPY:.3f} of the measured HBM copy rate ({HBM_COPY / 1e12:.2f} TB/s)", flush=True)
        if stats["split_stitch_steps"]:
            print(f"{name}: tk_k_split_stitch per step: {per['tk_k_split_stitch'] * 1e3 / stats['split_stitch_steps']:.3f} us (steps of all documents, walked in parallel "
                  f"across documents and in order inside one)", flush=True)
        print(f"{name}: split / encode step = {t_split[0] / t_enc[0]:.3f} (wall clock), {total * 1e-3 / t_enc[0]:.3f} (split kernels), {(total + spans) * 1e-3 / t_enc[0]:.3f} "
              f"(with spans); host route {t_host * 1e3:.0f} ms ({t_copy * 1e3:.0f} ms of it the copies) = {t_host / t_split[0]:.0f}x", flush=True)
        if t_host < t_split[0]:
            slower.append(name)
    return slower


n = mib << 20
blob, off = gen_corpus(0x5EED0003, 1, n, 16)  # (the bench's corpus)
blob = blob[:n]
slower = run(f"split_path {mib} MiB", blob, off, (0, 64))
one = 64 << 20
head = blob[:one] if len(blob) >= one else np.resize(blob, one)
while one and (head[one - 1] & 0xC0) == 0x80:  # (do not end inside a char)
    one -= 1
one -= 1 if one and head[one - 1] >= 0xC0 else 0
slower += run("split_path one document of 64 MiB, paragraphs", np.ascontiguousarray(head[:one]), np.array([0, one], np.uint64), (0,))
slower += run("split_path one document of 64 MiB, no separator", np.full(64 << 20, 0x37, np.uint8), np.array([0, 64 << 20], np.uint64), (0,))
assert not slower, f"the device path is slower than the host route: {slower}"
