#!/usr/bin/env python3
"""What turning an encoded batch into padded model inputs costs on one GPU, beside the encode step it follows and beside the same rule
written with torch calls on the same device tensors.

    python tools/padded_path.py [MiB]      (default: 256 MiB of the bench corpus, o200k-shaped)

The batch is encoded device-resident (tk_encode_batch_device), then padded (tk_pad_batch_device) in two configurations:
    windows     max_len 512, TK_PAD_WINDOWS, stride 64, eos after every row's body, padded with eos
    truncation  max_len 8192, one row per document (its head), width_multiple 64, no bos / eos, padded with the eot id
Reported per configuration: the time of the padded kernels from HIP events (tk_get_kernel_ms) over the repetitions after warm-up, the wall
clock of the call, the algorithmic bytes -- 4 bytes per body token that lands in a row + 8 (n_docs + 1) read, 5 R W + 12 R + 4 (n_docs + 1)
written -- and the rate they make beside the HBM copy rate recorded in profiles/rows_path.txt; the torch restatement (cumsum,
repeat_interleave, a gather, where), wall clock with torch.cuda.synchronize() on both sides; and the encode step's own wall clock in the
same process.  The two results are compared, array by array, before anything is timed.  Every figure is the median of 20 calls after 3
warm-up calls, with the least and the most; by then torch's caching allocator holds every block the restatement asks for."""
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
WARMUP, REPS = 3, 20
HBM_COPY = 6.29e12  # measured with a float4 copy kernel (profiles/rows_path.txt)
KERNELS = ("tk_k_pad_count", "tk_k_pad_scan", "tk_k_pad_rows", "tk_k_pad_write")

spec = amd_shaped.ENCODING_CONSTRUCTORS["o200k_shaped"]()
enc = Encoding("o200k_shaped_padded_path", pat_str=spec["pat_str"], mergeable_ranks=spec["mergeable_ranks"], special_tokens=spec["special_tokens"])
core = enc._core_bpe
EOS = enc.eot_token
CONFIGS = (("windows", dict(max_length=512, windows=True, stride=64, eos=EOS)), ("truncation", dict(max_length=8192, pad_to_multiple_of=64, pad=EOS)))
n = mib << 20
blob, off = gen_corpus(0x5EED0003, 1, n, 16)  # (the bench's corpus)
blob = blob[:n]
n_docs = len(off) - 1
dev = torch.device("cuda")
d_text = torch.zeros(n + 256, dtype=torch.uint8, device=dev)
d_text[:n] = torch.from_numpy(blob).cuda()
d_off = torch.from_numpy(off.view(np.int64)).cuda()
torch.cuda.synchronize()


class _Dev:
    def __init__(self, ptr, count, typestr):
        self.__cuda_array_interface__ = {"shape": (count,), "typestr": typestr, "data": (ptr, False), "version": 2}


def view(ptr, count, typestr="<i4"):
    return torch.as_tensor(_Dev(ptr, count, typestr), device=dev)


def encode():
    out = core.encode_batch_device(d_text.data_ptr(), n, d_off.data_ptr(), off, n_docs)
    torch.cuda.synchronize()
    return out


def torch_padded(tok, tok_off, max_length, windows=False, stride=0, eos=None, pad=None, pad_to_multiple_of=None):
    """The rule with torch calls: right padding, no bos, the head of a document that is cut."""
    T, nd = tok.numel(), tok_off.numel() - 1
    k = 0 if eos is None else 1
    pad = eos if pad is None else pad
    c = max_length - k
    step = c - stride
    nd_tok = tok_off[1:] - tok_off[:-1]
    w = torch.where(nd_tok <= c, 1, 1 + (nd_tok - c + step - 1) // step) if windows else torch.ones_like(nd_tok)
    doc_row = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(w, 0)])
    R = int(doc_row[-1])
    row_doc = torch.repeat_interleave(torch.arange(nd, device=dev), w, output_size=R)
    row_tok = (torch.arange(R, device=dev) - doc_row[row_doc]) * step if windows else torch.zeros(R, dtype=torch.int64, device=dev)
    length = torch.clamp(nd_tok[row_doc] - row_tok, max=c) + k
    W = max_length if not pad_to_multiple_of else min(max_length, -(-int(length.max()) // pad_to_multiple_of) * pad_to_multiple_of)
    col = torch.arange(W, device=dev)
    mask = col[None, :] < length[:, None]
    src = ((tok_off[row_doc] + row_tok)[:, None] + col[None, :]).clamp_(max=max(T - 1, 0))
    ids = tok[src]
    if eos is not None:
        ids = torch.where(col[None, :] + 1 == length[:, None], eos, ids)
    ids = torch.where(mask, ids, pad)
    return ids.reshape(-1), mask.to(torch.uint8).reshape(-1), length.to(torch.int32), row_doc.to(torch.int32), row_tok.to(torch.int32), doc_row.to(torch.int32)


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


def kernel_ms_per_call(f):
    """Summed HIP-event time of the padded kernels, call by call: (median, min, max) in ms and the per-kernel medians."""
    core.set_profiling(True)
    for _ in range(WARMUP):
        f()
    sums, per = [], {name: [] for name in KERNELS}
    for _ in range(REPS):
        core.reset_kernel_ms()
        f()
        for name in KERNELS:
            per[name].append(core.kernel_ms(name)[0])
        sums.append(sum(per[name][-1] for name in KERNELS))
    core.set_profiling(False)
    return (statistics.median(sums), min(sums), max(sums)), {name: statistics.median(v) for name, v in per.items()}


t_enc = med(encode)
print(f"padded_path {mib} MiB: encode step (tk_encode_batch_device, wall clock): median {t_enc[0] * 1e3:.3f} ms (min {t_enc[1] * 1e3:.3f}, max {t_enc[2] * 1e3:.3f})", flush=True)
dt, nt, dof = encode()
tok, tok_off = view(dt, nt), view(dof, n_docs + 1, "<i8")
slower = []
for cfg_name, cfg in CONFIGS:
    tag = f"padded_path {mib} MiB, {cfg_name}"

    def pad():
        r = core.pad_batch_device(dt, nt, dof, n_docs, **cfg)
        torch.cuda.synchronize()
        return r

    r = pad()
    R, W = r.n_rows, r.width
    print(f"{tag}: {nt} tokens in {n_docs} documents -> {R} rows of {W}", flush=True)
    # equal arrays first
    want = torch_padded(tok, tok_off, **cfg)
    got = (view(r.input_ids, R * W), view(r.attention_mask, R * W, "|u1"), view(r.lengths, R), view(r.row_doc, R), view(r.row_tok, R), view(r.doc_row, n_docs + 1))
    for name, g, w in zip(("input_ids", "attention_mask", "lengths", "row_doc", "row_tok", "doc_row"), got, want):
        assert g.shape == w.shape and bool(torch.equal(g, w)), (cfg_name, name)
    body = int(want[2].sum()) - R * (1 if cfg.get("eos") is not None else 0)
    print(f"{tag}: the hand-written path and the torch restatement give equal input_ids, attention_mask, lengths, row_doc, row_tok and doc_row", flush=True)
    del want, got
    t_pad = med(pad)
    print(f"{tag}: tk_pad_batch_device (wall clock, the call waits for the rows): median {t_pad[0] * 1e3:.3f} ms (min {t_pad[1] * 1e3:.3f}, max {t_pad[2] * 1e3:.3f})", flush=True)
    t_torch = med(lambda: torch_padded(tok, tok_off, **cfg))
    print(f"{tag}: torch restatement (wall clock, caching allocator warm): median {t_torch[0] * 1e3:.3f} ms (min {t_torch[1] * 1e3:.3f}, max {t_torch[2] * 1e3:.3f})", flush=True)
    torch.cuda.empty_cache()
    (total, t_min, t_max), per = kernel_ms_per_call(pad)
    for name in KERNELS:
        print(f"{tag}: {name}: median {per[name]:.4f} ms per call", flush=True)
    rd, wr = 4 * body + 8 * (n_docs + 1), 5 * R * W + 12 * R + 4 * (n_docs + 1)
    rate = (rd + wr) / (total * 1e-3)
    wr_rate = 5 * R * W / (per["tk_k_pad_write"] * 1e-3)
    print(f"{tag}: padded kernels, summed (HIP events, {REPS} calls): median {total:.4f} ms (min {t_min:.4f}, max {t_max:.4f}); algorithmic bytes {rd} read + {wr} written = "
          f"{(rd + wr) / 1e6:.1f} MB -> {rate / 1e9:.0f} GB/s = {rate / HBM_COPY:.2f} of the measured HBM copy rate ({HBM_COPY / 1e12:.2f} TB/s); the write pass alone stores "
          f"{wr_rate / 1e9:.0f} GB/s = {wr_rate / HBM_COPY:.2f} of it", flush=True)
    print(f"{tag}: padding / encode step = {t_pad[0] / t_enc[0]:.3f} (wall clock), {total * 1e-3 / t_enc[0]:.3f} (kernels); torch restatement / hand-written = "
          f"{t_torch[0] / t_pad[0]:.1f}x (wall clock)", flush=True)
    if t_pad[0] > t_torch[0]:
        slower.append(cfg_name)
assert not slower, f"the hand-written path is slower than the torch restatement: {slower}"
