#!/usr/bin/env python3
"""What packing an encoded batch into training rows costs on one GPU, beside the encode step it follows and beside the same rule written
with torch calls on the same device tensors.

    python tools/rows_path.py [MiB] [seq_len]      (default: 256 MiB of the bench corpus, o200k-shaped, rows of 4096, eos after every document)

The batch is encoded device-resident (tk_encode_batch_device), then packed (tk_pack_rows_device).  Reported: the summed time of the row
kernels from HIP events (tk_get_kernel_ms) over the repetitions after warm-up, the wall clock of the call, the algorithmic bytes --
4 T + 8 (n_docs + 1) read, 12 M + 4 (n_segs + R + 2) written -- and the rate they make beside the HBM figures; the torch restatement
(repeat_interleave, gathers, nonzero, searchsorted), wall clock with torch.cuda.synchronize() on both sides; and the encode step's own
wall clock in the same process.  The two results are compared, array by array, before anything is timed.  Every figure is the median of
20 calls after 3 warm-up calls, with the least and the most; by then torch's caching allocator holds every block the restatement asks for,
so its time is its kernels and launches, not allocation."""
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
L = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
WARMUP, REPS = 3, 20
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12  # spec; measured with a float4 copy kernel
KERNELS = ("tk_k_rows_mark", "tk_k_rows_count", "tk_k_rows_scan", "tk_k_rows_write")

spec = amd_shaped.ENCODING_CONSTRUCTORS["o200k_shaped"]()
enc = Encoding("o200k_shaped_rows_path", pat_str=spec["pat_str"], mergeable_ranks=spec["mergeable_ranks"], special_tokens=spec["special_tokens"])
core = enc._core_bpe
EOS = enc.eot_token
n = mib << 20
blob, off = gen_corpus(0x5EED0003, 1, n, 16)  # (the bench's corpus)
blob = blob[:n]
n_docs = len(off) - 1
dev = torch.device("cuda")
d_text = torch.zeros(n + 256, dtype=torch.uint8, device=dev)
d_text[:n] = torch.from_numpy(blob).cuda()
d_off = torch.from_numpy(off.view(np.int64)).cuda()
torch.cuda.synchronize()
tag = f"rows_path {mib} MiB, seq_len {L}"


class _Dev:
    def __init__(self, ptr, count, typestr):
        self.__cuda_array_interface__ = {"shape": (count,), "typestr": typestr, "data": (ptr, False), "version": 2}


def view(ptr, count, typestr="<i4"):
    return torch.as_tensor(_Dev(ptr, count, typestr), device=dev)


def encode():
    out = core.encode_batch_device(d_text.data_ptr(), n, d_off.data_ptr(), off, n_docs)
    torch.cuda.synchronize()
    return out


def pack(dt, nt, dof):
    r = core.pack_rows_device(dt, nt, dof, n_docs, seq_len=L, eos=EOS)
    torch.cuda.synchronize()
    return r


def torch_rows(tok, tok_off):
    """The rule with torch calls: eos after every document, padded with eos, no bos."""
    T, nd = tok.numel(), tok_off.numel() - 1
    out_off = tok_off + torch.arange(nd + 1, device=dev)
    S = T + nd
    R = -(-S // L)
    M = R * L
    doc = torch.repeat_interleave(torch.arange(nd, device=dev), out_off[1:] - out_off[:-1], output_size=S)
    j = torch.arange(M, device=dev)
    is_eos = (j[:S] + 1) == out_off[doc + 1]
    ids = torch.full((M,), EOS, dtype=torch.int32, device=dev)
    ids[:S] = torch.where(is_eos, EOS, tok[(j[:S] - doc).clamp_(max=max(T - 1, 0))])
    start = torch.full((M,), S, dtype=torch.int64, device=dev)
    start[:S] = out_off[doc]
    pos = j - torch.maximum(start, (j // L) * L)
    doc_full = torch.full((M,), -1, dtype=torch.int32, device=dev)
    doc_full[:S] = doc
    seg = torch.nonzero(pos == 0).flatten()
    cu = torch.cat([seg, torch.tensor([M], device=dev)]).to(torch.int32)
    row_seg = torch.searchsorted(seg, torch.arange(R + 1, device=dev) * L).to(torch.int32)
    return ids, doc_full, pos.to(torch.int32), cu, row_seg


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


dt, nt, dof = encode()
tok, tok_off = view(dt, nt), view(dof, n_docs + 1, "<i8")
r = pack(dt, nt, dof)
M = r.n_rows * L + r.n_tail
print(f"{tag}: {nt} tokens in {n_docs} documents -> stream of {r.n_stream}, {r.n_rows} rows, {r.n_segs} segments", flush=True)
# equal arrays first
want = torch_rows(tok, tok_off)
got = (view(r.ids, M), view(r.doc, M), view(r.pos, M), view(r.cu_seqlens, r.n_segs + 1), view(r.row_seg, r.n_rows + 1))
for name, g, w in zip(("ids", "doc", "pos", "cu_seqlens", "row_seg"), got, want):
    assert g.shape == w.shape and bool(torch.equal(g, w)), name
print(f"{tag}: the hand-written path and the torch restatement give equal ids, doc, pos, cu_seqlens and row_seg", flush=True)
del want, got

t_enc = med(encode)
print(f"{tag}: encode step (tk_encode_batch_device, wall clock): median {t_enc[0] * 1e3:.3f} ms (min {t_enc[1] * 1e3:.3f}, max {t_enc[2] * 1e3:.3f})", flush=True)
dt, nt, dof = encode()
tok, tok_off = view(dt, nt), view(dof, n_docs + 1, "<i8")
t_pack = med(lambda: pack(dt, nt, dof))
print(f"{tag}: tk_pack_rows_device (wall clock, the call waits for the rows): median {t_pack[0] * 1e3:.3f} ms (min {t_pack[1] * 1e3:.3f}, max {t_pack[2] * 1e3:.3f})", flush=True)
t_torch = med(lambda: torch_rows(tok, tok_off))
print(f"{tag}: torch restatement (wall clock, caching allocator warm): median {t_torch[0] * 1e3:.3f} ms (min {t_torch[1] * 1e3:.3f}, max {t_torch[2] * 1e3:.3f})", flush=True)


def kernel_ms_per_call(f):
    """Summed HIP-event time of the row kernels, call by call: (median, min, max) in ms and the per-kernel medians."""
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


(total, t_min, t_max), per = kernel_ms_per_call(lambda: pack(dt, nt, dof))
for name in KERNELS:
    print(f"{tag}: {name}: median {per[name]:.4f} ms per call", flush=True)
rd, wr = 4 * nt + 8 * (n_docs + 1), 12 * M + 4 * (r.n_segs + r.n_rows + 2)
rate = (rd + wr) / (total * 1e-3)
print(f"{tag}: row kernels, summed (HIP events, {REPS} calls): median {total:.4f} ms (min {t_min:.4f}, max {t_max:.4f}); algorithmic bytes {rd} read + {wr} written = {(rd + wr) / 1e6:.1f} MB -> "
      f"{rate / 1e9:.0f} GB/s = {rate / HBM_COPY:.2f} of the measured HBM copy rate ({HBM_COPY / 1e12:.2f} TB/s), {rate / HBM_PEAK:.2f} of the 8 TB/s peak", flush=True)
print(f"{tag}: packing / encode step = {t_pack[0] / t_enc[0]:.3f} (wall clock), {total * 1e-3 / t_enc[0]:.3f} (kernels); torch restatement / hand-written = "
      f"{t_torch[0] / t_pack[0]:.1f}x (wall clock)", flush=True)
# the same batch without bos / eos (k = 0, drop_last): the stream is the token array and a lane's ids arrive as two 16-byte loads
(k0, k0_min, k0_max), _ = kernel_ms_per_call(lambda: (core.pack_rows_device(dt, nt, dof, n_docs, seq_len=L, drop_last=True), torch.cuda.synchronize()))
print(f"{tag}: row kernels without eos (k = 0, drop_last; 16-byte loads of the ids): median {k0:.4f} ms (min {k0_min:.4f}, max {k0_max:.4f})", flush=True)
assert t_pack[0] <= t_torch[0], "the hand-written path is slower than the torch restatement"
