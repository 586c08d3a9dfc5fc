#!/usr/bin/env python3
"""What packing supervised samples several to a row costs on one GPU, beside one row per sample on the same ids in the same process.

    python tools/sample_rows_path.py [MiB] [out.txt]      (default: 256 MiB of the bench corpus, o200k-shaped)

The workload is tools/samples_path.py's: the batch is encoded device-resident (tk_encode_batch_device); its documents are the parts, four
to a sample, with alternating roles -- an untrained one and a trained one, each with 4 before ids and 2 after ids --, max_len 4096, an
eos behind every sample.  tk_pack_samples_device packs them next-fit; the yardstick, tk_assemble_samples_device with width_multiple 64,
runs on the same ids.  Before anything is timed every element of the packed rows is compared with the yardstick's row of its sample
(ids and labels at [seg, pos]), and the segment arrays with the positions.  Reported: rows and fill of both forms, the time of every
kernel from HIP events (tk_get_kernel_ms), medians of 20 calls after 3 warm-up calls, the packing passes as a total, and both write passes
as time per byte written -- 16 bytes per position here (ids, labels, seg, pos), 9 there (ids, labels, mask).  The bar: tk_k_srow_write at
most 1.5 times slower per written byte than tk_k_smp_write."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (first: its HIP runtime has to be the one that is loaded)

from bench import gen_corpus  # noqa: E402
from tiktoken_amd import Encoding, Role  # noqa: E402
from tiktoken_ext import amd_shaped  # noqa: E402

mib = int(sys.argv[1]) if len(sys.argv) > 1 else 256
out_path = sys.argv[2] if len(sys.argv) > 2 else None
WARMUP, REPS = 3, 20
SHARED = ("tk_k_smp_count", "tk_k_smp_scan", "tk_k_smp_samples")
PACKING = ("tk_k_srow_plen", "tk_k_srow_sums", "tk_k_srow_succ", "tk_k_srow_double", "tk_k_srow_rows", "tk_k_srow_place", "tk_k_srow_segs")
SROW_KERNELS = SHARED + PACKING + ("tk_k_srow_write",)
SMP_KERNELS = SHARED + ("tk_k_smp_write",)
MAX_LEN, MULTIPLE, PER_SAMPLE = 4096, 64, 4
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


spec = amd_shaped.ENCODING_CONSTRUCTORS["o200k_shaped"]()
enc = Encoding("o200k_shaped_sample_rows_path", pat_str=spec["pat_str"], mergeable_ranks=spec["mergeable_ranks"], special_tokens=spec["special_tokens"])
core = enc._core_bpe
EOS = enc.eot_token
ROLES = (Role((EOS, 200001, 200002, 200003), (200004, 200005), False), Role((EOS, 200001, 200006, 200003), (200004, 200007), True))
n = mib << 20
blob, off = gen_corpus(0x5EED0003, 1, n, 16)  # (the bench's corpus)
blob = blob[:n]
n_parts = len(off) - 1
dev = torch.device("cuda")
d_text = torch.zeros(n + 256, dtype=torch.uint8, device=dev)
d_text[:n] = torch.from_numpy(blob).cuda()
d_off = torch.from_numpy(off.view(np.int64)).cuda()
part_role = (np.arange(n_parts) % 2).astype(np.uint8)
sample_off = np.append(np.arange(0, n_parts, PER_SAMPLE), n_parts).astype(np.uint64)
n_samples = len(sample_off) - 1
d_role = torch.from_numpy(part_role).cuda()
d_so = torch.from_numpy(sample_off.view(np.int64)).cuda()
torch.cuda.synchronize()


class _Dev:
    def __init__(self, ptr, count, typestr):
        self.__cuda_array_interface__ = {"shape": (count,), "typestr": typestr, "data": (ptr, False), "version": 2}


def view(ptr, count, typestr="<i4"):
    return torch.as_tensor(_Dev(ptr, count, typestr), device=dev)


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


def kernel_ms_per_call(f, kernels):
    """HIP-event time of the kernels, call by call: the per-kernel medians in ms (a kernel launched several times in a call: their sum)"""
    core.set_profiling(True)
    for _ in range(WARMUP):
        f()
    per = {name: [] for name in kernels}
    for _ in range(REPS):
        core.reset_kernel_ms()
        f()
        for name in kernels:
            per[name].append(core.kernel_ms(name)[0])
    core.set_profiling(False)
    return {name: statistics.median(v) for name, v in per.items()}


tag = f"sample_rows_path {mib} MiB"
dt, nt, dof = core.encode_batch_device(d_text.data_ptr(), n, d_off.data_ptr(), off, n_parts)
torch.cuda.synchronize()


def packed():
    r = core.pack_samples_device(dt, nt, dof, n_parts, d_role.data_ptr(), d_so.data_ptr(), n_samples, ROLES, max_length=MAX_LEN, eos=EOS, pad=EOS)
    torch.cuda.synchronize()
    return r


def samples():
    r = core.assemble_samples_device(dt, nt, dof, n_parts, d_role.data_ptr(), d_so.data_ptr(), n_samples, ROLES, max_length=MAX_LEN, pad_to_multiple_of=MULTIPLE, eos=EOS, pad=EOS)
    torch.cuda.synchronize()
    return r


p, s = packed(), samples()
R, L, SR, SW = p.n_rows, MAX_LEN, s.n_rows, s.width
ids, labels, seg, pos = (view(x, R * L).long() for x in (p.input_ids, p.labels, p.segment_ids, p.position_ids))
s_ids, s_labels, s_len = view(s.input_ids, SR * SW).long(), view(s.labels, SR * SW).long(), view(s.length, SR).long()
element = seg != -1  # (the int32 view of TK_ROWS_NO_TOKEN)
at = seg[element] * SW + pos[element]
assert int(element.sum()) == int(s_len.sum()) and bool(torch.equal(ids[element], s_ids[at])) and bool(torch.equal(labels[element], s_labels[at]))
assert bool((ids[~element] == EOS).all()) and bool((labels[~element] == -100).all())
cu = view(p.cu_seqlens, p.n_segs + 1).long()
assert bool(torch.equal(torch.nonzero(pos == 0).reshape(-1), cu[:-1])) and int(cu[-1]) == R * L
row_seg = view(p.row_seg, R + 1).long()
assert bool(torch.equal(row_seg, torch.searchsorted(cu[:-1].contiguous(), torch.arange(R + 1, device=dev) * L)))
assert bool(torch.equal(view(p.length, n_samples), view(s.length, SR))) and bool(torch.equal(view(p.n_trained, n_samples), view(s.n_trained, SR)))
elements = int(element.sum())
say(f"{tag}: {nt} tokens in {n_parts} parts, {n_samples} samples of {PER_SAMPLE} parts, {elements} elements after the cut at {MAX_LEN}")
say(f"{tag}: one row per sample (tk_assemble_samples_device): {SR} rows of {SW}, fill {elements / (SR * SW):.4f}")
say(f"{tag}: packed (tk_pack_samples_device): {R} rows of {L} in {p.n_segs} segments, fill {elements / (R * L):.4f}; {SR * SW / (R * L):.3f} times fewer positions")
say(f"{tag}: every packed element equals the yardstick's at [seg, pos] (ids and labels); cu_seqlens and row_seg agree with pos")
del ids, labels, seg, pos, s_ids, s_labels, element, at
torch.cuda.empty_cache()
t_p, t_s = med(packed), med(samples)
say(f"{tag}: tk_pack_samples_device (wall clock, the call waits for the rows): median {t_p[0] * 1e3:.3f} ms (min {t_p[1] * 1e3:.3f}, max {t_p[2] * 1e3:.3f})")
say(f"{tag}: yardstick: tk_assemble_samples_device (wall clock): median {t_s[0] * 1e3:.3f} ms (min {t_s[1] * 1e3:.3f}, max {t_s[2] * 1e3:.3f})")
per = kernel_ms_per_call(packed, SROW_KERNELS)
for name in SROW_KERNELS:
    say(f"{tag}: {name}: median {per[name]:.4f} ms per call" + (" (all rounds of a call)" if name == "tk_k_srow_double" else ""))
per_s = kernel_ms_per_call(samples, SMP_KERNELS)
for name in SMP_KERNELS:
    say(f"{tag}: yardstick: {name}: median {per_s[name]:.4f} ms per call")
packing = sum(per[k] for k in PACKING)
say(f"{tag}: the packing passes (placed lengths, sums, successor, doubling, marks, place, segments) together: {packing:.4f} ms per call; the write pass: "
    f"{per['tk_k_srow_write']:.4f} ms -> the packing passes {'EXCEED' if packing > per['tk_k_srow_write'] else 'stay below'} the write pass")
p_bytes, s_bytes = 16 * R * L, 9 * SR * SW
p_ps, s_ps = per["tk_k_srow_write"] * 1e9 / p_bytes, per_s["tk_k_smp_write"] * 1e9 / s_bytes
ratio = p_ps / s_ps
say(f"{tag}: tk_k_srow_write writes {p_bytes} bytes (16 per position): {p_ps:.4f} ps per byte = {p_bytes / per['tk_k_srow_write'] / 1e6:.0f} GB/s; tk_k_smp_write writes "
    f"{s_bytes} bytes (9 per position): {s_ps:.4f} ps per byte = {s_bytes / per_s['tk_k_smp_write'] / 1e6:.0f} GB/s; ratio {ratio:.3f} "
    f"(the bar: at most 1.5) -> {'met' if ratio <= 1.5 else 'NOT met'}")
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
