#!/usr/bin/env python3
"""What turning an encoded batch into supervised samples costs on one GPU, beside the padded pass on the same ids.

    python tools/samples_path.py [MiB]      (default: 256 MiB of the bench corpus, o200k-shaped)

The batch is encoded device-resident (tk_encode_batch_device); its documents are the parts, four to a sample, with alternating roles -- an
untrained one and a trained one, each with 4 before ids and 2 after ids --, max_len 4096, width_multiple 64, eos behind every sample
(tk_assemble_samples_device).  The arrays are compared with the same rule written with torch calls before anything is timed.  Reported:
the time of every samples kernel from HIP events (tk_get_kernel_ms), medians of 20 calls after 3 warm-up calls, and the wall clock of the
call.  The yardstick is measured in the same run: tk_pad_batch_device on the same ids in the truncation configuration of
tools/padded_path.py (max_len 8192, width_multiple 64, no bos / eos), and both write passes as time per byte written -- 9 bytes per
position here (ids, labels, mask), 5 there (ids, mask).  The bar: tk_k_smp_write at most 1.5 times slower per written byte than
tk_k_pad_write."""
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
WARMUP, REPS = 3, 20
SMP_KERNELS = ("tk_k_smp_count", "tk_k_smp_scan", "tk_k_smp_samples", "tk_k_smp_write")
PAD_KERNELS = ("tk_k_pad_count", "tk_k_pad_scan", "tk_k_pad_rows", "tk_k_pad_write")
MAX_LEN, MULTIPLE, PER_SAMPLE = 4096, 64, 4

spec = amd_shaped.ENCODING_CONSTRUCTORS["o200k_shaped"]()
enc = Encoding("o200k_shaped_samples_path", pat_str=spec["pat_str"], mergeable_ranks=spec["mergeable_ranks"], special_tokens=spec["special_tokens"])
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


def torch_samples(tok, tok_off):
    """The rule with torch calls: the head of an over-long sample, right padding, no bos, an eos."""
    nb = torch.tensor([len(r.before) for r in ROLES], device=dev)
    na = torch.tensor([len(r.after) for r in ROLES], device=dev)
    trains = torch.tensor([r.train for r in ROLES], device=dev)
    table = torch.tensor([list(r.before) + list(r.after) for r in ROLES], device=dev)  # (every role has nb + na = 6 ids here)
    role = d_role.long()
    n_body = tok_off[1:] - tok_off[:-1]
    pstart = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(nb[role] + n_body + na[role], 0)])
    so = d_so
    full = pstart[so[1:]] - pstart[so[:-1]] + 1
    length = torch.clamp(full, max=MAX_LEN)
    W = min(MAX_LEN, -(-int(length.max()) // MULTIPLE) * MULTIPLE)
    col = torch.arange(W, device=dev)[None, :]
    mask = col < length[:, None]
    is_eos = mask & (col + 1 == full[:, None])
    in_part = mask & ~is_eos
    g = (pstart[so[:-1]][:, None] + col).clamp_(max=int(pstart[-1]) - 1)
    part = torch.searchsorted(pstart, g, right=True) - 1
    i = g - pstart[part]
    r = role[part]
    body = (i >= nb[r]) & (i < nb[r] + n_body[part])
    src = (tok_off[part] + i - nb[r]).clamp_(min=0, max=tok.numel() - 1)
    slot = torch.where(i < nb[r], i, i - n_body[part]).clamp_(min=0, max=table.shape[1] - 1)
    ids = torch.where(body, tok[src].long(), table[r, slot])
    trained = in_part & trains[r] & (i >= nb[r])
    last_trains = trains[role[(so[1:] - 1).clamp_(min=0)]] & (so[1:] > so[:-1])
    trained = trained | (is_eos & last_trains[:, None])
    ids = torch.where(is_eos, EOS, ids)
    ids = torch.where(mask, ids, EOS)
    labels = torch.where(trained, ids, -100)
    return (ids.to(torch.int32).reshape(-1), mask.to(torch.uint8).reshape(-1), labels.to(torch.int32).reshape(-1), length.to(torch.int32), full,
            trained.sum(1).to(torch.int32))


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
    """HIP-event time of the kernels, call by call: the per-kernel medians in ms"""
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


def encode():
    out = core.encode_batch_device(d_text.data_ptr(), n, d_off.data_ptr(), off, n_parts)
    torch.cuda.synchronize()
    return out


tag = f"samples_path {mib} MiB"
t_enc = med(encode)
print(f"{tag}: encode step (tk_encode_batch_device, wall clock): median {t_enc[0] * 1e3:.3f} ms (min {t_enc[1] * 1e3:.3f}, max {t_enc[2] * 1e3:.3f})", flush=True)
dt, nt, dof = encode()
tok, tok_off = view(dt, nt), view(dof, n_parts + 1, "<i8")


def samples():
    r = core.assemble_samples_device(dt, nt, dof, n_parts, d_role.data_ptr(), d_so.data_ptr(), n_samples, ROLES, max_length=MAX_LEN, pad_to_multiple_of=MULTIPLE, eos=EOS, pad=EOS)
    torch.cuda.synchronize()
    return r


def padded():
    r = core.pad_batch_device(dt, nt, dof, n_parts, max_length=8192, pad_to_multiple_of=64, pad=EOS)
    torch.cuda.synchronize()
    return r


r = samples()
R, W = r.n_rows, r.width
print(f"{tag}: {nt} tokens in {n_parts} parts -> {R} samples of {PER_SAMPLE} parts, rows of {W}", flush=True)
want = torch_samples(tok, tok_off)
got = (view(r.input_ids, R * W), view(r.attention_mask, R * W, "|u1"), view(r.labels, R * W), view(r.length, R), view(r.full_length, R, "<i8"), view(r.n_trained, R))
for name, g, w in zip(("input_ids", "attention_mask", "labels", "length", "full_length", "n_trained"), got, want):
    assert g.shape == w.shape and bool(torch.equal(g, w)), name
elements, trained, cut = int(want[3].sum()), int(want[5].sum()), int((want[4] > MAX_LEN).sum())
print(f"{tag}: the hand-written path and the torch restatement give equal input_ids, attention_mask, labels, length, full_length and n_trained "
      f"({elements} elements, {trained} of them trained, {cut} samples cut)", flush=True)
del want, got
torch.cuda.empty_cache()
t_smp = med(samples)
print(f"{tag}: tk_assemble_samples_device (wall clock, the call waits for the rows): median {t_smp[0] * 1e3:.3f} ms (min {t_smp[1] * 1e3:.3f}, max {t_smp[2] * 1e3:.3f})", flush=True)
per = kernel_ms_per_call(samples, SMP_KERNELS)
for name in SMP_KERNELS:
    print(f"{tag}: {name}: median {per[name]:.4f} ms per call", flush=True)
p = padded()
PR, PW = p.n_rows, p.width
t_pad = med(padded)
print(f"{tag}: yardstick: tk_pad_batch_device, truncation (max_len 8192, width_multiple 64) on the same ids -> {PR} rows of {PW}; wall clock median {t_pad[0] * 1e3:.3f} ms", flush=True)
per_pad = kernel_ms_per_call(padded, PAD_KERNELS)
for name in PAD_KERNELS:
    print(f"{tag}: yardstick: {name}: median {per_pad[name]:.4f} ms per call", flush=True)
smp_bytes, pad_bytes = 9 * R * W, 5 * PR * PW
smp_ps, pad_ps = per["tk_k_smp_write"] * 1e9 / smp_bytes, per_pad["tk_k_pad_write"] * 1e9 / pad_bytes
ratio = smp_ps / pad_ps
print(f"{tag}: tk_k_smp_write writes {smp_bytes} bytes (9 per position): {smp_ps:.4f} ps per byte = {smp_bytes / per['tk_k_smp_write'] / 1e6:.0f} GB/s; tk_k_pad_write writes "
      f"{pad_bytes} bytes (5 per position): {pad_ps:.4f} ps per byte = {pad_bytes / per_pad['tk_k_pad_write'] / 1e6:.0f} GB/s; ratio {ratio:.3f} "
      f"(the bar: at most 1.5) -> {'met' if ratio <= 1.5 else 'NOT met'}", flush=True)
print(f"{tag}: samples / encode step = {t_smp[0] / t_enc[0]:.3f} (wall clock), {sum(per.values()) * 1e-3 / t_enc[0]:.3f} (kernels)", flush=True)
