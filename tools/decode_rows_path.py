#!/usr/bin/env python3
"""What trimming an id matrix costs on one GPU, beside the decode step it feeds and beside the same rule written with torch calls on the
same device tensor.

    python tools/decode_rows_path.py [MiB] [ROWS] [COLUMNS] [--out FILE]
    (default: 64 MiB of the bench corpus, o200k-shaped, as 4096 rows of 2048 columns; FILE: profiles/decode_rows_path.txt)

The workload has the shape a generation loop hands back: the corpus is encoded device-resident, its ids fill an int64 matrix [R, W] that is
a column slice of a wider one (64 prompt columns in front, so the rows are ld = W + 64 apart and start 512 bytes behind each other's
ends), every row has a random begin in its first quarter and one stop id at a random column behind it, with a pad id outside the
vocabulary from there to the row's end.  tk_decode_rows_device runs with that stop id, that pad id in skip_ids and TK_DROWS_SKIP_SPECIAL.
Reported: the time of every new kernel from HIP events (tk_get_kernel_ms) and of the decode kernels behind them, the wall clock of the call;
the same rule with torch calls (isin, argmax, cumsum, a boolean gather), compared array by array with the kernels' result before anything is
timed; tk_decode_batch_device on the already-compact ids in the same process -- the step the new passes feed --; and the bytes the new
passes read and write beside the HBM copy rate recorded in profiles/rows_path.txt.  Every figure is the median of 20 calls after 3 warm-up
calls, with the least and the most."""
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

args = sys.argv[1:]
out_path = os.path.join(ROOT, "profiles", "decode_rows_path.txt")
if "--out" in args:
    at = args.index("--out")
    out_path = args[at + 1]
    del args[at: at + 2]
mib, R, W = (int(args[i]) if len(args) > i else d for i, d in enumerate((64, 4096, 2048)))
PROMPT = 64
WARMUP, REPS = 3, 20
HBM_COPY = 6.29e12  # measured with a float4 copy kernel (profiles/rows_path.txt)
NEW = ("tk_k_drows_stop", "tk_k_drows_count", "tk_k_drows_scan", "tk_k_drows_rows", "tk_k_drows_write")
DECODE = ("tk_k_dec_len", "tk_k_dec_copy")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


spec = amd_shaped.ENCODING_CONSTRUCTORS["o200k_shaped"]()
enc = Encoding("o200k_shaped_decode_rows_path", pat_str=spec["pat_str"], mergeable_ranks=spec["mergeable_ranks"], special_tokens=spec["special_tokens"])
core = enc._core_bpe
EOS, PAD = enc.eot_token, enc.max_token_value + 1000
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
    return torch.as_tensor(_Dev(ptr, count, typestr), device=dev) if count else torch.zeros(0, dtype=torch.int32, device=dev)


dt, nt, _ = core.encode_batch_device(d_text.data_ptr(), n, d_off.data_ptr(), off, n_docs)
torch.cuda.synchronize()
assert nt >= R * W, f"{mib} MiB give {nt} ids: fewer than {R} x {W}"
gen = torch.Generator(device=dev)
gen.manual_seed(0x5EED)
wide = torch.full((R, W + PROMPT), PAD, dtype=torch.int64, device=dev)
ids = wide[:, PROMPT:]  # the slice a caller holds: out[:, prompt_len:]
ids.copy_(view(dt, R * W).to(torch.int64).reshape(R, W))
begin = torch.randint(0, max(W // 4, 1), (R,), device=dev, generator=gen)
stop_at = begin + torch.randint(0, W - W // 4, (R,), device=dev, generator=gen)
col = torch.arange(W, device=dev)
ids[col[None, :] == stop_at[:, None]] = EOS
ids[col[None, :] > stop_at[:, None]] = PAD
d_begin = begin.to(torch.int32).contiguous()
is_special = torch.zeros(enc.max_token_value + 2, dtype=torch.bool, device=dev)
is_special[torch.tensor(sorted(enc._special_tokens.values()), device=dev)] = True
stop_ids, skip_ids = torch.tensor([EOS], device=dev), torch.tensor([PAD], device=dev)
torch.cuda.synchronize()


def rows():
    r = core.decode_rows_device(ids.data_ptr(), R, W, W + PROMPT, dtype=np.int64, d_begin=d_begin.data_ptr(), stop=[EOS], skip=[PAD], skip_special=True)
    torch.cuda.synchronize()
    return r


def torch_rows():
    """The rule with torch calls (no id of this workload is without a token: the check for one is left out)."""
    from_begin = col[None, :] >= begin[:, None]
    is_stop = torch.isin(ids, stop_ids) & from_begin
    stop_col = torch.where(is_stop.any(1), is_stop.to(torch.uint8).argmax(1), W)
    live = from_begin & (col[None, :] < stop_col[:, None])
    keep = live & ~torch.isin(ids, skip_ids)
    keep &= ~is_special[ids.clamp(0, is_special.numel() - 1)]
    n_kept = keep.sum(1)
    tok_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(n_kept, 0)])
    return ids[keep].to(torch.int32), tok_off, n_kept.to(torch.int32), stop_col.to(torch.int32)


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


def kernel_ms_per_call(f, names):
    """Summed HIP-event time of the named kernels, call by call: (median, min, max) in ms and the per-kernel medians."""
    core.set_profiling(True)
    for _ in range(WARMUP):
        f()
    sums, per = [], {name: [] for name in names}
    for _ in range(REPS):
        core.reset_kernel_ms()
        f()
        for name in names:
            per[name].append(core.kernel_ms(name)[0])
        sums.append(sum(per[name][-1] for name in names))
    core.set_profiling(False)
    return (statistics.median(sums), min(sums), max(sums)), {name: statistics.median(v) for name, v in per.items()}


tag = f"decode_rows_path {mib} MiB, {R} x {W} int64, ld {W + PROMPT}"
r = rows()
K = r.n_tokens
say(f"{tag}: {R * W} ids -> {K} kept ids, {r.n_bytes} bytes of text")
# equal arrays first
want = torch_rows()
got = (view(r.tokens, K), view(r.tok_off, R + 1, "<i8"), view(r.n_kept, R), view(r.stop_col, R))
for name, g, w in zip(("tokens", "tok_off", "n_kept", "stop_col"), got, want):
    assert g.shape == w.shape and bool(torch.equal(g, w)), name
live = int((want[3].to(torch.int64) - begin).sum())
scanned = int((W - begin).sum())
say(f"{tag}: the hand-written path and the torch restatement give equal tokens, tok_off, n_kept and stop_col")
del want, got
tokens, tok_off = r.tokens, r.tok_off  # (the decode-rows buffers: a decode call leaves them alone)


def decode():
    out = core.decode_batch_device(tokens, K, tok_off, R)
    torch.cuda.synchronize()
    return out


t_rows = med(rows)
say(f"{tag}: tk_decode_rows_device (wall clock, new passes and decode passes, the call waits for the bytes): median {t_rows[0] * 1e3:.3f} ms "
    f"(min {t_rows[1] * 1e3:.3f}, max {t_rows[2] * 1e3:.3f})")
t_dec = med(decode)
say(f"{tag}: tk_decode_batch_device on the compact ids (wall clock): median {t_dec[0] * 1e3:.3f} ms (min {t_dec[1] * 1e3:.3f}, max {t_dec[2] * 1e3:.3f})")
t_torch = med(torch_rows)
say(f"{tag}: torch restatement of the new passes (wall clock, caching allocator warm): median {t_torch[0] * 1e3:.3f} ms (min {t_torch[1] * 1e3:.3f}, max {t_torch[2] * 1e3:.3f})")
torch.cuda.empty_cache()
(total, t_min, t_max), per = kernel_ms_per_call(rows, NEW + DECODE)
for name in NEW + DECODE:
    say(f"{tag}: {name}: median {per[name]:.4f} ms per call")
new_ms, dec_ms = sum(per[k] for k in NEW), sum(per[k] for k in DECODE)
tiles = R * max(1, -(-W // 2048))
rd = 8 * (scanned + 2 * live) + 8 * R * 3 + 16 * tiles
wr = 4 * K + 16 * R + 8 + 8 * tiles * 2 + 4 * R
rate = (rd + wr) / (new_ms * 1e-3)
say(f"{tag}: new kernels, summed (HIP events, {REPS} calls): median {new_ms:.4f} ms; decode kernels behind them {dec_ms:.4f} ms; algorithmic bytes of the new passes "
    f"{rd} read (the stop pass reads [begin, W), the count and the write pass the live range each) + {wr} written = {(rd + wr) / 1e6:.1f} MB -> {rate / 1e9:.0f} GB/s = "
    f"{rate / HBM_COPY:.2f} of the measured HBM copy rate ({HBM_COPY / 1e12:.2f} TB/s)")
wall_new = t_rows[0] - t_dec[0]
say(f"{tag}: new passes / decode step behind them = {new_ms / dec_ms:.3f} (kernels), {wall_new / t_dec[0]:.3f} (wall clock: the call's minus the decode call's, "
    f"{wall_new * 1e3:.3f} ms, over the decode call's)")
say(f"{tag}: new passes / torch restatement = {new_ms * 1e-3 / t_torch[0]:.3f} (kernels over its wall clock), {wall_new / t_torch[0]:.3f} (wall clock over wall clock)")
say(f"{tag}: if the share looks too high, next: count in the stop pass -- every tile counts up to its own first stop, and the scan drops the tiles behind the row's "
    f"stop -- which takes one of the three reads of the matrix away; then int64 rows staged through LDS so that misaligned rows load 16 bytes at a time too")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
