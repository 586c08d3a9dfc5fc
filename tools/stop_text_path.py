#!/usr/bin/env python3
"""What stop strings on the device cost on one GPU.

    python tools/stop_text_path.py [MiB] [ROWS] [COLUMNS] [--out FILE]
    (default: 256 MiB of the bench corpus, 4096 rows of 2048 columns; FILE: profiles/stop_text_path.txt)

(a) Clean text, no hit: MiB of the bench corpus, o200k-shaped, encoded and decoded device-resident, with the four stop strings "\\n\\n",
    "Question:", "</s>" and "###" broken wherever the corpus holds one (the last byte of every match replaced: the first bytes, the
    candidates of the search, stay).  tk_stop_text_device beside tk_utf8_repair_device on the same buffer: both are one read pass and
    no write.
(b) Rows: the case of tools/decode_rows_path.py -- an int64 matrix, a slice of a wider one, a random begin and one stop id per row, pad
    behind it -- with one of the four strings planted in every row's live range as byte-level ids: decode_rows_until_device
    (errors="replace") beside tk_decode_rows_text_device alone, and beside the host route it replaces: text and offsets copied to the
    host, find per row and per string, a slice.
Every figure is the median of 20 calls after 3 warm-up calls, with the least and the most.  (The encode benchmark beside the parent's
library is bench.py's own run; its figures are appended to the file by hand.)"""
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
out_path = os.path.join(ROOT, "profiles", "stop_text_path.txt")
if "--out" in args:
    at = args.index("--out")
    out_path = args[at + 1]
    del args[at: at + 2]
mib, R, W = (int(args[i]) if len(args) > i else d for i, d in enumerate((256, 4096, 2048)))
PROMPT = 64
WARMUP, REPS = 3, 20
STOPS = ["\n\n", "Question:", "</s>", "###"]
STOPS_B = [s.encode() for s in STOPS]
FIND = ("tk_k_u8r_check", "tk_k_stops_find", "tk_k_stops_rows", "tk_k_stops_scan", "tk_k_stops_docs", "tk_k_stops_cut", "tk_k_stops_ntok")
REPAIR = ("tk_k_span_mark", "tk_k_u8r_count", "tk_k_u8r_scan", "tk_k_u8r_docs", "tk_k_u8r_write")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


spec = amd_shaped.ENCODING_CONSTRUCTORS["o200k_shaped"]()
enc = Encoding("o200k_shaped_stop_text_path", pat_str=spec["pat_str"], mergeable_ranks=spec["mergeable_ranks"], special_tokens=spec["special_tokens"])
core = enc._core_bpe
EOS, PAD = enc.eot_token, enc.max_token_value + 1000
dev = torch.device("cuda")


class _Dev:
    def __init__(self, ptr, count, typestr):
        self.__cuda_array_interface__ = {"shape": (count,), "typestr": typestr, "data": (ptr, False), "version": 2}


def view(ptr, count, typestr="<i4"):
    return torch.as_tensor(_Dev(ptr, count, typestr), device=dev) if count else torch.zeros(0, dtype=torch.int32, device=dev)


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


def kernel_ms_per_call(f, names, reps=REPS):
    core.set_profiling(True)
    for _ in range(WARMUP):
        f()
    per = {name: [] for name in names}
    for _ in range(reps):
        core.reset_kernel_ms()
        f()
        for name in names:
            per[name].append(core.kernel_ms(name)[0])
    core.set_profiling(False)
    return {name: statistics.median(v) for name, v in per.items()}


def ms(t):
    return f"median {t[0] * 1e3:.3f} ms (min {t[1] * 1e3:.3f}, max {t[2] * 1e3:.3f})"


# ---------------------------------------------------------------- (a) clean text, no hit
n = mib << 20
blob, off = gen_corpus(0x5EED0003, 1, n, 16)  # (the bench's corpus)
blob = blob[:n]
n_docs = len(off) - 1
d_text = torch.zeros(n + 256, dtype=torch.uint8, device=dev)
d_text[:n] = torch.from_numpy(blob).cuda()
d_off = torch.from_numpy(off.view(np.int64)).cuda()
torch.cuda.synchronize()
dt, nt, dto = core.encode_batch_device(d_text.data_ptr(), n, d_off.data_ptr(), off, n_docs)
ids_all = view(dt, nt).clone()
tok_off_all = view(dto, n_docs + 1, "<i8").clone()
torch.cuda.synchronize()
db, nb, dbo = core.decode_batch_device(ids_all.data_ptr(), nt, tok_off_all.data_ptr(), n_docs)
assert nb == n
clean = torch.zeros(n + 256, dtype=torch.uint8, device=dev)  # (torch allocations are aligned well beyond 16 bytes)
clean[:n] = view(db, nb, "|u1")
clean_off = view(dbo, n_docs + 1, "<i8").clone()
broken = 0
for s, alt in zip(STOPS_B, b" ;)+"):
    m = torch.ones(n - len(s) + 1, dtype=torch.bool, device=dev)
    for j, b in enumerate(s):
        m &= clean[j: j + n - len(s) + 1] == b
    at = m.nonzero().flatten()
    broken += int(at.numel())
    clean[at + len(s) - 1] = alt
    del m, at
torch.cuda.synchronize()
tag = f"stop_text_path (a) {mib} MiB of decoded bench corpus, {n_docs} documents, 4 stop strings, no hit ({broken} matches of the corpus broken at their last byte)"


def stop_clean():
    return core.stop_text_device(clean.data_ptr(), n, clean_off.data_ptr(), n_docs, STOPS)


def repair_clean():
    return core.utf8_repair_device(clean.data_ptr(), n, clean_off.data_ptr(), n_docs, "replace")


r = stop_clean()
assert r.n_hit == 0 and r.data == clean.data_ptr() and r.n_bytes == n
assert repair_clean().n_replaced == 0
t_stop, t_rep = med(stop_clean), med(repair_clean)
per_s, per_r = kernel_ms_per_call(stop_clean, FIND), kernel_ms_per_call(repair_clean, ("tk_k_u8r_check",) + REPAIR)
say(f"{tag}: tk_stop_text_device (wall clock, the call waits): {ms(t_stop)}; tk_utf8_repair_device on the same buffer: {ms(t_rep)}; ratio {t_stop[0] / t_rep[0]:.2f}")
for name in FIND[:5]:
    say(f"{tag}: {name}: median {per_s[name]:.4f} ms per call")
say(f"{tag}: tk_k_u8r_count (the repair's read pass): median {per_r['tk_k_u8r_count']:.4f} ms per call; tk_k_stops_find / tk_k_u8r_count = "
    f"{per_s['tk_k_stops_find'] / per_r['tk_k_u8r_count']:.2f}; the find pass reads {n / 1e6:.0f} MB: {n / (per_s['tk_k_stops_find'] * 1e-3) / 1e9:.0f} GB/s")
del clean, clean_off

# ---------------------------------------------------------------- (b) rows, a hit in every row
assert nt >= R * W, f"{mib} MiB give {nt} ids: fewer than {R} x {W}"
gen = torch.Generator(device=dev)
gen.manual_seed(0x5EED)
wide = torch.full((R, W + PROMPT), PAD, dtype=torch.int64, device=dev)
ids = wide[:, PROMPT:]
ids.copy_(ids_all[: R * W].to(torch.int64).reshape(R, W))
begin = torch.randint(0, max(W // 4, 1), (R,), device=dev, generator=gen)
stop_at = begin + torch.randint(16, W - W // 4, (R,), device=dev, generator=gen)
col = torch.arange(W, device=dev)
ids[col[None, :] == stop_at[:, None]] = EOS
ids[col[None, :] > stop_at[:, None]] = PAD
plant = begin + torch.div((stop_at - begin - 12) * torch.randint(0, 1000, (R,), device=dev, generator=gen), 1000, rounding_mode="floor")
rows = torch.arange(R, device=dev)
for k, s in enumerate(STOPS_B):
    sel = rows[rows % len(STOPS_B) == k]
    for j, b in enumerate(s):
        ids[sel, plant[sel] + j] = enc._mergeable_ranks[bytes([b])]
d_begin = begin.to(torch.int32).contiguous()
torch.cuda.synchronize()
tag = f"stop_text_path (b) {R} x {W} int64, ld {W + PROMPT}"
KW = dict(dtype=np.int64, d_begin=d_begin.data_ptr(), stop=[EOS], skip=[PAD], skip_special=True)


def rows_until():
    return core.decode_rows_until_device(ids.data_ptr(), R, W, W + PROMPT, stop_text=STOPS, errors="replace", **KW)


def rows_text():
    return core.decode_rows_text_device(ids.data_ptr(), R, W, W + PROMPT, errors="replace", **KW)


def host_route():
    t = rows_text()
    data = view(t.data, t.n_bytes, "|u1").cpu().numpy().tobytes()
    bounds = view(t.byte_off, R + 1, "<i8").cpu().numpy().tolist()
    out = []
    for a, b in zip(bounds[:-1], bounds[1:]):
        cut = b
        for s in STOPS_B:
            p = data.find(s, a, cut)
            if p >= 0:
                cut = p
        out.append(data[a:cut])
    return out


r = rows_until()
say(f"{tag}: {r.n_tokens} kept ids, {r.n_bytes} bytes of text kept, a hit in {r.n_hit} of {R} rows")
assert r.n_hit == R
got = view(r.data, r.n_bytes, "|u1").cpu().numpy().tobytes()
assert got == b"".join(host_route())
say(f"{tag}: the cut text equals the host route's, byte for byte")
t_until, t_text, t_host = med(rows_until), med(rows_text), med(host_route)
per = kernel_ms_per_call(rows_until, FIND + REPAIR)
say(f"{tag}: decode_rows_until_device (wall clock): {ms(t_until)}; tk_decode_rows_text_device alone: {ms(t_text)}; the stop strings add {(t_until[0] - t_text[0]) * 1e3:.3f} ms")
for name in FIND + REPAIR:
    say(f"{tag}: {name}: median {per[name]:.4f} ms per call")
say(f"{tag}: the host route (tk_decode_rows_text_device, text and offsets copied to the host, find per row and per string, a slice): {ms(t_host)}; "
    f"without its device call {(t_host[0] - t_text[0]) * 1e3:.3f} ms; device route / host route = {t_until[0] / t_host[0]:.3f}")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
