#!/usr/bin/env python3
"""What UTF-8 repair on the device costs on one GPU.

    python tools/utf8_repair_path.py [MiB] [ROWS] [COLUMNS] [WORST_MiB] [--out FILE]
    (default: 256 MiB of the bench corpus, 4096 rows of 2048 columns, 64 MiB of 0x80; FILE: profiles/utf8_repair_path.txt)

(a) Clean text: MiB of the bench corpus, o200k-shaped, encoded and decoded device-resident; tk_utf8_repair_device over the decoded bytes
    (nothing is replaced: the count pass, the scan and the per-document pass run, no write pass) beside tk_k_utf8_docs, the strict check,
    alone on the same bytes (timed inside tk_decode_batch_spans with validate on).
(b) Rows: the case of tools/decode_rows_path.py -- an int64 matrix, a slice of a wider one, a random begin and one stop per row, pad behind
    it -- with byte-level ids of multi-byte chars mixed in, so that begin and the stop cut chars: tk_decode_rows_text_device, its repair
    kernels beside the decode kernels behind them, and beside the host loop str(view[a:b], "utf-8", "replace") over the same rows (time only:
    that loop also makes the str objects).
(c) The worst case: WORST_MiB of 0x80 in one document, three-fold growth, for the write pass's rate.
Every figure is the median of 20 calls after 3 warm-up calls, with the least and the most."""
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
out_path = os.path.join(ROOT, "profiles", "utf8_repair_path.txt")
if "--out" in args:
    at = args.index("--out")
    out_path = args[at + 1]
    del args[at: at + 2]
mib, R, W, worst_mib = (int(args[i]) if len(args) > i else d for i, d in enumerate((256, 4096, 2048, 64)))
PROMPT = 64
WARMUP, REPS = 3, 20
REPAIR = ("tk_k_u8r_check", "tk_k_span_mark", "tk_k_u8r_count", "tk_k_u8r_scan", "tk_k_u8r_docs", "tk_k_u8r_write")
DECODE = ("tk_k_dec_len", "tk_k_dec_copy")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


spec = amd_shaped.ENCODING_CONSTRUCTORS["o200k_shaped"]()
enc = Encoding("o200k_shaped_utf8_repair_path", pat_str=spec["pat_str"], mergeable_ranks=spec["mergeable_ranks"], special_tokens=spec["special_tokens"])
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


# ---------------------------------------------------------------- (a) clean text
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
tag = f"utf8_repair_path (a) {mib} MiB of decoded bench corpus, {n_docs} documents, clean"


def repair_clean():
    return core.utf8_repair_device(db, nb, dbo, n_docs, "replace")


r = repair_clean()
assert r.n_replaced == 0 and r.data == db and r.n_bytes == n
t_a = med(repair_clean)
per = kernel_ms_per_call(repair_clean, REPAIR)
assert per["tk_k_u8r_write"] == 0
rep_ms = sum(per.values())
say(f"{tag}: tk_utf8_repair_device (wall clock, the call waits): {ms(t_a)}; no write pass")
for name in REPAIR:
    say(f"{tag}: {name}: median {per[name]:.4f} ms per call")
h_ids, h_tok_off = ids_all.cpu().numpy().view(np.uint32), tok_off_all.cpu().numpy().astype(np.uint64)


def strict():
    return core.decode_batch_spans_packed(h_ids, h_tok_off, want_bytes=False, validate=True)


strict_ms = kernel_ms_per_call(strict, ("tk_k_utf8_docs",), reps=5)["tk_k_utf8_docs"]
say(f"{tag}: tk_k_utf8_docs alone on the same bytes: median {strict_ms:.4f} ms; tk_k_u8r_count / tk_k_utf8_docs = {per['tk_k_u8r_count'] / strict_ms:.2f}, "
    f"all repair kernels / tk_k_utf8_docs = {rep_ms / strict_ms:.2f}; the count pass reads {n / 1e6:.0f} MB and writes {n / 8 / 1e6:.0f} MB of lane places: "
    f"{(n + n / 8) / (per['tk_k_u8r_count'] * 1e-3) / 1e9:.0f} GB/s")
del h_ids, h_tok_off

# ---------------------------------------------------------------- (b) rows
assert nt >= R * W, f"{mib} MiB give {nt} ids: fewer than {R} x {W}"
gen = torch.Generator(device=dev)
gen.manual_seed(0x5EED)
wide = torch.full((R, W + PROMPT), PAD, dtype=torch.int64, device=dev)
ids = wide[:, PROMPT:]
ids.copy_(ids_all[: R * W].to(torch.int64).reshape(R, W))
# byte-level ids mixed in: every 16th group of four columns spells U+1F600 with the ids of its four bytes
smile = torch.tensor([enc._mergeable_ranks[bytes([b])] for b in "😀".encode()], dtype=torch.int64, device=dev)
ids.view(R, W // 4, 4)[:, ::16, :] = smile
begin = torch.randint(0, max(W // 4, 1), (R,), device=dev, generator=gen)
stop_at = begin + torch.randint(0, W - W // 4, (R,), device=dev, generator=gen)
col = torch.arange(W, device=dev)
ids[col[None, :] == stop_at[:, None]] = EOS
ids[col[None, :] > stop_at[:, None]] = PAD
d_begin = begin.to(torch.int32).contiguous()
torch.cuda.synchronize()
tag = f"utf8_repair_path (b) {R} x {W} int64, ld {W + PROMPT}"


def rows_text():
    return core.decode_rows_text_device(ids.data_ptr(), R, W, W + PROMPT, dtype=np.int64, d_begin=d_begin.data_ptr(), stop=[EOS], skip=[PAD], skip_special=True)


def rows_bytes():
    return core.decode_rows_device(ids.data_ptr(), R, W, W + PROMPT, dtype=np.int64, d_begin=d_begin.data_ptr(), stop=[EOS], skip=[PAD], skip_special=True)


r = rows_text()
repl = view(r.repl_off, R + 1, "<i8").cpu().numpy()
cut_rows = int((np.diff(repl) > 0).sum())
say(f"{tag}: {r.n_tokens} kept ids, {r.n_bytes} bytes of text, {r.n_replaced} units replaced in {cut_rows} of {R} rows ({cut_rows / R:.2f})")
rb = rows_bytes()
data = view(rb.data, rb.n_bytes, "|u1").cpu().numpy()
bounds = view(rb.byte_off, R + 1, "<i8").cpu().numpy().tolist()
mv = memoryview(data)
want = "".join(str(mv[a:b], "utf-8", "replace") for a, b in zip(bounds[:-1], bounds[1:])).encode()
assert bytes(view(r.data, r.n_bytes, "|u1").cpu().numpy()) == want
say(f"{tag}: the repaired text equals the host loop's, byte for byte")
t_text, t_bytes = med(rows_text), med(rows_bytes)


def host_loop():
    return [str(mv[a:b], "utf-8", "replace") for a, b in zip(bounds[:-1], bounds[1:])]


t_host = med(host_loop)
per = kernel_ms_per_call(rows_text, REPAIR + DECODE)
rep_ms, dec_ms = sum(per[k] for k in REPAIR), sum(per[k] for k in DECODE)
say(f"{tag}: tk_decode_rows_text_device (wall clock): {ms(t_text)}; tk_decode_rows_device: {ms(t_bytes)}; the repair adds {(t_text[0] - t_bytes[0]) * 1e3:.3f} ms")
for name in REPAIR + DECODE:
    say(f"{tag}: {name}: median {per[name]:.4f} ms per call")
say(f"{tag}: repair kernels {rep_ms:.4f} ms / decode kernels behind them {dec_ms:.4f} ms = {rep_ms / dec_ms:.2f}")
say(f"{tag}: host loop str(view[a:b], 'utf-8', 'replace') over the same rows, bytes already on the host: {ms(t_host)} (it also makes the str objects: time only); "
    f"repair by wall clock / host loop = {(t_text[0] - t_bytes[0]) / t_host[0]:.3f}")

# ---------------------------------------------------------------- (c) the worst case
wn = worst_mib << 20
bad = torch.full((wn + 16,), 0x80, dtype=torch.uint8, device=dev)
bad_off = torch.tensor([0, wn], dtype=torch.int64, device=dev)
torch.cuda.synchronize()
tag = f"utf8_repair_path (c) {worst_mib} MiB of 0x80, one document"


def worst():
    return core.utf8_repair_device(bad.data_ptr(), wn, bad_off.data_ptr(), 1, "replace")


r = worst()
assert r.n_bytes == 3 * wn and r.n_replaced == wn
t_c = med(worst)
per = kernel_ms_per_call(worst, REPAIR)
say(f"{tag}: tk_utf8_repair_device (wall clock): {ms(t_c)}")
for name in REPAIR:
    say(f"{tag}: {name}: median {per[name]:.4f} ms per call")
say(f"{tag}: write pass: {wn / 1e6:.0f} MB read, {3 * wn / 1e6:.0f} MB written: {4 * wn / (per['tk_k_u8r_write'] * 1e-3) / 1e9:.0f} GB/s; "
    f"count pass {wn / (per['tk_k_u8r_count'] * 1e-3) / 1e9:.0f} GB/s of input (every lane takes the step, none the ASCII shortcut)")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
