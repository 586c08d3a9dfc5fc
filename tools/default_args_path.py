#!/usr/bin/env python3
"""What the disallowed-special check costs, on one GPU, for the library $TIKTOKEN_AMD_LIB selects (default: the tree's build).

    python tools/default_args_path.py device [MiB]   tk_encode_batch_device against tk_encode_batch_device_checked (all specials disallowed, no hit)
    python tools/default_args_path.py host [MiB]     tk_encode_batch against tk_encode_batch_checked, host buffers in and out
    python tools/default_args_path.py python [MiB]   Encoding.encode_batch_packed(list[str]) with default arguments, split into pack / check /
                                                     encode: the per-text pack and host search (the form before the device check, restated
                                                     here) against today's pack and the checked call; the same for the ASCII texts alone

A library without the checked entry points (an older build) gives the unchecked figures only.  One line per figure; times are the
median of the runs after one warm-up, wall clock around calls that return when the work is done."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (first: its HIP runtime has to be the one that is loaded)

from bench import gen_corpus  # noqa: E402
from tiktoken_amd import Encoding, _lib  # noqa: E402
from tiktoken_ext import amd_shaped  # noqa: E402

what = sys.argv[1] if len(sys.argv) > 1 else "device"
mib = int(sys.argv[2]) if len(sys.argv) > 2 else (256 if what == "python" else 1024)
runs = 7
spec = amd_shaped.ENCODING_CONSTRUCTORS["o200k_shaped"]()
enc = Encoding("o200k_shaped_default_args", pat_str=spec["pat_str"], mergeable_ranks=spec["mergeable_ranks"], special_tokens=spec["special_tokens"])
core = enc._core_bpe
checked = hasattr(_lib.lib(), "tk_encode_batch_checked")
n = mib << 20
blob, off = gen_corpus(0x5EED0003, 1, n, 16)  # (the C3 generator)
blob = blob[:n]
nd = len(off) - 1
tag = f"{os.path.basename(os.environ.get('TIKTOKEN_AMD_LIB') or 'tree')} {what} {mib} MiB"


def med(f):
    f()
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def line(name, t):
    print(f"{tag}: {name}: median {t[0] * 1e3:.3f} ms (min {t[1] * 1e3:.3f}, max {t[2] * 1e3:.3f}), {n / t[0] / 1e9:.2f} GB/s", flush=True)


if what == "device":
    d_text = torch.zeros(n + 256, dtype=torch.uint8, device="cuda")
    d_text[:n] = torch.from_numpy(blob).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    torch.cuda.synchronize()

    def run(dis):
        core.encode_batch_device(d_text.data_ptr(), n, d_off.data_ptr(), off, nd, **({"disallowed_special": dis} if dis else {}))
        torch.cuda.synchronize()

    # interleaved: unchecked, checked, unchecked, checked
    for rep in range(2):
        line("tk_encode_batch_device", med(lambda: run(None)))
        if checked:
            line("tk_encode_batch_device_checked", med(lambda: run("all")))
    if checked:
        core.set_profiling(True)
        core.reset_kernel_ms()
        for _ in range(5):
            run("all")
        ms, k = core.kernel_ms("tk_k_spec_find")
        core.set_profiling(False)
        print(f"{tag}: tk_k_spec_find: {ms / k:.3f} ms per launch over {k} launches, {n / (ms / k * 1e-3) / 1e9:.0f} GB/s of text read", flush=True)
elif what == "host":
    for rep in range(2):
        line("tk_encode_batch", med(lambda: core.encode_batch_packed(blob, off)))
        if checked:
            line("tk_encode_batch_checked", med(lambda: core.encode_batch_packed(blob, off, disallowed_special="all")))
else:
    bb = blob.tobytes()
    texts = [bb[int(a):int(b)].decode("utf-8") for a, b in zip(off[:-1], off[1:])]
    del bb
    runs = 3
    dis = frozenset(enc.special_tokens_set)

    def _utf8(t):
        try:
            return t.encode("utf-8")
        except UnicodeEncodeError:
            return t.encode("utf-16", "surrogatepass").decode("utf-16", "replace").encode("utf-8")

    def old_pack():
        chunks = [_utf8(t) for t in texts]
        o = np.zeros(len(chunks) + 1, dtype=np.uint64)
        np.cumsum(np.fromiter((len(c) for c in chunks), dtype=np.uint64, count=len(chunks)), out=o[1:])
        return np.frombuffer(b"".join(chunks), dtype=np.uint8), o

    def host_check():
        for t in texts:
            enc._reject_disallowed(t, dis)

    pb, po = old_pack()
    line("before: pack (an encode per text)", med(old_pack))
    line("before: check (host search per text)", med(host_check))
    line("before: encode (unchecked call)", med(lambda: core.encode_batch_packed(pb, po, set())))
    line("after: pack (Encoding._pack_repaired)", med(lambda: enc._pack_repaired(texts)))
    if checked:
        line("after: check + encode (checked call)", med(lambda: core.encode_batch_packed(pb, po, set(), disallowed_special=dis)))
        before = core.stat("spec_find_launches")
        line("after: Encoding.encode_batch_packed(texts), default arguments", med(lambda: enc.encode_batch_packed(texts)))
        assert core.stat("spec_find_launches") > before
    # the same documents with every non-ASCII char dropped
    texts = [t.encode("ascii", "ignore").decode("ascii") for t in texts]
    n = sum(map(len, texts))
    tag += " (ASCII only)"
    line("before: pack (an encode per text)", med(old_pack))
    line("after: pack (Encoding._pack_repaired)", med(lambda: enc._pack_repaired(texts)))
