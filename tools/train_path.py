#!/usr/bin/env python3
"""BPE training (tk_train_bpe) on the bench corpus under the o200k pattern: wall time to 8 192 and to 32 768 tokens, split into
pre-tokenise, word table (+ one step) and merge loop; per-kernel times of a short profiled run (tk_get_kernel_ms); beside it the
HuggingFace `tokenizers` BpeTrainer on the same pieces (its tie rule differs: time only) and the Python restatement of the rule
(tests/train_ref.py) on the largest prefix it finishes within --ref-seconds.

Usage: python tools/train_path.py [--mib 64] [--sizes 8192 32768] [--profile-merges 256] [--ref-seconds 60] [--no-tokenizers]
"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from bench import gen_corpus
from tiktoken_amd._tiktoken import CoreBPE
from tiktoken_ext import openai_public as pub

KERNELS = ["tk_k_front", "tk_k_train_tab_init", "tk_k_train_words", "tk_k_train_blob", "tk_k_train_rehash", "tk_k_train_expand", "tk_train_pair_clear",
           "tk_k_train_count", "tk_k_train_best", "tk_k_train_pick", "tk_k_train_breaks", "tk_k_train_carry", "tk_k_train_decide", "tk_k_train_offsets",
           "tk_k_train_rewrite"]

ap = argparse.ArgumentParser()
ap.add_argument("--mib", type=int, default=64)
ap.add_argument("--sizes", type=int, nargs="*", default=[8192, 32768])
ap.add_argument("--profile-merges", type=int, default=256)
ap.add_argument("--ref-seconds", type=float, default=60.0)
ap.add_argument("--no-tokenizers", action="store_true")
a = ap.parse_args()

pat = pub.o200k_pat_str
core = CoreBPE({bytes([b]): b for b in range(256)}, {}, pat)
blob, off = gen_corpus(0x5EED0003, 1, a.mib << 20, 16)
n = int(off[-1])
blob = blob[:n]
res = {"bytes": n, "docs": len(off) - 1, "pat_str": "o200k"}


def wall(f):
    t0 = time.perf_counter()
    r = f()
    return time.perf_counter() - t0, r


core.train_bpe_packed(blob[: 1 << 20], np.array([0, 1 << 20], dtype=np.uint64), 260)  # warm-up: buffers, code objects
t_pre, starts = wall(lambda: core.pretokenize_packed(blob, off))
res["pieces"] = len(starts) - 1
res["pretokenize_s"] = t_pre
t_one, _ = wall(lambda: core.train_bpe_packed(blob, off, 257))
res["pretokenize_word_table_one_step_s"] = t_one
for size in a.sizes:
    t, (pairs, counts) = wall(lambda: core.train_bpe_packed(blob, off, size))
    res[f"train_{size}_s"] = t
    res[f"merge_loop_{size}_s"] = t - t_one
    res[f"last_count_{size}"] = int(counts[-1])
    print(f"vocab {size}: {t:.2f} s in all, {t - t_one:.2f} s merge loop = {(t - t_one) / (size - 256) * 1e3:.3f} ms per merge", flush=True)
core.set_profiling(True)
core.reset_kernel_ms()
core.train_bpe_packed(blob, off, 256 + a.profile_merges)
core.set_profiling(False)
res["profiled_merges"] = a.profile_merges
res["kernel_ms"] = {k: {"ms": round(ms, 3), "launches": ln} for k in KERNELS for ms, ln in [core.kernel_ms(k)] if ln}
for k, v in res["kernel_ms"].items():
    print(f"  {k}: {v['ms']:.2f} ms in {v['launches']} launches", flush=True)

if not a.no_tokenizers:
    try:
        import tokenizers
        from tokenizers import Tokenizer, models, trainers

        os.environ.setdefault("RAYON_NUM_THREADS", "16")
        raw = blob.tobytes()
        b2u = {}  # bytes -> printable chars, one char per byte (what a byte-level pre-tokeniser feeds the trainer)
        for b in range(256):
            b2u[b] = chr(b) if 33 <= b < 127 else chr(256 + b)
        table = "".join(b2u[b] for b in range(256))
        st = starts.tolist()
        t_prep, pieces = wall(lambda: [raw[x:y].decode("latin-1").translate({i: ord(c) for i, c in enumerate(table)}) for x, y in zip(st[:-1], st[1:])])
        for size in a.sizes:
            tok = Tokenizer(models.BPE())
            trainer = trainers.BpeTrainer(vocab_size=size, initial_alphabet=list(table), show_progress=False)
            t, _ = wall(lambda: tok.train_from_iterator(pieces, trainer=trainer))
            res[f"tokenizers_{size}_s"] = t
            print(f"tokenizers {tokenizers.__version__} BpeTrainer, vocab {size}: {t:.2f} s (+ {t_prep:.1f} s to hand it the pieces)", flush=True)
        res["tokenizers_version"] = tokenizers.__version__
    except ImportError as e:
        res["tokenizers"] = f"not installed: {e}"

if a.ref_seconds > 0:
    import train_ref as tr

    size, kb, last = a.sizes[0] if a.sizes else 8192, 64, None
    while kb << 10 <= n:
        cut = int(off[np.searchsorted(off, kb << 10, side="right") - 1]) or (kb << 10)
        text = blob[:cut].tobytes().decode("utf-8", "ignore")
        try:
            t, _ = wall(lambda: tr.train_text(text, size, pat))
        except ValueError:
            t = None
        if t is None or t > a.ref_seconds:
            break
        last = (cut, t)
        kb *= 2 if t < a.ref_seconds / 4 else 10**9
    if last:
        res["train_ref_bytes"], res["train_ref_s"], res["train_ref_vocab"] = last[0], last[1], size
        print(f"train_ref: {last[0]} bytes to {size} tokens in {last[1]:.1f} s", flush=True)
print(json.dumps(res), flush=True)
