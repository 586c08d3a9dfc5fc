#!/usr/bin/env python3
"""What near-duplicate grouping and the selection of the kept documents cost on one GPU, beside the steps before them and beside the host
route they replace.

    python tools/groups_path.py [MiB]      (default: 256 MiB of the bench corpus, o200k-shaped; k = 5, P = 128, B = 16, threshold 0.8)

Three batches of the same number of documents: the corpus as it is; the corpus with SHARE of its documents replaced by an exact copy of
an earlier document; the same with EDITS ids of every such copy changed.  Per batch: tk_fingerprint_groups_device and
tk_select_docs_device (wall clock around the call and a synchronise of its stream) and each of their kernels from HIP events
(tk_get_kernel_ms); the host route on the same arrays -- Fingerprints.duplicate_groups, then numpy filtering of the ids copied out --,
timed once; the check that the device result equals the host route's, made before anything is timed.  For scale, on the first batch: the
encode step and tk_fingerprint_device.  Last, the batch in which every document is the first one: the contended slots.  Every device
figure is the median of 10 calls after 2 warm-up calls."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (first: its HIP runtime has to be the one that is loaded)

from bench import gen_corpus  # noqa: E402
from tiktoken_amd import Encoding, Fingerprints  # noqa: E402
from tiktoken_ext import amd_shaped  # noqa: E402

mib = int(sys.argv[1]) if len(sys.argv) > 1 else 256
WARMUP, REPS = 2, 10
K, P, B, SEED, TH = 5, 128, 16, 0, 0.8
SHARE, EDITS = 0.2, 4
GRP_KERNELS = ("tk_k_grp_clear", "tk_k_grp_claim", "tk_k_grp_join", "tk_k_grp_flat")
SEL_KERNELS = ("tk_k_sel_count", "tk_k_sel_scan", "tk_k_sel_place", "tk_k_sel_copy")

spec = amd_shaped.ENCODING_CONSTRUCTORS["o200k_shaped"]()
enc = Encoding("o200k_shaped_groups_path", pat_str=spec["pat_str"], mergeable_ranks=spec["mergeable_ranks"], special_tokens=spec["special_tokens"])
core = enc._core_bpe
dev = torch.device("cuda", core.device)


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


def ms(t):
    return f"median {t[0] * 1e3:.3f} ms (min {t[1] * 1e3:.3f}, max {t[2] * 1e3:.3f})"


def kernels(f, names):
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
    return ", ".join(f"{name} {statistics.median(v):.4f}" for name, v in per.items())


def up(a, as_type):
    return torch.from_numpy(np.ascontiguousarray(a).view(as_type).copy()).to(dev)


n = mib << 20
blob, off = gen_corpus(0x5EED0003, 1, n, 16)  # (the bench's corpus)
blob, off = np.ascontiguousarray(blob[:int(off[-1])]), np.ascontiguousarray(off, dtype=np.uint64)
n_docs = len(off) - 1
d_text, d_doc_off = torch.from_numpy(blob).to(dev), torch.from_numpy(off.view(np.int64)).to(dev)
torch.cuda.synchronize()
t_enc = med(lambda: core.encode_batch_device(d_text.data_ptr(), len(blob), d_doc_off.data_ptr(), off, n_docs))
tok0, off0 = core.encode_batch_packed(blob, off, None)
print(f"groups_path {mib} MiB: {n_docs} documents, {len(tok0)} ids; k = {K}, P = {P}, B = {B}, threshold {TH}", flush=True)
print(f"groups_path {mib} MiB: encode step (tk_encode_batch_device, wall clock): {ms(t_enc)}", flush=True)


def repeated(edits):
    """SHARE of the documents replaced by a copy of an earlier one, `edits` ids of the copy changed"""
    rng = np.random.default_rng(7)
    src = np.arange(n_docs)
    picks = rng.choice(np.arange(1, n_docs), int(SHARE * n_docs), replace=False)
    src[picks] = (rng.random(len(picks)) * picks).astype(np.int64)  # (an earlier document, possibly a copy itself: its source then)
    src[picks] = np.where(np.isin(src[picks], picks), 0, src[picks])
    docs = [tok0[int(off0[s]):int(off0[s + 1])] for s in src]
    for d in picks if edits else ():
        if len(docs[d]) > 8 * edits:
            docs[d] = docs[d].copy()
            docs[d][rng.integers(0, len(docs[d]), edits)] ^= np.uint32(1)
    lens = np.array([len(x) for x in docs], dtype=np.uint64)
    return np.concatenate(docs), np.concatenate([np.zeros(1, np.uint64), np.cumsum(lens, dtype=np.uint64)])


def run(tag, tok, tok_off, scale=False):
    tag = f"groups_path {mib} MiB, {tag}"
    T = len(tok)
    d_tok, d_off = up(tok, np.int32), up(tok_off, np.int64)
    sig, band = torch.empty((n_docs, P), dtype=torch.int32, device=dev), torch.empty((n_docs, B), dtype=torch.int64, device=dev)
    nsh = torch.empty(n_docs, dtype=torch.int64, device=dev)
    group, keep, n_kept = torch.empty(n_docs, dtype=torch.int32, device=dev), torch.empty(n_docs, dtype=torch.uint8, device=dev), torch.empty(1, dtype=torch.int64, device=dev)
    o_tok, o_off = torch.empty(T, dtype=torch.int32, device=dev), torch.empty(n_docs + 1, dtype=torch.int64, device=dev)
    o_doc, o_cnt = torch.empty(n_docs, dtype=torch.int32, device=dev), torch.empty(2, dtype=torch.int64, device=dev)

    def fingerprint():
        core.fingerprint_device(d_tok, d_off, ngram=K, n_perm=P, bands=B, seed=SEED, sig=sig.view(-1), band=band.view(-1), n_shingles=nsh)

    def groups():
        core.fingerprint_groups_device(sig, band, nsh, TH, group=group, keep=keep, n_kept=n_kept)

    def select():
        core.select_docs_device(d_tok, d_off, keep, tokens_out=o_tok, tok_off_out=o_off, doc_out=o_doc, counts_out=o_cnt)

    fingerprint(), groups(), select()
    torch.cuda.synchronize()
    fp = Fingerprints(sig.cpu().numpy().view(np.uint32), band.cpu().numpy().view(np.uint64), np.zeros(n_docs, np.uint64), nsh.cpu().numpy().view(np.uint64), np.diff(tok_off))
    t0 = time.perf_counter()
    want = fp.duplicate_groups(TH)
    t_groups = time.perf_counter() - t0
    t0 = time.perf_counter()
    kept = np.flatnonzero(want == np.arange(n_docs))
    want_off = np.concatenate([np.zeros(1, np.uint64), np.cumsum(np.diff(tok_off)[kept], dtype=np.uint64)])
    want_tok = tok[np.repeat(tok_off[kept] - want_off[:-1], np.diff(tok_off)[kept].astype(np.int64)) + np.arange(int(want_off[-1]), dtype=np.uint64)]
    t_filter = time.perf_counter() - t0
    cnt = o_cnt.cpu().numpy()
    assert np.array_equal(group.cpu().numpy().view(np.uint32), want) and int(n_kept.cpu()) == len(kept) == int(cnt[0]) and int(cnt[1]) == len(want_tok)
    assert np.array_equal(o_doc.cpu().numpy()[:len(kept)], kept) and np.array_equal(o_off.cpu().numpy().view(np.uint64)[:len(kept) + 1], want_off)
    assert np.array_equal(o_tok.cpu().numpy().view(np.uint32)[:len(want_tok)], want_tok)
    print(f"{tag}: {T} ids; kept {len(kept)} of {n_docs} documents, {len(want_tok)} ids; the device result equals the host route's", flush=True)
    if scale:
        print(f"{tag}: tk_fingerprint_device (wall clock, call and synchronise): {ms(med(fingerprint))}", flush=True)
    t_g, t_s = med(groups), med(select)
    print(f"{tag}: tk_fingerprint_groups_device (wall clock, call and synchronise): {ms(t_g)}", flush=True)
    print(f"{tag}: its kernels, ms per call: {kernels(groups, GRP_KERNELS)}", flush=True)
    print(f"{tag}: tk_select_docs_device (wall clock, call and synchronise): {ms(t_s)} = {2 * len(want_tok) * 4 / t_s[0] / 1e9:.0f} GB/s of kept ids read and written",
          flush=True)
    print(f"{tag}: its kernels, ms per call: {kernels(select, SEL_KERNELS)}", flush=True)
    print(f"{tag}: host route: duplicate_groups {t_groups:.2f} s, numpy filtering of the ids {t_filter:.2f} s; host / device = {(t_groups + t_filter) / (t_g[0] + t_s[0]):.0f}x",
          flush=True)
    return sig, band, nsh


first = run("as it is", tok0, off0, scale=True)
run(f"{SHARE:.0%} exact copies", *repeated(0))
run(f"{SHARE:.0%} copies with {EDITS} ids changed", *repeated(EDITS))
sig, band, nsh = (t[:1].expand(n_docs, *t.shape[1:]).contiguous() for t in first)
group, n_kept = torch.empty(n_docs, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int64, device=dev)


def identical():
    core.fingerprint_groups_device(sig, band, nsh, TH, group=group, n_kept=n_kept)


identical()
assert int(n_kept.cpu()) == 1 and not group.cpu().numpy().any()
print(f"groups_path {mib} MiB, {n_docs} identical documents: one group; tk_fingerprint_groups_device: {ms(med(identical))}", flush=True)
print(f"groups_path {mib} MiB, {n_docs} identical documents: its kernels, ms per call: {kernels(identical, GRP_KERNELS)}", flush=True)
