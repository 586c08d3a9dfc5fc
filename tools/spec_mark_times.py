#!/usr/bin/env python3
"""C5 (o200k + 8 custom special tokens, 256 MiB of web text, allowed_special="all"): the durations of tk_k_spec_cand and tk_k_spec_resolve
from the library's own event timers (the ones bench.py --full and tools/bench_configs.py read), three profiled passes behind two warm-up
passes.  One JSON line per pass.  $TIKTOKEN_AMD_LIB names another build of the library (the parent's, for a comparison);
usage: python tools/spec_mark_times.py [label]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch

    import helpers as h
    from tiktoken_amd._tiktoken import CoreBPE
    from tiktoken_ext import amd_shaped

    label = sys.argv[1] if len(sys.argv) > 1 else "this"
    _, _, _, blob, off, allowed = h.baseline_config("C5")
    spec = amd_shaped.ENCODING_CONSTRUCTORS["o200k_custom8"]()
    core = CoreBPE(spec["mergeable_ranks"], spec["special_tokens"], spec["pat_str"])
    n, nd = len(blob), len(off) - 1
    host = np.zeros(n + 64, np.uint8)
    host[:n] = blob
    d_text = torch.from_numpy(host).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    for _ in range(2):
        core.encode_batch_device(d_text.data_ptr(), n, d_off.data_ptr(), off, nd, allowed)
    torch.cuda.synchronize()
    for run in range(3):
        core.set_profiling(True)
        core.reset_kernel_ms()
        _, nt, _ = core.encode_batch_device(d_text.data_ptr(), n, d_off.data_ptr(), off, nd, allowed)
        torch.cuda.synchronize()
        core.set_profiling(False)
        print(json.dumps({"lib": label, "run": run, "bytes": n, "tokens": int(nt),
                          **{k: round(core.kernel_ms(k)[0], 4) for k in ("tk_k_spec_cand", "tk_k_spec_resolve", "tk_k_front")}}), flush=True)


if __name__ == "__main__":
    main()
