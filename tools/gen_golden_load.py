#!/usr/bin/env python3
"""Writes tests/golden/reference_load.json: what the reference's tiktoken/load.py makes of the synthetic data-gym files of
tests/helpers.py data_gym_files() and of the .tiktoken file this package writes for their table -- sizes and digests of the
resulting rank tables, which tests/test_api_surface.py compares with this package's results.

Usage: python tools/gen_golden_load.py REFERENCE_DIR   (a source tree of openai/tiktoken: REFERENCE_DIR/tiktoken/load.py)
"""
import hashlib
import importlib.util
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import helpers as h  # noqa: E402
from tiktoken_amd import vocab_io  # noqa: E402

spec = importlib.util.spec_from_file_location("reference_load", os.path.join(sys.argv[1], "tiktoken", "load.py"))
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)
os.environ["TIKTOKEN_CACHE_DIR"] = ""  # (no cache: local files)
with tempfile.TemporaryDirectory() as d:
    g = h.data_gym_files(d)
    a = ref.data_gym_to_mergeable_bpe_ranks(g["bpe"], g["enc"])
    b = ref.data_gym_to_mergeable_bpe_ranks(g["bpe2"], g["enc2"])
    try:
        ref.data_gym_to_mergeable_bpe_ranks(g["bpe2"], g["enc"])
        raised = None
    except Exception as e:
        raised = type(e).__name__
    path = os.path.join(d, "t.tiktoken")
    vocab_io.dump_tiktoken_bpe(g["ranks"], path)
    with open(path, "rb") as f:
        file_sha = hashlib.sha256(f.read()).hexdigest()
    c = ref.load_tiktoken_bpe(path)
out = {"source": "tiktoken/load.py of openai/tiktoken 0.14.0 on the files of tests/helpers.py data_gym_files(); [entries, helpers.ranks_digest]",
       "data_gym": [len(a), h.ranks_digest(a)], "data_gym_duplicate_merge": [len(b), h.ranks_digest(b)],
       "data_gym_mismatched_files_raise": raised, "dumped_tiktoken_file_sha256": file_sha,
       "load_tiktoken_bpe_of_dumped_file": [len(c), h.ranks_digest(c)]}
dst = os.path.join(ROOT, "tests", "golden", "reference_load.json")
with open(dst, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out), "->", dst)
