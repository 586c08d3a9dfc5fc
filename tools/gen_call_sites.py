#!/usr/bin/env python3
"""Writes tests/golden/reference_call_sites.json: every place where the reference's Python layer calls into its native core
(`self._core_bpe.<method>(...)`, `_tiktoken.CoreBPE(...)` in REFERENCE_DIR/tiktoken/core.py) as [line, method, positional arity, keywords].

Data derived from the reference's AST, not its text: the reference's sources are not part of this repository, and
tests/test_reference_package.py uses this list to drive the shim in the forms the reference uses.
Usage: python tools/gen_call_sites.py REFERENCE_DIR   (a source tree of openai/tiktoken)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from test_reference_package import CALL_SITES, core_bpe_call_sites  # noqa: E402

REF = sys.argv[1]
sites = core_bpe_call_sites(os.path.join(REF, "tiktoken", "core.py"))
with open(CALL_SITES, "w") as f:
    f.write('{"source": "tiktoken/core.py of openai/tiktoken 0.14.0", "fields": ["line", "method", "n_positional", "keywords"],\n "call_sites": [\n  ')
    f.write(",\n  ".join(json.dumps(s) for s in sites) + "\n ]}\n")
print(len(sites), "call sites ->", CALL_SITES)
