#!/usr/bin/env python3
"""Generate tests/golden/train_cases.json.gz by running the REFERENCE's own trainer, `tiktoken._educational.bpe_train(..., visualise=None)`,
imported from the reference's read-only tree with the native module stubbed (as tools/gen_golden.py does).  Every text is made here from
seeded `random`; nothing of the reference is used as data.  Per case the file holds the text (by name), pat_str, vocab_size and the
resulting token byte strings in id order -- or "exhausted" where the reference raises ValueError from max() over no pairs.

Usage: python tools/gen_golden_train.py
"""
import base64
import gzip
import json
import os
import random
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"

stub = types.ModuleType("tiktoken._tiktoken")
stub.CoreBPE = type("CoreBPE", (), {"__init__": lambda self, *a, **k: None})
sys.modules["tiktoken._tiktoken"] = stub
sys.path.insert(0, REF)
import tiktoken  # noqa: E402  (the reference package)
import tiktoken._educational as edu  # noqa: E402

assert tiktoken.__file__.startswith(REF), tiktoken.__file__
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import py_oracle as po  # noqa: E402  (pattern strings only)

sys.path.insert(0, os.path.join(ROOT, "tests"))
import train_ref  # noqa: E402  (only to find the step at which the Zipf text runs out of pairs)

GENERIC_PAT = r"\p{L}+|\p{N}{1,3}|[^\s\p{L}\p{N}]+"  # leaves white space unmatched: gap chars


def two_letter_words(rng):
    return " ".join(rng.choice("abcdefghijkl") + rng.choice("abcdefghijkl") for _ in range(420))


def mixed(rng):
    latin = ["the", "quick", "brown", "fox", "jumps", "over", "lazy", "dog", "and", "then", "there", "were", "none", "Hello", "World", "THE", "It", "we", "you"]
    accented = ["café", "naïve", "über", "señor", "façade", "żółć", "Ångström", "crème"]
    cjk = ["中文", "文本", "日本語", "テキスト", "한국어", "中", "语言模型"]
    emoji = ["😀", "🚀", "👍🏽", "❤️", "🙂🙂"]
    contr = ["don't", "I'm", "we'll", "they've", "it's", "you're", "he'd", "DON'T", "I'M"]
    punct = [".", ",", "!", "?", "...", " - ", ";", ":", "(", ")", "\"", "/", "//", "#"]
    out = []
    for _ in range(1500):
        u = rng.random()
        if u < 0.45:
            out.append(rng.choice(latin))
        elif u < 0.55:
            out.append(rng.choice(accented))
        elif u < 0.63:
            out.append(rng.choice(cjk))
        elif u < 0.67:
            out.append(rng.choice(emoji))
        elif u < 0.77:
            out.append(rng.choice(contr))
        elif u < 0.87:
            out.append(str(rng.randrange(10 ** rng.randrange(1, 6))))
        else:
            out.append(rng.choice(punct))
        v = rng.random()
        out.append(" " if v < 0.8 else ("\n" if v < 0.88 else ("  " if v < 0.93 else ("\n\n" if v < 0.96 else ("\t" if v < 0.98 else "")))))
    return "".join(out)


def zipf_words(rng):
    letters = "etaoinshrdlucmfw"
    vocab = []
    while len(vocab) < 110:
        w = "".join(rng.choice(letters) for _ in range(rng.randrange(2, 7)))
        if w not in vocab:
            vocab.append(w)
    weights = [1.0 / (r + 1) for r in range(len(vocab))]
    return " ".join(rng.choices(vocab, weights=weights, k=20000))


def main():
    rng = random.Random(0x7A11)
    texts = {
        "hand": "aaaa aaaa abab abab baba",
        "two_letter": two_letter_words(rng),
        "mixed": mixed(rng),
        "runs": "x" * 40 + " " + "xy" * 30,
        "zipf": zipf_words(rng),
        "ab": "ab",
    }
    # the Zipf text: the largest vocab_size at which the reference still returns = 256 + the merges it has pairs for
    words = train_ref.distinct_words(train_ref.pieces_of([texts["zipf"]], po.R50K_PAT))
    n = 0
    try:
        train_ref.train_words(words, 5000)
    except train_ref.Exhausted as e:
        n = e.done
    assert 100 < n < 1000, n
    plan = [
        ("hand", "hand", po.R50K_PAT, 261),
        ("two_letter", "two_letter", po.R50K_PAT, 300),
        ("mixed_gpt2", "mixed", po.R50K_PAT, 420),
        ("mixed_cl100k", "mixed", po.CL100K_PAT, 420),
        ("mixed_o200k", "mixed", po.O200K_PAT, 420),
        ("mixed_generic_gaps", "mixed", GENERIC_PAT, 420),
        ("runs", "runs", po.R50K_PAT, 266),
        ("zipf_last_size", "zipf", po.R50K_PAT, 256 + n),
        ("zipf_one_more", "zipf", po.R50K_PAT, 256 + n + 1),
        ("exhausted", "ab", po.R50K_PAT, 300),
    ]
    cases = []
    for name, text, pat, size in plan:
        t0 = time.time()
        try:
            ranks = edu.bpe_train(texts[text], size, pat, visualise=None)
        except ValueError:
            cases.append({"name": name, "text": text, "pat_str": pat, "vocab_size": size, "exhausted": True})
            print(f"{name}: exhausted ({time.time() - t0:.1f} s)")
            continue
        assert list(ranks.values()) == list(range(len(ranks))) and len(ranks) == size, (name, len(ranks))  # (no duplicate spelling: ids have no holes)
        cases.append({"name": name, "text": text, "pat_str": pat, "vocab_size": size, "tokens": [base64.b64encode(t).decode() for t in ranks]})
        print(f"{name}: {len(ranks)} tokens ({time.time() - t0:.1f} s)")
    assert [c["name"] for c in cases if c.get("exhausted")] == ["zipf_one_more", "exhausted"]
    out = os.path.join(ROOT, "tests", "golden", "train_cases.json.gz")
    with gzip.GzipFile(out, "wb", mtime=0) as f:
        f.write(json.dumps({"texts": texts, "cases": cases}, ensure_ascii=False, sort_keys=True).encode("utf-8"))
    print(out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < 100_000


if __name__ == "__main__":
    main()
