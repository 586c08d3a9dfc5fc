"""Allowed special tokens in raw text, stated from the rule (src/lib.rs:386-402 as oracle/py_oracle.py find_special resolves it), not from
the kernels: inside every document, at the leftmost position at which an allowed special token matches, the LONGEST one that matches
there is taken, and the search goes on behind it.  A special token never crosses a document start.  From the (start, length) lists
come the three bitmaps the marking passes (tk_k_spec_cand, tk_k_spec_resolve) leave: spec_start, spec_in, brk.

Also here: the case list (a) - (g) that tests/test_spec_mark_sim.py runs through the CPU simulation and tests/test_gpu_special_overlap.py
through the device.  A case is a set of registered special tokens, an allowed subset and a packed batch of documents."""
from __future__ import annotations

import functools
import itertools

import numpy as np

FIRST_ID = 100000  # (above every rank of the vocabularies the cases are run with)


def find_specials(doc: bytes, allowed) -> list[tuple[int, int]]:
    """(start, length) of the special tokens a left-to-right search takes in one document; `allowed`: their byte strings."""
    allowed = [s for s in allowed if s]
    firsts = {s[0] for s in allowed}
    out, i, n = [], 0, len(doc)
    while i < n:
        if doc[i] in firsts:
            best = max((len(s) for s in allowed if doc.startswith(s, i)), default=0)
            if best:
                out.append((i, best))
                i += best
                continue
        i += 1
    return out


def plain_walk(doc: bytes, specials: dict[str, int], allowed) -> list[int]:
    """The ids of one document under a vocabulary of the 256 single bytes (id = byte): at each position the longest allowed special
    token that matches, else one byte."""
    by_bytes = {s.encode(): i for s, i in specials.items() if s in allowed}
    out, at = [], 0
    for a, ln in find_specials(doc, list(by_bytes)):
        out += list(doc[at:a]) + [by_bytes[doc[a:a + ln]]]
        at = a + ln
    return out + list(doc[at:])


def bitmaps(docs: list[bytes], allowed, d0: int = 0, d1: int | None = None, found=None):
    """(spec_start, spec_in, brk) as bool arrays over the bytes of documents [d0, d1) run as one chunk: a special token's first byte;
    its other bytes; document starts, special tokens' first bytes and the byte behind each of them (inside the chunk).
    found: the (start, length) lists per document, if the caller has them."""
    d1 = len(docs) if d1 is None else d1
    n = sum(len(d) for d in docs[d0:d1])
    ss, brk, cov = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n + 1, np.int64)
    allowed = [s.encode() if isinstance(s, str) else s for s in allowed]
    at = 0
    for k, d in enumerate(docs[d0:d1]):
        if at < n:
            brk[at] = True
        f = np.asarray(found[d0 + k] if found is not None else find_specials(d, allowed), np.int64).reshape(-1, 2)
        a, e = at + f[:, 0], at + f[:, 0] + f[:, 1]
        ss[a] = brk[a] = True
        brk[e[e < n]] = True
        np.add.at(cov, a + 1, 1)  # (taken special tokens do not overlap: +1 behind the first byte, -1 at the end)
        np.add.at(cov, e, -1)
        at += len(d)
    si = np.cumsum(cov)[:n] > 0
    return ss, si, brk


class Case:
    def __init__(self, name: str, specials, allowed, docs, chunks=()):
        """specials: the registered strings in order (ids FIRST_ID, + 1, ...); allowed: a subset; docs: str or bytes;
        chunks: document ranges (d0, d1) the CPU simulation also runs as chunks of their own."""
        self.name = name
        self.specials = {s: FIRST_ID + k for k, s in enumerate(specials)}
        self.allowed = [s for s in specials if s in set(allowed)]
        assert self.allowed and len(self.allowed) == len(set(allowed)), name
        self.docs = [d.encode() if isinstance(d, str) else d for d in docs]
        self.chunks = tuple(chunks)
        self.found = None  # per document, (start, length) of the special tokens the rule takes there, once somebody has worked them out

    def also(self, extra: str, tag: str) -> "Case":
        """The same case in a core that registers, and allows, one more special token (one that never occurs in the text)."""
        assert not any(extra.encode()[:1] in d for d in self.docs)
        v = Case(f"{self.name} {tag}", list(self.specials) + [extra], self.allowed + [extra], self.docs, self.chunks)
        v.found = self.found  # (the extra one occurs nowhere)
        return v


# a special token of 65 bytes keeps the head walk on the 64-bit window of the candidate bitmap, one of 66 switches the whole core to the
# walk bit by bit (tk_spec_resolve_one); neither occurs in any text below
NEVER65, NEVER66 = "\x7f" + "~" * 64, "\x7f" + "~" * 65
S3 = ["aa", "aba", "bab"]
S3_ALLOWED = (S3, ["aa", "bab"], ["aba"])
RUN_LENGTHS = list(range(1, 10)) + [31, 32, 33, 34] + list(range(62, 68)) + [127, 128, 129, 130, 2047, 4096]
RUN_BEHIND = (0, 1, 15, 16, 63, 64)
XY_LENGTHS = (33, 65, 67, 105, 201)
MAX_CLUSTER = 4096  # the head walk costs about L * L / 2 probes for a cluster of L bytes: no case has a longer one


@functools.lru_cache(maxsize=None)
def ab_strings() -> tuple:
    return tuple("".join(p) for n in range(13) for p in itertools.product("ab", repeat=n))


def xy(length: int) -> str:
    assert length % 2 == 1
    return "xy" * (length // 2) + "x"


def aligned(docs: list[tuple[int, str]], unit: int = 64) -> list[str]:
    """Documents [(behind, text)] packed so that each `text` lies exactly `behind` bytes behind a multiple of `unit` of the batch: a
    document of filler in front of each ('.' * k, k = 0: an empty document), the `behind` bytes are filler of the document itself."""
    out, at = [], 0
    for behind, text in docs:
        pad = -at % unit
        out += ["." * pad, "." * behind + text]
        at += pad + behind + len(text)
    return out


def cases_a() -> list[Case]:
    """(a) every string over {a, b} of 0 .. 12 bytes as a document of its own (the joined form: joined_a below)"""
    return [Case(f"a: 8191 documents, allowed {'+'.join(al)}", S3, al, ab_strings(), chunks=((100, 3000), (4000, 8191))) for al in S3_ALLOWED]


def joined_a(prefix: int) -> str:
    """(a) the same strings joined by 'c' into ONE document behind `prefix` bytes of 'c'"""
    return "c" * prefix + "c".join(ab_strings())


JOINED_PREFIXES = range(0, 71)


def cases_b() -> list[Case]:
    """(b) runs of 'a' of every length of RUN_LENGTHS behind 0, 1, 15, 16, 63 and 64 other bytes, special token aa; aaa in a second core"""
    docs = aligned([(behind, "a" * k) for k in RUN_LENGTHS for behind in RUN_BEHIND])
    return [Case("b: runs of a, special aa", ["aa"], ["aa"], docs), Case("b: runs of a, special aaa", ["aaa"], ["aaa"], docs),
            Case("b: runs of a, specials aa and aaa", ["aa", "aaa"], ["aa", "aaa"], docs)]


def cases_d() -> list[Case]:
    """(d) long special tokens that overlap themselves"""
    out = []
    for upto in XY_LENGTHS:  # (cores whose longest special token has 33 / 65 bytes keep the 64-bit window, the others walk bit by bit)
        toks = [xy(ln) for ln in XY_LENGTHS if ln <= upto]
        docs = []
        for ln in XY_LENGTHS:
            for r in (ln - 2, ln - 1, ln, ln + 1, ln + 2, 2 * ln - 1, 2 * ln, 2 * ln + 1, 3 * ln - 1, 3 * ln, 3 * ln + 1):
                docs += [(b, ("xy" * r)[:r]) for b in (0, 5, 63)] + [(0, ("yx" * r)[:r] + ".")]
        out.append(Case(f"d: xy tokens up to {upto} bytes", toks, toks, aligned(docs)))
    b70 = "b" * 70
    docs = aligned([(b, "b" * k) for k in (69, 70, 71, 139, 140, 141, 210) for b in (0, 1, 33)])
    out.append(Case("d: b*70", [b70], [b70], docs))
    out.append(Case("d: b*70 beside short tokens", S3 + [b70], S3 + [b70], docs + ["ab" * 40 + "b" * 75 + "ab", "b" * 69 + "ab" + "b" * 70]))
    return out


def cases_e() -> list[Case]:
    """(e) documents"""
    out = []
    for toks in (["aa"], ["aaa"], ["aa", "aaa"]):
        docs, empty = [], []
        for cut in range(1, 41):  # a run of 41 a, cut by a document start: each document resolves on its own
            docs += ["a" * cut, "a" * (41 - cut)]
            empty += ["a" * cut, "", "a" * (41 - cut), "", ""]
        out.append(Case(f"e: a run cut at 1..40, {'+'.join(toks)}", toks, toks, docs, chunks=((1, 4), (7, 60), (79, 80))))
        out.append(Case(f"e: a run cut at 1..40 with empty documents, {'+'.join(toks)}", toks, toks, ["", ""] + empty, chunks=((0, 2), (3, 11), (50, 52))))
    for tok in ("[SEP]", "aba", xy(67)):  # a special token cut at every byte is no candidate, a whole one right behind it is
        docs = []
        for cut in range(1, len(tok)):
            docs += ["abc" + tok[:cut], tok[cut:] + tok + "d", "..." + tok[:cut], "", tok[cut:]]
        out.append(Case(f"e: {tok[:5]} ({len(tok)} bytes) cut at every byte", [tok] + S3[:1], [tok] + S3[:1], docs, chunks=((0, 1), (1, 3), (2, 5))))
    # a cluster that ends on the text's last byte
    for tail in ("ababab", "abaa", "babab", "aaa", "bbabaabab"):
        out.append(Case(f"e: the text ends with {tail}", S3, S3, ["." * 50, "c" + tail], chunks=((1, 2),)))
    return out


def cases_f() -> list[Case]:
    """(f) bytes"""
    out = []
    x_docs = ["x", "xx", "xxx", "axxb", "x" * 70, ".x.x..xx" * 9, "", "x"]
    out.append(Case("f: a one-byte special token", ["x"], ["x"], x_docs))
    out.append(Case("f: x and xx", ["x", "xx"], ["x", "xx"], x_docs))
    out.append(Case("f: x and xx, xx allowed", ["x", "xx"], ["xx"], x_docs))
    out.append(Case("f: a control byte and a line break pair", ["\x01", "\n\n"], ["\x01", "\n\n"], ["a\x01\x01b\n\n\n\n\nc\n", "\n\n\n", "\x01"]))
    six = ["<|a|>", "[SEP]", "]x[", "{pad}", "#eos#", "@@bos", "«fin»"]  # more than four distinct first bytes: the 256-bit set decides
    docs = ["[SEP]x[SEP]", "a[SEP]x[x[SEP]]x[", "nothing [SEP here {pad #eos @bos «fin ]x", "«f «fin» ©«fin»»«", "{pad}#eos#@@bos@@@bos<|a|>",
            "." * 13 + "[SEP]x[SEP]x[SEP]"]
    out.append(Case("f: seven first bytes", six, six, docs))
    out.append(Case("f: seven first bytes, ]x[ without [SEP]", six, [t for t in six if t != "[SEP]"], docs))
    out.append(Case("f: a multi-byte first char", ["«fin»"], ["«fin»"], ["«f «fin» ©«fin»»«", "«" * 20 + "fin»", "««fin»Â"]))
    # the four-first-bytes test marks the byte above a true hit when it is the first byte ^ 1 ('<' then '='): a false candidate that must
    # leave no token, at every position of the sixteen-byte lane
    stock = ["<|a|>", "<=|>"]  # ('=' is a second byte as well: the false candidate gets as far as tk_special_at)
    docs = aligned([(a, t) for a in range(17) for t in ("<=", "<=|a|>", "<<|", "<<|a|>", "<=<|a|>", "<<=|>=|a|>", "<=|", "<<<===")], unit=32)
    out.append(Case("f: the borrow of the byte test", stock, stock, docs))
    out.append(Case("f: the borrow of the byte test, <|a|> alone", stock, stock[:1], docs))
    return out


def cases_g() -> list[Case]:
    """(g) special tokens that are prefixes of one another.  The reference builds an alternation in hash-map order, so which one it takes is
    unspecified; what is expected here is the oracle's rule: the longest allowed one at the leftmost position."""
    toks = ["<|a|>", "<|a|><|b|>", "<|a"]
    docs = ["..<|a|>..", "..<|a|><|b|>..", "<|a|><|b|", "<|a<|a|><|b|>", "<|a|><|a|><|b|><|b|>", "<|", "<|a", "x<|a|" * 5, "<|a|><|b|>" * 7, "<|a|><|b" + "|>"]
    return [Case(f"g: allowed {'+'.join(sub)}", toks, sub, docs) for k in (1, 2, 3) for sub in itertools.combinations(toks, k)]


def head_walk_forms(cases: list[Case]) -> list[Case]:
    """(c) every case again in a core with a 65-byte special token and in one with a 66-byte one: the same marks through either form"""
    return [c.also(extra, tag) for c in cases for extra, tag in ((NEVER65, "+65"), (NEVER66, "+66"))]


def small_cases() -> list[Case]:
    """(d) - (g)"""
    return cases_d() + cases_e() + cases_f() + cases_g()
