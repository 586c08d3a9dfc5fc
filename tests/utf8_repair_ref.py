"""The UTF-8 repair rule of include/tiktoken_amd.h (tk_utf8_repair_device) as plain Python loops, written from the header's text: a
document's bytes fall into units -- ASCII bytes, well-formed sequences, ill-formed units (a lead and what it accepted, or a single
byte) -- and an ill-formed unit becomes EF BF BD (replace) or nothing (ignore).  Shared by the CPU simulation's and the GPU's tests,
together with the inputs both use."""
import itertools
import random
import re

import numpy as np

REPLACE, IGNORE = 0, 1
ERRORS = {REPLACE: "replace", IGNORE: "ignore"}
FFFD = b"\xef\xbf\xbd"
# the boundary bytes of the rule: ASCII, the edges of the continuation range and of the narrowed ranges, and of every class of lead
BOUNDARY = bytes([0x41, 0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC0, 0xC1, 0xC2, 0xDF, 0xE0, 0xE1, 0xEC, 0xED, 0xEE, 0xEF, 0xF0, 0xF1, 0xF3, 0xF4, 0xF5, 0xFF])
NARROW = {0xE0: (0xA0, 0xBF), 0xED: (0x80, 0x9F), 0xF0: (0x90, 0xBF), 0xF4: (0x80, 0x8F)}
_ASCII_RUN = re.compile(rb"[\x00-\x7f]+")


def declared(b: int) -> int:
    return 2 if 0xC2 <= b <= 0xDF else 3 if 0xE0 <= b <= 0xEF else 4 if 0xF0 <= b <= 0xF4 else 0


def repair(doc: bytes, mode: int):
    """(text, chars, replaced) of one document"""
    out, chars, replaced, i = bytearray(), 0, 0, 0
    while i < len(doc):
        b = doc[i]
        L = declared(b)
        if b < 0x80:  # ASCII bytes are units of their own, copied: a run of them in one step
            j = _ASCII_RUN.match(doc, i).end()
            out += doc[i:j]
            chars += j - i
            i = j
            continue
        took = 1
        if L:
            while took < L and i + took < len(doc):
                lo, hi = NARROW.get(b, (0x80, 0xBF)) if took == 1 else (0x80, 0xBF)
                if not lo <= doc[i + took] <= hi:
                    break
                took += 1
        if L and took == L:
            out += doc[i:i + L]
            chars += 1
        else:
            replaced += 1
            if mode == REPLACE:
                out += FFFD
                chars += 1
        i += took
    return bytes(out), chars, replaced


def repair_batch(docs, mode: int):
    """(text, text_off, char_off, repl_off) of a batch, the offsets as lists of n + 1"""
    text, to, co, ro = bytearray(), [0], [0], [0]
    for d in docs:
        t, c, r = repair(d, mode)
        text += t
        to.append(len(text))
        co.append(co[-1] + c)
        ro.append(ro[-1] + r)
    return bytes(text), to, co, ro


def check_against_cpython(docs, mode: int):
    """the restatement is CPython's decoder on these inputs: the bytes, and len(str) for the chars"""
    for d in set(docs):
        s = d.decode("utf-8", ERRORS[mode])
        t, c, _ = repair(d, mode)
        assert t == s.encode("utf-8") and c == len(s), d


# ---------------------------------------------------------------- inputs
def exhaustive():
    """every sequence of 0 .. 4 boundary bytes, each a document: 346 201 documents"""
    return [bytes(t) for k in range(5) for t in itertools.product(BOUNDARY, repeat=k)]


SEQS = [b"\xc3\xa9", "中".encode(), "😀".encode(), b"\xe0\xa0\x80", b"\xed\x9f\xbf", b"\xf0\x90\x80\x80", b"\xf4\x8f\xbf\xbf", b"\xe0\x9f\xbf", b"\xed\xa0\x80", b"\xf0\x8f\xbf\xbf",
        b"\xf4\x90\x80\x80"]


def sliding(lane: int, wave: int, block: int):
    """Each sequence, whole and truncated, at every offset 12 .. 19 of a lane, across byte `wave` and across the workgroup's edge `block`;
    a document boundary at every position inside it; a document over three workgroups.  Returns a list of batches (lists of documents)."""
    batches = []
    for seq in SEQS:
        for cut in range(1, len(seq) + 1):
            part = seq[:cut]
            for edge in (lane, wave, block):
                for o in range(12, 20):
                    pad = edge - lane + o
                    batches.append([b"x" * pad + part + b"yz"])
                    batches.append([b"x" * pad + part])  # the text ends in it
                    batches.append([b"\xc3\xa9" * (pad // 2) + b"x" * (pad % 2) + part + seq])
            for o in range(12, 20):  # a boundary at every position inside the sequence
                for at in range(0, len(part) + 1):
                    batches.append([b"q" * (block - lane + o) + part[:at], part[at:] + b"r" * 5, b"", seq])
    long_doc = ("The quick brown fox. 中文😀é " * (3 * block // 30 + 1)).encode()[: 2 * block + 100]
    batches.append([b"ab", long_doc[1:], b"\x80" + long_doc[:-1], b"\xf0\x9f\x98"])
    return batches


def empties():
    body = [b"a\xe4", b"\xb8\xad", "中文".encode() * 9, b"\xf0\x9f"]
    out = []
    for k in (1, 2, 70):
        e = [b""] * k
        out += [e + body, body[:2] + e + body[2:], body + e, e + body[:1] + e + body[1:] + e, e]
    return out


def random_batches(seed: int, count: int):
    rng = random.Random(seed)
    units = [b"a", b"hello wor", "é".encode(), "中".encode(), "😀".encode(), b"\x80", b"\xbf", b"\xc2", b"\xe0\xa0", b"\xed\xa0\x80", b"\xf0\x90\x80", b"\xf4\x90", b"\xff",
             b"\xc0\x80", b"The quick brown fox jumps over the lazy dog. "]
    out = []
    for _ in range(count):
        docs = []
        for _ in range(rng.choice([1, 3, 8, 30])):
            if rng.random() < 0.3:
                docs.append(bytes(rng.choice([rng.randrange(256), rng.randrange(0x80, 0x100), rng.choice(BOUNDARY)]) for _ in range(rng.randrange(0, 60))))
            else:
                docs.append(b"".join(rng.choice(units) for _ in range(rng.choice([0, 1, 2, 5, 40, 400]))))
        out.append(docs)
    return out


def growth(block: int):
    """Batches (each meant to start at a workgroup's first byte) whose output per workgroup of `block` bytes is as large as 'replace' can
    make it: every byte an ill-formed unit of its own, three bytes each, and before them a lead at the end of the workgroup before, whose
    replacement is charged to the byte that does not continue it -- 3 x block + 3 bytes from one workgroup (`charged`)."""
    cont, ff = b"\x80" * block, b"\xff" * block
    out = [[cont]]
    out += [[lead, cont] for lead in (b"\xe4", b"\xf0\x9f", b"\xf0\x9f\x98")]  # the same document 1, 2 and 3 bytes behind a lead that its document's end cuts
    for lead, run in ((b"\xf0", cont), (b"\xe0", cont), (b"\xf4", b"\x90" * block), (b"\xc2", ff), (b"\xf0\x9f", ff), (b"\xf0\x9f\x98", ff)):
        out.append([b"x" * (block - len(lead)) + lead + run + b"z"])  # the lead inside the document: the next workgroup pays for it
    out.append([b"\xff" * (3 * block + 5)])
    out.append([b"\xf0\x9f\x98" * (block // 3 + 2)])  # every unit keeps its length
    out.append([b"\xc2" * (block + 7)])  # every unit grows, and each is charged to the byte behind it
    out.append([b"ab", b"\xf0\x9f\x98" * (2 * block // 3), b"\xc2" * block, b"\x80"])
    return out


def charged(docs, block: int):
    """The bytes that 'replace' leaves per `block` bytes of the packed documents, a unit counted at the byte where its fate is known (the
    lane rule of tk_utf8_repair_rule.h) -- by CPython's incremental decoder, which holds back exactly a sequence that may still continue."""
    import codecs

    out = [0] * (sum(map(len, docs)) // block + 1)
    pos = 0
    for d in docs:
        dec = codecs.getincrementaldecoder("utf-8")("replace")
        i = 0
        while i < len(d):
            j = min(len(d), i + block - pos % block)  # up to the next workgroup's first byte
            out[pos // block] += len(dec.decode(d[i:j], final=j == len(d)).encode())
            pos += j - i
            i = j
    return out


def pack(docs):
    """(bytes uint8 with 16 readable bytes behind them that are not zero, n, byte_off uint64[n + 1])"""
    n = sum(len(d) for d in docs)
    blob = np.frombuffer(b"".join(docs) + b"\xa5" * 16, np.uint8)
    off = np.zeros(len(docs) + 1, np.uint64)
    if docs:
        off[1:] = np.cumsum([len(d) for d in docs], dtype=np.uint64)
    return blob, n, off


# ---------------------------------------------------------------- pooled batches: very many documents drawn from a few dozen
# What a batch of a million documents can show lies in the code around the lanes (the second workgroup of a scan, the second trip of a
# grid-stride loop), not in the documents: these are drawn from a small pool, the rule runs once per pool entry, and numpy spreads the
# result over the batch.  One batch of WIDE_N documents; every smaller size is a prefix of it, and its reference a slice.
WIDE_N = (1 << 20) + 1030
WIDE_PREFIXES = (1024, 1025, 2051, (1 << 20) - 1, 1 << 20, WIDE_N)
# the documents on both sides of the 1024-document workgroups' edges and of the 2^20 items of a capped grid, and the last
WIDE_FORCED = (1023, 1024, 1025, 2047, 2048, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, WIDE_N - 1)


def draw(n_pool: int, forced, seed: int, n: int = WIDE_N, at=WIDE_FORCED):
    """the pool entry of each of n documents: uniform, seeded; the documents `at` take the entries `forced` in turn"""
    idx = np.random.default_rng(seed).integers(0, n_pool, n)
    forced = list(forced)
    for k, d in enumerate(at):
        idx[d] = forced[k % len(forced)]
    return idx


def spread(parts, idx, dtype=np.uint8):
    """parts[i] (bytes, or a list of numbers) for every i of idx back to back: (the elements as one array, offsets uint64[len(idx) + 1])"""
    lens = np.array([len(p) for p in parts], np.int64)
    table = np.zeros((len(parts), max(int(lens.max()), 1)), dtype)
    for i, p in enumerate(parts):
        table[i, :len(p)] = np.frombuffer(p, np.uint8) if isinstance(p, bytes) else p
    took = lens[idx]
    off = np.zeros(len(idx) + 1, np.uint64)
    off[1:] = np.cumsum(took)
    return table[idx][np.arange(table.shape[1]) < took[:, None]], off


def running(per_entry, idx):
    """the running total, n + 1 entries, of a figure known per pool entry"""
    out = np.zeros(len(idx) + 1, np.uint64)
    out[1:] = np.cumsum(np.asarray(per_entry, np.int64)[idx])
    return out


WIDE_POOL = [
    # well-formed: empty, ASCII, whole chars of two, three and four bytes
    b"", b"", b"a", b" ", b"hello", b"12345678", b"The quick br", "é".encode(), "中".encode(), "😀".encode(), "文😀".encode(), "aé中😀".encode(), "żółć".encode(),
    # a lead that its document's end cuts ...
    b"ab\xe4", b"x\xe4\xb8", b"\xf0\x9f\x98", b"\xc3", b"q\xf0", b"\xf0\x9f", "中".encode() + b"\xe4",
    # ... and the continuation bytes it misses at the start of another
    b"\xb8\xad", b"\xad z", b"\x80", b"\x98\x80ok", b"\xa9",
    # lone continuation bytes, C0, F5, FF, and leads whose first continuation byte is outside the narrowed range
    b"a\x80b", b"\xbf\xbf", b"\xc0\x80", b"x\xf5y", b"\xff", b"\xff\xff\xff", b"\xed\xa0\x80", b"\xe0\x9f\xbf", b"\xf4\x90\x80\x80",
]


def wide_batch():
    """(pool, idx): WIDE_N documents; those of WIDE_FORCED hold an ill-formed unit"""
    ill = [i for i, p in enumerate(WIDE_POOL) if repair(p, REPLACE)[2]]
    return WIDE_POOL, draw(len(WIDE_POOL), ill, 0x81DE)


def pooled_docs(pool, idx, lo: int = 0, hi=None):
    return [pool[i] for i in idx[lo:hi].tolist()]


def pooled_repair(pool, idx, mode: int):
    """`repair_batch` of the documents pool[idx], the rule run once per pool entry: (text uint8[...], text_off, char_off, repl_off), arrays"""
    per = [repair(p, mode) for p in pool]
    text, text_off = spread([t for t, _, _ in per], idx)
    return text, text_off, running([c for _, c, _ in per], idx), running([r for _, _, r in per], idx)
