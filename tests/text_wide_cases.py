"""Two batches of packed text that are wider than one trip of the text passes' carry kernels (tk_words.h, tk_lines.h, tk_line_set.h,
tk_clean.h): a thread of the carry takes per = ceil(n_tiles / 1024) tiles, and the kept-byte scans make a second trip from tile 1024 on.
  per2: 1090 tiles, a stretch of two tiles per thread          per3: 2050 tiles, three per thread, the last active thread one tile
Built from the geometry, never from literals of positions: T bytes a tile, LANE bytes a lane, BLOCK threads in the carry's workgroup,
WAVE of them a wavefront.  A STRETCH EDGE is byte per * k * T, a WAVEFRONT EDGE byte WAVE * per * k * T.  Every landmark is placed by
filling with seeded lines up to an exact byte position; the builder asserts what it places.  Nothing from the code under test."""
import functools

import numpy as np

import clean_ref as cr
import words_ref as wr

T, LANE, BLOCK, WAVE = 4096, 16, 1024, 64
N_TILES = {"per2": 1090, "per3": 2050}
PER = {"per2": 2, "per3": 3}
NAMES = tuple(N_TILES)
DROPPED = (b"too few.\n", b"this one has no end at all\n", b"and this one just trails off...\n", b"We use cookies on this site today.\n")  # a line each that one rule drops
DOC_PHRASE_LINE = b"Here we quote Lorem Ipsum as every page does.\n"


class Build:
    """documents under construction; pos: the bytes so far"""

    def __init__(self, seed, n_bytes):
        self.rng = np.random.default_rng(seed)
        self.docs, self.cur, self.pos = [], [], 0
        rng = self.rng
        self.plain = [bytes(rng.integers(97, 123, int(rng.integers(1, 11)), dtype=np.uint8)) for _ in range(4000)]
        u = lambda s: s.encode()  # noqa: E731
        special = list(wr.GOPHER) * 12 + [u(w) for w in ("caf\xe9", "\u4e2d\u6587", "\u03a9mega", "#", "#tag", "em\u2003space", "wide\u3000space", "nb\xa0sp", "tab\ttab", "1234",
                                                          "wait...", "so\u2026", "U.S.A.", "Capital", "UPPER", "na\xefve", "\u2026")] * 6
        self.vocab = self.plain + special
        self.p_cut = 28 / (n_bytes / 560)  # a document boundary behind a line: about 28 of them over the batch
        self.may_cut = True

    def put(self, b):
        self.cur.append(b)
        self.pos += len(b)

    def end_doc(self):
        self.docs.append(b"".join(self.cur))
        self.cur = []

    def words(self, n, vocab=None):
        vocab = vocab or self.vocab
        return [vocab[i] for i in self.rng.integers(0, len(vocab), n)]

    def line(self):
        """a seeded line with its newline: 1 to 3 T bytes, kept by C4's rules or dropped by one of them"""
        rng = self.rng
        r, kind = rng.random(), rng.random()
        n = int(rng.integers(5, 30) if r < .6 else rng.integers(30, 150) if r < .9 else rng.integers(150, 400) if r < .98 else rng.integers(400, 1500))
        if kind < .04:
            return b"\n"
        if kind < .08:
            return (b"Home", b"Menu | About | Contact", b"Read more...", b"Next page.")[int(rng.integers(4))] + b"\n"
        if kind < .20:
            return b" ".join(self.words(int(rng.integers(1, 5)))) + b".\n"  # too few words
        w = self.words(n)
        if kind < .32:
            return b" ".join(w) + (b"", b",", b":", b";")[int(rng.integers(4))] + b"x\n"  # no terminal byte
        if kind < .40:
            return b" ".join(w) + (b"...", "\u2026".encode(), b"... \t", "\u2026 \r".encode())[int(rng.integers(4))] + b"\n"
        if kind < .46:
            p = cr.LINE_PHRASES[int(rng.integers(len(cr.LINE_PHRASES)))]
            w.insert(int(rng.integers(len(w))), (p, p.upper(), p.title())[int(rng.integers(3))])
        if kind < .50:
            w.insert(0, (b"-", b"*", "\u2022".encode(), "\u25cf".encode())[int(rng.integers(4))])
        out = b" ".join(w)[:3 * T - 2]
        return out.decode("utf-8", "ignore").encode().rstrip() + (b".", b"!", b"?", b"\"")[int(rng.integers(4))] + b"\n"

    def exact_line(self, n, newline=True):
        """a line of ASCII words, n bytes with its end: a full stop and, if `newline`, a newline"""
        body = n - 1 - newline
        assert body >= 16
        out = bytearray(b" ".join(self.words(body // 5 + 8, self.plain))[:body])
        assert len(out) == body
        if out[-1:] == b" ":
            out[-1:] = b"x"
        return bytes(out) + b"." + b"\n" * newline

    def fill_to(self, target, newline=True):
        """seeded lines up to exactly `target` bytes; the last of them ends there, with a newline or without"""
        assert target - self.pos >= 64, ("two landmarks too close", self.pos, target)
        while True:
            line = self.line()
            if self.pos + len(line) > target - 64:
                break
            self.put(line)
            if self.may_cut and self.rng.random() < self.p_cut:
                self.end_doc()
                if self.rng.random() < .2:
                    self.end_doc()  # (an empty document)
        self.put(self.exact_line(target - self.pos, newline))
        assert self.pos == target


@functools.lru_cache(maxsize=None)
def batch(name):
    """(the documents, the landmarks' positions): see the module's docstring and the asserts below"""
    per, n_tiles = PER[name], N_TILES[name]
    N = (n_tiles - 1) * T + 1001
    S, WE = per * T, WAVE * per * T
    assert N // T + 1 == n_tiles and -(-n_tiles // BLOCK) == per and N % LANE != 0 and (per != 3 or n_tiles % 3 != 0)
    b = Build(n_tiles, N)
    mark = {"N": N, "n_tiles": n_tiles, "per": per, "newlines": [], "boundaries": []}

    def newline_at(pos, i):
        """a newline at `pos`, a line that a rule drops right behind it"""
        b.fill_to(pos + 1)
        b.put(DROPPED[i % len(DROPPED)])
        mark["newlines"].append(pos)

    for i, (k, d) in enumerate(((3, -1), (4, 0), (5, 1))):
        newline_at(k * S + d, i)
    # a short run of dots that ends 1 or 2 bytes behind a stretch edge
    short_end = 9 * S + (1 if per == 2 else 2)
    b.fill_to(short_end - 7 - len(b"aa bb cc dd wait"))
    b.put(b"aa bb cc dd wait" + b"." * 7 + b" and then it goes on as before.\n")
    mark["short dots"] = (short_end - 7, short_end)
    # a document boundary exactly at a stretch edge, behind an open line
    b.fill_to(20 * S, newline=False)
    b.end_doc()
    mark["boundaries"].append(20 * S)
    # landmark 1: one run without white space from tile WAVE per - 3 to tile 2 WAVE per + 1, in a line of nine words that ends in '.'
    b.fill_to((WAVE * per - 3) * T + 100)
    head, tail = b"Here the one long run starts ", b" and here it ends."
    run_start, run_end = b.pos + len(head), (2 * WAVE * per + 1) * T + 777
    chunks, left = [], run_end - run_start
    while left > 2000:
        chunks.append(bytes(b.rng.integers(97, 123, int(b.rng.integers(500, 1500)), dtype=np.uint8)) + ("\xe9", "\u4e2d", "\u03a9", "\u6587")[len(chunks) % 4].encode())
        left -= len(chunks[-1])
    run = b"".join(chunks) + bytes(b.rng.integers(97, 123, left, dtype=np.uint8))
    long_line = head + run + tail
    assert len(run) == run_end - run_start and len(run.split()) == 1 and len(run.decode()) < len(run) and not any(p in long_line.lower() for p in cr.LINE_PHRASES + cr.DOC_PHRASES)
    assert run_start // T == WAVE * per - 3 and (run_end - 1) // T == 2 * WAVE * per + 1 and run_start < WE < 2 * WE < run_end
    b.may_cut = False  # the third copy lies in the first copy's document
    first = b.pos
    b.put(long_line + b"\n")
    mark["long line"] = [first]
    mark["long doc"] = len(b.docs)
    for _ in range(30):
        b.put(b.line())
    b.fill_to(b.pos + 400 + (first + 3 - b.pos - 400) % LANE)
    assert (b.pos - first) % LANE == 3
    mark["long line"].append(b.pos)
    b.put(long_line + b"\n")
    b.may_cut = True
    assert b.pos < 4 * WE - 2 * S
    # newlines at wavefront edges; between them the long run of dots, over more than two whole stretches
    newline_at(4 * WE - 1, 3)
    dots_start = (4 * WAVE + 10) * S - 100
    n_dots = 2 * S + 200
    n_dots += (3 - per - n_dots) % 3  # 1 mod 3 in per2, 2 mod 3 in per3
    assert n_dots % 3 == 3 - per and dots_start // S + 3 <= (dots_start + n_dots) // S
    b.fill_to(dots_start - len(b"and so it goes on "))
    b.put(b"and so it goes on " + b"." * n_dots + b"\n")
    mark["long dots"] = (dots_start, dots_start + n_dots)
    newline_at(5 * WE, 4)
    newline_at(6 * WE + 1, 5)
    # a document boundary exactly at a wavefront edge, two empty documents at the same position
    b.fill_to(7 * WE)
    b.end_doc(), b.end_doc(), b.end_doc()
    mark["boundaries"].append(7 * WE)
    # the long line once more, in another document, shifted against the 16-byte grid by an odd amount
    at = (7 * WAVE * per + 5) * T
    b.fill_to(at + (first + 5 - at) % LANE)
    assert (b.pos - first) % LANE == 5 and len(b.docs) > mark["long doc"] + 1
    mark["long line"].append(b.pos)
    b.put(long_line + b"\n")
    b.may_cut = False
    b.fill_to(b.pos + 3000)
    # the one document that says a document phrase, wholly behind tile 1024
    b.end_doc()
    assert b.pos > (BLOCK + 1) * T
    mark["phrase doc"] = len(b.docs)
    b.fill_to(b.pos + 20000)
    b.put(DOC_PHRASE_LINE)
    b.fill_to(b.pos + 20000)
    b.end_doc()
    b.may_cut = True
    # newlines at the last three stretch edges before N; the last document ends in an open line
    k_last = (N - 1) // S
    for i, (k, d) in enumerate(((k_last - 2, -1), (k_last - 1, 1), (k_last, 0))):
        newline_at(k * S + d, 6 + i)
    assert (k_last + 1) * S >= N > k_last * S + 200
    b.may_cut = False
    last = b"and the last line stays open"
    b.fill_to(N - len(last))
    b.put(last)
    b.end_doc()
    docs = b.docs
    text = b"".join(docs)
    assert len(text) == N and not docs[-1].endswith(b"\n") and 30 <= len(docs) <= 60, (len(text), len(docs))
    assert all(text[p:p + 1] == b"\n" for p in mark["newlines"]) and any(p % WE == 0 for p in mark["newlines"]) and mark["newlines"][-1] == k_last * S
    assert {p % S - (p % S > 1) * S for p in mark["newlines"]} == {-1, 0, 1}
    off = np.concatenate([[0], np.cumsum([len(d) for d in docs])])
    assert all(p in off for p in mark["boundaries"]) and (off == 7 * WE).sum() == 3 and text[20 * S - 1:20 * S] == b"."
    assert all(text[p:p + len(long_line) + 1] == long_line + b"\n" for p in mark["long line"])
    assert [int(np.searchsorted(off, p, "right")) - 1 for p in mark["long line"]][:2] == [mark["long doc"]] * 2
    assert sum(d.lower().count(p) for d in docs for p in cr.DOC_PHRASES) == 1 and b"lorem ipsum" in docs[mark["phrase doc"]].lower()
    assert b"\n" in text[:T] and b" " in text[:T] and text.count(b"\n") < 100_000
    a, e = mark["long dots"]
    assert text[a:e] == b"." * (e - a) and text[a - 1:a] != b"." and text[e:e + 1] == b"\n"
    a, e = mark["short dots"]
    assert text[a:e] == b"." * 7 and text[a - 1:a] != b"." and text[e:e + 1] == b" "
    text.decode()  # (well-formed: the references take their plain paths)
    return docs, mark
