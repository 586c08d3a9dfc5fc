"""Buffers for the JSON Lines tests: the hand-written edge cases and the seeded generator, shared by the CPU simulation's tests and the GPU's."""
import json
import random

WORDS = ["a", "the", "token", 'quo"te', "back\\slash", "tab\there", "line\nbreak", "é", "日本語", "😀", "naïve", " ", "\x7f", "/", "\x01", "𝄞"]


def record(rng, field="text"):
    text = " ".join(rng.choice(WORDS) for _ in range(rng.randint(0, 12)))
    obj = {"id": rng.randint(0, 999), field: text, "meta": {"k": [1, 2, {"x": "y"}], field: "nested"}}
    if rng.random() < 0.3:
        obj = {field: text}
    if rng.random() < 0.2:
        obj = {"meta": obj["meta"] if "meta" in obj else {}, field + "2": "longer key", field: text}
    return obj


def dumps(rng, obj) -> bytes:
    sep = rng.choice([None, (",", ":"), (" , ", " : ")])
    return json.dumps(obj, ensure_ascii=rng.random() < 0.5, separators=sep, indent=None).encode("utf-8")


def mutate(rng, line: bytes, field="text") -> bytes:
    """one of the issue's mutations"""
    f = field.encode()
    k = rng.randrange(14)
    if k == 0 and b'"' in line:  # a dropped quote
        i = rng.choice([i for i, c in enumerate(line) if c == 0x22])
        return line[:i] + line[i + 1:]
    if k == 1 and line.endswith(b'"}'):  # a stray backslash before the closing quote
        return line[:-2] + b'\\"}'
    if k == 2:  # a raw control byte
        i = rng.randrange(len(line) + 1)
        return line[:i] + bytes([rng.choice([1, 9, 13, 31])]) + line[i:]
    if k == 3:  # a truncated \u escape
        return b'{"' + f + b'":"ab\\u12' + rng.choice([b'"}', b'g4"}', b'3"}'])
    if k == 4:  # lone and swapped surrogates
        return b'{"' + f + b'":"' + rng.choice([b"\\ud83d", b"\\ude00", b"\\ude00\\ud83d", b"\\ud83d\\ud83d\\ude00", b"\\uD83Dx\\uDE00", b"\\ud83d\\n", b"\\\\ud83d\\ude00"]) + b'"}'
    if k == 5:  # duplicate keys
        return b'{"' + f + b'":"first","' + f + b'":' + rng.choice([b'"second"', b"null", b"12", b'{"a":1}']) + b"}"
    if k == 6:  # the field at depth 2 only
        return b'{"a":{"' + f + b'":"deep"},"b":[{"' + f + b'":"deeper"}]}'
    if k == 7:  # the field as a substring of a longer key
        return b'{"' + f + b'2":"x","x' + f + b'":"y"}'
    if k == 8:  # a value of every non-string type
        return b'{"' + f + b'" : ' + rng.choice([b"null", b"true", b"-1.5e3", b"[1]", b'{"' + f + b'":"in"}', b""]) + b"}"
    if k == 9:  # blank lines
        return rng.choice([b"", b"  ", b"\t\r", b" \r"])
    if k == 10:  # CRLF
        return line + b"\r"
    if k == 11:  # ill-formed UTF-8, raw
        return b'{"' + f + b'":"' + rng.choice([b"\xc3", b"\xa9", b"\xe2\x82", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\xc0\xaf", b"\xe2\\n\x82\xac", b"ok \xe2\x82\xac"]) + b'"}'
    if k == 12:  # not an object, trailing garbage, unbalanced
        return rng.choice([b"[1,2]", b'"str"', line + b" {}", line[:-1], line + b"}", b"}{", b'{"' + f + b'":"a"}]'])
    return b'{"' + f + b'":"' + rng.choice([b"\\q", b"\\", b"\\u00e9\\/\\b\\f\\r\\t\\\"", b"\\u0000", b"a\\\\", b"\\\\\\\""]) + b'"}'


def buffer(rng, n_lines: int, bad_rate: float, field="text", bom=None, final_newline=None) -> bytes:
    lines = []
    for _ in range(n_lines):
        line = dumps(rng, record(rng, field))
        if rng.random() < bad_rate:
            line = mutate(rng, line, field)
        assert b"\n" not in line
        lines.append(line)
    buf = b"\n".join(lines)
    if (rng.random() < 0.5) if final_newline is None else final_newline:
        buf += b"\n"
    if (rng.random() < 0.2) if bom is None else bom:
        buf = b"\xef\xbb\xbf" + buf
    return buf


def straddle(T: int, item: bytes, at: int, tail: bytes = b'"}') -> bytes:
    """one line {"text":"xxx<item>...} whose item starts at byte `at` of the buffer"""
    head = b'{"text":"'
    assert at >= len(head)
    return head + b"x" * (at - len(head)) + item + tail + b"\n"


def edge_buffers(T: int):
    """(name, buffer): the tile-edge cases -- each item starting at T - 12 .. T --, the long lines and the edge statuses"""
    out = []
    items = [("odd backslash run", b"\\" * 7 + b'"'), ("even backslash run", b"\\" * 8), ("surrogate pair", b"\\ud83d\\ude00"),
             ("lone high then escape", b"\\ud83d\\n"), ("low without high", b"\\ude00"), ("raw char", "€😀".encode())]
    for name, item in items:
        for at in range(T - 12, T + 1):
            out.append((f"{name} at {at}", straddle(T, item, at) + b'{"text":"next"}\n'))
    for at in range(T - 12, T + 1):  # the key's closing quote, the whitespace, the colon
        pad = b'{"pad":"' + b"p" * (at - 15) + b'",'
        out.append((f"key ends at {at}", pad + b'"text" \t : \t "v' + str(at).encode() + b'"}\n'))
        out.append((f"key opens at {at}", b'{"pad":"' + b"p" * (at - 10) + b'","text":"w"}\n'))
    for end in (T - 1, T):  # the value's closing quote at byte T - 1 and at byte T
        out.append((f"closing quote at {end}", b'{"text":"' + b"v" * (end - 9) + b'"}\n{"text":"b"}'))
    long_line = b'{"text":"' + b"L" * (5 * T + 3 - 11) + b'"}'
    assert len(long_line) == 5 * T + 3
    out.append(("long line", long_line + b'\n{"text":"short"}\n'))
    out.append(("64 KiB of backslash pairs", b'{"text":"' + b"\\\\" * 32768 + b'"}\n'))
    out.append(("open string over tiles", b'{"text":"' + b"o" * (2 * T) + b'\n{"text":"after"}\n'))
    out.append(("deep over tiles", b'{"a":' + b"[" * (T + 5) + b"]" * (T + 5) + b',"text":"deep"}\n{"text":' + b"[" * T + b"\n"))
    out.append(("whitespace over tiles", b" " * (T + 3) + b'{"text":"ws"}' + b" " * T + b"\n" + b" " * (2 * T) + b"\n" + b" " * T + b"x\n"))
    for name, buf in (("empty", b""), ("one newline", b"\n"), ("three newlines", b"\n\n\n"), ("no final newline", b'{"text":"a"}\n{"text":"b"}'),
                      ("bom", b'\xef\xbb\xbf{"text":"a"}\n{"text":"b"}\n'), ("bom only", b"\xef\xbb\xbf"), ("bom blank", b"\xef\xbb\xbf \n"),
                      ("absent", b'{"id":1}\n'), ("depth 2 only", b'{"a":{"text":"x"}}\n'), ("text2 before text", b'{"text2":"no","text":"yes"}\n'),
                      ("duplicate keys", b'{"text":"one","text":"two"}\n'), ("duplicate, last not a string", b'{"text":"one","text":2}\n'),
                      ("escaped key", b'{"te\\u0078t":"x"}\n'), ("crlf", b'{"text":"a"}\r\n\r\n{"text":"b"}\r\n')):
        out.append((name, buf))
    return out
