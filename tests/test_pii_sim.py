"""The masking rule on the CPU (tests/hostsim/pii_sim.cpp over tk_pii_rule.h): candidate-by-candidate decisions against re.sub with the
expression of tests/pii_ref.py, on the strings the rule's notes name and on random strings over a small alphabet of units."""
import ctypes

import numpy as np
import pytest

import helpers as h
import pii_ref as ref

SRCS = ("pii_sim.cpp", "tk_pii_rule.h", "tk_rows_rule.h", "tk_common.h")
UNITS = [b"a", b"1", b"25", b"255", b"256", b".", b"@", b"-", b"_", b"%", b"com", b" ", b"\n", b"\xc3\xa9"]
NAMED = [b"a@b.com.", b"a@b.com1", b"a@b..com", b"v1.2.3.4", b"01.2.3.4", b"1.2.3.256", b"1.2.3.4.5", b"10.0.0.1.", b"8.8.8.8.", b"a@bb.cc@dd.ee", b"1.2.3.4@example.com",
         b"a-1.2.3.4@x.com", b"a@b-1.2.3.4.com", b"a@bb.cc.x-1.2.3.4", b"a@b.com_", b"a@b.com-", b"a@b.co.uk,", b"a@b.c", b"@b.com", b"x" * 64 + b"@b.com", b"x" * 65 + b"@b.com",
         b"a@" + b"x" * 249 + b".com", b"a@" + b"x" * 250 + b".com", b"a@b.com." + b"x" * 246, b"a@b.com." + b"x" * 247, b"1.2.3.4", b"0.0.0.0 255.255.255.255 1.2.3.4",
         b"1.2.3.4 9.9.9.9", b"1.2.3.04", b"1.2.3", b"1..2.3.4", b"1.2.3.4a", b"1.2.3.4_", b"-1.2.3.4-", b"1234.1.1.1", b"a@-.cc", b"a@b.-.cc", b"", b"@", b"1"]
_lib = None


def sim(doc, email=ref.EMAIL_PH, ip=ref.IP_PH, public_ip_only=True):
    global _lib
    if _lib is None:
        _lib = h.build_sim("libpii_sim.so", SRCS, ("-Wall", "-Werror", "-Wno-unknown-pragmas"))
        _lib.pii_sim_mask.restype = ctypes.c_int64
        _lib.pii_sim_mask.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint32] + [ctypes.c_void_p, ctypes.c_uint64] * 1 + [ctypes.c_void_p]
    out, counts = np.zeros(len(doc) * 33 // 7 + 64, np.uint8), np.zeros(2, np.uint64)
    n = _lib.pii_sim_mask(doc, len(doc), email, len(email), ip, len(ip), int(public_ip_only), out.ctypes.data, len(out), counts.ctypes.data)
    assert 0 <= n <= len(out), (doc, n)
    return bytes(out[:n]), int(counts[0]), int(counts[1])


@pytest.mark.parametrize("spec", [dict(), dict(public_ip_only=False), dict(email=b"", ip=b"", public_ip_only=False), dict(email=b"E" * 32, ip=b"\xe2\x80\xa6" * 10)])
def test_named_strings(spec):
    for doc in NAMED:
        assert sim(doc, **spec) == ref.mask_doc(doc, **spec), doc
    assert ref.mask_doc(b"a@b.com. 10.0.0.1. 8.8.8.8.", **spec)[1:] == (1, 1 if spec.get("public_ip_only", True) else 2)


def random_doc(rng, n):
    """n units; three times in four the next unit is one that can continue an address: a dot behind a number, '.' or '@' behind letters,
    a number or letters behind '.' and '@'"""
    num, word, dot, at = (1, 2, 3, 4), (0, 10), 5, 6
    out, k = [], int(rng.integers(len(UNITS)))
    for _ in range(n):
        out.append(UNITS[k])
        follow = (dot,) if k in num else num + word if k in (dot, at) else (dot, dot, at) if k in word else ()
        k = int(rng.choice(follow)) if follow and rng.random() < 0.75 else int(rng.integers(len(UNITS)))
    return b"".join(out)


@pytest.mark.parametrize("seed", range(4))
def test_random_strings_over_the_units(seed):
    rng = np.random.default_rng(0x504949 + seed)
    hits = 0
    for _ in range(1500):
        doc = random_doc(rng, 12 if seed < 2 else 40)
        want = ref.mask_doc(doc, public_ip_only=bool(seed & 1))
        hits += want[1] + want[2] > 0
        assert sim(doc, public_ip_only=bool(seed & 1)) == want, doc
    assert hits * 20 >= 1500, hits
