"""The masking rule of tk_pii_mask as Python states it: re.sub with the expression of include/tiktoken_amd.h, per document."""
import re
from typing import NamedTuple

import numpy as np

L = rb"A-Za-z0-9._%+\-"
EMAIL = rb"(?<![" + L + rb"@])[" + L + rb"]{1,64}@(?=[A-Za-z0-9.\-]{1,253}(?![A-Za-z0-9.\-]))(?:[A-Za-z0-9\-]+\.)+[A-Za-z]{2,}(?![A-Za-z0-9_\-])"
OCT = rb"(?:25[0-5]|2[0-4][0-9]|1[0-9][0-9]|[1-9]?[0-9])"
IP = rb"(?<![A-Za-z0-9_.])" + OCT + rb"(?:\." + OCT + rb"){3}(?![A-Za-z0-9_])(?!\.[0-9])"
BOTH = re.compile(rb"(" + EMAIL + rb")|(" + IP + rb")")
EMAIL_PH, IP_PH = b"email@example.com", b"22.214.171.124"


class Ref(NamedTuple):
    text: np.ndarray
    doc_off: np.ndarray
    n_email: np.ndarray
    n_ip: np.ndarray
    counts: np.ndarray  # bytes, e-mails, addresses, overflow


def private(addr: bytes) -> bool:
    a, b = (int(x) for x in addr.split(b".")[:2])
    return a in (0, 10, 127) or a >= 224 or (a == 100 and 64 <= b <= 127) or (a, b) in ((169, 254), (192, 168)) or (a == 172 and 16 <= b <= 31)


def mask_doc(doc: bytes, email=EMAIL_PH, ip=IP_PH, public_ip_only=True):
    """(the masked document, e-mails, addresses)"""
    n = [0, 0]

    def repl(m):
        if m.group(1) is not None:
            n[0] += 1
            return email
        if public_ip_only and private(m.group(2)):
            return m.group(2)
        n[1] += 1
        return ip

    return BOTH.sub(repl, doc), n[0], n[1]


def pack(docs):
    off = np.zeros(len(docs) + 1, np.uint64)
    np.cumsum([len(d) for d in docs], out=off[1:])
    return np.frombuffer(b"".join(docs), np.uint8), off


def mask(docs, **spec) -> Ref:
    res = [mask_doc(d, **spec) for d in docs]
    text, off = pack([r[0] for r in res])
    ne, ni = np.array([r[1] for r in res], np.uint64), np.array([r[2] for r in res], np.uint64)
    return Ref(text, off, ne, ni, np.array([len(text), ne.sum(), ni.sum(), 0], np.uint64))
