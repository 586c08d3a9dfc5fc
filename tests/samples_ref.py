"""The rule of the supervised samples (include/tiktoken_amd.h, tk_assemble_samples_device) restated as plain Python loops over lists, from
its description -- not from the kernels: the host loop an SFT script writes, with truncation, padding and n_trained.  What
tests/test_samples_sim.py and tests/test_gpu_samples.py compare the CPU simulation and the device with."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

IGNORE = -100


class Role(NamedTuple):
    before: tuple = ()
    after: tuple = ()
    train: bool = False


class Samples(NamedTuple):
    ids: np.ndarray  # uint32[R, W]
    mask: np.ndarray  # uint8[R, W]
    labels: np.ndarray  # int32[R, W]
    len: np.ndarray  # uint32[R]
    full_len: np.ndarray  # uint64[R]
    n_trained: np.ndarray  # uint32[R]


class Refused(ValueError):
    pass


def samples_rule(tokens, tok_off, part_role, sample_off, roles, max_len: int, *, width_multiple: int = 0, bos=None, eos=None, pad: int = 0, ignore: int = IGNORE,
                 keep_tail: bool = False, left: bool = False) -> Samples:
    tokens = [int(x) for x in tokens]
    off = [int(x) for x in tok_off]
    so = [int(x) for x in sample_off]
    part_role = [int(x) for x in part_role]
    n_parts, R = len(off) - 1, len(so) - 1
    if max_len == 0:
        raise Refused("max_len")
    if not roles and n_parts:
        raise Refused("no roles")
    if len(roles) > 256 or sum(len(r.before) + len(r.after) for r in roles) > 4096:
        raise Refused("role table")
    if off[0] != 0 or off[-1] != len(tokens) or any(a > b for a, b in zip(off, off[1:])):
        raise Refused("tok_off")
    if so[0] != 0 or so[-1] != n_parts or any(a > b for a, b in zip(so, so[1:])):
        raise Refused("sample_off")
    if any(r >= len(roles) for r in part_role):
        raise Refused("part_role")
    rows = []
    for s in range(R):
        ids, trained = ([bos], [False]) if bos is not None else ([], [])
        last_trains = False
        for p in range(so[s], so[s + 1]):
            role = roles[part_role[p]]
            head, body, tail = list(role.before), tokens[off[p]:off[p + 1]], list(role.after)
            ids += head + body + tail
            trained += [False] * len(head) + [bool(role.train)] * (len(body) + len(tail))
            last_trains = bool(role.train)
        if eos is not None:
            ids.append(eos)
            trained.append(last_trains)
        full = len(ids)
        n = min(full, max_len)
        if keep_tail:
            ids, trained = ids[full - n:], trained[full - n:]
        else:
            ids, trained = ids[:n], trained[:n]
        rows.append((ids, trained, full))
    longest = max((len(r[0]) for r in rows), default=0)
    W = max_len if width_multiple == 0 else min(max_len, -(-longest // width_multiple) * width_multiple)
    total = sum(len(r.before) + len(r.after) for r in (roles[x] for x in part_role)) + len(tokens)
    if len(tokens) >= 2**32 or n_parts >= 2**32 - 1 or R >= 2**32 - 1 or total >= 2**32 or R * W >= 2**32:
        raise Refused("32-bit")
    out_ids, out_mask, out_lab = [], [], []
    for ids, trained, _ in rows:
        n = len(ids)
        fill = W - n
        lab = [v if t else ignore for v, t in zip(ids, trained)]
        if left:
            out_ids.append([pad] * fill + ids)
            out_mask.append([0] * fill + [1] * n)
            out_lab.append([ignore] * fill + lab)
        else:
            out_ids.append(ids + [pad] * fill)
            out_mask.append([1] * n + [0] * fill)
            out_lab.append(lab + [ignore] * fill)
    lab64 = np.array(out_lab, dtype=np.int64).reshape(R, W)
    lab64[lab64 >= 2**31] -= 2**32  # (an id of 2^31 and more, seen as the int32 the labels are)
    return Samples(np.array(out_ids, dtype=np.uint32).reshape(R, W), np.array(out_mask, dtype=np.uint8).reshape(R, W), lab64.astype(np.int32),
                   np.array([len(r[0]) for r in rows], dtype=np.uint32), np.array([r[2] for r in rows], dtype=np.uint64),
                   np.array([sum(r[1]) for r in rows], dtype=np.uint32))


def same(got: Samples, want: Samples, ctx):
    for name in Samples._fields:
        g, w = getattr(got, name), getattr(want, name)
        assert g.dtype == w.dtype, (name, ctx, g.dtype, w.dtype)
        assert g.shape == w.shape and np.array_equal(g, w), (name, ctx, np.argwhere(g != w)[:5].tolist() if g.shape == w.shape else (g.shape, w.shape))


def pack(samples):
    """samples: a list of samples, each a list of (role index, [body ids]) -> (tokens uint32, tok_off uint64, part_role uint8, sample_off uint64)"""
    tokens, tok_off, part_role, sample_off = [], [0], [], [0]
    for parts in samples:
        for role, body in parts:
            tokens += body
            tok_off.append(len(tokens))
            part_role.append(role)
        sample_off.append(len(part_role))
    return np.array(tokens, dtype=np.uint32), np.array(tok_off, dtype=np.uint64), np.array(part_role, dtype=np.uint8), np.array(sample_off, dtype=np.uint64)


# three role tables: a chat template (system and user untrained, assistant trained; role 3 has no ids at all), everything trained, nothing trained
CHAT = (Role((90001, 90002), (90003,), False), Role((90001, 90004, 90005), (90003, 90006), False), Role((90001, 90007), (90003,), True), Role((), (), True),
        Role((), (90008,), False), Role((90009,), (), True))
ALL_TRAINED = tuple(r._replace(train=True) for r in CHAT)
NONE_TRAINED = tuple(r._replace(train=False) for r in CHAT)
SPECIALS = [(None, None), (1, None), (None, 2), (1, 2)]  # (bos, eos)


def settings():
    """What a max_len is crossed with: head / tail, padding behind / in front, the width multiples"""
    return [dict(keep_tail=kt, left=left, width_multiple=wm) for kt in (False, True) for left in (False, True) for wm in (0, 1, 8)]


def cases(block: int, rng):
    """The case list of both test files around workgroups of `block` positions: (name, samples, [max_len ...]); a sample is a list of
    (role, body).  Ids are random below 50000, roles index CHAT.  The callers cross every max_len with bos / eos and settings()."""
    def body(n):
        return rng.integers(0, 50000, size=n).tolist()

    def sample(*sizes):
        return [(int(rng.integers(0, len(CHAT))), body(n)) for n in sizes]

    def empties(n):  # parts that contribute no element: no body, a role without ids
        return [(3, [])] * n

    B = block
    return [
        ("empty batch", [], [1, 7]),
        ("only empty samples", [[], [], []], [1, 4, 9]),
        ("empty samples first, middle and last", [[], sample(3, 0, 5), [], [], sample(9), []], [1, 3, 7, 8, 9, 17]),
        ("only parts without elements", [empties(3), empties(1), []], [1, 5]),
        ("one token", [[(3, body(1))]], [1, 3, 8]),
        ("runs of empty parts at the start, middle and end", [empties(40) + sample(5) + empties(70) + sample(20, 3) + empties(9), sample(4)], [3, 7, 8, 64]),
        ("runs of empty parts across a sample boundary", [sample(6) + empties(5), empties(7) + sample(2), empties(3), empties(2) + [(3, body(4))] + empties(2)], [1, 3, 7, 9, 17]),
        ("one sample over three workgroups", [sample(B, 7, B // 2, 0, B // 2 + 11)], [7, B, 2 * B + 5, 3 * B]),
        ("row boundaries at block - 1, block, block + 1", [[(3, body(B - 1))], [(3, body(1))], [(3, body(B))], [(3, body(B + 1))], sample(B // 2 + 3)], [7, 8, B - 1, B, B + 1]),
        ("conversations", [sample(*rng.integers(0, 30, size=int(rng.integers(1, 9))).tolist()) for _ in range(40)], [1, 3, 7, 8, 9, 17, 64]),
    ]
