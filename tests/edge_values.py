"""Gradient buckets with the values a mixed-precision overflow step produces
(shared by the edge-value golden fixtures and GPU parity tests; not a test
module).

``edge_input(kind, n, seed_bucket, it)`` starts from
``synth(n, seed_for(seed_bucket, it), D1)`` and plants, at positions and with
signs drawn from synth.py's integer-only splitmix64 (never numpy.random: the
GPU side regenerates these inputs and must get the same bits):

inf            5 elements set to +-inf (both signs), each in a line of its own
inf_first      the same with max(5, n // 1024) infinities, so that for k about
               n / 100 (and for the small-k cases) at least k / 16 + 1 line
               sums are inf and the first threshold is inf
huge           4 whole lines of +-3e38: finite values, |x| sum = +inf
denorm_half    half the elements scaled by 1e-36 (in float64, rounded once)
denorm_all     every element scaled by 1e-37
negzero        97 % of the elements set to -0.0
wide_exp       magnitude bits uniform in [0, 0x7f800000), random sign
nan_steady     calls 0 and 1 clean; from call 2 on five NaNs of different
               payloads and signs, one of them in the last whole line and one
               in the ragged tail
nan_tail_only  calls 0 and 1 clean; from call 2 on one NaN in the ragged tail

A NaN in a key's first call is out of scope.
"""
from __future__ import annotations

import hashlib

import numpy as np

from stellatrain_amd.synth import D1, _splitmix64, seed_for, synth

FINITE_KINDS = ("inf", "inf_first", "huge", "denorm_half", "denorm_all", "negzero", "wide_exp")
NAN_KINDS = ("nan_steady", "nan_tail_only")
KINDS = FINITE_KINDS + NAN_KINDS

_NAN_PAYLOADS = (0x7FC00000, 0xFFC00001, 0x7FD2345F, 0xFFFFFFFF, 0x7FC0BEEF)


def draws(kind: str, seed_bucket: int, it: int, m: int) -> np.ndarray:
    """m 64-bit draws of the (kind, seed_bucket, it) stream."""
    salt = int.from_bytes(hashlib.sha256(kind.encode()).digest()[:4], "little")
    base = ((seed_for(seed_bucket, it) << 32) ^ salt) & 0xFFFFFFFFFFFFFFFF
    with np.errstate(over="ignore"):
        return _splitmix64(np.uint64(base) + np.arange(m, dtype=np.uint64) * np.uint64(0x9E3779B1))


def distinct(r: np.ndarray, mod: int, m: int) -> np.ndarray:
    """The first m distinct values of r % mod, in draw order."""
    c = (r % np.uint64(mod)).astype(np.int64)
    _, first = np.unique(c, return_index=True)
    out = c[np.sort(first)][:m]
    assert out.size == m, (mod, m)
    return out


def _f32(bits) -> np.ndarray:
    return np.asarray(bits, np.uint32).view(np.float32)


def edge_input(kind: str, n: int, seed_bucket: int, it: int) -> np.ndarray:
    x = synth(n, seed_for(seed_bucket, it), D1)
    lines, tail = n // 16, n % 16
    if kind in ("inf", "inf_first"):
        m = 5 if kind == "inf" else max(5, n // 1024)
        r = draws(kind, seed_bucket, it, 8 * m + 64)
        ln = distinct(r, lines, m)
        pos = ln * 16 + ((r[:m] >> np.uint64(40)) % np.uint64(16)).astype(np.int64)
        x[pos] = _f32(np.where(np.arange(m) & 1, 0xFF800000, 0x7F800000))
    elif kind == "huge":
        r = draws(kind, seed_bucket, it, 96)
        for j, l in enumerate(distinct(r, lines, 4)):
            neg = (r[32 + j] >> np.arange(16, dtype=np.uint64)) & np.uint64(1)
            x[l * 16:l * 16 + 16] = np.where(neg == 1, np.float32(-3e38), np.float32(3e38))
    elif kind == "denorm_half":
        half = (draws(kind, seed_bucket, it, n) >> np.uint64(33)) & np.uint64(1)
        x = np.where(half == 1, x.astype(np.float64) * 1e-36, x.astype(np.float64)).astype(np.float32)
    elif kind == "denorm_all":
        x = (x.astype(np.float64) * 1e-37).astype(np.float32)
    elif kind == "negzero":
        z = (draws(kind, seed_bucket, it, n) >> np.uint64(20)) % np.uint64(100)
        x[z < 97] = np.float32(-0.0)
    elif kind == "wide_exp":
        r = draws(kind, seed_bucket, it, n)
        mag = ((r >> np.uint64(8)) % np.uint64(0x7F800000)).astype(np.uint32)
        x = _f32(mag | ((r & np.uint64(1)).astype(np.uint32) << np.uint32(31))).copy()
    elif kind in NAN_KINDS:
        if it >= 2:
            r = draws(kind, seed_bucket, it, 64)
            # the ragged tail (the last whole line where there is none)
            tail_pos = lines * 16 + int(r[0] % np.uint64(tail)) if tail else n - 1 - int(r[0] % np.uint64(16))
            if kind == "nan_tail_only":
                pos = np.array([tail_pos], np.int64)
            else:
                last_line = (lines - 1) * 16 + int(r[1] % np.uint64(16))
                if last_line == tail_pos:
                    last_line -= 1
                body = distinct(r[8:], max(lines - 1, 1), 3) * 16 + ((r[2:5] >> np.uint64(40)) % np.uint64(16)).astype(np.int64)
                pos = np.concatenate([[tail_pos, last_line], body])
            xb = x.view(np.uint32)
            rot = int(r[5] % np.uint64(5))
            xb[pos] = np.array([_NAN_PAYLOADS[(rot + j) % 5] for j in range(pos.size)], np.uint32)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x, np.float32)


def sha_input(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()
