"""Yardstick and inputs of the parameter-publish tests
(tests/test_publish_host.py, tests/test_gpu_publish.py).

``f32_to_bf16_bits`` / ``f32_to_f16_bits`` are integer models of the float32
-> bfloat16 / float16 conversion with round to nearest even: overflow goes to
inf, float16 subnormals are kept, a NaN stays a NaN (quiet bit set, payload
otherwise truncated; its payload is no property a caller may rely on).  The
host test pins them against torch's CPU ``.to()``; the GPU test computes its
expected replicas with them.

``expected_replica`` is the publish call's definition restated in numpy: the
replica's old words, with ``cvt(master[j])`` at every ``j = idx[i] < n`` for
``i`` below the count, and nothing changed when the count exceeds the
buffer's slots.
"""
from __future__ import annotations

import numpy as np

DT_F32, DT_BF16, DT_F16 = 0, 1, 2


def f32_to_bf16_bits(x: np.ndarray) -> np.ndarray:
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7fffffff) > 0x7f800000
    r = (u + 0x7fff + ((u >> np.uint64(16)) & 1)) >> np.uint64(16)
    r = np.where(nan, (u >> np.uint64(16)) | 0x40, r)
    return (r & 0xffff).astype(np.uint16)


def f32_to_f16_bits(x: np.ndarray) -> np.ndarray:
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.int64)
    sign = (u >> 16) & 0x8000
    a = u & 0x7fffffff
    e = (a >> 23) - 127
    sig = (a & 0x7fffff) | 0x800000
    # normal results (e >= -14): 10 of the 23 fraction bits stay; a carry out of
    # the fraction moves into the exponent, and out of exponent 30 into inf
    hn = ((e + 15) << 10) + ((sig >> 13) & 0x3ff)
    remn = sig & 0x1fff
    hn = hn + ((remn > 0x1000) | ((remn == 0x1000) & ((hn & 1) == 1)))
    # subnormal results (e < -14): the significand in units of 2^-24
    s = np.clip(-e - 1, 14, 40)
    hs = sig >> s
    rems = sig & ((np.int64(1) << s) - 1)
    half = np.int64(1) << (s - 1)
    hs = hs + ((rems > half) | ((rems == half) & ((hs & 1) == 1)))
    h = np.where(e >= -14, hn, hs)
    h = np.where(a < 0x00800000, 0, h)                    # float32 zeros and subnormals: far below 2^-25
    h = np.where((e > 15) | (h > 0x7c00), 0x7c00, h)      # overflow, inf
    h = np.where(a > 0x7f800000, 0x7e00 | ((a >> 13) & 0x3ff), h)  # NaN
    return (sign | h).astype(np.uint16)


def is_nan_bits(bits: np.ndarray, dtype: int) -> np.ndarray:
    if dtype == DT_F32:
        return (bits & 0x7fffffff) > 0x7f800000
    if dtype == DT_BF16:
        return (bits & 0x7fff) > 0x7f80
    return (bits & 0x7fff) > 0x7c00


def cvt_bits(master: np.ndarray, dtype: int) -> np.ndarray:
    """The replica words of a float32 array: uint32 (F32) or uint16."""
    if dtype == DT_F32:
        return np.ascontiguousarray(master, np.float32).view(np.uint32).copy()
    return f32_to_bf16_bits(master) if dtype == DT_BF16 else f32_to_f16_bits(master)


def expected_replica(old_bits: np.ndarray, master: np.ndarray, idx: np.ndarray, count: int, dtype: int):
    """(expected words, published element mask) of one replica."""
    out = old_bits.copy()
    pub = np.zeros(master.size, bool)
    if count <= idx.size:
        j = idx[:count].astype(np.int64)
        j = j[j < master.size]
        pub[j] = True
        out[pub] = cvt_bits(master, dtype)[pub]
    return out, pub


def exponent_class_values() -> np.ndarray:
    """float32 values over every exponent, both signs: fractions at, just below
    and just above the rounding ties of both 16-bit formats, fractions that
    round up into the next binade, +-0, subnormals, the values around each
    format's overflow threshold, +-inf and a few NaNs."""
    fr = np.array([0, 1, 0xfff, 0x1000, 0x1001, 0x1fff, 0x2000, 0x2fff, 0x3000, 0x3001, 0x7fff, 0x8000, 0x8001,
                   0x17fff, 0x18000, 0x18001, 0x7f7fff, 0x7f8000, 0x7fe000, 0x7fefff, 0x7ff000, 0x7ff001,
                   0x7fffff, 0x400000, 0x2aaaaa, 0x555555], np.uint32)
    ex = np.arange(256, dtype=np.uint32)
    u = (ex[:, None] << 23 | fr[None, :]).reshape(-1)
    rng = np.random.default_rng(5)
    u = np.concatenate([u, rng.integers(0, 1 << 31, 20000, dtype=np.uint32)])
    u = np.concatenate([u, u | 0x80000000])
    return u.view(np.float32)
