"""Inputs and expected values of the wire-form MERGE tests
(tests/test_wire_merge_host.py, tests/test_gpu_wire_merge.py).

A case is ``world`` rank streams of ``per_rank`` pairs in the wire form of
``flag``.  Its expected value is the oracle pair: ``oracle.wire_decode`` per
rank (the restatement tests/test_wire_oracle.py pins), then
``oracle.merge_decompress`` on the decoded pairs back to back.  The oracle's
merge indexes its dense array unchecked, as the reference would, so the pairs
the device drops (index >= n) are sent to a spare slot n that is cut from the
output.

Two input families:

* ``encoded``: u32 / f32 pairs with indices over [0, n), packed by the
  oracle's ``wire_encode`` -- the bytes the device's ``wire_encode`` writes
  (tests/test_gpu_wire.py).  With u16 indices every block index >= 32768
  saturates to 32767, so a rank repeats it and its last occurrence wins; tail
  indices >= 32768 truncate to themselves and survive.
* ``raw``: wire words as a peer could send them.  u16 block indices all
  >= 0x8000 (sign extension sends every one past n: dropped); special values
  (+-0, +-inf, NaN payloads, subnormals, 65504).

Values stay within the fp16 range and every non-finite value sits at an index
no other rank uses: inf + -inf and NaN + NaN pick their payload differently on
x86 and on the GPU, which is no property of the code under test.  With u32
indices one repeat and one index >= n are planted per rank (where per_rank
leaves room), since 2^20 random indices seldom give either.
"""
from __future__ import annotations

import zlib

import numpy as np

PER_RANK = [1, 7, 8, 9, 17, 1023, 1024, 1025, 4099]
FLAGS = [0, 1, 2, 3]
WORLDS = [1, 2, 3, 8]
FAMILIES = ["encoded", "raw"]

F32_SPECIAL = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc12345, 0x7fc00001,
                        0x00000001, 0x807fffff, 0x477fe000], np.uint32).view(np.float32)
F16_SPECIAL = np.array([0x0000, 0x8000, 0x7c00, 0xfc00, 0x7e00, 0xfe55, 0x7e01, 0x0001, 0x83ff, 0x7bff], np.uint16)
NSPEC = 10
SPEC_BASE = 64  # rank r's specials sit at indices SPEC_BASE + r * NSPEC + q, which no other pair takes


def n_of(flag: int) -> int:
    return 60000 if flag & 1 else 1 << 20


def wend(per_rank: int) -> int:
    return 8 * ((per_rank - 1) // 8) if per_rank else 0


def _values(rng, m):
    return (rng.standard_normal(m) * 10.0 ** rng.integers(-9, 4, m)).astype(np.float32)


def _indices(rng, m, n, world):
    """Indices over [0, n) clear of the specials' slots."""
    lo = SPEC_BASE + world * NSPEC
    return rng.integers(lo, n, m, dtype=np.uint32)


def make_streams(oracle, family: str, per_rank: int, flag: int, world: int, seed: int = 0, specials: bool = True):
    """``world`` streams [(widx, wval, flag)] as numpy arrays of exactly
    ``per_rank`` elements: u16 or u32 indices, u16 (fp16 bits) or f32 values.
    ``specials=False`` leaves the special values out (optimizer runs, where
    one inf would freeze amsgrad's running maximum for good)."""
    n = n_of(flag)
    we = wend(per_rank)
    rng = np.random.default_rng([zlib.crc32(family.encode()), per_rank, flag, world, seed])
    out = []
    for r in range(world):
        idx = _indices(rng, per_rank, n, world)
        val = _values(rng, per_rank)
        ns = min(NSPEC, we) if specials else 0  # in the block part only: the tail's fp16 form is an integer
        idx[:ns] = SPEC_BASE + r * NSPEC + np.arange(ns, dtype=np.uint32)
        if not flag & 1 and per_rank >= 3:
            idx[per_rank - 1] = idx[per_rank // 2]       # a repeat: the later one wins
            idx[per_rank // 2 + 1 if per_rank > 3 else 0] = n + r  # dropped
        if family == "encoded":
            val[:ns] = F32_SPECIAL[:ns]
            wi, wv = oracle.wire_encode(idx, val, flag)
        else:
            if flag & 1:
                wi = idx.astype(np.uint16)               # the tail: any 16-bit word (some >= n: dropped)
                wi[we:] = rng.integers(0, 65536, per_rank - we).astype(np.uint16)
                wi[:we] = rng.integers(0x8000, 0x10000, we).astype(np.uint16)  # blocks: all sign-extend past n
                wi[we] = rng.integers(0, n)              # ... but one survives
                if per_rank - we >= 2:
                    wi[per_rank - 1] = wi[we]            # and repeats within the tail
            else:
                wi = idx
            if flag & 2:
                _, wv = oracle.wire_encode(idx, val, 2)
                wv[we:] = rng.integers(0, 65536, per_rank - we).astype(np.uint16)
                wv[:ns] = F16_SPECIAL[:ns]
            else:
                wv = val
                wv[:ns] = F32_SPECIAL[:ns]
        out.append((np.ascontiguousarray(wi), np.ascontiguousarray(wv), flag))
    return out


def expected(oracle, streams, per_rank: int, n: int):
    """(decoded idx, decoded val, merged idx, merged val, stats): the decoded
    pairs back to back, the oracle's merge of them (index-ascending), and what
    the case exercises -- ``dups`` (pairs that lose to a later occurrence in
    their rank), ``dropped`` (index >= n) and ``tail`` (pairs of the scalar tail
    that reach the output)."""
    world = len(streams)
    we = wend(per_rank)
    di, dv = [], []
    dups = dropped = tail = 0
    for wi, wv, flag in streams:
        i, v = oracle.wire_decode(wi[:per_rank], wv[:per_rank], flag)
        di.append(i)
        dv.append(v)
        keep = i < n
        dropped += int((~keep).sum())
        pos = np.nonzero(keep)[0][::-1]
        _, first = np.unique(i[pos], return_index=True)
        last = pos[first]  # each surviving index's last position in the rank
        dups += int(keep.sum()) - last.size
        tail += int((last >= we).sum())
    idx = np.concatenate(di) if di else np.zeros(0, np.uint32)
    val = np.concatenate(dv) if dv else np.zeros(0, np.float32)
    spare = np.where(idx < n, idx, np.uint32(n)).astype(np.uint32)
    oi, ov = oracle.merge_decompress(spare, val, per_rank, world, n + 1)
    cut = oi < n
    return idx, val, oi[cut], ov[cut], {"dups": dups, "dropped": dropped, "tail": tail}


def all_cases():
    for family in FAMILIES:
        for flag in FLAGS:
            for world in WORLDS:
                for per_rank in PER_RANK:
                    yield family, per_rank, flag, world
