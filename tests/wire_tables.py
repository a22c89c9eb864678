"""Input tables of the wire-cast parity tests (tests/test_wire_isa_host.py,
tests/test_gpu_wire_exhaustive.py).  Test infrastructure, not a test module.

Everything here is deterministic and built from integer arithmetic on bit
patterns (no float16 cast of numpy's, no conversion under test) or from
synth.py's splitmix64:

* ``F32_BOUNDARY``  every float32 at which a float32 -> binary16 conversion
  can go wrong: each non-NaN binary16 value, each midpoint between
  neighbouring magnitudes (ties; 65,520 above 0x7bff), each of those +-1 and
  +-2 float32 ulps, both signs; the zeros, infinities, float32 subnormals, the
  2^-25 flush edge, FLT_MAX; NaNs over the whole payload range.
* ``F16_ALL``       all 65,536 16-bit words (value words and index words).
* ``TAIL_F32``      edges of the tail's truncation to int32 / low 16 bits.
* ``IDX_U32``       edges of the index casts.
* ``TAIL_U16``      16-bit words of the receiver's tail casts.
* ``tail_streams``  a table laid out over streams of 1-8, 9, 16 and 17 pairs
  so that every entry sits at a tail position (and at block positions too).
* ``boundary_bucket``  gradient buckets made of boundary values only, for the
  writers that fuse the encode into a compress.
"""
from __future__ import annotations

import functools

import numpy as np

from stellatrain_amd.synth import _splitmix64, seed_for

SIGN = 0x80000000


def simd_end(m: int) -> int:
    """First tail position of a stream of m pairs (comm_manager.cpp: blocks while i + 8 < m)."""
    return 8 * ((m - 1) // 8) if m else 0


def _ilog2(q: np.ndarray) -> np.ndarray:
    q = q.astype(np.int64)
    p = np.zeros(q.shape, np.int64)
    for s in (16, 8, 4, 2, 1):
        big = (q >> (p + s)) > 0
        p += np.where(big, s, 0)
    return p


def scaled_bits(q, e: int) -> np.ndarray:
    """float32 bit patterns of q * 2^e for integers 0 < q < 2^24 (exact), 0 for q = 0."""
    q = np.asarray(q, np.int64)
    p = _ilog2(np.maximum(q, 1))
    ex = p + e + 127
    assert (ex[q > 0] > 0).all() and (ex < 255).all()
    bits = (ex << 23) | ((q << (23 - p)) & 0x7FFFFF)
    return np.where(q > 0, bits, 0).astype(np.int64)


def f16_exact_bits(mag) -> np.ndarray:
    """float32 bit patterns (int64) of the finite binary16 magnitudes 0..0x7bff."""
    mag = np.asarray(mag, np.int64)
    assert ((mag >= 0) & (mag <= 0x7BFF)).all()
    ex, man = mag >> 10, mag & 0x3FF
    normal = ((ex + 112) << 23) | (man << 13)
    return np.where(ex > 0, normal, scaled_bits(man, -24))


def f16_mid_bits(mag) -> np.ndarray:
    """float32 bit patterns of the midpoint between magnitude word `mag` and
    mag + 1: an exact tie of round-to-nearest.  0x7bff gives 65,520."""
    mag = np.asarray(mag, np.int64)
    ex, man = mag >> 10, mag & 0x3FF
    normal = (((ex + 112) << 23) | (man << 13)) + 0x1000
    return np.where(ex > 0, normal, scaled_bits(2 * man + 1, -25))


def is_tie(val: np.ndarray) -> np.ndarray:
    """Which float32 values lie exactly halfway between two neighbouring
    binary16 values (65,520 counts: halfway to the binade binary16 lacks)."""
    u = np.ascontiguousarray(val, np.float32).view(np.uint32).astype(np.int64) & 0x7FFFFFFF
    ex, man = u >> 23, u & 0x7FFFFF
    normal = (ex >= 113) & (ex <= 142) & ((man & 0x1FFF) == 0x1000)
    sh = np.clip(126 - ex, 14, 24)            # bits dropped in the binary16 subnormal range
    full = man | 0x800000
    sub = (ex >= 102) & (ex <= 112) & ((full & ((1 << sh) - 1)) == (1 << (sh - 1)))
    return normal | sub


def _draws(seed: int, n: int) -> np.ndarray:
    with np.errstate(over="ignore"):
        return _splitmix64(np.uint64(seed) * np.uint64(0x100000001B3) + np.arange(n, dtype=np.uint64))


FIXED_NANS = (0x7F800001, 0x7FBFFFFF, 0x7FC00000, 0xFFC12345, 0x7FFFFFFF)
NANS_PER_SIGN = 4096


def _nans() -> np.ndarray:
    out = []
    for s, sign in enumerate((0, SIGN)):
        r = _draws(0xA11 + s, NANS_PER_SIGN)
        payload = (r % np.uint64(0x7FFFFF)).astype(np.int64) + 1       # 1 .. 0x7fffff
        out.append(sign | 0x7F800000 | payload)
    # payloads that live in the 13 dropped bits only: without the quiet bit they would become inf
    low = np.array([1, 2, 0xFFF, 0x1000, 0x1FFF], np.int64)
    out += [0x7F800000 | low, SIGN | 0x7F800000 | low, np.array(FIXED_NANS, np.int64)]
    return np.concatenate(out)


@functools.lru_cache(maxsize=None)
def f32_boundary() -> np.ndarray:
    mags = np.arange(0x7C00, dtype=np.int64)
    base = np.concatenate([f16_exact_bits(mags), f16_mid_bits(mags)])
    near = np.concatenate([base + d for d in (0, -1, 1, -2, 2)])
    near = near[near >= 0]                                              # 0 - 1 ulp, 0 - 2 ulps do not exist
    extra = np.array([0x00000000, 0x7F800000, 0x00000001, 0x007FFFFF, 0x32FFFFFF, 0x33000000, 0x33000001,
                      0x7F7FFFFF], np.int64)
    mag = np.concatenate([near, extra])
    assert (mag <= 0x7F800000).all()
    bits = np.concatenate([mag, mag | SIGN, _nans()]).astype(np.uint32)
    bits.setflags(write=False)
    return bits


def as_f32(bits) -> np.ndarray:
    return np.ascontiguousarray(bits, np.uint32).view(np.float32)


def block_pad(a: np.ndarray) -> np.ndarray:
    """`a` followed by 8 zero elements: every element of `a` is a block position."""
    out = np.concatenate([a, np.zeros(8, a.dtype)])
    assert simd_end(out.size) >= a.size
    return out


F16_ALL = np.arange(65536, dtype=np.uint32).astype(np.uint16)
F16_ALL.setflags(write=False)
F16_NAN_WORDS = int(np.count_nonzero((F16_ALL & 0x7FFF) > 0x7C00))     # 2,046
F16_SNAN_WORDS = int(np.count_nonzero(((F16_ALL & 0x7FFF) > 0x7C00) & ((F16_ALL & 0x0200) == 0)))  # 1,022


def _f(x) -> int:
    return int(np.array([x], np.float32).view(np.uint32)[0])


TAIL_F32_BITS = np.array(
    [0x00000000, 0x80000000, _f(0.5), _f(-0.5), 0x3F7FFFFF, _f(1.0), _f(-1.0), _f(-0.99),
     _f(65535.0), _f(65535.996), _f(65536.0), _f(65537.5), _f(131071.5),
     _f(-32768.5), _f(-65536.0), _f(-65537.0),
     0x4EFFFFFF, 0x4F000000, 0x4F000001, 0xCF000000, 0xCF000001,          # 2^31 - 128, 2^31, 2^31 + 256, -2^31, -2^31 - 256
     _f(3e9), _f(-3e9), 0x4F800000, 0x7F800000, 0xFF800000,               # +-3e9, 2^32, +-inf
     0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFBFFFFF,                      # NaNs of both signs, quiet and signalling
     0x00000001, 0x80000001, _f(1e38), _f(-1e38),                         # +-1e-45, +-1e38
     _f(1.5), _f(-1.5), _f(32767.9), _f(32768.0), _f(-32769.0), _f(4294901760.0)], np.uint32)
TAIL_F32 = TAIL_F32_BITS.view(np.float32)
assert TAIL_F32[4] == np.float32(0.99999994) and TAIL_F32[16] == np.float32(2147483520.0)

IDX_U32 = np.array([0, 1, 32766, 32767, 32768, 32769, 65535, 65536, 65537, 0x7FFFFFFF, 0x80000000, 0x80000001,
                    0xFFFF7FFF, 0xFFFF8000, 0xFFFF8001, 0xFFFFFFFF], np.uint32)

TAIL_U16 = np.array([0, 1, 2, 0x3FF, 0x400, 0x3C00, 0x7BFF, 0x7C00, 0x7C01, 0x7DFF, 0x7E00, 0x7FFF, 0x8000, 0x8001,
                     0x83FF, 0xFBFF, 0xFC00, 0xFC01, 0xFDFF, 0xFE00, 0xFFFF, 32767, 32768, 32769, 65535], np.uint16)

TAIL_LENGTHS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17)


def tail_streams(table: np.ndarray, streams: int = 0) -> list:
    """Index sets into `table`, one per stream, stream lengths cycling through
    TAIL_LENGTHS until every entry has sat at a tail position (and at least
    `streams` streams and every length exist).  A stream's tail takes the next
    entries not yet seen there; its block positions (lengths 9, 16, 17) take
    the entries that follow, so entries reach block positions as well.
    Returns [positions (int64 array of the stream's length, blocks first)]."""
    t = table.size
    out, nxt, j = [], 0, 0
    while nxt < t or j < max(streams, len(TAIL_LENGTHS)):
        m = TAIL_LENGTHS[j % len(TAIL_LENGTHS)]
        j += 1
        se = simd_end(m)
        tail = (nxt + np.arange(m - se)) % t
        nxt += m - se
        blocks = (nxt + np.arange(se)) % t
        out.append(np.concatenate([blocks, tail]).astype(np.int64))
    return out


def tail_cases(values: np.ndarray, indices: np.ndarray) -> list:
    """(idx, val) streams carrying a value table and an index table through
    tail_streams: every value entry and every index entry at a tail position.
    Stream j has the same length for both; the shorter table repeats."""
    ns = max(len(tail_streams(values)), len(tail_streams(indices)))
    vs, xs = tail_streams(values, ns), tail_streams(indices, ns)
    assert len(vs) == len(xs) == ns
    return [(np.ascontiguousarray(indices[px]), np.ascontiguousarray(values[pv])) for pv, px in zip(vs, xs)]


def covers_tail(cases, table: np.ndarray, which: int) -> bool:
    """Every entry of `table` (by bit pattern) sits at a tail position of some case."""
    seen = set()
    for c in cases:
        a = np.ascontiguousarray(c[which])
        a = a.view(np.uint32) if a.itemsize == 4 else a.view(np.uint16)
        seen.update(a[simd_end(a.size):].tolist())
    t = np.ascontiguousarray(table)
    t = t.view(np.uint32) if t.itemsize == 4 else t.view(np.uint16)
    return set(t.tolist()) <= seen


# ---------------------------------------------------------------------------
# boundary buckets
# ---------------------------------------------------------------------------
BANDS = ("normal", "sub", "top")


def boundary_bucket(n: int, seed_bucket: int, it: int, band: str) -> np.ndarray:
    """A gradient bucket of n float32 elements every one of which is a
    boundary value: element i is (exact | mid - 1 ulp | mid | mid + 1 ulp) of a
    drawn binary16 magnitude word, with a drawn sign.  Bands:

    * ``normal``  exponent fields 10-20 (2^-5 .. 2^6);
    * ``sub``     words 1-0x3ff; one draw in eight takes word 0, 1 or 0x3ff
                  instead: the midpoints of 0 and 1 are 2^-25 (the flush edge)
                  and 1.5 * 2^-24, their exact values 0 and 2^-24, and the
                  midpoint of 0x3ff rounds up into the first normal, 0x0400;
    * ``top``     words 0x7800-0x7bff; one draw in eight takes 0x7bff, whose
                  midpoint is 65,520 (rounds to inf) and mid + 1 ulp lies above it.
    """
    r = _draws(seed_for(seed_bucket, it), n)
    kind = (r & np.uint64(3)).astype(np.int64)
    neg = ((r >> np.uint64(2)) & np.uint64(1)).astype(np.int64)
    edge = ((r >> np.uint64(3)) & np.uint64(7)).astype(np.int64) == 0
    a = ((r >> np.uint64(8)) & np.uint64(0xFFFF)).astype(np.int64)
    b = ((r >> np.uint64(24)) & np.uint64(0xFFFF)).astype(np.int64)
    if band == "normal":
        word = ((10 + a % 11) << 10) | (b & 0x3FF)
    elif band == "sub":
        word = np.where(edge, np.choose(a & 3, [0, 1, 0x3FF, 0x3FF]), 1 + b % 0x3FF)
    elif band == "top":
        word = np.where(edge, 0x7BFF, 0x7800 + (b & 0x3FF))
    else:
        raise ValueError(band)
    exact, mid = f16_exact_bits(word), f16_mid_bits(word)
    bits = np.choose(kind, [exact, mid - 1, mid, mid + 1])
    return (bits | (neg << 31)).astype(np.uint32).view(np.float32)


# Sequences of section D (tests/test_gpu_wire_exhaustive.py), pinned on the CPU by
# tests/test_wire_isa_host.py: (key, n, k, bands per call, seed bucket)
SEQ_BANDS = (("normal",) * 3, ("sub",) * 3, ("top",) * 3, ("normal", "sub", "top", "normal"))
D_N, D_K = (1 << 18) - 19, 2621                   # ragged last line; k % 8 != 0: the stream has a tail
D_ONE = tuple((f"bb{j}@w", D_N, D_K, bands, 3000 + j) for j, bands in enumerate(SEQ_BANDS))
D_BATCH = (("bn@w", 100013, 1007, ("normal",) * 3, 3010), ("bs@w", 65541, 655, ("sub",) * 3, 3011),
           ("bt@w", D_N, D_K, ("top",) * 3, 3012))
# send path: exact binary16 values in source 0, zeros in source 1 (their sum is again a boundary value)
D_SEND = (("sn@s", 60013, ("normal",) * 3, 3020), ("st@s", 40013, ("top",) * 3, 3021),
          ("sm@s", 60000, ("normal", "sub", "top", "normal"), 3022))


# ---------------------------------------------------------------------------
# streams shared by the host and the GPU tests
# ---------------------------------------------------------------------------
def boundary_stream():
    """(idx, val): F32_BOUNDARY in one stream, all of it at block positions;
    the indices count up from 0, so the block cast meets 32,766-32,769 and
    65,535-65,537 as well."""
    val = block_pad(as_f32(f32_boundary()))
    return np.arange(val.size, dtype=np.uint32), val


def table_block_stream():
    """(idx, val): TAIL_F32 and IDX_U32 (repeated to the same length) at block positions."""
    m = max(TAIL_F32.size, IDX_U32.size)
    return block_pad(np.resize(IDX_U32, m)), block_pad(np.resize(TAIL_F32, m))


@functools.lru_cache(maxsize=None)
def encode_tail_cases():
    """[(idx u32, val f32)]: TAIL_F32 and IDX_U32 through the tail streams."""
    cases = tail_cases(TAIL_F32, IDX_U32)
    assert covers_tail(cases, TAIL_F32, 1) and covers_tail(cases, IDX_U32, 0)
    assert {c[0].size for c in cases} == set(TAIL_LENGTHS)
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def decode_tail_cases():
    """[(widx u16, wval u16)]: TAIL_U16 as index and as value words through the tail streams."""
    cases = tail_cases(TAIL_U16, TAIL_U16[::-1].copy())
    assert covers_tail(cases, TAIL_U16, 0) and covers_tail(cases, TAIL_U16, 1)
    return tuple(cases)


def f16_all_stream():
    """(widx u16, wval u16): all 65,536 words at block positions (plus 8)."""
    return block_pad(F16_ALL), block_pad(F16_ALL)


def wide_forms(w16_idx: np.ndarray, w16_val: np.ndarray, flag: int):
    """The received arrays of a decode case in the form `flag` names: the
    16-bit words where its bit is set, else 32-bit arrays of the same length
    (indices spread over the u32 range, values from F32_BOUNDARY)."""
    m = w16_idx.size
    wi = w16_idx if flag & 1 else (w16_idx.astype(np.uint32) * np.uint32(65537))
    wv = w16_val if flag & 2 else as_f32(np.resize(f32_boundary()[::97], m)).copy()
    return np.ascontiguousarray(wi), np.ascontiguousarray(wv)


def sha(a: np.ndarray) -> str:
    import hashlib
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.view(np.uint8).tobytes()).hexdigest()


def table_digests() -> dict:
    out = {"F32_BOUNDARY": sha(f32_boundary()), "F16_ALL": sha(F16_ALL), "TAIL_F32": sha(TAIL_F32_BITS),
           "IDX_U32": sha(IDX_U32), "TAIL_U16": sha(TAIL_U16)}
    for band in BANDS:
        out[f"boundary_bucket/{band}"] = sha(boundary_bucket(4099, 3000, 1, band))
    return out


def isa_digests(isa) -> dict:
    """SHA-256 of what each instruction gives on the tables (oracle.IsaWire)."""
    b = as_f32(f32_boundary())
    idx = np.concatenate([IDX_U32, np.arange(0, 1 << 17, dtype=np.uint32), np.uint32(0xFFFFFFFF) - np.arange(1 << 17, dtype=np.uint32)])
    return {"cvtps_ph/F32_BOUNDARY": sha(isa.cvtps_ph(b)), "cvtps_ph/TAIL_F32": sha(isa.cvtps_ph(TAIL_F32)),
            "cvtph_ps/F16_ALL": sha(isa.cvtph_ps(F16_ALL)),
            "packs_epi32/IDX": sha(isa.packs_epi32(idx)), "cvtepi16_epi32/F16_ALL": sha(isa.cvtepi16_epi32(F16_ALL)),
            "cvttss_lo16/TAIL_F32": sha(isa.cvttss_lo16(TAIL_F32)), "cvttss_lo16/F32_BOUNDARY": sha(isa.cvttss_lo16(b)),
            "u16_to_f32/F16_ALL": sha(isa.u16_to_f32(F16_ALL))}


@functools.lru_cache(maxsize=None)
def bucket_sequence(oracle, key: str, n: int, k: int, bands: tuple, seed_bucket: int, gathered: bool = False):
    """The oracle's thresholdv16 results for one key called once per entry of
    `bands` on boundary_bucket(n, seed_bucket, call, band): out[call] = (src,
    count, idx, val, state after, state before).  `gathered`: the bucket is the
    gather-add of the boundary bucket and a source of zeros (x + 0: every -0
    becomes +0, everything else stays).  Computed once, read-only."""
    h = oracle.tv16_new()
    out = []
    for it, band in enumerate(bands):
        x = boundary_bucket(n, seed_bucket, it, band)
        if gathered:
            x = (x + np.zeros(n, np.float32)).astype(np.float32)
        before = oracle.tv16_state(h, key)
        co, io, vo = oracle.tv16_compress(h, key, x, k)
        for a in (x, io, vo):
            a.setflags(write=False)
        out.append((x, co, io, vo, oracle.tv16_state(h, key), before))
    oracle.tv16_free(h)
    return tuple(out)


def d_sequences(oracle):
    """Every boundary_bucket sequence of section D as bucket_sequence's
    arguments (key, n, k, bands, seed bucket, gathered)."""
    return tuple(c + (False,) for c in D_ONE + D_BATCH) + send_sequences(oracle)


def send_sequences(oracle):
    """The send path's: k as the engine picks it (ratio 0.99), the gather-add applied."""
    return tuple((key, n, oracle.merge_numel(n, 0.99), bands, sb, True) for key, n, bands, sb in D_SEND)
