"""Pin the wire-format oracle (oracle/stg_oracle.cpp orc_wire_*) to the x86
instructions the reference's casts execute, on the CPU.

``oracle.IsaWire`` (oracle/isa_wire.cpp) runs the instructions themselves --
vcvtps2ph, vcvtph2ps, packssdw, vpmovsxwd, vcvttss2si -- and composes the
block / tail rule in Python; it shares no conversion code with the oracle's
restatement or with csrc/wire_dev.h (whose fp16 casts are the oracle's text).
The inputs are tests/wire_tables.py: every binary16 word, every float32 at a
rounding boundary of the narrowing, NaNs over the payload range, the edges of
the index and tail casts, each in block and in tail positions.

Also here: the tables' and the instruction outputs' SHA-256 against
tests/golden/manifest_wire_isa.json (another CPU or compiler that changes the
yardstick is noticed), numpy restatements of wrong conversions that the tables
must tell from the right ones, and the conditions the boundary buckets of
tests/test_gpu_wire_exhaustive.py section D rely on.
"""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

import wire_tables as T
from geometry import tv16_head

MANIFEST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "manifest_wire_isa.json")


@pytest.fixture(scope="module")
def isa():
    from oracle.oracle import IsaWire
    return IsaWire()


def _u(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16) if a.itemsize == 2 else a.view(np.uint32)


def _diff(a, b):
    a, b = _u(a), _u(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    return np.flatnonzero(a != b)


def _encode_streams():
    yield ("boundary",) + T.boundary_stream()
    yield ("tables in blocks",) + T.table_block_stream()
    for j, (idx, val) in enumerate(T.encode_tail_cases()):
        yield (f"tail stream {j} ({idx.size})", idx, val)


def _decode_streams(all_tails: bool):
    yield ("f16 all",) + T.f16_all_stream()
    for j, (wi, wv) in enumerate(T.decode_tail_cases()):
        yield (f"tail stream {j} ({wi.size})", wi, wv)
    if all_tails:  # every word at a tail position: 8,192 streams of 8 (all tail)
        for j in range(0, 65536, 8):
            yield (f"f16 words {j}..{j + 7} as a tail", T.F16_ALL[j:j + 8], T.F16_ALL[j:j + 8][::-1].copy())


# ---------------------------------------------------------------------------
# 1. the oracle equals the instructions, bit for bit, NaNs included
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("flag", [0, 1, 2, 3])
def test_oracle_encode_equals_instructions(oracle, isa, flag):
    for name, idx, val in _encode_streams():
        oi, ov = oracle.wire_encode(idx, val, flag)
        ei, ev = isa.encode(idx, val, flag)
        assert not _diff(oi, ei).size, (name, flag)
        bad = _diff(ov, ev)
        assert not bad.size, (name, flag, bad.size, hex(int(_u(val)[bad[0]])), hex(int(_u(ov)[bad[0]])),
                              hex(int(_u(ev)[bad[0]])))


@pytest.mark.parametrize("flag", [0, 1, 2, 3])
def test_oracle_decode_equals_instructions(oracle, isa, flag):
    """Fails on the sNaN words alone (1,022 of them in the full stream) when
    the oracle's widening leaves a signalling NaN signalling."""
    for name, w16i, w16v in _decode_streams(all_tails=True):
        wi, wv = T.wide_forms(w16i, w16v, flag)
        oi, ov = oracle.wire_decode(wi, wv, flag)
        ei, ev = isa.decode(wi, wv, flag)
        assert not _diff(oi, ei).size, (name, flag)
        bad = _diff(ov, ev)
        assert not bad.size, (name, flag, f"{bad.size} words differ", hex(int(_u(wv)[bad[0]])),
                              hex(int(_u(ov)[bad[0]])), hex(int(_u(ev)[bad[0]])))


def test_round_trip_through_the_instructions_is_the_identity(isa):
    """Table sanity: every finite binary16 word widens and narrows to itself,
    every NaN word to itself with the quiet bit."""
    f = isa.cvtph_ps(T.F16_ALL)
    back = isa.cvtps_ph(f)
    nan = (T.F16_ALL & 0x7FFF) > 0x7C00
    assert np.array_equal(back[~nan], T.F16_ALL[~nan])
    assert np.array_equal(back[nan], T.F16_ALL[nan] | 0x0200)
    assert int(nan.sum()) == T.F16_NAN_WORDS == 2046 and T.F16_SNAN_WORDS == 1022
    # the table's own integer widening is the instruction's
    mags = np.arange(0x7C00)
    assert np.array_equal(T.f16_exact_bits(mags).astype(np.uint32), f[:0x7C00].view(np.uint32))


def test_tables_hold_what_they_promise(isa):
    b = T.f32_boundary()
    assert b.size >= 640000
    val = T.as_f32(b)
    nan = np.isnan(val)
    assert int((nan & (b < 0x80000000)).sum()) >= 4096 and int((nan & (b >= 0x80000000)).sum()) >= 4096
    for x in T.FIXED_NANS + (0, 0x80000000, 0x7F800000, 0xFF800000, 1, 0x007FFFFF, 0x32FFFFFF, 0x33000000,
                             0x33000001, 0x7F7FFFFF, 0x477FF000):
        assert (b == x).any(), hex(x)
    ties = T.is_tie(val[~nan])
    assert np.unique(b[~nan][ties]).size == 2 * 0x7C00         # one per magnitude word and sign
    # is_tie against the instruction: a tie is where +1 ulp and -1 ulp round to different words
    t = b[~nan][ties]
    lo, hi = isa.cvtps_ph(T.as_f32(t - 1)), isa.cvtps_ph(T.as_f32(t + 1))
    assert np.all((hi & 0x7FFF) == (lo & 0x7FFF) + 1)
    # block positions
    idx, v = T.boundary_stream()
    assert T.simd_end(v.size) >= b.size
    assert T.simd_end(T.f16_all_stream()[0].size) >= 65536
    # tail positions: every entry of the tail tables, every stream length
    enc = T.encode_tail_cases()
    assert T.covers_tail(enc, T.TAIL_F32, 1) and T.covers_tail(enc, T.IDX_U32, 0)
    assert {c[0].size for c in enc} == {1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17}
    dec = T.decode_tail_cases()
    assert T.covers_tail(dec, T.TAIL_U16, 0) and T.covers_tail(dec, T.TAIL_U16, 1)


# ---------------------------------------------------------------------------
# 2. the yardstick itself is pinned
# ---------------------------------------------------------------------------
def test_manifest_pins_tables_and_instruction_outputs(isa):
    with open(MANIFEST) as f:
        m = json.load(f)
    assert T.table_digests() == m["tables"]
    assert T.isa_digests(isa) == m["instructions"]


# ---------------------------------------------------------------------------
# 3. do the tables discriminate?  numpy restatements, right and wrong
# ---------------------------------------------------------------------------
def np_f32_to_f16(bits, tie="even", flush_sub=False, saturate=False, sub_carry=True, flush_below=-10,
                  nan_quiet=True):
    u = np.ascontiguousarray(bits, np.uint32).astype(np.int64)
    sign, ex, man = (u >> 16) & 0x8000, (u >> 23) & 0xFF, u & 0x7FFFFF
    e = ex - 112

    def up(rem, half, h):
        if tie == "even":
            return (rem > half) | ((rem == half) & ((h & 1) == 1))
        if tie == "up":
            return rem >= half
        return np.zeros(rem.shape, bool)                       # truncation

    hn = (np.clip(e, 1, 30) << 10) | (man >> 13)
    hn = hn + up(man & 0x1FFF, 0x1000, hn)
    sh = np.clip(14 - e, 14, 24)
    full = man | 0x800000
    hs = full >> sh
    inc = up(full & ((1 << sh) - 1), 1 << (sh - 1), hs)
    hs = hs + inc if sub_carry else np.minimum(hs + inc, 0x3FF)
    h = np.where(e >= 31, 0x7C00, np.where(e >= 1, hn, np.where(e < flush_below, 0, 0 if flush_sub else hs)))
    if saturate:
        h = np.minimum(h, 0x7BFF)
    nan = (0x7C00 | (0x200 if nan_quiet else 0) | (man >> 13))
    h = np.where(ex == 0xFF, np.where(man > 0, nan, 0x7C00), h)
    return (sign | h).astype(np.uint16)


def np_f16_to_f32(words, nan_quiet=True, sub_bias=103):
    h = np.ascontiguousarray(words, np.uint16).astype(np.int64)
    sign, ex, man = (h & 0x8000) << 16, (h >> 10) & 0x1F, h & 0x3FF
    p = T._ilog2(np.maximum(man, 1))
    sub = np.where(man > 0, ((p + sub_bias) << 23) | ((man << (23 - p)) & 0x7FFFFF), 0)
    top = 0x7F800000 | (man << 13) | np.where((man > 0) & nan_quiet, 0x00400000, 0)
    u = np.where(ex == 0x1F, top, np.where(ex > 0, ((ex + 112) << 23) | (man << 13), sub))
    return (sign | u).astype(np.uint32).view(np.float32)


def np_trunc_lo16(val, saturate=False):
    val = np.ascontiguousarray(val, np.float32)
    t = np.full(val.size, -2**31, np.int64)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(val) & (val > np.float32(-2147483904.0)) & (val < np.float32(2147483648.0))
    t[ok] = np.trunc(val[ok].astype(np.float64)).astype(np.int64)
    if saturate:
        return np.clip(t, 0, 65535).astype(np.uint16)
    return (t & 0xFFFF).astype(np.uint16)


def np_encode(idx, val, flag, idx_block_sat=True, idx_tail_sat=False, val_tail_sat=False, **f16):
    se = T.simd_end(idx.size)
    sat = np.clip(idx.view(np.int32).astype(np.int64), -32768, 32767).astype(np.int16).view(np.uint16)
    low = idx.astype(np.uint16)
    wi = np.concatenate([(sat if idx_block_sat else low)[:se], (sat if idx_tail_sat else low)[se:]]) if flag & 1 \
        else idx.copy()
    wv = np.concatenate([np_f32_to_f16(val.view(np.uint32)[:se], **f16), np_trunc_lo16(val[se:], val_tail_sat)]) \
        if flag & 2 else val.copy()
    return wi, wv


def np_decode(wi, wv, flag, **f16):
    se = T.simd_end(wi.size)
    idx = np.concatenate([wi[:se].view(np.int16).astype(np.int32).view(np.uint32), wi[se:].astype(np.uint32)]) \
        if flag & 1 else wi.copy()
    val = np.concatenate([np_f16_to_f32(wv[:se], **f16), wv[se:].astype(np.float32)]) if flag & 2 else wv.copy()
    return idx, val


def _encode_mismatches(isa, **kw):
    n = 0
    for name, idx, val in _encode_streams():
        gi, gv = np_encode(idx, val, 3, **kw)
        ei, ev = isa.encode(idx, val, 3)
        n += _diff(gi, ei).size + _diff(gv, ev).size
    return n


def _decode_mismatches(isa, **kw):
    n = 0
    for name, wi, wv in _decode_streams(all_tails=False):
        gi, gv = np_decode(wi, wv, 3, **kw)
        ei, ev = isa.decode(wi, wv, 3)
        n += _diff(gi, ei).size + _diff(gv, ev).size
    return n


def test_right_restatements_pass(isa):
    assert _encode_mismatches(isa) == 0
    assert _decode_mismatches(isa) == 0


WRONG_ENCODE = {
    "round half up": dict(tie="up"),
    "truncation": dict(tie="down"),
    "fp16 subnormals flushed": dict(flush_sub=True),
    "overflow saturates to 65504": dict(saturate=True),
    "no carry from 0x03ff into 0x0400": dict(sub_carry=False),
    "2^-25 edge one binade up": dict(flush_below=-9),
    "2^-25 edge one binade down": dict(flush_below=-11),
    "NaN without the quiet bit": dict(nan_quiet=False),
    "index blocks truncate": dict(idx_block_sat=False),
    "index tail saturates": dict(idx_tail_sat=True),
    "value tail saturates": dict(val_tail_sat=True),
}
WRONG_DECODE = {
    "NaN without the quiet bit (the code before this test)": dict(nan_quiet=False),
    "subnormal normalisation one binade up": dict(sub_bias=104),
    "subnormal normalisation one binade down": dict(sub_bias=102),
}


@pytest.mark.parametrize("what", list(WRONG_ENCODE))
def test_wrong_encode_is_caught(isa, what):
    assert _encode_mismatches(isa, **WRONG_ENCODE[what]) > 0


@pytest.mark.parametrize("what", list(WRONG_DECODE))
def test_wrong_decode_is_caught(isa, what):
    n = _decode_mismatches(isa, **WRONG_DECODE[what])
    assert n > 0
    if what.startswith("NaN"):  # exactly the signalling words at block positions: 1,022 in the full stream
        def snan(w):
            return int(np.count_nonzero(((w & 0x7FFF) > 0x7C00) & ((w & 0x0200) == 0)))
        assert snan(T.f16_all_stream()[1]) == T.F16_SNAN_WORDS == 1022
        assert n == sum(snan(wv[:T.simd_end(wv.size)]) for _, _, wv in _decode_streams(all_tails=False))


# ---------------------------------------------------------------------------
# 4. the boundary buckets reach what section D needs (oracle alone)
# ---------------------------------------------------------------------------
def test_boundary_buckets_are_boundary_values():
    for band in T.BANDS:
        x = T.boundary_bucket(1 << 16, 3000, 0, band)
        mag = x.view(np.uint32) & 0x7FFFFFFF
        table = np.unique(T.f32_boundary() & 0x7FFFFFFF)
        assert np.isin(mag, table).all(), band
        assert 0.2 < T.is_tie(x).mean() < 0.3, band


def test_boundary_sequences_emit_ties_subnormals_and_infinities(oracle):
    for key, n, k, bands, sb, ga in T.d_sequences(oracle):
        assert n <= 1 << 18
        for it, (x, co, io, vo, after, before) in enumerate(T.bucket_sequence(oracle, key, n, k, bands, sb, ga)):
            v = vo[:co]
            assert int(T.is_tie(v).sum()) >= 64, (key, it, int(T.is_tie(v).sum()))
            w = oracle.wire_encode(io[:co], v, 2)[1][:T.simd_end(co)]
            mag = w & 0x7FFF
            if bands[it] == "sub":
                assert int(((mag > 0) & (mag < 0x400)).sum()) >= 64, (key, it)
                assert int((mag == 0x400).sum()) >= 8, (key, it)   # carries out of 0x03ff into the first normal
            if bands[it] == "top":
                assert int((mag == 0x7C00).sum()) >= 16, (key, it)
                assert np.isfinite(v).all()                        # infinities made by the cast, not fed in


def test_mixed_sequence_meets_both_regimes(oracle):
    """normal -> sub -> top -> normal on one key: the drop is a regime-B fill
    (the scan's head stays below k), the rise fills every slot from the scan."""
    for key, n, k, bands, sb, ga in T.d_sequences(oracle):
        if len(set(bands)) == 1:
            continue
        regimes = []
        for it, (x, co, io, vo, after, before) in enumerate(T.bucket_sequence(oracle, key, n, k, bands, sb, ga)):
            if before is not None:
                regimes.append("B" if tv16_head(oracle, x, k, before[0]) < k else "A")
        assert "A" in regimes and "B" in regimes, (key, regimes)
        b = regimes.index("B") + 1
        seq = T.bucket_sequence(oracle, key, n, k, bands, sb, ga)
        head = tv16_head(oracle, seq[b][0], k, seq[b][5][0])
        assert int(T.is_tie(seq[b][3][head:seq[b][1]]).sum()) >= 64, key   # ties among the fill's own pairs
