"""Buffer geometry for the compress parity tests (test infrastructure, no conftest).

The compress kernels choose their loads and stores by the addresses they are
given: 16-byte alignment of source, index and value buffer together selects
the vector emission, anything else the scalar one; top-k reads a source that
is not 16-byte aligned element by element.  Freshly allocated tensors are
256-byte aligned, so tests that want the other branches carve their buffers
out of a larger allocation at a chosen phase (``carve``), and the rest of that
allocation holds a sentinel, so that a store outside the buffer is seen
(``assert_guards``).

The case tables of tests/test_gpu_geometry.py live here too:
tests/test_geometry_host.py pins them with the oracle alone (both thresholdv16
regimes, the ragged last line, both sides of threshold-v's cap, ...), so that a
pass on the GPU means the branches were reached.
"""
from __future__ import annotations

import functools

import numpy as np

from stellatrain_amd.synth import D1, D2, seed_for, synth

# ---------------------------------------------------------------------------
# carved buffers
# ---------------------------------------------------------------------------
# Every 16-bit word of an allocation holds this pattern: a NaN as float32
# (0xffa5ffa5) and as float16, an index past any bucket as uint32 / uint16.  A
# source guard that leaks into a line sum poisons it.
SENTINEL16 = 0xFFA5
SENTINEL8 = 0xA5               # around 1-byte elements (the MERGE marks): a set mark

PHASES4 = (0, 4, 8, 12)        # 4-byte elements: every dword phase of a 16-byte word
PHASES2 = (0, 2, 6, 8, 14)     # 16-bit wire outputs


def carve(torch, gpu, numel, dtype, phase_bytes, guard=64):
    """A contiguous view of `numel` elements of `dtype` whose address is
    `phase_bytes` past a 16-byte boundary, inside a larger allocation filled
    with SENTINEL16 (SENTINEL8 around 1-byte elements), at least `guard`
    elements of it on either side.  The allocation travels with the view
    (``view._carve``) for assert_guards."""
    item = torch.empty(0, dtype=dtype).element_size()
    assert item in (1, 2, 4) and phase_bytes % item == 0 and 0 <= phase_bytes < 16
    # the allocation is one of 16-bit words, or of SENTINEL8 bytes around 1-byte
    # elements (a buffer of an odd number of bytes ends inside a word)
    unit = min(item, 2)
    w = item // unit                               # words (bytes) per element
    lead = (guard * item + 15) // 16 * 16          # bytes ahead of the 16-byte boundary the phase counts from
    total = (lead + 16 + numel * item + guard * item + 16) // unit
    if unit == 2:
        raw = torch.full((total,), SENTINEL16 - 0x10000, dtype=torch.int16, device=gpu)
    else:
        raw = torch.full((total,), SENTINEL8, dtype=torch.uint8, device=gpu)
    base = raw.data_ptr()
    lo = (lead + (-base) % 16 + phase_bytes) // unit  # first word of the view
    assert (base + unit * lo) % 16 == phase_bytes and lo >= guard * w
    hi = lo + numel * w
    assert total - hi >= guard * w
    view = raw[lo:hi].view(dtype)
    assert view.is_contiguous() and view.numel() == numel
    if numel:
        # which branch a kernel takes is a pure function of this address
        assert view.data_ptr() % 16 == phase_bytes, (view.data_ptr(), phase_bytes)
    view._carve = (raw, lo, hi)
    return view


def assert_guards(view, what=""):
    """Every word of the allocation outside the view still holds the sentinel."""
    raw, lo, hi = view._carve
    for side, g in (("before", raw[:lo]), ("after", raw[hi:])):
        a = g.cpu().numpy()
        bits = 8 * a.itemsize
        a = a.view(np.uint16 if bits == 16 else np.uint8)
        bad = np.flatnonzero(a != (SENTINEL16 if bits == 16 else SENTINEL8))
        if bad.size:
            raise AssertionError(f"{what}: {bad.size} {bits}-bit words {side} the buffer were overwritten, first at "
                                 f"word {int(bad[0])} of {a.size} (0x{int(a[bad[0]]):04x})")


# ---------------------------------------------------------------------------
# call sequences
# ---------------------------------------------------------------------------
# per-call gradient scale of tests/test_gpu_wire_fused.py: the 100x drops are
# window misses of the regime-B fill, the 30x rise fills every slot from the scan
SCALES = (1.0, 1.0, 0.01, 0.01, 1.0, 30.0)
SCALES4 = (1.0, 0.01, 0.01, 30.0)               # the same in four calls
SCALES_CHILD = (1.0, 1.0, 1.0, 1.0, 0.01, 0.01, 0.01)  # tests/phase_child.py
# threshold-v: a drop leaves count < k, the rise after it overflows the cap
SCALES_TV = (1.0, 1.0, 0.01, 3000.0, 1.0, 1.0)
SCALES_TV4 = (1.0, 0.01, 3000.0, 1.0)

# The ragged last line (n % 16 elements) is judged on its signed sum, so random
# data almost never emits it.  Call `it` replaces it by |x| * TAIL_BOOST[it % 3]:
# x8 makes it the first pop of a regime-B fill after a 100x drop, x1000 passes
# the threshold inside the scan even then (the fill then starts at a count that
# is no multiple of 4).  A key's first call is left alone: its threshold comes
# from the line sums.
TAIL_BOOST = (1.0, 8.0, 1000.0)


def call_data(n, bucket, it, scale=1.0, dist=D1, tail=True, ties=0):
    """Call `it` of the sequence of bucket id `bucket` (tail: with TAIL_BOOST).
    With `ties`, the second line of every ties-th pair of lines is the first
    one negated: equal line sums next to each other in the scan, told apart in
    the stream by index and by value."""
    x = synth(n, seed_for(bucket, it), dist)
    full = n // 16 * 16
    if ties:
        lines = x[:full].reshape(-1, 16)
        a = np.arange(0, lines.shape[0] - 1, 2 * ties)
        lines[a + 1] = -lines[a]
    boost = TAIL_BOOST[it % 3] if tail else 1.0
    if full < n and boost != 1.0:
        x[full:] = np.abs(x[full:]) * np.float32(boost)
    if scale != 1.0:
        x = (x * np.float32(scale)).astype(np.float32)
    return x


def tv16_head(oracle, src, cap, t):
    """Pairs the ordered scan emits at threshold `t` (stages 1 to 3 of
    thresholdv16.cpp restated on the oracle's line sums): the offset at which a
    regime-B fill starts.  head < cap is regime B."""
    src = np.ascontiguousarray(src, np.float32)
    n = src.size
    t = np.float32(t)
    q = int(np.count_nonzero(oracle.tv16_block_sums(src) >= t)) if n >= 16 else 0
    d16, tl = cap - cap % 16, n % 16
    cnt = min(q, d16 // 16) * 16
    if q > d16 // 16 and cnt < cap:
        return cap                                   # stage 2: a qualifying line donates the rest
    if tl and cnt < cap:
        s = np.float32(0)
        for v in src[n - tl:]:
            s = np.float32(s + v)
        if np.float32(s * np.float32(16)) >= np.float32(t * np.float32(tl)):
            cnt += min(cap - cnt, tl)
    return cnt


@functools.lru_cache(maxsize=None)
def tv16_batch_sequence(oracle, items, scales, bucket0, ties=0):
    """The oracle's results for the buckets `items` = ((key, n, k, dist,
    idx_offset), ...) called in this order once per entry of `scales` (a key
    may repeat): out[call][item] = (src, count, idx, val, state after, head,
    regime), regime 'A' / 'B', or None on the key's first call.  Item j's data
    is call_data(n, bucket0 + j, call, scale, dist).  Computed once and shared
    (read-only)."""
    h = oracle.tv16_new()
    out = []
    for it, sc in enumerate(scales):
        row = []
        for j, (key, n, k, dist, off) in enumerate(items):
            x = call_data(n, bucket0 + j, it, sc, dist, ties=ties)
            tb = oracle.tv16_state(h, key)
            co, io, vo = oracle.tv16_compress(h, key, x, k, idx_offset=off)
            head = tv16_head(oracle, x, k, tb[0]) if tb is not None else None
            for a in (x, io, vo):
                a.setflags(write=False)
            row.append((x, co, io, vo, oracle.tv16_state(h, key), head,
                        None if tb is None else ("B" if head < k else "A")))
        out.append(tuple(row))
    oracle.tv16_free(h)
    return tuple(out)


def tv16_sequence(oracle, n, k, bucket, scales, dist=D1, off=0, ties=0):
    """One key's calls: out[call] = (src, count, idx, val, state, head, regime)."""
    return tuple(r[0] for r in tv16_batch_sequence(oracle, (("g", n, k, dist, off),), tuple(scales), bucket, ties))


@functools.lru_cache(maxsize=None)
def tv_sequence(oracle, n, k, bucket, scales):
    """Threshold-v, cap = k: out[call] = (src, count, idx, val, threshold
    after, uncapped count).  Computed once and shared (read-only)."""
    h = oracle.tv_new()
    out = []
    for it, sc in enumerate(scales):
        x = call_data(n, bucket, it, sc, tail=False)
        tb = oracle.tv_state(h, 1)
        if tb is None:
            tb = oracle.tv_first_threshold(x, k)
        co, io, vo = oracle.tv_compress(h, 1, x, k)
        above = int(np.count_nonzero(np.abs(x) >= np.float32(tb)))
        for a in (x, io, vo):
            a.setflags(write=False)
        out.append((x, co, io, vo, oracle.tv_state(h, 1), above))
    oracle.tv_free(h)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def topk_call(oracle, n, k, bucket, it, exact, off):
    """Top-k call `it` of a key (the oracle keeps no state): (src, count, idx, val)."""
    x = call_data(n, bucket, it, dist=D2, tail=False)
    co, io, vo = oracle.topk_compress(x, k, idx_offset=off, bug_compat=not exact)
    for a in (x, io, vo):
        a.setflags(write=False)
    return x, co, io, vo


# ---------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------
# (src, idx, val) byte phases
TRIPLES_A = ((4, 0, 0), (8, 0, 0), (12, 0, 0),       # a misaligned source alone
             (0, 4, 0), (0, 8, 0), (0, 12, 0),       # the index buffer alone
             (0, 0, 4), (0, 0, 8), (0, 0, 12),       # the value buffer alone
             (4, 8, 12), (12, 12, 12))
SIZES_A = ((4103, 40), (65541, 655), ((1 << 20) + 13, 10485))
OFFSET_RUN_A = ((65541, 655), (4, 8, 12), 77)        # one run with an idx_offset
BUCKET_A = 800                                        # seed bucket ids (synth.seed_for)

CHILD = ((1 << 20) + 13, 10485)
BUCKET_CHILD = 810
TIES_CHILD = 4    # every fourth pair of lines ties (call_data): the fills' orderers have equal sums to order
TRIPLES_CHILD = ((4, 0, 0), (0, 8, 12))

# C: (key, n, k, dist, idx_offset, (src, idx, val) phases); c0@w repeats: the launch splits
BATCH_C = (
    ("c0@w", 131072 + 13, 1310, D1, 0, (4, 0, 0)),
    ("c1@w", 65541, 655, D2, 1 << 20, (0, 8, 0)),
    ("c2@b", 1000, 7, D1, 0, (0, 0, 12)),
    ("c0@w", 131072 + 13, 1310, D1, 0, (12, 4, 8)),
    ("c3@w", 4103, 40, D1, 5, (8, 12, 4)),
    ("c4@w", 49152 + 5, 491, D1, 0, (4, 4, 4)),
    ("c5@w", 33, 3, D1, 0, (12, 0, 4)),
    ("c6@w", 100013, 1007, D2, 0, (0, 0, 0)),
    ("c7@w", 8195, 81, D1, 0, (8, 8, 8)),
)
BUCKET_C = 820
# wire launch: (key, n, k, dist, flag, idx_offset, phases); 16-bit outputs at the 2-byte phases
WIRE_C = (
    ("w0@w", 60013, 600, D1, 1, 70000, (4, 2, 0)),
    ("w1@w", 131072 + 13, 1310, D1, 2, 0, (0, 4, 6)),
    ("w2@w", 100007, 1000, D2, 3, 100, (8, 14, 2)),
    ("w3@w", 65541, 655, D1, 0, 5, (12, 8, 4)),
    ("w4@w", 4103, 40, D1, 3, 30000, (0, 6, 14)),
    ("w5@w", 4119, 41, D1, 3, 0, (0, 0, 8)),
    ("w6@w", 100013, 1007, D1, 1, 0, (0, 14, 0)),
)
BUCKET_W = 840
# residual launch: (key, n, k, phases, residual phase)
RESID_C = (
    ("r0@w", 131072 + 13, 1310, (4, 0, 0), 0),
    ("r1@w", 65541, 655, (0, 8, 12), 4),
    ("r2@w", 4103, 40, (12, 4, 8), 8),
    ("r3@w", 100013, 1007, (8, 12, 4), 12),
)
BUCKET_R = 860

TRIPLES_D = ((0, 0, 0), (4, 0, 0), (8, 0, 0), (12, 0, 0), (0, 4, 8))
TV_D = ((100013, 100), (5000, 4999))
TOPK_D = ((100013, 1000), (4099, 41), (4099, 4099))   # the last: k == n
BUCKET_D = 870

TRIPLES_E = ((0, 0, 0), (4, 8, 12))
TINY_N = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33)
BOUNDS = (256, 8192, 32768, 65536)     # the wave step, LCHUNK lines / TV_TILE, TV16_CHUNK lines, two of them
DELTAS = (-17, -16, -1, 0, 1, 15, 16, 17)
BUCKET_E = 880


def tiny_cases(over_cap):
    """(n, k): k in {0, 1, min(n, 16), n}, and n + 3 (with cap = k) where the codec allows it."""
    out = []
    for n in TINY_N:
        ks = {0, 1, min(n, 16), n}
        if over_cap:
            ks.add(n + 3)
        out += [(n, k) for k in sorted(ks)]
    return tuple(out)


def boundary_cases(b):
    """(n, k) around the geometry constant b: k = max(1, n // 100), and at
    b - 1, b, b + 1 also the k nearest to it with k % 16 in {0, 1, 15}."""
    out = []
    for d in DELTAS:
        n = b + d
        k0 = max(1, n // 100)
        ks = {k0}
        if d in (-1, 0, 1):
            k16 = max(16, k0 - k0 % 16)
            ks |= {k16, k16 + 1, k16 + 15}
        out += [(n, k) for k in sorted(ks)]
    return tuple(out)


FAMILIES = ("tiny", "b256", "b8192", "b32768", "b65536")
TV_FAMILIES = ("tiny", "b256", "b8192")


def family_cases(codec, family):
    """The (n, k) table of one (codec, size family) of section E.  Exact top-k
    gets one k == n entry per boundary family on top of the issue's."""
    if family == "tiny":
        return tiny_cases(over_cap=codec in ("thresholdv16", "thresholdv"))
    b = int(family[1:])
    cases = boundary_cases(b)
    if codec.startswith("topk"):
        cases += ((b + 1, b + 1),)
    return cases


def family_bucket(family, j):
    return BUCKET_E + 10 * FAMILIES.index(family) + j % 10


SCALES8 = tuple(SCALES[i % len(SCALES)] for i in range(8))   # section A: 8 calls


def one(n, k, dist=D1, off=0):
    return (("g", n, k, dist, off),)


def tv16_tables():
    """Every thresholdv16 sequence of tests/test_gpu_geometry.py as (label,
    items, scales, bucket0, ties), the arguments of tv16_batch_sequence."""
    out = [(f"A:{n}", one(n, k), SCALES8, BUCKET_A + j, 0) for j, (n, k) in enumerate(SIZES_A)]
    (n, k), _, off = OFFSET_RUN_A
    out.append(("A:offset", one(n, k, D1, off), SCALES8, BUCKET_A + SIZES_A.index((n, k)), 0))
    out.append(("B:child", one(*CHILD), SCALES_CHILD, BUCKET_CHILD, TIES_CHILD))
    out.append(("C:batch", tuple(b[:5] for b in BATCH_C), SCALES, BUCKET_C, 0))
    out.append(("C:wire", tuple((key, n, k, dist, off) for key, n, k, dist, _, off, _ in WIRE_C), SCALES, BUCKET_W, 0))
    out.append(("C:resid", tuple((key, n, k, D1, 0) for key, n, k, _, _ in RESID_C), SCALES4, BUCKET_R, 0))
    for fam in FAMILIES:
        for j, (n, k) in enumerate(family_cases("thresholdv16", fam)):
            out.append((f"E:{fam}:{n},{k}", one(n, k), SCALES4, family_bucket(fam, j), 0))
    return out


def tv_tables():
    """Every threshold-v sequence as (label, n, k, bucket, scales)."""
    out = [(f"D:{n}", n, k, BUCKET_D + j, SCALES_TV) for j, (n, k) in enumerate(TV_D)]
    for fam in TV_FAMILIES:
        for j, (n, k) in enumerate(family_cases("thresholdv", fam)):
            out.append((f"E:{fam}:{n},{k}", n, k, family_bucket(fam, j), SCALES_TV4))
    return out


def topk_tables():
    """Every top-k (n, k) table by name."""
    out = {"D": TOPK_D}
    for fam in FAMILIES:
        out[f"E:{fam}"] = family_cases("topk_exact", fam)
    return out
