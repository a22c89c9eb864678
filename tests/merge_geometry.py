"""Buffer geometry for the receive-side parity tests (test infrastructure, no
conftest): the case tables and stream maker of tests/test_gpu_merge_geometry.py.

The MERGE decompress and the optimizer steps choose their loads by the
addresses and sizes they are given -- a mark array's ragged last 16, a second
round of the tile-count scan, wire blocks of 8 and a scalar tail, vector loads
where a stream is 16-byte aligned -- and drop every index >= n.  The GPU tests
therefore carve every buffer out of a sentinel-filled allocation at a chosen
phase (``geometry.carve``) and plant, in every rank stream, the pairs that reach
those branches.  tests/test_merge_geometry_host.py pins what each case claims
with the oracle alone, so that a pass on the GPU means the branches ran.

Expected values are the oracle chain ``wire_decode`` -> ``merge_decompress``
(``wire_merge_cases.expected``) -> ``sgd_apply`` / ``adam_apply``.  Values are
tame (finite, far inside the fp16 range, sums finite): every comparison is of
bits, with no NaN rule.
"""
from __future__ import annotations

import functools

import numpy as np

import wire_merge_cases as W
from geometry import PHASES2, PHASES4

WORLDS = (1, 2, 3, 8)
FLAGS = (0, 1, 2, 3)
MERGE_TILE = 4096          # marks per tile of the world > 1 emission (ws.h)
SCAN_ROUND = 4096          # tiles per round of mark_scan

TINY_N = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33)
EDGE_B = (1024, 4096, 8192, 65536)   # win_emit1t / ADAM_TILE / MERGE_BATCH_TILE; MERGE_TILE; two of them; the u16 range
EDGE_M = (1023, 1024, 1025, 4095, 4096, 4097, 8191, 8193)   # 8 k +- 1: wend at both ends of a tile
# u16 indices: up to here every planted index (n + 63 the largest) is its own
# wire word; above, block indices saturate (the one saturating family: 65,536 +- 1)
U16_EXACT = 32767 - 63

SIZE_SCAN = (1 << 24) + 4096 + 5     # 4,098 tiles: a second mark_scan round of two, the last ragged
SCAN_PER_RANK = 2000
SCAN_WORLD = 2


def tiny_per_rank(n):
    return tuple(sorted({0, 1, min(n, 4), n, n + 3}))    # n + 3 forces repeats


def edge_per_rank(n):
    return tuple(m for m in EDGE_M if m <= n + 3)


SIZES_TINY = tuple((n, m) for n in TINY_N for m in tiny_per_rank(n))
SIZES_EDGE = tuple((b + d, m) for b in EDGE_B for d in (-1, 0, 1) for m in edge_per_rank(b + d))
# the fused steps: tiny, and the 1,024 / 4,096 edges
SIZES_STEP = SIZES_TINY + tuple((n, m) for n, m in SIZES_EDGE if n <= 4097)
FAMILIES = {"tiny": SIZES_TINY, "edge": SIZES_EDGE, "step": SIZES_STEP}


# ---------------------------------------------------------------------------
# phases
# ---------------------------------------------------------------------------
def triples(flag):
    """(stream idx, stream val, outputs) byte phases in the style of
    geometry.TRIPLES_A: each buffer alone at every phase of its element size,
    then all three apart, and all aligned.  16-bit streams take PHASES2."""
    pi = PHASES2 if flag & 1 else PHASES4
    pv = PHASES2 if flag & 2 else PHASES4
    po = PHASES4
    return tuple([(p, 0, 0) for p in pi[1:]] + [(0, p, 0) for p in pv[1:]] + [(0, 0, p) for p in po[1:]]
                 + [(pi[1], pv[2], po[3]), (pi[-1], pv[-1], po[-1]), (0, 0, 0)])


def phases(flag, k, rank=0):
    """Case k's (idx, val, out_idx, out_val) phases; the ranks of one case rotate
    through the table, the outputs do not."""
    t = triples(flag)
    i, v, _ = t[(k + rank) % len(t)]
    o = t[k % len(t)][2]
    return i, v, o, (16 - o) % 16


# ---------------------------------------------------------------------------
# streams
# ---------------------------------------------------------------------------
KINDS = ("planted", "unique")
RAW_DROPS = (0x8000, 0x8001, 0x803f, 0xffff)   # u16 block words: sign extension sends them past any n


def drops(n):
    return (n, n + 1, n + 63, 0xffffffff)


def saturating(n, flag):
    return bool(flag & 1) and n > U16_EXACT


def planted(n, rank, flag):
    """What rank `rank` plants, most wanted first (a short stream holds the
    head of the list): the last element n - 1 -- shared by every rank, so the
    sum runs in rank order over all of them --, one index >= n, the first
    element of the ragged last 16, element 0, the other indices >= n.  The
    saturating family plants its dropped indices as raw block words instead."""
    d = drops(n)
    first = d[rank % 4]
    p = [n - 1]
    if not saturating(n, flag):
        p.append(first)
    rag = n - n % 16
    if n % 16 and rag not in p:
        p.append(rag)
    if 0 not in p:
        p.append(0)
    if not saturating(n, flag):
        p += [x for x in d if x != first]
    return p


def room(m):
    """Plants a stream of m pairs holds: with m >= 3 pair 0 is the repeat."""
    return m - 1 if m >= 3 else m


def _values(rng, m):
    return (rng.standard_normal(m) * 10.0 ** rng.integers(-3, 3, m)).astype(np.float32)


def make_streams(oracle, n, per_rank, flag, world, seed=0, kind="planted", extra=()):
    """``world`` wire streams [(widx, wval, flag)] of exactly ``per_rank``
    pairs over a tensor of ``n`` elements.

    ``planted``: random indices over [0, n) and, from the last pair
    backwards (the scalar tail of the wire form, where a u16 index is never
    saturated), the list of ``planted``; with per_rank >= 3 pair 0 repeats the
    last pair's index n - 1 with another value (the last occurrence wins).
    ``extra`` indices go to pairs 1, 2, ... (SIZE_SCAN's tiles).  In the
    saturating family pairs 1-4 are RAW_DROPS.
    ``unique``: per_rank distinct indices below n, nothing planted: at world 1
    the emission's copy-through path (u16 forms: n <= 32,768 only)."""
    m = per_rank
    assert kind in KINDS and (kind == "planted" or (m <= n and not (flag & 1 and n > 32768)))
    rng = np.random.default_rng([n, m, flag, world, seed, KINDS.index(kind)])
    out = []
    for r in range(world):
        val = _values(rng, m)
        if kind == "unique":
            idx = rng.choice(n, m, replace=False).astype(np.uint32)
        else:
            idx = rng.integers(0, n, m, dtype=np.uint32)
            for q, j in enumerate(extra):
                idx[1 + q] = j
            for q, j in enumerate(planted(n, r, flag)[:room(m)]):
                idx[m - 1 - q] = j
            if m >= 3:
                idx[0] = idx[m - 1]
        wi, wv = oracle.wire_encode(idx, val, flag)
        if kind == "planted" and saturating(n, flag):
            assert W.wend(m) >= 8 and not extra
            wi[1:5] = RAW_DROPS
        out.append((np.ascontiguousarray(wi), np.ascontiguousarray(wv), flag))
    return out


@functools.lru_cache(maxsize=None)
def case(oracle, n, per_rank, flag, world, seed=0, kind="planted"):
    """(streams, decoded idx, decoded val, merged idx, merged val, stats) of one
    case, computed once and shared (read-only)."""
    streams = make_streams(oracle, n, per_rank, flag, world, seed, kind)
    return _frozen(streams, W.expected(oracle, streams, per_rank, n))


def _frozen(streams, exp):
    idx, val, ei, ev, st = exp
    for a in [idx, val, ei, ev] + [x for wi, wv, _ in streams for x in (wi, wv)]:
        a.setflags(write=False)
    return tuple(streams), idx, val, ei, ev, st


def scan_extra(n=SIZE_SCAN):
    """Indices in tile 0, the first round's last tile (4,095), the second
    round's first (4,096, the last full tile) and a tile in between; the ragged
    tail (tile 4,097) gets n - 1 and n - n % 16 from ``planted``."""
    t = MERGE_TILE
    return (5, 4095 * t, 4095 * t + t - 1, 4096 * t, 4096 * t + t - 1, 2048 * t + 17)


@functools.lru_cache(maxsize=None)
def scan_case(oracle, flag):
    """SIZE_SCAN at world 2.  Flag 0 carries ``scan_extra``; the u16 form cannot
    address past 65,535, so flag 3 draws below 32,768 (exact) and only its tail
    words reach further."""
    n, m = SIZE_SCAN, SCAN_PER_RANK
    if flag & 1:
        streams = make_streams_scan16(oracle, flag)
    else:
        streams = make_streams(oracle, n, m, flag, SCAN_WORLD, extra=scan_extra())
    return _frozen(streams, W.expected(oracle, streams, m, n))


def make_streams_scan16(oracle, flag):
    n, m = SIZE_SCAN, SCAN_PER_RANK
    rng = np.random.default_rng([n, m, flag])
    out = []
    for r in range(SCAN_WORLD):
        idx = rng.integers(0, 32768, m, dtype=np.uint32)
        idx[m - 1] = 65535                      # the tail: zero-extended, the largest u16 index
        idx[m - 2] = 40000 + r
        idx[m - 3] = 0
        idx[0] = idx[m - 4]                     # a repeat
        wi, wv = oracle.wire_encode(idx, _values(rng, m), flag)
        wi[1:5] = RAW_DROPS
        out.append((np.ascontiguousarray(wi), np.ascontiguousarray(wv), flag))
    return out


def stream_order(idx, val, n):
    """World 1: the winners in stream order (each index's last occurrence, where
    it stands), value (0.0f + v) / 1.0f."""
    keep = np.flatnonzero(idx < n)
    _, first = np.unique(idx[keep][::-1], return_index=True)
    pos = np.sort(keep[::-1][first])
    return idx[pos], (np.float32(0) + val[pos]) / np.float32(1)


def merge_restated(idx, val, per_rank, world, n):
    """MERGE decompress in numpy, sharing no text with the oracle: per rank the
    last occurrence of an index wins; float32 sum in rank order from +0.0;
    divided by float32(world); the union ascending.  Indices >= n are dropped."""
    acc = np.zeros(n, np.float32)
    hit = np.zeros(n, bool)
    for r in range(world):
        tmp = np.zeros(n, np.float32)
        for j, v in zip(idx[r * per_rank:(r + 1) * per_rank].tolist(), val[r * per_rank:(r + 1) * per_rank]):
            if j < n:
                tmp[j] = v
                hit[j] = True
        acc = (acc + tmp).astype(np.float32)
    acc = (acc / np.float32(world)).astype(np.float32)
    oi = np.flatnonzero(hit)
    return oi.astype(np.uint32), acc[oi]


# ---------------------------------------------------------------------------
# what a case claims
# ---------------------------------------------------------------------------
PROPS = ("dups", "dropped", "tail", "last", "ragged", "zero", "shared")

# Every exemption, by name: (property, predicate(n, m, flag, world)).  A
# planted case claims every property no exemption takes from it.
def _short(n, m, flag, j):
    """The stream has no room for the plant j (n = 1 cannot hold a repeat and a
    distinct second index at once: its plants are one element)."""
    return planted(n, 0, flag).index(j) >= room(m)


EXEMPT = {
    "an empty stream claims nothing": (PROPS, lambda n, m, f, w: m == 0),
    "fewer than 3 pairs hold no repeat": (("dups",), lambda n, m, f, w: m < 3),
    "one pair is the last element alone": (("dropped",), lambda n, m, f, w: m < 2),
    "no ragged end": (("ragged",), lambda n, m, f, w: n % 16 == 0),
    "too short for the ragged plant": (("ragged",), lambda n, m, f, w: n % 16 != 0 and _short(n, m, f, n - n % 16)),
    "too short for element 0": (("zero",), lambda n, m, f, w: _short(n, m, f, 0)),
    "one rank shares with nobody": (("shared",), lambda n, m, f, w: w == 1),
    # the saturating family (u16 indices, n about 65,536)
    "u16 cannot address element 65,536": (("last", "ragged"), lambda n, m, f, w: f & 1 and n > 65536),
    "a one-pair tail saturates the ragged plant": (("ragged",),
                                                   lambda n, m, f, w: saturating(n, f) and m - W.wend(m) < 2),
}


def claims(n, m, flag, world):
    out = set(PROPS)
    for props, pred in EXEMPT.values():
        if pred(n, m, flag, world):
            out -= set(props)
    return out


def holds(n, per_rank, world, idx, ei, st):
    """The properties a computed case has."""
    got = {k for k in ("dups", "dropped", "tail") if st[k] > 0}
    if ei.size and int(ei[-1]) == n - 1:
        got.add("last")
    if n % 16 and (n - n % 16) in ei:
        got.add("ragged")
    if ei.size and int(ei[0]) == 0:
        got.add("zero")
    if world > 1 and per_rank:
        ranks = [set(idx[r * per_rank:(r + 1) * per_rank].tolist()) for r in range(world)]
        if any(j < n for j in set.intersection(*ranks)):
            got.add("shared")
    return got


# ---------------------------------------------------------------------------
# the tables of the GPU tests
# ---------------------------------------------------------------------------
def merge_cases(family):
    """Section A: (k, n, per_rank, kind) -- every size planted, and a unique
    twin (world 1's copy-through path) of every size that can hold one."""
    out = []
    for n, m in FAMILIES[family]:
        out.append((len(out), n, m, "planted"))
        if 0 < m <= n:
            out.append((len(out), n, m, "unique"))
    return tuple(out)


EDGE_WORLDS = (1, 3)
EDGE_FLAGS = (0, 3)
STEP_WORLDS = (1, 3)
STEP_CALLS = 4
SGD_OPTS = {
    "plain": dict(lr=0.05),
    "nesterov_wd": dict(lr=0.05, momentum=0.9, nesterov=True, weight_decay=0.01),
    "smart": dict(lr=0.05, momentum=0.9, dampening=0.1, smart_momentum=True),
}
ADAM_OPTS = {
    "adam": dict(lr=0.01, weight_decay=0.01),
    "amsgrad": dict(lr=0.01, weight_decay=0.01, amsgrad=True),
}


def step_cases():
    """Section C: (k, n, per_rank, flag, param phase); the flag and the phase
    rotate so that every size family meets every one of them."""
    return tuple((k, n, m, k % 4, PHASES4[(k // 4 + k) % 4]) for k, (n, m) in enumerate(SIZES_STEP))


def step_kind(world, call):
    """The calls of one name: planted (the election), and at world 1 every
    second call unique where the size can hold it."""
    return "unique" if world == 1 and call % 2 else "planted"


# Section D: optimize_raw
RAW_LENS = (0, 1, 3, 1023, 1024, 1025, 2049)
RAW_N = 4099
RAW_TAIL = 37               # pairs of capacity past grad_len when a device length is given
TRIPLES_RAW = ((0, 0, 0), (4, 0, 0), (0, 8, 0), (0, 0, 12), (4, 8, 12), (12, 12, 4), (8, 4, 8))  # (grad, gidx, param)


def raw_variants(grad_len):
    """(capacity, device length or None): the host length alone; grad_len - 1
    and 0 on the device below a larger capacity."""
    out = [(grad_len, None)]
    if grad_len:
        out.append((grad_len + RAW_TAIL, grad_len - 1))
    out.append((grad_len + RAW_TAIL, 0))
    return tuple(out)


def raw_case(grad_len, cap, seed):
    """(gidx, grad) of `cap` pairs over RAW_N elements: distinct indices (first
    and last element among the first pairs), and past grad_len valid indices
    with gradients of 1e6 -- a step on them changes the parameter."""
    rng = np.random.default_rng([grad_len, cap, seed])
    gidx = rng.choice(RAW_N, cap, replace=False).astype(np.uint32)
    for q, j in enumerate((RAW_N - 1, 0)[:grad_len]):
        at = np.flatnonzero(gidx == j)
        if at.size:
            gidx[at[0]] = gidx[q]
        gidx[q] = j
    grad = _values(rng, cap)
    grad[grad_len:] = np.float32(1e6)
    return gidx, grad


# Section E: one batched call
BATCH_N = (1, 2, 15, 16, 17, 33, 4095, 4096, 4097, 8199)
BATCH_WORLDS = (1, 3)
BATCH_GROUP = 16            # MERGE_BATCH: tensors per launch
BATCH_EMPTY = 20


def batch_plan(specs):
    """Tensors per shared launch as codec.h documents the closing rule (names
    distinct, one world, far below the element caps): full at BATCH_GROUP; an
    empty task runs alone (0 in the plan) and closes what is pending."""
    groups, cur = [], 0
    for _, _, m, _, _ in specs:
        if m == 0 or cur == BATCH_GROUP:
            if cur:
                groups.append(cur)
            cur = 0
        if m == 0:
            groups.append(0)
        else:
            cur += 1
    return groups + ([cur] if cur else [])


def batch_specs(world):
    """24 tasks (name, n, per_rank, flag, param phase): a group of 16 closes in
    the middle of the sizes' second round; task BATCH_EMPTY has per_rank 0 (it
    runs on its own at its place and closes the group before it)."""
    out = []
    for i in range(24):
        n = BATCH_N[i % len(BATCH_N)]
        m = (1, min(n, 4), n, n + 3)[i % 4] if n <= 33 else EDGE_M[i % 6] if n < 8199 else 1025
        if i == BATCH_EMPTY:
            m = 0
        out.append((f"g{i}", n, m, i % 4, PHASES4[i % 4]))
    return tuple(out)
