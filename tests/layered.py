"""Gradient buckets whose large values cluster by position (shared by the
layered golden fixtures, the reach-condition test and the GPU parity tests; not
a test module).

A bucket is a concatenation of layers: a bias or norm slice many times the
scale of the weights next to it, an embedding slice that is zero but for a few
rows.  ``synth()`` and every kind of tests/edge_values.py draw each element
independently of its position, so no chunk, tile or heap subtree ever sees
more of the large values than its neighbours.  These kinds put them in one
place.

``layered_input(kind, n, seed_bucket, it)`` starts, like ``edge_input``, from
``synth(n, seed_for(seed_bucket, it), dist)``, draws positions and signs from
``edge_values.draws`` (integer-only, never numpy.random: the GPU side
regenerates these inputs and must get the same bits), scales in float64 and
rounds once to float32.  A line is 16 floats, ``L = n // 16``, "hot" means
multiplied by ``S``, and ``H = hot_lines(n)`` is 1.5 (k / 16).

front        the first H lines hot
back         the last H lines and the ragged tail hot, the tail by TAIL_S
straddle     H hot lines centred on line 2048 c + 512 d - 3, c and d drawn per
             seed bucket
stripes      every 8th 512-line chunk hot, at a phase of 5 lines (stripe edges
             are no chunk edges); the odd stripes by S / 4 only (see below)
ramp         +-RAMP_BASE (1 + u 2^-12), u and the sign drawn, times a scale
             that falls from 2 to 1 over the bucket in steps of RAMP_STEP lines
plateau      8 position slices of PLATEAU_WIDTHS / 64 of the bucket, slice j
             scaled by exactly 2^-j; magnitudes PLATEAU_BASE * {1, 3/4, 1/2},
             the middle one with probability 1 - 2 / PLATEAU_SIDE, random sign
moving       front whose hot region starts H / 2 lines later on every call, at
             S * MOVING_ODD on odd calls and S * MOVING_EVEN on even ones
sparse_rows  D3 with SPARSE_ZP / 10^4 zeros but for sparse_lines(n, it) dense
             lines (D1) at an offset drawn per seed bucket
caps         ramp's base at scale 1 but for k / 16 + 1 lines at scale 2, which
             alone qualify: caps_plan(n) puts exactly 65, 64, 33 and 32 of them
             (every 5th line from line 3 of a chunk on) into chunks 1, 2, 5
             and 6 as far as k / 16 + 1 goes, and the rest 48 to a chunk from
             the last chunk backwards: one chunk one line past LQCAP beside one
             exactly at it and no other past it (the finish inside the scan
             launch, which runs from 128 chunks on, gives the call up for that
             one line), and the same for LWCAP on the calls whose threshold
             stands 1 % above them all

What was tuned on the CPU, against the reach conditions of
tests/test_layered_host.py, and why:

* stripes.  With every stripe at S the k / 16 qualifying lines spread over
  1 / 8 of the bucket: 41 per 512-line chunk at every size, never past the 64
  a chunk lists.  With the odd stripes at S / 4 they fall into the even
  stripes alone: about 82 per stripe, so one call has chunks over 64, chunks
  under it and empty ones.
* ramp.  A scale falling by 1 / L per line moves a line sum by 2^-14 of itself
  or less, 4 lines per 256-ulp window bin at the most.  Falling in steps of
  RAMP_STEP = 256 lines, the lines of a step differ by the drawn noise alone (about
  200 ulps of the sum), so a bin holds far more than 32 of them.
* plateau.  With 8 equal slices and equal probabilities the pops are 1 line
  in 12 of the first slice (a tenth of them heap neighbours) and no sum has
  512 lines among them.  With a first slice of L / 64 lines and
  PLATEAU_SIDE = 128, 78 % of its lines are sixteen middle magnitudes: one
  sum, 557 of the 656 pops at the largest size, nearly all of them adjacent.
* moving.  A hot region of the same scale elsewhere meets the old threshold
  like the old one did, and the heap gives a dozen scattered lines.  At
  0.85 S on odd calls half the qualifying lines fall below t and the heap
  gives hundreds of adjacent ones; 1.05 S on even calls brings regime A back.
* sparse_rows.  With 99.9 % zeros 1.6 % of the lines hold a value, more than
  the k / 16 = 1 % a call asks for, and no fill reaches the zero run.  With
  99.98 % zeros 0.3 % do; the dense lines are 5/4 k / 16 on the first call
  (a threshold above zero), 1/2 k / 16 on odd calls (the fill ends in the zero
  run) and 3/2 k / 16 on even ones (regime A).
* back.  A tail of n % 16 elements is judged on its signed sum; at S it
  passes the threshold on 4 % of the calls.  At TAIL_S = 4 S it passes on
  about a third and is a heap candidate on the rest.
"""
from __future__ import annotations

import numpy as np

from edge_values import draws
from stellatrain_amd.synth import D1, D3, seed_for, synth

KINDS = ("front", "back", "straddle", "stripes", "ramp", "plateau", "moving", "sparse_rows", "caps")
HOT_KINDS = ("front", "back", "straddle", "stripes")
SIZES = (65541, (1 << 18) + 5, (1 << 20) + 13)  # 8, 32 and 128 one-bucket chunks
K = {65541: 655, (1 << 18) + 5: 2621, (1 << 20) + 13: 10485}  # merge_numel(n, 0.99); k % 16 > 3
CALLS = 6
SEED_BUCKET = 1100  # kind j uses SEED_BUCKET + 10 j + SEED_OFFSET (seed_bucket_of)

S = 16.0
TAIL_S = 4 * S
RAMP_BASE = 1e-3
RAMP_STEP = 256
PLATEAU_BASE = 2.0 ** -10
PLATEAU_SIDE = 128
PLATEAU_WIDTHS = (1, 1, 2, 4, 8, 16, 16, 16)  # slice widths in 64ths of the bucket
MOVING_ODD, MOVING_EVEN = 0.85, 1.05
CAPS_COUNTS, CAPS_CHUNKS, CAPS_REST = (65, 64, 33, 32), (1, 2, 5, 6), 48
SPARSE_DENSE = (5, 6, 2)  # dense lines in quarters of k / 16: first call, even calls, odd calls
SPARSE_ZP = 9998

LINE = 16
CHUNK = 512  # lines per one-bucket scan chunk (tv16_dev.h)
BATCH_CHUNK = 2048  # lines per batched scan chunk
LQCAP, LWCAP, LBCAP = 64, 32, 32  # per-chunk capacities of the scan's lists (tv16_dev.h, tv16lfin.h)
WINDOW_ULPS = 1 << 18
TOPK_TILE, TOPK_SUP_CAP = 8192, 1024  # topk1.hip
# threshold-v: a call of n floats runs min(CUs, TV_MAXG, ceil(n / 4 / 4096))
# ranges (tv.hip:366-367, launch geometry; 256 CUs on the MI355X) and lists at
# most LCAP = TV_SCAP * TWG / 1024 = 4096 qualifiers per range in LDS
# (tv.hip:42, TV_SCAP ws.h:21); a range past it is scanned again in order
TV_LCAP, TV_RANGE_F4, TV_CUS = 4096, 4096, 256


# the seed bucket of each kind: the first of ten at which every reach condition
# of tests/test_layered_host.py holds at every size (both regimes within six
# calls is a matter of the drawn noise at 65,541 floats)
SEED_OFFSET = {"front": 1, "back": 1, "straddle": 7, "ramp": 1}


FULL_STREAM_MAX_N = 65541  # the fixtures keep whole streams up to this size, hashes above
TV_KINDS = ("front", "back", "stripes")
TV_SIZES = (65541, (1 << 20) + 13)  # 5 and 65 ranges
TOPK_KINDS = ("front", "back", "stripes", "moving")
TOPK_SIZES = (65541, (1 << 20) + 13)  # 9 and 129 tiles
TOPK_CALLS = CALLS  # a first call and the hinted ones after it


def tv16_cases():
    return [(kind, n) for kind in KINDS for n in SIZES]


def tv_cases():
    return [(kind, n) for kind in TV_KINDS for n in TV_SIZES]


def topk_cases():
    return [(kind, n) for kind in TOPK_KINDS for n in TOPK_SIZES]


def seed_bucket_of(kind: str) -> int:
    return SEED_BUCKET + 10 * KINDS.index(kind) + SEED_OFFSET.get(kind, 0)


def merge_k(n: int, world: int = 1) -> int:
    from stellatrain_amd import merge_numel
    return merge_numel(n, 0.99, world)


def hot_lines(n: int) -> int:
    return 3 * (K[n] // LINE) // 2


def sparse_lines(n: int, it: int) -> int:
    """Dense lines of sparse_rows on call `it`, in quarters of k / 16."""
    return K[n] // LINE * SPARSE_DENSE[0 if it == 0 else 1 + it % 2] // 4


def caps_plan(n: int):
    """[(chunk, hot lines)]: CAPS_COUNTS in order while k / 16 + 1 lines last,
    what is left over CAPS_REST to a chunk from the last chunk backwards."""
    left, plan = K[n] // LINE + 1, []
    for c, m in zip(CAPS_CHUNKS, CAPS_COUNTS):
        if left >= m:
            plan.append((c, m))
            left -= m
    c = n // LINE // CHUNK - 1
    while left:
        plan.append((c, min(left, CAPS_REST)))
        left -= plan[-1][1]
        c -= 1
    return plan


def caps_lines(n: int) -> np.ndarray:
    out = []
    for c, m in caps_plan(n):
        out.append(c * CHUNK + 3 + 5 * np.arange(m))
    return np.concatenate(out)


def straddle_centre(n: int, seed_bucket: int) -> int:
    r = draws("straddle", seed_bucket, 0, 2)
    c = 1 + int(r[0] % np.uint64(max(n // LINE // BATCH_CHUNK - 1, 1)))
    d = int(r[1] % np.uint64(4))
    return BATCH_CHUNK * c + CHUNK * d - 3


def hot_scale(kind: str, n: int, seed_bucket: int, it: int) -> np.ndarray:
    """Per-element scale (float64) of the kinds built on synth D1."""
    lines, h = n // LINE, hot_lines(n)
    sc = np.ones(lines + 1, np.float64)  # per line; the last entry is the ragged tail's
    if kind == "front":
        sc[:h] = S
    elif kind == "moving":
        a = it * (h // 2)
        sc[a:a + h] = S * (MOVING_ODD if it % 2 else MOVING_EVEN if it else 1.0)
    elif kind == "back":
        sc[lines - h:lines] = S
        sc[lines] = TAIL_S
    elif kind == "straddle":
        a = straddle_centre(n, seed_bucket) - h // 2
        sc[a:a + h] = S
    elif kind == "stripes":
        ln = np.arange(lines + 1) - 5
        stripe = ln // CHUNK
        hot = (ln >= 0) & (stripe % 8 == 0)
        sc[hot] = np.where((stripe[hot] // 8) % 2 == 0, S, S / 4)
    else:
        raise ValueError(kind)
    return np.repeat(sc, LINE)[:n]


def layered_input(kind: str, n: int, seed_bucket: int, it: int) -> np.ndarray:
    lines = n // LINE
    if kind in ("front", "back", "straddle", "stripes", "moving"):
        x = synth(n, seed_for(seed_bucket, it), D1).astype(np.float64) * hot_scale(kind, n, seed_bucket, it)
    elif kind == "ramp":
        r = draws(kind, seed_bucket, it, n)
        u = ((r >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.float64) / float(1 << 24)
        sign = 1.0 - 2.0 * (r & np.uint64(1)).astype(np.float64)
        ln = np.minimum(np.arange(n) // LINE, lines)
        scale = 2.0 - (ln // RAMP_STEP * RAMP_STEP).astype(np.float64) / lines
        x = sign * RAMP_BASE * (1.0 + u / 4096.0) * scale
    elif kind == "caps":
        r = draws(kind, seed_bucket, it, n)
        u = ((r >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.float64) / float(1 << 24)
        sign = 1.0 - 2.0 * (r & np.uint64(1)).astype(np.float64)
        sc = np.ones(lines + 1, np.float64)
        sc[caps_lines(n)] = 2.0
        x = sign * RAMP_BASE * (1.0 + u / 4096.0) * np.repeat(sc, LINE)[:n]
    elif kind == "plateau":
        r = draws(kind, seed_bucket, it, n)
        c = ((r >> np.uint64(8)) % np.uint64(PLATEAU_SIDE)).astype(np.int64)
        mag = np.where(c == 0, 1.0, np.where(c == 1, 0.5, 0.75))  # 3/4 but for 2 draws in PLATEAU_SIDE
        sign = 1.0 - 2.0 * (r & np.uint64(1)).astype(np.float64)
        edges = np.cumsum(PLATEAU_WIDTHS) * lines // sum(PLATEAU_WIDTHS)
        sl = np.minimum(np.searchsorted(edges, np.arange(n) // LINE, side="right"), 7)
        x = sign * PLATEAU_BASE * mag * np.exp2(-sl.astype(np.float64))
    elif kind == "sparse_rows":
        x = synth(n, seed_for(seed_bucket, it), D3, SPARSE_ZP)
        h = sparse_lines(n, it)
        a = int(draws(kind, seed_bucket, 0, 1)[0] % np.uint64(lines - sparse_lines(n, 2)))
        x[a * LINE:(a + h) * LINE] = synth(n, seed_for(seed_bucket, it), D1)[a * LINE:(a + h) * LINE]
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x.astype(np.float32))


# ---------------------------------------------------------------------------
# what one thresholdv16 call asks of the kernels, from the oracle alone
# ---------------------------------------------------------------------------
def _per(mask: np.ndarray, width: int) -> np.ndarray:
    """Set entries of a per-line mask per chunk of `width` lines."""
    return np.add.reduceat(mask.astype(np.int64), np.arange(0, mask.size, width))


def _longest_run(a: np.ndarray) -> int:
    if a.size == 0:
        return 0
    edges = np.flatnonzero(np.concatenate([[True], a[1:] != a[:-1], [True]]))
    return int(np.diff(edges).max())


def probe(oracle, src: np.ndarray, k: int, t_before: float, t_after: float, count: int, idx: np.ndarray) -> dict:
    """The call `oracle.tv16_compress(h, key, src, k)` that met threshold
    `t_before`, left `t_after` and wrote `count` pairs with indices `idx`."""
    n = src.size
    lines, tail = n // LINE, n % LINE
    sums = oracle.tv16_block_sums(src)
    t = np.float32(t_before)
    qual = sums >= t
    q = int(np.count_nonzero(qual))
    head = min(q, k // LINE) * LINE  # slots written by whole qualifying lines (stage 1)
    stage2 = q > k // LINE and k % LINE != 0  # the next qualifying line gives a prefix
    out = {"q": q, "head": head, "qual_512": _per(qual, CHUNK), "regime": "B" if t_after < t_before else "A"}
    # stage 3 (thresholdv16.cpp:212-236): the ragged tail on its signed sum
    out["tail_stage3"] = False
    if tail and not stage2 and head < k:
        s = np.float32(0)
        for v in src[lines * LINE:]:
            s = np.float32(s + v)
        out["tail_stage3"] = bool(np.float32(s * np.float32(LINE)) >= np.float32(t * np.float32(tail)))
    if stage2 or head == k:  # the ordered scan ran into the output limit: the line that took the last slot
        out["limit_line"] = int(idx[count - 1]) // LINE
    tb = int(t.view(np.uint32))
    sb = sums.view(np.uint32).astype(np.int64)  # |x| sums: non-negative, bits order as values
    win = (sb >= max(tb - WINDOW_ULPS, 0)) & (sb < tb)
    out["win_512"], out["win_2048"] = _per(win, CHUNK), _per(win, BATCH_CHUNK)
    bins = (tb - 1 - sb[win]) >> 8
    out["bin_max"] = int(np.bincount(bins).max()) if bins.size else 0
    if out["regime"] == "B":
        first = head + (min(tail, k - head) if out["tail_stage3"] else 0)
        pops = np.asarray(idx[first:count:LINE], np.int64) // LINE  # one entry per popped line, pop order
        # heap position = index in the oracle's cand order: the lines below t
        # in scan order, then the tail where stage 3 did not emit it
        pos_of = np.cumsum(~qual) - 1
        is_tail = pops >= lines
        hp = np.where(is_tail, int(np.count_nonzero(~qual)), pos_of[np.minimum(pops, lines - 1)])
        out["tail_cand"] = bool(tail and not out["tail_stage3"])
        out["tail_popped"] = bool(is_tail.any())
        popped = np.zeros(int(np.count_nonzero(~qual)) + 2, bool)
        popped[hp] = True
        parent = np.where(hp > 0, (hp - 1) // 2, hp)
        sibling = np.where(hp > 0, ((hp - 1) ^ 1) + 1, hp)
        near = (popped[parent] & (hp > 0)) | (popped[np.minimum(sibling, popped.size - 1)] & (hp > 0))
        out["M"] = int(pops.size)
        out["near_frac"] = float(np.count_nonzero(near)) / max(pops.size, 1)
        out["run"] = _longest_run(sums[pops[~is_tail]])
        out["pop_zero"] = int(np.count_nonzero(sums[pops[~is_tail]] == 0))
    return out


def tv_ranges(n: int) -> np.ndarray:
    """Start (in floats) of every threshold-v range of a call of n floats, and n."""
    n4 = n // 4
    # (a mirror of the launch geometry only while the 4,096-float4 rule gives
    # fewer ranges than the device has CUs: below 2^22 floats on 256 CUs)
    assert (n4 + TV_RANGE_F4 - 1) // TV_RANGE_F4 < TV_CUS, n
    g = max(1, min(TV_CUS, (n4 + TV_RANGE_F4 - 1) // TV_RANGE_F4))
    w = np.arange(g + 1, dtype=np.int64)
    lo = (w * (n4 // g) + np.minimum(w, n4 % g)) * 4
    lo[-1] = n
    return lo
