"""Shared case table of the ratio-change parity tests (test infrastructure).

The engine moves a key's k at run time (configure_compression_ratio, then
k = numel * (1 - ratio) / world per task), while all of the key's state -- the
thresholdv16 threshold and its increment, the threshold-v threshold, the top-k
hint -- outlives the change.  The schedules below change k between calls of one
key: tenfold down and up, to a half, and to the whole bucket (ratio 0).

Used by tests/golden/make_golden_ratio.py (fixtures from the reference),
tests/test_oracle_golden_ratio.py (CPU oracle against them, and that the table
reaches what it is for) and tests/test_gpu_ratio.py (HIP against the oracle).
"""
from __future__ import annotations

import hashlib

import numpy as np

from stellatrain_amd.synth import D1, D3, seed_for, synth

# one call per entry
RATIOS = [0.99, 0.99, 0.99, 0.9, 0.9, 0.9, 0.999, 0.999, 0.999, 0.5, 0.5, 0.99, 0.99, 0.99, 0.0, 0.99, 0.99]
SEED_BUCKET = 900
# 4103: k = 4 < 16 at ratio 0.999 (no whole-line slot).  (1 << 18) + 5 at ratio
# 0 and (1 << 20) + 13 at 0.5 fill more than three tiles of 4,096 lines.
SIZES = [4103, 65541, (1 << 18) + 5, (1 << 20) + 13]
FULL_STREAM_MAX_N = 65541  # fixtures keep whole streams up to this size, hashes above
FULL_STREAM_MAX_COUNT = 8192  # ... and up to this many pairs per call, hashes above

# the batched launch: key j of a launch starts at offset 3 j of RATIOS
BATCH_KEYS = 6
BATCH_SIZES = [65541, (1 << 18) + 5]
BATCH_STEPS = len(RATIOS)

# exact-zero lines tying at the cut of a large fill.  With 90 % zeros about 22 %
# of the lines sum to exactly 0; ratio 0 pops every line, so no zero line is
# left at the cut: the 0.1 calls pop 90 % of the lines and cut inside the run.
D3_ZP = 9000
D3_SIZES = [65541, (1 << 18) + 5]
D3_SEED_BUCKET = 910
D3_RATIOS = RATIOS + [0.1, 0.1, 0.99]

# threshold-v, one source address per schedule.  RATIOS leaves cnt_found / k
# between 0.002 and 14; the spike schedule converges at k = n / 10 and then asks
# for n / 10000, so cnt_found / k is in the hundreds and the step
# 0.01 * cnt_found / k * grad_abs_max throws the threshold above every element.
TV_SIZES = [65541, (1 << 20) + 13]
TV_SCHEDULES = {"ratios": RATIOS, "spike": [0.9, 0.9, 0.9, 0.9999, 0.9999, 0.9, 0.9]}
TV_SEED_BUCKET = {"ratios": SEED_BUCKET, "spike": 920}

TOPK_N = (1 << 20) + 5
TOPK_SEED_BUCKET = 930

WINDOW_ULPS = 1 << 18  # the scan lists the lines with sum in [t - 2^18 ulps, t)


def merge_k(n: int, ratio: float, world: int = 1) -> int:
    from stellatrain_amd import merge_numel
    return merge_numel(n, ratio, world)


def ratio_input(n: int, it: int, dist: int = D1, param: int = 0, bucket: int = SEED_BUCKET) -> np.ndarray:
    return synth(n, seed_for(bucket, it), dist, param)


def schedule(n: int, world: int = 1, ratios=None):
    """[(it, ratio, k)] of a one-key schedule (RATIOS by default)."""
    return [(it, r, merge_k(n, r, world)) for it, r in enumerate(RATIOS if ratios is None else ratios)]


def batch_ratio(j: int, step: int) -> float:
    return RATIOS[(3 * j + step) % len(RATIOS)]


def batch_schedule(n: int):
    """[[(key, seed bucket, it, ratio, k) per key] per launch]: key j is 3 j
    entries ahead in RATIOS, so one launch mixes keys whose k just grew, just
    shrank and stayed."""
    return [[(f"rb{j}@weight", SEED_BUCKET + 1 + j, step, batch_ratio(j, step), merge_k(n, batch_ratio(j, step)))
             for j in range(BATCH_KEYS)] for step in range(BATCH_STEPS)]


def topk_ks(n: int = TOPK_N):
    return [n // 100, n // 10, n // 1000, n // 2, n // 100, 0, n // 100]


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def fill_probe(oracle, src: np.ndarray, k: int, t_before: float, count: int):
    """What a regime-B call asks of the fill, from the oracle's line sums:
    (q, head, M, window) -- q whole lines at or above the threshold, head slots
    written by the ordered scan, M lines needed from the heap, and the number
    of lines the scan's window [t - 2^18 ulps, t) holds."""
    sums = oracle.tv16_block_sums(src)
    t = np.float32(t_before)
    q = int(np.count_nonzero(sums >= t))
    head = min(q, k // 16) * 16
    m = -(-(count - head) // 16)
    tb = int(t.view(np.uint32))
    sb = sums.view(np.uint32).astype(np.int64)  # |x| sums: non-negative, bits order as values
    window = int(np.count_nonzero((sb >= max(tb - WINDOW_ULPS, 0)) & (sb < tb)))
    return q, head, m, window
