"""Cases and the CPU reference of the threshold-v one-call send path (shared by
tests/test_tv_send_host.py and tests/test_gpu_tv_send.py; not a test module).

A case is one task of ``stg_merge_send_batch_device`` on a threshold-v handle:
``n`` floats, ``k``, ``cap`` index slots (``W = min(cap, n)`` of them are
sent), wire flag, ``N`` local gradient sources, residual or not.  ``grads(it)``
are the fresh gradients of call ``it``: synth buckets scaled by
``scales[it % len(scales)]`` (tests/test_gpu_send_batch.py's SCALES by
default), the first one an ``edge_values`` bucket when ``kind`` is given.

``Ref`` is what the engine computes for a case, call after call, with the
oracle: ``gather_add``, ``tv_compress`` into ``cap`` zeroed slots, the wire
form of the first ``W`` slots, the error feedback over all ``cap`` slots by
numpy (compress.cpp:178-179: the unused slots hold index 0).  It also counts,
per call, what the kernel's paths depend on -- every qualifier (not capped) and
the qualifiers of each range the batched scan cuts the bucket into -- from the
threshold the oracle held before the call.
"""
from __future__ import annotations

import numpy as np

from edge_values import edge_input
from stellatrain_amd.synth import D1, seed_for, synth

SCALES = [1.0, 1.0, 0.01, 0.01, 1.0, 30.0]  # tests/test_gpu_send_batch.py's
NAN_SCALES = [1.0, 1.0, 4.0, 1.0, 4.0, 1.0]  # a NaN call (from the third on) with a large gradient
LCAP = 4096       # qualifiers a range lists in LDS (ws.h TV_SCAP)
RANGE_F4 = 4096   # float4 per range at most (ws.h TV_BATCH_RANGE)
SEQ_CALLS = 12    # SCALES twice through


def ranges_of(n: int) -> int:
    return max(1, (n // 4 + RANGE_F4 - 1) // RANGE_F4)


def range_bounds(n: int):
    """[lo, hi) in floats of the ranges of an n-float task (tv_batch.hip's
    split of n / 4 float4; the n % 4 tail belongs to the last range)."""
    n4, g = n // 4, ranges_of(n)
    per, rem = divmod(n4, g)
    out = []
    for w in range(g):
        lo = w * per + min(w, rem)
        ln = per + (1 if w < rem else 0)
        out.append((4 * lo, n if w == g - 1 else 4 * (lo + ln)))
    return out


class Case:
    def __init__(self, n, k, flag, N, dist=D1, resid=True, cap=None, shift=False, seed=0, kind=None, scales=SCALES,
                 bf16=False):
        self.n, self.k, self.flag, self.N, self.dist = n, k, flag, N, dist
        self.resid, self.cap, self.shift, self.seed = resid, k if cap is None else cap, shift, seed
        self.kind, self.scales, self.bf16 = kind, scales, bf16
        self.W = min(self.cap, n)

    def __repr__(self):
        return (f"n={self.n} k={self.k} cap={self.cap} flag={self.flag} N={self.N} resid={self.resid} "
                f"shift={self.shift} kind={self.kind} bf16={self.bf16}")

    def grads(self, it):
        """The call's sources as float32 arrays (a bf16 source: already rounded
        to bf16, so widening it back is exact)."""
        s = np.float32(self.scales[it % len(self.scales)])
        out = []
        for r in range(self.N):
            if r == 0 and self.kind:
                x = edge_input(self.kind, self.n, 700 + 20 * self.seed, it)
            else:
                x = synth(self.n, seed_for(700 + 20 * self.seed + r, it), self.dist)
            x = (x * s).astype(np.float32)
            if self.bf16 and r == 1:
                x = (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)  # (truncated: a bf16 value)
            out.append(x)
        return out

    def resid0(self):
        return (synth(self.n, seed_for(699 + 20 * self.seed, 0)) * np.float32(0.25)).astype(np.float32)


class Step:
    """One call's reference results and path counts."""
    __slots__ = ("grad", "count", "idx", "wi", "wv", "t_next", "found", "per_range")


class Ref:
    """The reference side of one case over its calls (one oracle key each)."""

    def __init__(self, oracle, handle, key: int, case: Case):
        self.o, self.h, self.key, self.c = oracle, handle, key, case
        self.r = case.resid0() if case.resid and case.n else None

    def step(self, srcs) -> Step:
        o, c = self.o, self.c
        x = srcs[0].copy()
        if c.resid:
            for r in range(c.N):  # every local rank's slice: the whole bucket
                o.gather_add([x] + list(srcs[1:]), self.r, r)
        else:
            for s in srcs[1:]:
                x = (x + s).astype(np.float32)
        t = o.tv_state(self.h, self.key)
        if t is None:
            t = o.tv_first_threshold(x, c.k)
        with np.errstate(invalid="ignore"):
            q = np.abs(x) >= np.float32(t)
        st = Step()
        st.found = int(np.count_nonzero(q))
        st.per_range = [int(np.count_nonzero(q[a:b])) for a, b in range_bounds(c.n)]
        st.count, io, vo = o.tv_compress(self.h, self.key, x, c.k, cap=c.cap)
        assert st.count == min(st.found, c.cap), (st.count, st.found, c)
        st.idx = io
        st.wi, st.wv = o.wire_encode(io[:c.W], vo[:c.W], c.flag)
        if c.resid:
            x[io[:c.cap]] = 0  # all numel slots, the unused ones holding index 0
            self.r = x.copy()
        st.grad = x
        st.t_next = o.tv_state(self.h, self.key)
        return st


def run_ref(oracle, case: Case, calls: int):
    """The steps of `calls` calls of one case on a fresh oracle handle."""
    h = oracle.tv_new()
    try:
        ref = Ref(oracle, h, 1, case)
        return [ref.step(case.grads(it)) for it in range(calls)]
    finally:
        oracle.tv_free(h)


# ---- the cases of tests/test_gpu_tv_send.py ----

SINGLE_N = (1, 3, 5, 4099, 16384, 16388, 16391)


def single_cases(n):
    """One-task calls at size n: every flag, N in {1, 2, 9}, with and without a
    residual, the residual and the sources at another 16-byte phase."""
    k = max(1, n // 100)
    return [Case(n, k, 0, 1, seed=1), Case(n, k, 1, 2, seed=2, shift=True), Case(n, k, 2, 9, seed=3, resid=False),
            Case(n, k, 3, 2, seed=4, shift=True, resid=False), Case(n, k, 3, 9, seed=5)]


# the 12-call sequences: each must meet every situation test_tv_send_host.py lists
SEQ_CASES = {
    "n60000": Case(60000, 600, 1, 2, seed=6),            # u16 indices past 32,767; four ranges of 15,000 floats
    "n16391_shift": Case(16391, 163, 3, 2, seed=7, shift=True),  # two ranges, the n % 4 tail, scalar residual stores
}
NAN_CASE = Case(16391, 163, 0, 1, seed=8, kind="nan_steady", scales=NAN_SCALES)
NAN_CALLS = 6

# The data seed at which, with n = 4099, k = 41 and 400 slots (the first calls
# find more than k, and only the first `cap` in index order are emitted), a
# reference stream holds an element of the n % 4 tail (indices 4096..4098) in
# one of the first three calls: found with the oracle, which
# tests/test_tv_send_host.py asserts.
TAIL_N, TAIL_K, TAIL_CAP, TAIL_CALLS = 4099, 41, 400, 3


def tail_case(seed):
    return Case(TAIL_N, TAIL_K, 3, 3, seed=seed, cap=TAIL_CAP)


TAIL_SEED = 0

# idx_cap > n: W = n = 40 of the 48 slots are sent
CAP_PAST_N = Case(40, 4, 1, 2, cap=48, seed=9)


def batch_sizes():
    """40 sizes from 1 to 300,007: one to five and 19 ranges, ragged
    and not; index 20 is the empty task."""
    base = (1, 1000, 4099, 16384, 16388, 60000, 70001, 300007, 7, 33333)
    out = [b if b == 300007 else b + j // len(base) for j, b in ((j, base[j % len(base)]) for j in range(40))]
    out[20] = 0
    return out


LATE = (3, 11, 17, 25, 38)   # tasks whose key first appears at call 2
BF16_TASK = 5                # the task with a bf16 source (the typed entry point)
BATCH_CALLS = 4


def batch_cases(engine: bool):
    from stellatrain_amd import merge_numel, wire_flag
    out = []
    for j, n in enumerate(batch_sizes()):
        f = (j // 3) % 4
        if engine:
            k, flag = merge_numel(n, 0.99), wire_flag(n)
        else:
            k = max(1, n // 100) if n else 0
            flag = f if not (f & 1) or n < 65536 else wire_flag(n, bool(f & 2))
        N = 2 if j == BF16_TASK else (1, 2, 4)[j % 3]
        out.append(Case(n, k, flag, N, resid=j % 5 != 4, seed=10 + j, bf16=j == BF16_TASK,
                        cap=4 if not n and not engine else None))
    return out


def batch_live(it):
    """The tasks of call `it`, in order."""
    return [j for j in range(40) if it >= 2 or j not in LATE]


LARGE_N = (1 << 22) + 5  # 257 ranges: more than a 256-CU device's launch takes, so the task runs alone
