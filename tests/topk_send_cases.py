"""Cases and the CPU reference of the exact top-k one-call send path (shared by
tests/test_topk_send_host.py and tests/test_gpu_topk_send.py; not a test module).

A case is one task of ``stg_merge_send_batch_device`` on a ``"topk_exact"``
handle: ``n`` floats, ``k``, ``cap`` index slots (``W = min(cap, n)`` of them
are sent), wire flag, ``N`` local gradient sources, residual or not.
``grads(it)`` are the fresh gradients of call ``it``: synth buckets scaled by
``scales[it % len(scales)]`` (tests/tv_send_cases.py's SCALES by default), the
first one an ``edge_values`` bucket when ``kind`` is given, or -- ``gen ==
"ties"`` -- magnitudes quantised to 64 levels, ``+-(1 + h % 64) * 2^-10`` with
an integer hash h, whose sums stay exact multiples of 2^-10.

``Ref`` is what the engine computes for a case, call after call, with the
oracle: ``gather_add``, ``topk_compress(x, k, cap, bug_compat=False)`` into
``cap`` zeroed slots, the wire form of the first ``W`` slots, the error
feedback over all ``cap`` slots by numpy (compress.cpp:178-179: the unused
slots hold index 0).  Per call it also reports what the kernels branch on: the
k-th magnitude T, how many elements hold it and how many of those are taken,
the tiles and signs of the ties, the winners whose fresh gradient is below T.
"""
from __future__ import annotations

import numpy as np

from edge_values import edge_input
from stellatrain_amd.synth import D1, D3, _splitmix64, seed_for, synth
from tv_send_cases import SCALES

TILE = 8192      # floats per tile (ws.h TV_TILE)
SEQ_CALLS = 12   # SCALES twice through


def tiles_of(n: int) -> int:
    return max(1, (n + TILE - 1) // TILE)


def mag_bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)


def kth_bits(x, kk: int) -> int:
    """Bits of the kk-th largest magnitude (keys are bits & 0x7fffffff)."""
    m = mag_bits(x)
    return int(np.partition(m, m.size - kk)[m.size - kk])


def ties_bucket(n: int, seed: int) -> np.ndarray:
    with np.errstate(over="ignore"):
        h = _splitmix64(np.uint64(seed) * np.uint64(0x100000001B3) + np.arange(n, dtype=np.uint64))
    mag = (1 + (h % np.uint64(64)).astype(np.int64)).astype(np.float32) * np.float32(2.0 ** -10)
    return np.where((h >> np.uint64(40)) & np.uint64(1), -mag, mag).astype(np.float32)


class Case:
    def __init__(self, n, k, flag, N, dist=D1, param=0, resid=True, cap=None, shift=False, shift0=False, seed=0,
                 kind=None, scales=SCALES, bf16=False, gen="synth", resid_zero=False, off=0):
        self.n, self.k, self.flag, self.N, self.dist, self.param = n, k, flag, N, dist, param
        self.resid, self.cap, self.shift, self.shift0, self.seed = resid, k if cap is None else cap, shift, shift0, seed
        self.kind, self.scales, self.bf16, self.gen, self.resid_zero, self.off = kind, scales, bf16, gen, resid_zero, off
        self.W = min(self.cap, n)
        self.kk = min(k, n)

    def __repr__(self):
        return (f"n={self.n} k={self.k} cap={self.cap} flag={self.flag} N={self.N} resid={self.resid} "
                f"shift={self.shift}/{self.shift0} kind={self.kind} gen={self.gen} bf16={self.bf16} off={self.off}")

    def grads(self, it):
        """The call's sources as float32 arrays (a bf16 source: already rounded
        to bf16, so widening it back is exact)."""
        s = np.float32(self.scales[it % len(self.scales)])
        out = []
        for r in range(self.N):
            sd = seed_for(900 + 20 * self.seed + r, it)
            if self.gen == "ties":
                x = ties_bucket(self.n, sd)
            elif r == 0 and self.kind:
                x = edge_input(self.kind, self.n, 900 + 20 * self.seed, it)
            else:
                x = synth(self.n, sd, self.dist, self.param)
            x = (x * s).astype(np.float32)
            if self.bf16 and r == 1:
                x = (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)  # (truncated: a bf16 value)
            out.append(x)
        return out

    def resid0(self):
        if self.resid_zero:
            return np.zeros(self.n, np.float32)
        return (synth(self.n, seed_for(899 + 20 * self.seed, 0)) * np.float32(0.25)).astype(np.float32)


class Step:
    """One call's reference results and what the kernels branch on."""
    __slots__ = ("grad", "count", "idx", "wi", "wv", "T", "n_eq", "eq_taken", "eq_tiles", "eq_signs", "from_resid",
                 "bucket")


def gather(o, c, srcs, resid):
    """grad[0] after the call's gather-add (every local rank's slice)."""
    x = srcs[0].copy()
    if c.resid:
        for r in range(c.N):
            o.gather_add([x] + list(srcs[1:]), resid, r)
    else:
        for s in srcs[1:]:
            x = (x + s).astype(np.float32)
    return x


class Ref:
    """The reference side of one case over its calls."""

    def __init__(self, oracle, case: Case):
        self.o, self.c = oracle, case
        self.r = case.resid0() if case.resid and case.n else None

    def step(self, srcs) -> Step:
        o, c = self.o, self.c
        fresh = srcs[0].copy()
        for s in srcs[1:]:
            fresh = (fresh + s).astype(np.float32)
        x = gather(o, c, srcs, self.r)
        st = Step()
        st.bucket = x.copy()
        st.count, io, vo = o.topk_compress(x, c.k, cap=c.cap, idx_offset=c.off, bug_compat=False)
        assert st.count == c.cap, (st.count, c)
        st.idx = io
        st.wi, st.wv = o.wire_encode(io[:c.W], vo[:c.W], c.flag)
        st.T = kth_bits(x, c.kk) if c.kk else None
        st.n_eq = st.eq_taken = 0
        st.eq_tiles, st.eq_signs, st.from_resid = set(), set(), 0
        if c.kk:
            m = mag_bits(x)
            eq = np.flatnonzero(m == st.T)
            win = io[:c.kk].astype(np.int64) - c.off
            taken = np.intersect1d(eq, win)
            st.n_eq, st.eq_taken = int(eq.size), int(taken.size)
            st.eq_tiles = set((eq // TILE).tolist())
            st.eq_signs = set(np.signbit(x[eq]).tolist())
            st.from_resid = int(np.count_nonzero(mag_bits(fresh)[win] < st.T))
        if c.resid:
            sel = io[:c.cap]
            x[sel[sel < c.n]] = 0  # all numel slots, the unused ones holding index 0
            self.r = x.copy()
        st.grad = x
        return st


def run_ref(oracle, case: Case, calls: int):
    ref = Ref(oracle, case)
    return [ref.step(case.grads(it)) for it in range(calls)]


# ---- the cases of tests/test_gpu_topk_send.py ----

SINGLE_N = (1, 3, 5, 4099, 8191, 8192, 8193, 16391)


def single_cases(n):
    """One-task calls at size n: every flag, N in {1, 2, 9}, with and without a
    residual, the residual and the sources (and, once, the bucket itself) at
    another 16-byte phase, k in {1, max(1, n // 100), n}, idx_cap above k (and
    above n at the tiny sizes) and an index offset."""
    k1 = max(1, n // 100)
    return [Case(n, 1, 0, 1, seed=1), Case(n, k1, 1, 2, seed=2, shift=True), Case(n, n, 2, 9, seed=3, resid=False),
            Case(n, k1, 3, 2, seed=4, shift=True, shift0=True, resid=False, off=7), Case(n, n, 3, 9, seed=5),
            Case(n, k1, 0, 2, seed=6, cap=k1 + 3)]


# Situation 1 and 2: quantised magnitudes, n = 20,000 (three tiles), k = 777
TIES = Case(20000, 777, 0, 2, seed=7, gen="ties", scales=[1.0], resid_zero=True)
TIES_CALLS = 3
# Situation 3: 99.95 % zeros, k above the non-zero count, zeros taken in index order over two tiles
ZEROS = Case(20000, 9000, 1, 1, dist=D3, param=9995, seed=8, resid_zero=True)
ZEROS_CALLS = 3
# Situations 4 and 5: the 12-call sequences (n = 60,000, k = 600, flag 1: u16 indices past 32,767)
SEQ_CASES = {
    "n60000": Case(60000, 600, 1, 2, seed=9),
    "n16391_shift": Case(16391, 163, 3, 2, seed=10, shift=True),
}
# Situation 6: a winner among the last n % 4 elements of the last, partial tile
# (indices 8204..8206 of n = 8207); the data seed is found with the oracle, which
# tests/test_topk_send_host.py asserts
TAIL_N, TAIL_K, TAIL_CALLS, TAIL_SEED = 8207, 820, 3, 11


def tail_case(seed=TAIL_SEED):
    return Case(TAIL_N, TAIL_K, 3, 3, seed=seed)


# Situation 7: idx_cap > k (the unused slots' element 0 is zeroed) and idx_cap > n
CAP_PAST_K = Case(4099, 41, 1, 2, cap=64, seed=12)
CAP_PAST_N = Case(40, 4, 1, 2, cap=48, seed=13)

NAN_CASES = [Case(16391, 163, 0, 1, seed=14, kind="nan_steady"), Case(16391, 163, 3, 2, seed=15, kind="inf"),
             Case(8193, 81, 1, 2, seed=16, kind="nan_tail_only"), Case(16391, 163, 2, 1, seed=17, kind="inf_first"),
             Case(16391, 3, 0, 1, seed=18, kind="nan_steady")]
NAN_CALLS = 5


def batch_sizes():
    """40 sizes from 1 to 300,007 (one to 37 tiles, ragged and not); index 20
    is the empty task."""
    base = (1, 1000, 4099, 8192, 8193, 60000, 70001, 300007, 7, 33333)
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
        out.append(Case(n, k, flag, N, resid=j % 5 != 4, seed=20 + j, bf16=j == BF16_TASK,
                        cap=4 if not n and not engine else None))
    return out


def batch_live(it):
    """The tasks of call `it`, in order."""
    return [j for j in range(40) if it >= 2 or j not in LATE]
