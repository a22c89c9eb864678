"""CPU-only checks of the threshold-v one-call send path: (a) the grouping
arithmetic of its scan launches (``stg_debug_tv_batch_plan``, the rule the
entry point packs by), and (b) that the sequences tests/test_gpu_tv_send.py
runs meet, by the reference alone, every situation the kernels branch on -- a
sequence that misses one fails here instead of silently weakening the GPU
test."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import tv_send_cases as T

NONE = 0xFFFFFFFF


def _plan(sizes, num_cu=256):
    from stellatrain_amd._capi import lib
    n = (C.c_uint64 * max(len(sizes), 1))(*sizes)
    first = (C.c_uint32 * max(len(sizes), 1))()
    launch = (C.c_uint32 * max(len(sizes), 1))()
    rc = lib().stg_debug_tv_batch_plan(n, len(sizes), num_cu, first, launch)
    return rc, list(first)[:len(sizes)], list(launch)[:len(sizes)]


def test_header_declares_and_python_binds_the_plan_export():
    from stellatrain_amd._capi import _SIGS, header_symbols, lib
    assert "stg_debug_tv_batch_plan" in header_symbols()
    assert "stg_debug_tv_batch_plan" in _SIGS and hasattr(lib(), "stg_debug_tv_batch_plan")


def test_plan_ranges_per_size():
    """0: no launch; 1 and 16,384: one range; 16,388: two; 60,000: four (the
    first range of the next task says so); 2^22 + 5: 257, alone on 256 CUs."""
    sizes = [0, 1, 16384, 16388, 60000, 5, (1 << 22) + 5, 3]
    rc, first, launch = _plan(sizes)
    assert launch == [NONE, 0, 0, 0, 0, 0, 1, 2] and rc == 3
    assert first == [0, 0, 1, 2, 4, 8, 0, 0]
    assert [T.ranges_of(n) for n in sizes[1:7]] == [1, 1, 2, 4, 1, 257]
    # the same large task shares a launch on a wider device
    rc, first, launch = _plan([3, (1 << 22) + 5, 3], num_cu=304)
    assert rc == 1 and launch == [0, 0, 0] and first == [0, 1, 258]


def test_plan_40_tasks_split_into_groups_of_16():
    rc, first, launch = _plan([1000] * 40)
    assert rc == 3 and launch == [0] * 16 + [1] * 16 + [2] * 8
    assert first == list(range(16)) + list(range(16)) + list(range(8))


def test_plan_group_closes_before_the_range_cap():
    """60,000 floats are four ranges: on 10 CUs a launch takes two such tasks
    (a third would make 12 ranges), and the cap never passes TV_MAXG = 2048."""
    rc, first, launch = _plan([60000] * 5, num_cu=10)
    assert rc == 3 and launch == [0, 0, 1, 1, 2] and first == [0, 4, 0, 4, 0]
    n = 4 * 4096 * 200  # 200 ranges
    rc, first, launch = _plan([n] * 21, num_cu=100000)
    assert launch == [j // 10 for j in range(21)] and first == [200 * (j % 10) for j in range(21)]
    assert max(f + 200 for f in first) <= 2048


def test_plan_large_task_runs_alone_and_keeps_the_order():
    sizes = [1000, 60000, (1 << 22) + 5, 1000, 0, 4099]
    rc, first, launch = _plan(sizes)
    assert rc == 3 and launch == [0, 0, 1, 2, NONE, 2] and first == [0, 1, 0, 0, 0, 1]


def test_plan_first_range_is_monotonic_within_a_launch():
    sizes = T.batch_sizes()
    rc, first, launch = _plan(sizes)
    assert rc == max(l for l in launch if l != NONE) + 1
    for l in range(rc):
        tasks = [j for j in range(len(sizes)) if launch[j] == l]
        assert 1 <= len(tasks) <= 16
        want = 0
        for j in tasks:  # consecutive runs of ranges, from 0
            assert first[j] == want, (l, j)
            want += T.ranges_of(sizes[j])
        assert want <= 256
    assert launch[20] == NONE and sizes[20] == 0


def test_plan_refuses_null_arrays_and_no_cus():
    from stellatrain_amd._capi import lib
    f = lib().stg_debug_tv_batch_plan
    assert f(None, 2, 256, None, None) == -1
    assert _plan([5], num_cu=0)[0] == -1
    assert _plan([])[0] == 0


# ---- (b) the GPU test's sequences, by the reference alone ----

@pytest.mark.parametrize("name", sorted(T.SEQ_CASES))
def test_sequence_meets_every_situation(oracle, name):
    """Over SCALES twice through with the residual carried: a call that finds
    more than the capacity, a call that finds fewer (the unused slots: element
    0 zeroed), and a range with more qualifiers than the LDS list holds."""
    c = T.SEQ_CASES[name]
    steps = T.run_ref(oracle, c, T.SEQ_CALLS)
    found = [s.found for s in steps]
    assert any(f > c.cap for f in found), found
    assert any(0 <= f < c.cap for f in found), found
    assert any(max(s.per_range) > T.LCAP for s in steps), [s.per_range for s in steps]
    assert all(s.count == min(s.found, c.cap) for s in steps)


def test_sequence_n60000_matches_the_model(oracle):
    """n = 60,000, k = 600, N = 2: calls 0-5 find 601 to about 54,500, call 5
    more than 13,000 in one range of 15,000 floats; calls 6-10 find 0 to 4; and
    u16 indices past 32,767 are on the wire."""
    c = T.SEQ_CASES["n60000"]
    assert c.n == 60000 and c.k == 600 and c.N == 2 and c.flag & 1
    assert [b - a for a, b in T.range_bounds(c.n)] == [15000] * 4
    steps = T.run_ref(oracle, c, T.SEQ_CALLS)
    found = [s.found for s in steps]
    assert found[0] == 601 and all(601 <= f <= 60000 for f in found[:6]) and found[5] > 50000, found
    assert max(steps[5].per_range) > 13000
    assert all(0 <= f <= 4 for f in found[6:11]), found
    assert any((s.idx[:s.count] > 32767).any() for s in steps)


def test_nan_sequence_has_a_nan_call_that_finds_more_than_k(oracle):
    """From the third call on the bucket holds NaNs (carried by the residual
    too); on such a call k < cnt, so the threshold moves by gmax under the
    reference's NaN-restart rule, and the last NaN sits in the last range."""
    c = T.NAN_CASE
    steps = T.run_ref(oracle, c, T.NAN_CALLS)
    lo = T.range_bounds(c.n)[-1][0]
    hits = 0
    for it, s in enumerate(steps):
        # (the bucket after the error feedback: a NaN never qualifies, so it stays where it was)
        nan = np.flatnonzero(np.isnan(s.grad))
        assert (nan.size > 0) == (it >= 2), it
        if nan.size and s.found > c.k:
            hits += 1
            assert nan[-1] >= lo
    assert hits >= 2
    assert np.isfinite(steps[2].t_next)  # the restart rule, not a NaN threshold, on the first NaN call


def test_tail_seed_selects_an_element_of_the_ragged_tail(oracle):
    c = T.tail_case(T.TAIL_SEED)
    steps = T.run_ref(oracle, c, T.TAIL_CALLS)
    assert max(int((s.idx[:s.count] >= c.n // 4 * 4).sum()) for s in steps) > 0


def test_batch_cases_cover_what_the_gpu_test_claims():
    sizes = T.batch_sizes()
    assert len(sizes) == 40 and min(s for s in sizes if s) == 1 and max(sizes) == 300007 and sizes[20] == 0
    assert sorted({T.ranges_of(s) for s in sizes if s}) == [1, 2, 3, 4, 5, 19]
    for engine in (False, True):
        cs = T.batch_cases(engine)
        assert cs[T.BF16_TASK].bf16 and cs[T.BF16_TASK].N == 2 and cs[T.BF16_TASK].resid
        assert {c.flag for c in cs} >= ({0, 1} if engine else {0, 1, 2, 3})
        assert all(c.cap == c.k for c in cs if c.n)
    # first-call and steady keys share a launch at call 2
    _, _, launch = _plan([sizes[j] for j in T.batch_live(2)])
    live = T.batch_live(2)
    for l in set(launch) - {NONE}:
        group = [live[i] for i in range(len(live)) if launch[i] == l]
        if any(j in T.LATE for j in group):
            assert any(j not in T.LATE for j in group), group
    assert T.BF16_TASK not in T.LATE and 20 not in T.LATE
    assert T.ranges_of(T.LARGE_N) == 257
