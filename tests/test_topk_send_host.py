"""CPU-only checks of the exact top-k one-call send path: (a) the grouping
arithmetic of its select launches (``stg_debug_topk_batch_plan``, the rule the
entry point packs by), and (b) that the sequences tests/test_gpu_topk_send.py
runs meet, by the oracle alone, every situation the kernels branch on -- a
sequence that misses one fails here instead of silently weakening the GPU
test."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import topk_send_cases as T

NONE = 0xFFFFFFFF


def _plan(sizes, num_cu=256):
    from stellatrain_amd._capi import lib
    m = max(len(sizes), 1)
    n, first, launch, cap = (C.c_uint64 * m)(*sizes), (C.c_uint32 * m)(), (C.c_uint32 * m)(), C.c_uint32(0)
    rc = lib().stg_debug_topk_batch_plan(n, len(sizes), num_cu, first, launch, C.byref(cap))
    return rc, list(first)[:len(sizes)], list(launch)[:len(sizes)], cap.value


def test_header_declares_and_python_binds_the_plan_export():
    from stellatrain_amd._capi import _SIGS, header_symbols, lib
    assert "stg_debug_topk_batch_plan" in header_symbols()
    assert "stg_debug_topk_batch_plan" in _SIGS and hasattr(lib(), "stg_debug_topk_batch_plan")


def test_plan_tiles_per_size():
    """0: no group; 1 and 8,192: one tile; 8,193: two; 60,000: eight (the first
    tile of the next task says so); one tile over the cap: alone."""
    rc, _, _, cap = _plan([1])
    assert rc == 1 and cap == 256  # one tile per compute unit
    over = (cap + 1) * T.TILE
    sizes = [0, 1, 8192, 8193, 60000, 5, over, 3]
    rc, first, launch, _ = _plan(sizes)
    assert launch == [NONE, 0, 0, 0, 0, 0, 1, 2] and rc == 3
    assert first == [0, 0, 1, 2, 4, 12, 0, 0]
    assert [T.tiles_of(n) for n in sizes[1:7]] == [1, 1, 2, 8, 1, cap + 1]
    # the same task shares a group on a wider device, and exactly the cap still fits
    rc, first, launch, cap2 = _plan([3, over, 3], num_cu=304)
    assert cap2 == 304 and rc == 1 and launch == [0, 0, 0] and first == [0, 1, cap + 2]
    rc, first, launch, _ = _plan([cap * T.TILE, 3])
    assert rc == 2 and launch == [0, 1] and first == [0, 0]


def test_plan_40_tasks_split_into_groups_of_16():
    rc, first, launch, _ = _plan([1000] * 40)
    assert rc == 3 and launch == [0] * 16 + [1] * 16 + [2] * 8
    assert first == list(range(16)) + list(range(16)) + list(range(8))


def test_plan_group_closes_before_the_tile_cap():
    """60,000 floats are eight tiles: on 20 CUs a group takes two such tasks (a
    third would make 24 tiles)."""
    rc, first, launch, cap = _plan([60000] * 5, num_cu=20)
    assert cap == 20 and rc == 3 and launch == [0, 0, 1, 1, 2] and first == [0, 8, 0, 8, 0]


def test_plan_large_task_runs_alone_and_keeps_the_order():
    sizes = [1000, 60000, 257 * T.TILE, 1000, 0, 4099]
    rc, first, launch, _ = _plan(sizes)
    assert rc == 3 and launch == [0, 0, 1, 2, NONE, 2] and first == [0, 1, 0, 0, 0, 1]


def test_plan_first_tile_is_consecutive_within_a_group():
    sizes = T.batch_sizes()
    rc, first, launch, cap = _plan(sizes)
    assert rc == max(l for l in launch if l != NONE) + 1
    for l in range(rc):
        tasks = [j for j in range(len(sizes)) if launch[j] == l]
        assert 1 <= len(tasks) <= 16
        want = 0
        for j in tasks:  # consecutive runs of tiles, from 0
            assert first[j] == want, (l, j)
            want += T.tiles_of(sizes[j])
        assert want <= cap
    assert launch[20] == NONE and sizes[20] == 0


def test_plan_refuses_null_arrays_and_no_cus():
    from stellatrain_amd._capi import lib
    f = lib().stg_debug_topk_batch_plan
    cap = C.c_uint32(0)
    one = (C.c_uint64 * 1)(5)
    out = (C.c_uint32 * 1)()
    assert f(None, 1, 256, out, out, C.byref(cap)) == -1
    assert f(one, 1, 256, None, out, C.byref(cap)) == -1
    assert f(one, 1, 256, out, None, C.byref(cap)) == -1
    assert f(one, 1, 256, out, out, None) == -1
    assert _plan([5], num_cu=0)[0] == -1 and _plan([5], num_cu=-3)[0] == -1
    assert _plan([])[0] == 0


# ---- (b) the GPU test's sequences, by the oracle alone ----

def test_ties_are_partly_taken_span_tiles_and_hold_both_signs(oracle):
    """Situations 1 and 2: the k-th magnitude is shared by more elements than
    are taken, at least one is taken and one is not, the ties lie in more than
    one tile and carry both signs -- on every call; and on one call the taken
    ties themselves reach past the first tile."""
    c = T.TIES
    assert c.n == 20000 and c.k == 777 and c.gen == "ties"
    x = c.grads(0)[0]
    lv = np.abs(x) * np.float32(1024)
    assert np.array_equal(lv, np.round(lv)) and lv.min() >= 1 and lv.max() <= 64 and np.unique(lv).size == 64
    steps = T.run_ref(oracle, c, T.TIES_CALLS)
    past_first = 0
    for s in steps:
        assert 0 < s.eq_taken < s.n_eq, (s.eq_taken, s.n_eq)
        assert len(s.eq_tiles) > 1 and s.eq_signs == {False, True}
        eq = np.flatnonzero(T.mag_bits(s.bucket) == s.T)
        past_first += int(eq[s.eq_taken - 1] >= T.TILE)
    assert past_first


def test_zero_threshold_takes_zeros_in_index_order(oracle):
    """Situation 3: 99.95 % zeros and k above the non-zero count: T = 0, and
    the zeros taken are the first ones in index order, over two tiles."""
    c = T.ZEROS
    for s in T.run_ref(oracle, c, T.ZEROS_CALLS):
        nz = int(np.count_nonzero(s.bucket))
        assert 0 < nz < 20 and s.T == 0 and s.eq_taken == c.k - nz < s.n_eq
        win = s.idx[:c.kk].astype(np.int64)
        zeros = np.flatnonzero(T.mag_bits(s.bucket) == 0)
        assert np.array_equal(np.sort(np.concatenate([np.flatnonzero(s.bucket), zeros[:s.eq_taken]])), win)
        assert zeros[s.eq_taken - 1] >= T.TILE


@pytest.mark.parametrize("name", sorted(T.SEQ_CASES))
def test_sequence_error_feedback_changes_the_winners(oracle, name):
    """Situation 4: with the residual carried over SCALES twice through, some
    winners come from residual mass alone (their fresh gradient is below T)."""
    c = T.SEQ_CASES[name]
    steps = T.run_ref(oracle, c, T.SEQ_CALLS)
    assert sum(s.from_resid > 0 for s in steps) >= 6, [s.from_resid for s in steps]
    assert all(s.count == c.cap for s in steps)
    if name == "n60000":  # situation 5: u16 indices past 32,767 on the wire
        assert c.n == 60000 and c.k == 600 and c.flag == 1
        assert all((s.idx[:c.kk] > 32767).any() for s in steps)


def test_tail_seed_selects_an_element_of_the_ragged_tail(oracle):
    """Situation 6: a winner among the last n % 4 elements of the partial tile."""
    c = T.tail_case()
    assert c.n % 4 == 3 and T.tiles_of(c.n) == 2 and c.n % T.TILE < T.TILE
    steps = T.run_ref(oracle, c, T.TAIL_CALLS)
    assert max(int((s.idx[:c.kk] >= c.n // 4 * 4).sum()) for s in steps) > 0


def test_capacity_past_k_and_past_n_zero_element_0(oracle):
    """Situation 7: idx_cap > k and idx_cap > n: the unused slots hold index 0,
    so element 0 is zeroed although it is no winner."""
    for c in (T.CAP_PAST_K, T.CAP_PAST_N):
        assert c.cap > c.k and (c is T.CAP_PAST_K or c.cap > c.n)
        seen = 0
        for s in T.run_ref(oracle, c, 3):
            assert s.grad[0] == 0 and (s.idx[c.kk:] == 0).all()
            seen += int(0 not in s.idx[:c.kk].tolist() and s.bucket[0] != 0)
        assert seen


def test_batch_cases_cover_what_the_gpu_test_claims():
    sizes = T.batch_sizes()
    assert len(sizes) == 40 and min(s for s in sizes if s) == 1 and max(sizes) == 300007 and sizes[20] == 0
    assert sorted({T.tiles_of(s) for s in sizes if s}) == [1, 2, 5, 8, 9, 37]
    for engine in (False, True):
        cs = T.batch_cases(engine)
        assert cs[T.BF16_TASK].bf16 and cs[T.BF16_TASK].N == 2 and cs[T.BF16_TASK].resid
        assert {c.flag for c in cs} >= ({0, 1} if engine else {0, 1, 2, 3})
        assert all(c.cap == c.k for c in cs if c.n)
    # first-call and steady keys share a group at call 2
    live = T.batch_live(2)
    _, _, launch, _ = _plan([sizes[j] for j in live])
    for l in set(launch) - {NONE}:
        group = [live[i] for i in range(len(live)) if launch[i] == l]
        if any(j in T.LATE for j in group):
            assert any(j not in T.LATE for j in group), group
    assert T.BF16_TASK not in T.LATE and 20 not in T.LATE
