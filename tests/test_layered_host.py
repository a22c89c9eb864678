"""Do the layered inputs of tests/layered.py reach what they are for?  (CPU.)

Every condition below is computed with the oracle alone -- its line sums
(orc_tv16_block_sums), its thresholds (orc_tv16_state) and its streams -- over
the calls tests/test_gpu_layered.py runs: CALLS calls per key, every kind at
every size.  A failure here means the inputs no longer drive the kernels where
they should (the fixture is inadequate), not that a kernel is wrong.  The
constants of layered.py were tuned until all of them held; layered.py says
what was tuned and why.

Conditions that cannot hold at a size, and are asserted at the others only:

* a 512-line chunk with more than LQCAP = 64 qualifying lines, and the output
  limit inside one: not at 65,541 floats.  There k / 16 = 40, a steady
  threshold lets 41 lines through, and no chunk can hold 65 of them.
* a run of more than 256 equal sums among the pops: not at 2^18 + 5 floats,
  where a call pops k / 16 + 1 = 164 lines at the most.  The run asserted
  there is "more than 128", over three quarters of the pops.
* threshold-v, a range over LCAP = 4,096 qualifiers: at 2^20 + 13 floats only;
  k is 655 and 2,621 at the other two sizes.
"""
from __future__ import annotations

import numpy as np
import pytest

import layered as ly

LARGE = ly.SIZES[1:]


@pytest.fixture(scope="module")
def calls(oracle):
    """{(kind, n): [probe of every call after the first]}."""
    out = {}
    for kind in ly.KINDS:
        for n in ly.SIZES:
            h = oracle.tv16_new()
            rows = []
            for it in range(ly.CALLS):
                x = ly.layered_input(kind, n, ly.seed_bucket_of(kind), it)
                before = oracle.tv16_state(h, "p")
                cnt, idx, _ = oracle.tv16_compress(h, "p", x, ly.K[n])
                if before is not None:
                    rows.append(ly.probe(oracle, x, ly.K[n], before[0], oracle.tv16_state(h, "p")[0], cnt, idx))
                else:
                    assert oracle.tv16_state(h, "p")[0] > 0, (kind, n)  # a zero threshold never moves again
            oracle.tv16_free(h)
            out[(kind, n)] = rows
    return out


def _b(rows):
    return [r for r in rows if r["regime"] == "B"]


def test_sizes_and_k():
    from stellatrain_amd import merge_numel
    for n in ly.SIZES:
        assert ly.K[n] == merge_numel(n, 0.99) and ly.K[n] % 16 > 3 and n % 16


@pytest.mark.parametrize("kind", ly.KINDS)
def test_both_regimes_everywhere(calls, kind):
    for n in ly.SIZES:
        assert {r["regime"] for r in calls[(kind, n)]} == {"A", "B"}, n


@pytest.mark.parametrize("kind", ly.HOT_KINDS)
def test_overflowing_chunk_beside_empty_ones(calls, kind):
    """One call has a chunk with more than LQCAP qualifying lines and a chunk
    with none."""
    for n in LARGE:
        assert any(r["qual_512"].max() > ly.LQCAP and (r["qual_512"] == 0).any() for r in calls[(kind, n)]), n


def test_stripes_mix_listed_and_rescanned_chunks(calls):
    """stripes: one call has chunks over LQCAP, chunks with 1 .. LQCAP
    qualifying lines, and empty ones."""
    for n in LARGE:
        assert any(r["qual_512"].max() > ly.LQCAP and ((r["qual_512"] > 0) & (r["qual_512"] <= ly.LQCAP)).any()
                   and (r["qual_512"] == 0).any() for r in calls[("stripes", n)]), n


@pytest.mark.parametrize("kind", ly.HOT_KINDS)
def test_output_limit_inside_an_overflowing_chunk(calls, kind):
    """The ordered scan's stream ends at a line of an overflowing chunk that is
    not the chunk's last."""
    for n in LARGE:
        hit = [r for r in calls[(kind, n)] if "limit_line" in r
               and r["qual_512"][r["limit_line"] // ly.CHUNK] > ly.LQCAP
               and r["limit_line"] % ly.CHUNK != ly.CHUNK - 1 and r["limit_line"] != n // 16 - 1]
        assert hit, n


def test_straddle_crosses_both_chunk_edges():
    """The hot region crosses a 512-line edge at every size and a 2,048-line
    edge at one of them at least."""
    both = 0
    for n in ly.SIZES:
        c, h = ly.straddle_centre(n, ly.seed_bucket_of("straddle")), ly.hot_lines(n)
        a, b = c - h // 2, c - h // 2 + h - 1
        assert a // ly.CHUNK != b // ly.CHUNK and b < n // 16, n
        both += a // ly.BATCH_CHUNK != b // ly.BATCH_CHUNK
    assert both


def test_ramp_window_is_one_position_range(calls):
    for n in ly.SIZES:
        assert any(r["win_512"].max() > ly.LWCAP and r["win_2048"].max() > 64
                   and 2 * np.count_nonzero(r["win_512"] == 0) >= r["win_512"].size for r in _b(calls[("ramp", n)])), n


@pytest.mark.parametrize("kind", ["ramp", "plateau"])
def test_window_bin_overflows(calls, kind):
    for n in ly.SIZES:
        assert any(r["bin_max"] > ly.LBCAP for r in calls[(kind, n)]), n


@pytest.mark.parametrize("kind", ["ramp", "moving", "plateau"])
def test_pops_are_heap_neighbours(calls, kind):
    """A quarter of a regime-B call's pops have another pop at their heap
    parent or sibling (positions in the oracle's cand order)."""
    for n in ly.SIZES:
        assert any(r["near_frac"] >= 0.25 and r["M"] >= 16 for r in _b(calls[(kind, n)])), n


def test_plateau_runs_of_equal_sums(calls):
    assert max(r["run"] for r in _b(calls[("plateau", (1 << 18) + 5)])) > 128
    assert max(r["run"] for r in _b(calls[("plateau", (1 << 20) + 13)])) > 512


def test_back_tail_in_stage3_and_in_the_heap(calls):
    for n in ly.SIZES:
        rows = calls[("back", n)]
        assert any(r["tail_stage3"] for r in rows) and any(r.get("tail_cand") for r in _b(rows)), n


def test_sparse_rows_cut_in_the_zero_run(calls):
    for n in ly.SIZES:
        assert any(r["pop_zero"] > 0 for r in _b(calls[("sparse_rows", n)])), n


def test_caps_exactly_at_and_one_past_the_capacities(calls):
    """caps: a regime-A call whose qualifying lines are the plan's, chunk by
    chunk -- 65 = LQCAP + 1 beside 64 = LQCAP at the two larger sizes -- and
    a regime-B call whose window lines are the same lines: 33 = LWCAP + 1
    at every size, beside 32 = LWCAP at the largest.  Nothing qualifies
    outside the plan."""
    for n in ly.SIZES:
        plan = dict(ly.caps_plan(n))
        want = np.zeros(n // 16 // ly.CHUNK, np.int64)
        for c, m in plan.items():
            want[c] = m
        rows = calls[("caps", n)]
        assert any(r["regime"] == "A" and np.array_equal(r["qual_512"], want) for r in rows), n
        assert any(np.array_equal(r["win_512"], want) and r["q"] == 0 for r in _b(rows)), n
        assert ly.LWCAP + 1 in plan.values(), n
        if n != ly.SIZES[0]:
            assert plan[1] == ly.LQCAP + 1 and plan[2] == ly.LQCAP, n
        assert sorted(plan.values())[-2:] == [ly.LQCAP, ly.LQCAP + 1] or n == ly.SIZES[0], n  # no other chunk past LQCAP
    assert ly.LWCAP in dict(ly.caps_plan(ly.SIZES[2])).values()


def test_topk_tiles():
    """Some 8,192-element tile holds more than TOPK_SUP_CAP elements at or
    above the k-th magnitude and at least 100 tiles hold none."""
    n = (1 << 20) + 13
    for kind in ly.TOPK_KINDS:
        hit = False
        for it in range(ly.TOPK_CALLS):
            a = np.abs(ly.layered_input(kind, n, ly.seed_bucket_of(kind), it))
            kth = np.partition(a, n - ly.K[n])[n - ly.K[n]]
            per = np.add.reduceat((a >= kth).astype(np.int64), np.arange(0, n, ly.TOPK_TILE))
            hit |= bool(per.max() > ly.TOPK_SUP_CAP and np.count_nonzero(per == 0) >= 100)
        assert hit, kind
    assert -(-n // ly.TOPK_TILE) == 129


def test_thresholdv_range_overflows(oracle):
    """front, back: some range holds more qualifiers than LCAP and others hold
    none.  stripes (at most two hot chunks to a range, 1,310 qualifiers each):
    listed ranges beside empty ones, none past LCAP."""
    n = (1 << 20) + 13
    lo = ly.tv_ranges(n)
    for kind in ly.TV_KINDS:
        h = oracle.tv_new()
        hit = False
        for it in range(ly.CALLS):
            x = ly.layered_input(kind, n, ly.seed_bucket_of(kind), it)
            t = oracle.tv_state(h, 1)
            oracle.tv_compress(h, 1, x, ly.K[n])
            if t is not None:
                per = np.add.reduceat((np.abs(x) >= np.float32(t)).astype(np.int64), lo[:-1])
                if kind == "stripes":
                    hit |= bool(1024 < per.max() <= ly.TV_LCAP and 2 * np.count_nonzero(per == 0) >= per.size)
                else:
                    hit |= bool(per.max() > ly.TV_LCAP and (per == 0).any())
        oracle.tv_free(h)
        assert hit, kind
