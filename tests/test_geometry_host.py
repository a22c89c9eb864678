"""The case tables of tests/test_gpu_geometry.py, pinned with the oracle alone.

A pass of the GPU tests shows a branch correct only if the tables reach it:
both thresholdv16 regimes, the ragged last line, both sides of threshold-v's
cap, top-k with k == n and with k no multiple of 4, and regime-B fills that
start at a multiple of 4 and at none (the `cnt & 3` half of the emitters'
vector condition).  A table entry that fails one of these is replaced in
tests/geometry.py, not excused here.  What cannot hold is named:

* thresholdv16 sizes with fewer than 32 full lines (the tiny family, the
  b256 family and c2@b / c5@w of the batch) need not reach both regimes;
* a threshold-v sequence with k == 0 cannot count below k, one with cap > n
  (k = n + 3) cannot reach its cap, and with n < 4 and k <= 1 the first
  threshold is the only magnitude that matters; for the tiny family both
  outcomes are required of the family, not of each sequence.
"""
from __future__ import annotations

import numpy as np

import geometry as G


def _keys(items):
    return sorted({it[0] for it in items})


def test_thresholdv16_sequences_meet_both_regimes(oracle):
    exempt = []
    for label, items, scales, b0, ties in G.tv16_tables():
        seq = G.tv16_batch_sequence(oracle, items, scales, b0, ties)
        for key in _keys(items):
            js = [j for j, it in enumerate(items) if it[0] == key]
            n = items[js[0]][1]
            regimes = {row[j][6] for row in seq for j in js} - {None}
            if n // 16 < 32:
                exempt.append((label, key, n))
                continue
            assert regimes == {"A", "B"}, (label, key, n, regimes)
    assert exempt and all(n // 16 < 32 for _, _, n in exempt)
    # the exempt ones are the families named in the module docstring
    assert {lb.split(":")[1] for lb, _, _ in exempt} <= {"tiny", "b256", "batch"}, exempt


def test_thresholdv16_head_restates_the_oracle(oracle):
    """tv16_head (the scan's count, where a regime-B fill starts) agrees with
    the oracle's state update on every call: head < cap exactly where the
    threshold went down; the fill never writes below head."""
    for label, items, scales, b0, ties in G.tv16_tables():
        seq = G.tv16_batch_sequence(oracle, items, scales, b0, ties)
        before = {}
        for row in seq:
            for (key, n, k, _, _), (x, co, io, vo, st, head, regime) in zip(items, row):
                if regime is not None and before[key][0] > 0:
                    assert (regime == "B") == (st[0] < before[key][0]), (label, key)
                    assert head <= co <= k
                before[key] = st


def test_thresholdv16_ragged_line_is_emitted(oracle):
    seen = {}
    for label, items, scales, b0, ties in G.tv16_tables():
        seq = G.tv16_batch_sequence(oracle, items, scales, b0, ties)
        for row in seq:
            for (key, n, k, _, off), (x, co, io, vo, *_rest) in zip(items, row):
                if n % 16 and k:
                    pos = (io[:co].astype(np.int64) - off) % (1 << 32)
                    seen[n] = seen.get(n, False) or bool((pos >= n // 16 * 16).any())
    assert seen and all(seen.values()), sorted(n for n, s in seen.items() if not s)


def test_threshold_v_sequences_meet_both_sides_of_the_cap(oracle):
    tiny = {"below": 0, "cap": 0}
    for label, n, k, bucket, scales in G.tv_tables():
        seq = G.tv_sequence(oracle, n, k, bucket, scales)
        assert all(co == min(above, k) for _x, co, _i, _v, _t, above in seq), label
        below = any(above < k for *_x, above in seq)
        at_cap = any(above >= k and co == k for _x, co, _i, _v, _t, above in seq)
        if label.startswith("E:tiny"):
            tiny["below"] += below
            tiny["cap"] += at_cap
            if k == 0 or k > n or (n < 4 and k <= 1):
                continue
        assert below and at_cap, (label, [(co, above) for _x, co, _i, _v, _t, above in seq])
    assert tiny["below"] and tiny["cap"]


def test_topk_tables(oracle):
    for name, table in G.topk_tables().items():
        assert any(k == n for n, k in table), name
        assert any(k % 4 for n, k in table), name
        assert all(k <= n for n, k in table), name   # k > n is the reference's undefined behaviour


def test_fill_mode_sequence_starts_fills_on_both_sides_of_cnt_and_3(oracle):
    n, k = G.CHILD
    seq = G.tv16_sequence(oracle, n, k, G.BUCKET_CHILD, G.SCALES_CHILD, ties=G.TIES_CHILD)
    heads = [head for *_x, head, regime in seq if regime == "B"]
    assert any(h % 4 for h in heads) and any(h % 4 == 0 for h in heads), heads
    # and the fill emits the ragged line itself once (the tail's rank in the pop order)
    assert any(regime == "B" and (io[head:co] >= n // 16 * 16).any() for _x, co, io, _v, _s, head, regime in seq)
    # equal sums among the pops, at full scale (the window holds the fill) and
    # after the drop (the crew's calls): the path counters the parent asserts
    # count calls that had ties to order
    tied = []
    for (x, co, io, _v, _s, head, regime), scale in zip(seq, G.SCALES_CHILD):
        if regime == "B":
            sums = oracle.tv16_block_sums(x)
            lines = np.unique(io[head:co].astype(np.int64) // 16)
            popped = sums[lines[lines < sums.size]]
            tied.append((scale, popped.size - np.unique(popped).size))
    assert any(s == 1.0 and t for s, t in tied) and any(s != 1.0 and t for s, t in tied), tied


def test_case_tables_are_the_issue_s():
    assert G.PHASES4 == (0, 4, 8, 12) and G.PHASES2 == (0, 2, 6, 8, 14)
    assert {t[0] for t in G.TRIPLES_A} == set(G.PHASES4) and len(G.TRIPLES_A) == 11
    assert len(G.BATCH_C) == 9 and len({b[0] for b in G.BATCH_C}) == 8            # one repeated key
    assert len({b[5] for b in G.BATCH_C}) == 9                                      # a phase triple per bucket
    assert {b[4] for b in G.WIRE_C} == {0, 1, 2, 3}
    # every 2-byte phase is used by a 16-bit output of the wire launch
    ph = {b[6][1] for b in G.WIRE_C if b[4] & 1} | {b[6][2] for b in G.WIRE_C if b[4] & 2}
    assert ph >= set(G.PHASES2), ph
    assert [b[4] for b in G.RESID_C] == list(G.PHASES4)
    tiny = G.tiny_cases(True)
    assert {n for n, _ in tiny} == set(G.TINY_N)
    for n in G.TINY_N:
        assert {k for m, k in tiny if m == n} == {0, 1, min(n, 16), n, n + 3}
    for b in G.BOUNDS:
        cs = G.boundary_cases(b)
        assert {n - b for n, _ in cs} == set(G.DELTAS)
        for d in (-1, 0, 1):
            assert {k % 16 for n, k in cs if n == b + d} >= {0, 1, 15}
