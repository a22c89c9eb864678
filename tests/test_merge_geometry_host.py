"""The case tables of tests/test_gpu_merge_geometry.py, pinned with the oracle
alone (CPU): a pass on the GPU shows a branch correct only if the tables reach
it.

* Every planted case has what it claims (``merge_geometry.claims``): pairs that
  lose to a later occurrence, pairs dropped for an index >= n, scalar-tail
  pairs in the output, the last element n - 1 and the first element of the
  ragged last 16 in the merged set, element 0, and an index every rank holds.
  What cannot hold is an entry of ``merge_geometry.EXEMPT``, listed by name
  below; every entry is used, and none reaches beyond the cases named here.
* SIZE_SCAN has a merged index in tile 0, in the last tile of the first
  mark_scan round, in the first of the second (the last full tile), in between
  and in the ragged tail, and the two rounds count differently.
* World 1 meets the copy-through path and the election in every size family.
* ``oracle.merge_decompress`` is pinned at these shapes by a numpy restatement
  that shares no text with it (``merge_geometry.merge_restated``).
"""
from __future__ import annotations

import numpy as np

import geometry as G
import merge_geometry as M
import wire_merge_cases as W

EXEMPTIONS = {
    "an empty stream claims nothing",
    "fewer than 3 pairs hold no repeat",
    "one pair is the last element alone",
    "no ragged end",
    "too short for the ragged plant",
    "too short for element 0",
    "one rank shares with nobody",
    "u16 cannot address element 65,536",
    "a one-pair tail saturates the ragged plant",
}


def _grid(family):
    worlds, flags = (M.WORLDS, M.FLAGS) if family != "edge" else (M.EDGE_WORLDS, M.EDGE_FLAGS)
    for world in worlds:
        for flag in flags:
            for k, n, m, kind in M.merge_cases(family):
                if kind == "unique" and (world != 1 or (flag & 1 and n > 32768)):
                    continue
                yield k, n, m, kind, flag, world


def test_tables_are_the_issue_s():
    assert {n for n, _ in M.SIZES_TINY} == {1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33}
    for n in M.TINY_N:
        assert {m for x, m in M.SIZES_TINY if x == n} == {0, 1, min(n, 4), n, n + 3}
    assert {n for n, _ in M.SIZES_EDGE} == {b + d for b in (1024, 4096, 8192, 65536) for d in (-1, 0, 1)}
    for n in {n for n, _ in M.SIZES_EDGE}:
        ms = {m for x, m in M.SIZES_EDGE if x == n}
        assert ms >= {1023, 1024, 1025}, n
        assert n < 4095 or ms >= {4095, 4096, 4097}, n
        assert n < 8191 or ms >= {8191, 8193}, n
    # wend = 8 * ((m - 1) / 8) at both ends of a 1,024-pair tile
    assert W.wend(8193) % 1024 == 0 and W.wend(8191) % 1024 == 1024 - 8
    n = M.SIZE_SCAN
    tiles = -(-n // M.MERGE_TILE)
    assert tiles == 4098 and n % M.MERGE_TILE == 5 and tiles - M.SCAN_ROUND == 2
    assert M.WORLDS == (1, 2, 3, 8) and M.FLAGS == (0, 1, 2, 3)
    assert set(M.EXEMPT) == EXEMPTIONS
    # section C's sizes: tiny, and the 1,024 / 4,096 edges
    assert {n for n, _ in M.SIZES_STEP} == set(M.TINY_N) | {1023, 1024, 1025, 4095, 4096, 4097}
    assert M.RAW_LENS == (0, 1, 3, 1023, 1024, 1025, 2049)
    assert set(M.BATCH_N) == {1, 2, 15, 16, 17, 33, 4095, 4096, 4097, 8199}


def test_every_phase_is_met():
    """Streams, outputs and parameters at every phase of their element size,
    in every table that rotates them."""
    for family in ("tiny", "edge"):
        ks = [k for k, *_ in M.merge_cases(family)]
        for flag in M.FLAGS:
            ph = [M.phases(flag, k, r) for k in ks for r in range(3)]
            assert {p[0] for p in ph} == set(G.PHASES2 if flag & 1 else G.PHASES4), (family, flag)
            assert {p[1] for p in ph} == set(G.PHASES2 if flag & 2 else G.PHASES4), (family, flag)
            assert {p[2] for p in ph} == {p[3] for p in ph} == set(G.PHASES4), (family, flag)
            # ... each buffer also misaligned alone, and all aligned
            t = M.triples(flag)
            assert (0, 0, 0) in t and all(any(x[q] and not x[(q + 1) % 3] and not x[(q + 2) % 3] for x in t)
                                          for q in range(3))
    steps = M.step_cases()
    for fam in (lambda n: n <= 33, lambda n: 1023 <= n <= 1025, lambda n: 4095 <= n <= 4097):
        assert {ph for _, n, _, _, ph in steps if fam(n)} == set(G.PHASES4)
        assert {f for _, n, _, f, _ in steps if fam(n)} == set(M.FLAGS)
    for q in range(3):
        assert {t[q] for t in M.TRIPLES_RAW} == set(G.PHASES4)
    for world in M.BATCH_WORLDS:
        specs = M.batch_specs(world)
        assert {s[4] for s in specs} == set(G.PHASES4) and {s[3] for s in specs} == set(M.FLAGS)
        assert {s[1] for s in specs} == set(M.BATCH_N) and len({s[0] for s in specs}) == len(specs)
        assert [s[2] for s in specs].count(0) == 1
        # a full group closes in the middle, the empty task closes the next
        assert M.batch_plan(specs) == [16, 4, 0, 3]


def test_every_case_has_what_it_claims(oracle):
    used = set()
    paths = {}
    for family in ("tiny", "edge"):
        for k, n, m, kind, flag, world in _grid(family):
            streams, idx, val, ei, ev, st = M.case(oracle, n, m, flag, world, 0, kind)
            what = (family, n, m, kind, flag, world)
            assert len(streams) == world and idx.size == val.size == m * world, what
            for wi, wv, f in streams:
                assert wi.size == wv.size == m and f == flag, what
                assert wi.dtype == (np.uint16 if flag & 1 else np.uint32), what
                assert wv.dtype == (np.uint16 if flag & 2 else np.float32), what
            assert np.isfinite(val).all() and np.abs(val).max(initial=0) < 65536, what     # tame
            assert np.isfinite(ev).all(), what
            assert ei.size == 0 or (np.all(np.diff(ei.astype(np.int64)) > 0) and ei[-1] < n), what
            if kind == "unique":
                assert st["dups"] == 0 and st["dropped"] == 0 and ei.size == m > 0, what
                paths.setdefault((family, flag), set()).add("copy")
                continue
            want = M.claims(n, m, flag, world)
            got = M.holds(n, m, world, idx, ei, st)
            assert want <= got, (what, sorted(want - got))
            for name, (props, pred) in M.EXEMPT.items():
                if pred(n, m, flag, world):
                    used.add(name)
            if world == 1 and st["dups"] + st["dropped"]:
                paths.setdefault((family, flag), set()).add("elect")
    assert used == EXEMPTIONS, EXEMPTIONS - used
    # world 1: both paths in every size family, at every flag
    for family, flags in (("tiny", M.FLAGS), ("edge", M.EDGE_FLAGS)):
        for flag in flags:
            assert paths[(family, flag)] == {"copy", "elect"}, (family, flag)


def test_claims_are_not_vacuous():
    """What the exemptions leave: every property is claimed by most cases, the
    ragged end by every n % 16 != 0 with room for its plant."""
    for family in ("tiny", "edge"):
        cases = [(n, m, flag, world) for _, n, m, kind, flag, world in _grid(family) if kind == "planted" and m]
        for p in M.PROPS:
            claimed = [c for c in cases if p in M.claims(*c)]
            if p == "shared":
                assert len(claimed) == len([c for c in cases if c[3] > 1]), family
            elif p == "ragged":
                assert {c[0] for c in claimed} == {c[0] for c in cases if c[0] % 16 and not (c[2] & 1 and c[0] > 65536)}
            else:
                assert 2 * len(claimed) > len(cases), (family, p)
        for n, m, flag, world in cases:
            if m >= n + 3:
                assert {"dups", "dropped", "tail", "last", "zero"} <= M.claims(n, m, flag, world), (n, m, flag)
                assert n % 16 == 0 or (flag & 1 and n > 65536) or "ragged" in M.claims(n, m, flag, world), (n, m, flag)


def test_step_sequences_change_their_index_sets(oracle):
    """Section C: four calls on one name; the merged sets differ from call to
    call (elements skip iterations), every call is non-trivial where the size
    allows, and world 1 alternates election and copy-through."""
    for world in M.STEP_WORLDS:
        seen = set()
        for k, n, m, flag, _ in M.step_cases():
            sets = []
            for c in range(M.STEP_CALLS):
                kind = M.step_kind(world, c) if 0 < m <= n else "planted"
                _, idx, val, ei, ev, st = M.case(oracle, n, m, flag, world, c, kind)
                sets.append(tuple(ei.tolist()))
                if kind == "planted":
                    assert M.claims(n, m, flag, world) <= M.holds(n, m, world, idx, ei, st), (n, m, flag, world, c)
                else:
                    assert st["dups"] == st["dropped"] == 0
                    seen.add("copy")
                if world == 1:
                    si, sv = M.stream_order(idx, val, n)
                    o = np.argsort(si, kind="stable")
                    assert np.array_equal(si[o], ei) and np.array_equal(sv[o].view(np.uint32), ev.view(np.uint32))
            if m >= 8 and n >= 15:
                assert len(set(sets)) > 1, (n, m, flag, world)
        assert world > 1 or seen == {"copy"}


def test_scan_case_reaches_both_rounds(oracle):
    n, t = M.SIZE_SCAN, M.MERGE_TILE
    _, idx, val, ei, ev, st = M.scan_case(oracle, 0)
    tiles = ei.astype(np.int64) // t
    cnt = np.bincount(tiles, minlength=4098)
    # tile 0, the first round's last tile, the second round's first (the last
    # full tile), one in between, and the ragged tail
    for tile in (0, 2048, 4095, 4096, 4097):
        assert cnt[tile] > 0, tile
    assert n - 1 in ei and n - 5 in ei and (n - 5) % 16 == 0           # the tail's last and first element
    first, second = int(cnt[:M.SCAN_ROUND].sum()), int(cnt[M.SCAN_ROUND:].sum())
    assert first > 0 and second > 0 and first != second
    assert cnt[4096] != cnt[4097]                                        # the second round's prefixes differ too
    assert st["dups"] > 0 and st["dropped"] > 0 and st["tail"] > 0
    assert "shared" in M.holds(n, M.SCAN_PER_RANK, M.SCAN_WORLD, idx, ei, st)
    # u16 indices cannot address past 65,535: flag 3 runs the same n for its
    # fp16 values, its saturation-free block indices and its tail words
    _, idx, val, ei, ev, st = M.scan_case(oracle, 3)
    assert ei[-1] == 65535 and ei[0] == 0 and st["dups"] > 0 and st["dropped"] >= 4 * M.SCAN_WORLD and st["tail"] > 0
    assert np.isfinite(ev).all()


def test_merge_decompress_restated(oracle):
    """The oracle's merge at the new shapes against the numpy restatement."""
    checked = 0
    for family in ("tiny", "edge"):
        for k, n, m, kind, flag, world in _grid(family):
            _, idx, val, ei, ev, _ = M.case(oracle, n, m, flag, world, 0, kind)
            ri, rv = M.merge_restated(idx, val, m, world, n)
            assert np.array_equal(ri, ei), (n, m, kind, flag, world)
            assert np.array_equal(rv.view(np.uint32), ev.view(np.uint32)), (n, m, kind, flag, world)
            checked += 1
    assert checked > 1000


def test_raw_cases():
    """Section D: distinct indices, first and last element stepped, and past the
    device length valid indices with gradients that would show."""
    for grad_len in M.RAW_LENS:
        for cap, dlen in M.raw_variants(grad_len):
            gidx, grad = M.raw_case(grad_len, cap, 0)
            assert gidx.size == grad.size == cap and np.unique(gidx).size == cap and gidx.max(initial=0) < M.RAW_N
            assert dlen is None or (dlen < cap and (grad[grad_len:] == 1e6).all() and cap - grad_len == M.RAW_TAIL)
            if grad_len >= 3:
                assert gidx[0] == M.RAW_N - 1 and gidx[1] == 0
        assert {d for _, d in M.raw_variants(grad_len)} == ({None, grad_len - 1, 0} if grad_len else {None, 0})
