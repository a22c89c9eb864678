"""GPU parity of the batched MERGE decompress + optimizer step on world > 1
tasks (``merge_optimize_batch`` groups of one world sharing world + 4 launches,
merge_batch_world.hip) and the launch counter that shows the sharing
(``merge_batch_launches``).

Every comparison is bit for bit (uint32 views), against (a) the sequence the
call replaces -- ``merge_optimize_wire`` per tensor on a twin handle -- and,
for plain SGD and Adam, (b) the oracle: ``wire_decode`` -> ``merge_decompress``
-> ``sgd_apply`` / ``adam_apply``.  Inputs are tests/wire_merge_cases.py's, or
streams built here where a test needs a parameter length of its own; the
harness is tests/test_gpu_merge_batch.py's ``_Run``.
"""
from __future__ import annotations

import numpy as np
import pytest

import wire_merge_cases as W
from test_gpu_merge_batch import BASE, CAP, G, PR, _Run, _case, _sorted, _up

pytestmark = pytest.mark.gpu

GROUP_CAP = CAP // 2      # elements of one world > 1 group: two winner words each
BIG = (1 << 22) + 16      # above the cap: runs the per-tensor sequence
_CUSTOM = {}


class _BigScratch:
    """One caller dense / mark pair for every world > 1 task of a call (the
    largest n used here)."""

    def __init__(self, torch, gpu):
        self.dense = torch.zeros(BIG, dtype=torch.float32, device=gpu)
        self.mark = torch.zeros(BIG, dtype=torch.uint8, device=gpu)

    def is_zero(self, torch):
        return not bool(self.dense.view(torch.int32).any()) and not bool(self.mark.any())


@pytest.fixture(scope="module")
def big_scratch(gpu):
    import torch
    return _BigScratch(torch, gpu)


def _custom(oracle, n, per_rank, flag, world, seed):
    """(streams, merged idx, merged val) of `world` encoded ranks whose indices
    are drawn over the whole of [0, n) (the last element included), values over
    1e-9 .. 1e3; computed once and shared."""
    key = (n, per_rank, flag, world, seed)
    if key not in _CUSTOM:
        rng = np.random.default_rng([n, per_rank, flag, world, seed])
        streams = []
        for r in range(world):
            idx = rng.integers(0, n, per_rank, dtype=np.uint32)
            if r == world - 1:
                idx[0] = n - 1
            wi, wv = oracle.wire_encode(idx, W._values(rng, per_rank), flag)
            streams.append((wi, wv, flag))
        ei, ev = W.expected(oracle, streams, per_rank, n)[2:4]
        _CUSTOM[key] = (streams, ei, ev)
    return _CUSTOM[key]


class _WRun(_Run):
    """``_Run`` with a parameter length per task: a spec may carry ``n`` (then
    its streams are ``_custom``'s)."""

    def _param(self, name, n):
        if name not in self.params:
            p0 = np.resize(BASE, n) + np.float32(len(self.params))
            self.params[name] = (self.torch.from_numpy(p0).to(self.gpu), self.torch.from_numpy(p0).to(self.gpu),
                                 p0.copy())
        return self.params[name]

    def build(self, specs):
        torch, gpu, oracle = self.torch, self.gpu, self.oracle
        items, seq = [], []
        for s in specs:
            if "n" in s:
                n = s["n"]
                streams, ei, ev = _custom(oracle, n, s["per_rank"], s["flag"], s["world"], s["seed"])
            else:
                n = W.n_of(s["flag"])
                streams, ei, ev = _case(oracle, s["family"], s["per_rank"], s["flag"], s["seed"], s["world"])
            pa, pb, po = self._param(s["name"], n)
            dev = [(_up(torch, gpu, wi), _up(torch, gpu, wv), f) for wi, wv, f in streams]
            extra = (self.scratch.dense[:n], self.scratch.mark[:n]) if s["world"] > 1 else ()
            items.append((pa, s["name"], dev, s["per_rank"]) + extra)
            seq.append((pb, dev, extra, po, ei, ev))
        return items, seq

    def check(self, specs, got, seq):
        """The per-tensor loop on `b` and the oracle; every merged stream and
        count compared."""
        assert len(got) == len(specs)
        for s, g, (pb, dev, extra, po, ei, ev) in zip(specs, got, seq):
            kw = dict(dense=extra[0], mark=extra[1]) if extra else {}
            ref = _sorted(*self.b.merge_optimize_wire(pb, s["name"], dev, s["per_rank"], **kw))
            ga = _sorted(*g)
            assert np.array_equal(ga[0], ref[0]) and np.array_equal(ga[1], ref[1]), s
            assert np.array_equal(ga[0], ei) and np.array_equal(ga[1], ev.view(np.uint32)), s
            if s["world"] > 1:  # the merged stream itself is index-ascending, and each index once
                c = int(g[2].cpu().numpy().view(np.uint32)[0])
                assert np.array_equal(g[0].cpu().numpy().view(np.uint32)[:c], ei), s
            if self.h is not None:
                (self.oracle.sgd_apply if self.kind == "sgd" else self.oracle.adam_apply)(self.h, s["name"], po, ev, ei)

    def step(self, specs, prebuilt=False):
        items, seq = self.build(specs)
        if prebuilt:
            from stellatrain_amd import MergeTasks
            items = MergeTasks(items)
        got = self.a.merge_optimize_batch(items)
        self.check(specs, got, seq)


OPTS = {
    "sgd_momentum": ("sgd", dict(lr=0.05, momentum=0.9), True),
    "sgd_smart_nesterov_wd": ("sgd", dict(lr=0.05, momentum=0.9, nesterov=True, weight_decay=0.01,
                                          smart_momentum=True), True),
    "adam_wd": ("adam", dict(lr=0.01, weight_decay=0.01), True),
    "adam_amsgrad": ("adam", dict(lr=0.01, weight_decay=0.01, amsgrad=True), False),
}


def _specs(T, seed, world):
    """T tasks of one world: per_rank cycles through PR, flags 0-3 and both
    families mixed (n = 2^20 at flags 0 and 2, 60,000 at 1 and 3, so the cap
    closes groups as well as the group limit would)."""
    return [dict(name=f"t{i}", family=W.FAMILIES[(i // 2) % 2], per_rank=PR[i % len(PR)], flag=i % 4, seed=seed + i,
                 world=world) for i in range(T)]


def _plan(specs):
    """Tensors per group as the header documents the closing rule (all tasks of
    one world, names distinct)."""
    groups, cur, elems = [], 0, 0
    for s in specs:
        n = s.get("n", W.n_of(s["flag"]))
        if cur == G or (cur and elems + n > GROUP_CAP):
            groups.append(cur)
            cur, elems = 0, 0
        cur += 1
        elems += n
    return groups + [cur]


@pytest.mark.parametrize("opt", ["sgd_momentum", "sgd_smart_nesterov_wd", "adam_wd"])
@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("T", [1, 5, G, G + 1, 2 * G + 3])
def test_group_sizes(gpu, oracle, big_scratch, T, world, opt):
    """1. One task, part of a group, and sixteen and more tasks at world 2, 3
    and 8; per_rank over PR (the wire block / tail split at 8, the tile edges),
    flags 0-3 and both families mixed in one call."""
    import torch
    from stellatrain_amd import merge_batch_launches
    from stellatrain_amd.engine import scatter_merge_check
    kind, opts, with_oracle = OPTS[opt]
    r = _WRun(torch, gpu, oracle, big_scratch, kind, opts, with_oracle)
    specs = _specs(T, 1000, world)
    assert T < 4 or {s["flag"] for s in specs} == {0, 1, 2, 3}
    items, seq = r.build(specs)
    if T % 2 == 0:
        from stellatrain_amd import MergeTasks
        items = MergeTasks(items)
    before = merge_batch_launches()
    got = r.a.merge_optimize_batch(items)
    assert merge_batch_launches() - before == len(_plan(specs)) * (world + 4)
    r.check(specs, got, seq)
    if kind == "sgd":
        assert r.a.iteration == T
    r.compare()
    assert big_scratch.is_zero(torch)
    scatter_merge_check()
    r.close()


def test_launch_count(gpu, oracle, big_scratch):
    """2. 32 distinct world-2 tasks of 60,000 floats are two full groups: at most
    2 * (2 + 4) launches, where the per-tensor sequence takes 2 + 5 per task --
    which an amsgrad handle still does, inside the same call."""
    import torch
    from stellatrain_amd import merge_batch_launches
    from stellatrain_amd.engine import scatter_merge_check
    world, T = 2, 2 * G
    specs = [dict(name=f"c{i}", family="encoded", per_rank=600, flag=1 if i % 2 else 3, seed=2000 + i, world=world)
             for i in range(T)]
    assert _plan(specs) == [G, G]
    for opt, want in (("sgd_momentum", None), ("adam_wd", None), ("adam_amsgrad", T * (world + 5))):
        kind, opts, with_oracle = OPTS[opt]
        r = _WRun(torch, gpu, oracle, big_scratch, kind, opts, with_oracle)
        items, seq = r.build(specs)
        before = merge_batch_launches()
        got = r.a.merge_optimize_batch(items)
        used = merge_batch_launches() - before
        print(f"{opt}: {used} launches for {T} world-{world} tasks")
        if want is None:
            assert 0 < used <= 2 * (world + 4), (opt, used)
        else:
            assert used == want, (opt, used)
        r.check(specs, got, seq)
        r.compare()
        scatter_merge_check()
        r.close()


def test_rank_order_and_ragged_slices(gpu, oracle, big_scratch):
    """3. One world-8 group of n = 17, 4,099 and 60,007 (none a multiple of 16:
    load_marks' tail, slices that must not misalign their neighbours).  The
    n = 4,099 tensor has 8 x 1,025 pairs over 4,099 indices and values over
    twelve decades, so the float sum of an element depends on the rank order:
    checked on the CPU first."""
    import torch
    from stellatrain_amd import merge_batch_launches
    from stellatrain_amd.engine import scatter_merge_check
    world = 8
    specs = [dict(name="r17", n=17, per_rank=9, flag=3, seed=3000, world=world),
             dict(name="r4099", n=4099, per_rank=1025, flag=1, seed=3001, world=world),
             dict(name="r60007", n=60007, per_rank=1023, flag=3, seed=3002, world=world)]
    assert all(s["n"] < 65536 and s["n"] % 16 for s in specs) and _plan(specs) == [3]
    streams, ei, ev = _custom(oracle, 4099, 1025, 1, world, 3001)
    ri, rv = W.expected(oracle, streams[::-1], 1025, 4099)[2:4]
    assert np.array_equal(ri, ei) and (rv.view(np.uint32) != ev.view(np.uint32)).any()  # the case tells a wrong order
    assert ei.size > 3000  # and most indices are hit by several of the 8,200 pairs
    for opt in ("sgd_momentum", "adam_wd"):
        kind, opts, with_oracle = OPTS[opt]
        r = _WRun(torch, gpu, oracle, big_scratch, kind, opts, with_oracle)
        before = merge_batch_launches()
        r.step(specs)
        assert merge_batch_launches() - before == world + 4
        r.step(specs, prebuilt=True)  # the slices again, after a first use
        r.compare()
        assert big_scratch.is_zero(torch)
        scatter_merge_check()
        r.close()


@pytest.mark.parametrize("opt", ["sgd_momentum", "adam_wd"])
def test_caller_scratch_is_shared_and_stays_zero(gpu, oracle, opt):
    """4. Several world-2 tasks of one call given one caller dense / mark pair:
    they still share a group, and the pair is all zero afterwards."""
    import torch
    from stellatrain_amd import merge_batch_launches
    from stellatrain_amd.engine import scatter_merge_check
    kind, opts, with_oracle = OPTS[opt]

    class _Own:
        dense = torch.zeros(60000, dtype=torch.float32, device=gpu)
        mark = torch.zeros(60000, dtype=torch.uint8, device=gpu)

    r = _WRun(torch, gpu, oracle, _Own, kind, opts, with_oracle)
    specs = [dict(name=f"z{i}", family=W.FAMILIES[i % 2], per_rank=PR[(i + 3) % len(PR)], flag=1 if i % 2 else 3,
                  seed=4000 + i, world=2) for i in range(5)]
    items, seq = r.build(specs)
    assert len({it[4].data_ptr() for it in items}) == 1 and len({it[5].data_ptr() for it in items}) == 1
    before = merge_batch_launches()
    got = r.a.merge_optimize_batch(items)
    assert merge_batch_launches() - before == 2 + 4
    assert not bool(_Own.dense.view(torch.int32).any()) and not bool(_Own.mark.any())
    r.check(specs, got, seq)
    r.compare()
    scatter_merge_check()
    r.close()


@pytest.mark.parametrize("opt", ["sgd_momentum", "sgd_smart_nesterov_wd", "adam_wd"])
def test_mixed_call(gpu, oracle, big_scratch, opt):
    """5. In one call: a world-1 run, a world-2 run with a repeated name inside
    it, a world-3 task, an empty task and one tensor above the group cap --
    identical to the loop."""
    import torch
    from stellatrain_amd import merge_batch_launches
    from stellatrain_amd.engine import scatter_merge_check
    kind, opts, with_oracle = OPTS[opt]
    r = _WRun(torch, gpu, oracle, big_scratch, kind, opts, with_oracle)
    mk = lambda name, pr, flag, seed, world: dict(name=name, family="encoded", per_rank=pr, flag=flag, seed=seed,  # noqa: E731
                                                  world=world)
    specs = [mk("a", 1025, 1, 5000, 1), mk("b", 9, 0, 5001, 1), mk("c", 4099, 3, 5002, 1),
             mk("d", 1025, 1, 5003, 2), mk("e", 7, 3, 5004, 2), mk("d", 1024, 1, 5005, 2), mk("f", 1023, 0, 5006, 2),
             mk("g", 1025, 3, 5007, 3),
             dict(name="h", family="encoded", per_rank=0, flag=1, seed=0, world=1),
             dict(name="big", n=BIG, per_rank=9, flag=0, seed=5008, world=2)]
    assert BIG > GROUP_CAP
    before = merge_batch_launches()
    r.step(specs)
    # one world-1 pair; world-2 groups {d, e} and {d, f}; the world-3 group; the
    # big tensor's own 2 + 5 (the empty world-1 task launches nothing)
    assert merge_batch_launches() - before == 2 + 2 * (2 + 4) + (3 + 4) + (2 + 5)
    if kind == "sgd":
        assert r.a.iteration == len(specs)
    else:
        assert r.a.state("d", W.n_of(1))[3] == 3 and r.a.state("h", W.n_of(1))[3] == 2
    r.compare()
    assert big_scratch.is_zero(torch)
    scatter_merge_check()
    r.close()


@pytest.mark.parametrize("opt", ["sgd_smart_nesterov_wd", "adam_wd"])
def test_three_iterations_from_one_prebuilt_array(gpu, oracle, big_scratch, opt):
    """6. Three calls on one prebuilt MergeTasks (world-1, world-2 and world-8
    runs), with per-tensor world-1 and world-2 merges on the same stream in
    between: the scratch they share is zero whenever a call starts."""
    import torch
    from stellatrain_amd import MergeTasks, scatter_merge_wire
    from stellatrain_amd.engine import scatter_merge_check
    kind, opts, with_oracle = OPTS[opt]
    r = _WRun(torch, gpu, oracle, big_scratch, kind, opts, with_oracle)
    specs = ([dict(name=f"i{i}", family=W.FAMILIES[i % 2], per_rank=PR[i % len(PR)], flag=i % 4, seed=6000 + i,
                   world=[1, 2, 2, 2, 8, 8][i % 6]) for i in range(12)])
    items, seq = r.build(specs)
    tasks = MergeTasks(items)
    singles = []
    for world, per_rank, flag, seed in ((1, 4099, 0, 6100), (2, 1025, 1, 6101)):
        streams, ei, ev = _case(oracle, "encoded", per_rank, flag, seed, world)
        dev = [(_up(torch, gpu, wi), _up(torch, gpu, wv), f) for wi, wv, f in streams]
        singles.append((dev, per_rank, W.n_of(flag), ei, ev))

    def single():
        for dev, per_rank, n, ei, ev in singles:
            kw = dict(dense=big_scratch.dense[:n], mark=big_scratch.mark[:n]) if len(dev) > 1 else {}
            got = _sorted(*scatter_merge_wire(dev, per_rank, n, **kw))
            assert np.array_equal(got[0], ei) and np.array_equal(got[1], ev.view(np.uint32))

    single()
    for c in range(3):
        got = r.a.merge_optimize_batch(tasks)
        assert got is tasks.outputs
        r.check(specs, got, seq)
        single()
    if kind == "sgd":
        assert r.a.iteration == r.b.iteration == 3 * len(specs)
        assert r.a.last_buffer("i4", W.n_of(0)).max() == 2 * len(specs) + 4  # task 4 of the third call
    else:
        assert r.a.state("i0", W.n_of(0))[3] == 4
    r.compare()
    assert big_scratch.is_zero(torch)
    scatter_merge_check()
    r.close()
