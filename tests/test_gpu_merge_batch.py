"""GPU parity of the batched MERGE decompress + optimizer step
(``SparseSGD.merge_optimize_batch`` / ``SparseAdam.merge_optimize_batch``,
``stg_merge_optimize_{sgd,adam}_batch_device``).

Every comparison is bit for bit (uint32 views), against (a) the sequence the
call replaces -- ``merge_optimize_wire`` per tensor on a second handle with
the same settings and cloned parameters -- and, for plain SGD and Adam, (b)
the oracle: ``wire_decode`` -> ``merge_decompress`` -> ``sgd_apply`` /
``adam_apply``.  Inputs are tests/wire_merge_cases.py's
(``make_streams(..., specials=False)``, its PER_RANK, n_of and families).
"""
from __future__ import annotations

import os
import re

import numpy as np
import pytest

import wire_merge_cases as W

pytestmark = pytest.mark.gpu

_WS_H = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stellatrain_amd", "csrc", "ws.h")
G = int(re.search(r"constexpr uint32_t MERGE_BATCH = (\d+);", open(_WS_H).read()).group(1))  # tensors per launch pair
CAP = 1 << int(re.search(r"MERGE_BATCH_WIN_CAP = size_t\(1\) << (\d+);", open(_WS_H).read()).group(1))  # winner words
PR = [1, 7, 9, 1023, 1024, 1025, 4099]  # one-tile and five-tile tensors adjacent
BASE = np.random.default_rng(17).standard_normal(1 << 20).astype(np.float32)
_CACHE = {}


def _up(torch, gpu, a):
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _odd(torch, gpu, a):
    """The wire array one element into a larger tensor: only element-aligned."""
    t = _up(torch, gpu, a)
    big = torch.full((t.numel() + 25,), 0x7fff, dtype=t.dtype, device=gpu)
    big[1:1 + t.numel()] = t
    return big[1:1 + t.numel()]


def _unique_streams(oracle, per_rank, flag, world, seed):
    """No repeat, nothing dropped (indices below 32768, exact as u16): the
    emission's copy-through path."""
    rng = np.random.default_rng([per_rank, flag, world, seed])
    out = []
    for _ in range(world):
        idx = rng.choice(32768, per_rank, replace=False).astype(np.uint32)
        val = (rng.standard_normal(per_rank) * 10.0 ** rng.integers(-3, 4, per_rank)).astype(np.float32)
        wi, wv = oracle.wire_encode(idx, val, flag)
        out.append((wi, wv, flag))
    return out


def _case(oracle, family, per_rank, flag, seed, world=1):
    """(streams, merged idx, merged val) of one task, computed once and shared."""
    key = (family, per_rank, flag, seed, world)
    if key not in _CACHE:
        if per_rank == 0:
            streams = [(np.zeros(1, np.uint16 if flag & 1 else np.uint32),
                        np.zeros(1, np.uint16 if flag & 2 else np.float32), flag)] * world
            ei, ev = np.zeros(0, np.uint32), np.zeros(0, np.float32)
        else:
            streams = (_unique_streams(oracle, per_rank, flag, world, seed) if family == "unique"
                       else W.make_streams(oracle, family, per_rank, flag, world, seed=seed, specials=False))
            ei, ev = W.expected(oracle, streams, per_rank, W.n_of(flag))[2:4]
        _CACHE[key] = (streams, ei, ev)
    return _CACHE[key]


def _specs(T, seed, unique_every=0):
    """T tasks: per_rank cycles through PR, flags 0-3 and both families mixed.
    The u32-index streams (flags 0, 2) carry the planted repeat and
    out-of-range index and the raw u16 ones drop their blocks, so those take
    the ticketed path; per_rank 1 (and the `unique` family) copies through."""
    out = []
    for i in range(T):
        fam = W.FAMILIES[(i // 2) % 2]
        if unique_every and (i + seed) % unique_every == 0:
            fam = "unique"
        out.append(dict(name=f"t{i}", family=fam, per_rank=PR[i % len(PR)], flag=i % 4, seed=seed + i, world=1))
    return out


def _small_specs(T, seed):
    """T tasks of mostly 60,000-float tensors (flags 1 and 3; every eighth one
    a flag-0 tensor of 2^20): sixteen of them stay far below the winner word
    cap, so only the group limit closes a launch.  Raw u16 streams and the
    flag-0 ones take the ticketed path, per_rank 1 and the `unique` family
    copy through."""
    out = []
    for i in range(T):
        fam = "unique" if i % 5 == 2 else W.FAMILIES[(i // 2) % 2]
        flag = 0 if i % 8 == 3 else (1 if i % 2 else 3)
        out.append(dict(name=f"s{i}", family=fam, per_rank=PR[i % len(PR)], flag=flag, seed=seed + i, world=1))
    return out


def _plan(specs):
    """Tensors per launch as the header documents the closing rule (all tasks
    batchable, names distinct): a launch is full at G tensors, or closes before
    the sum of its tensors' n would pass the cap."""
    groups, cur, words = [], 0, 0
    for s in specs:
        n = W.n_of(s["flag"])
        if cur == G or (cur and words + n > CAP):
            groups.append(cur)
            cur, words = 0, 0
        cur += 1
        words += n
    return groups + [cur]


class _Scratch:
    def __init__(self, torch, gpu):
        self.dense = torch.zeros(60000, dtype=torch.float32, device=gpu)
        self.mark = torch.zeros(60000, dtype=torch.uint8, device=gpu)


@pytest.fixture(scope="module")
def scratch(gpu):
    import torch
    return _Scratch(torch, gpu)


def _sorted(oi, ov, cnt):
    c = int(cnt.cpu().numpy().view(np.uint32)[0])
    assert c != 0xffffffff
    i = oi.cpu().numpy().view(np.uint32)[:c]
    v = ov.cpu().numpy().view(np.uint32)[:c]
    o = np.argsort(i, kind="stable")
    return i[o], v[o]


class _Run:
    """A batched handle `a`, its per-tensor twin `b` and (where the oracle has
    the optimizer) an oracle handle, over one set of named parameters."""

    def __init__(self, torch, gpu, oracle, scratch, kind, opts, with_oracle=True):
        from stellatrain_amd import SparseAdam, SparseSGD
        self.torch, self.gpu, self.oracle, self.scratch, self.kind = torch, gpu, oracle, scratch, kind
        cls = SparseSGD if kind == "sgd" else SparseAdam
        self.a, self.b = cls(**opts), cls(**opts)
        self.h = None
        if with_oracle:
            self.h = oracle.sgd_new(**opts) if kind == "sgd" else oracle.adam_new(**opts)
        self.momentum = bool(opts.get("momentum"))
        self.params = {}  # name -> (pa, pb, po)

    def close(self):
        if self.h is not None:
            (self.oracle.sgd_free if self.kind == "sgd" else self.oracle.adam_free)(self.h)

    def _param(self, name, n):
        if name not in self.params:
            p0 = BASE[:n] + np.float32(len(self.params))
            self.params[name] = (self.torch.from_numpy(p0).to(self.gpu), self.torch.from_numpy(p0).to(self.gpu),
                                 p0.copy())
        return self.params[name]

    def step(self, specs, place=_up, prebuilt=False):
        """One batched call on `a` (from a prebuilt MergeTasks array if asked),
        the per-tensor loop on `b`, the oracle; the merged streams and counts
        compared here."""
        torch, gpu, oracle = self.torch, self.gpu, self.oracle
        items, seq = [], []
        for s in specs:
            n = W.n_of(s["flag"])
            streams, ei, ev = _case(oracle, s["family"], s["per_rank"], s["flag"], s["seed"], s["world"])
            pa, pb, po = self._param(s["name"], n)
            dev = [(place(torch, gpu, wi), place(torch, gpu, wv), f) for wi, wv, f in streams]
            extra = (self.scratch.dense[:n], self.scratch.mark[:n]) if s["world"] > 1 else ()
            items.append((pa, s["name"], dev, s["per_rank"]) + extra)
            seq.append((pb, dev, extra, po, ei, ev))
        if prebuilt:
            from stellatrain_amd import MergeTasks
            items = MergeTasks(items)
        got = self.a.merge_optimize_batch(items)
        assert len(got) == len(specs)
        for s, g, (pb, dev, extra, po, ei, ev) in zip(specs, got, seq):
            kw = dict(dense=extra[0], mark=extra[1]) if extra else {}
            ref = _sorted(*self.b.merge_optimize_wire(pb, s["name"], dev, s["per_rank"], **kw))
            ga = _sorted(*g)
            assert np.array_equal(ga[0], ref[0]) and np.array_equal(ga[1], ref[1]), s
            assert np.array_equal(ga[0], ei) and np.array_equal(ga[1], ev.view(np.uint32)), s
            if self.h is not None:
                (oracle.sgd_apply if self.kind == "sgd" else oracle.adam_apply)(self.h, s["name"], po, ev, ei)

    def compare(self):
        """Parameters and optimizer state of every name: a == b (== oracle)."""
        for name, (pa, pb, po) in self.params.items():
            n = po.size
            xa = pa.cpu().numpy().view(np.uint32)
            assert np.array_equal(xa, pb.cpu().numpy().view(np.uint32)), name
            if self.h is not None:
                assert np.array_equal(xa, po.view(np.uint32)), name
            if self.kind == "sgd":
                if self.momentum:
                    ma, mb = self.a.momentum_buffer(name, n), self.b.momentum_buffer(name, n)
                    assert ma is not None and np.array_equal(ma.view(np.uint32), mb.view(np.uint32)), name
                    if self.h is not None:
                        assert np.array_equal(ma.view(np.uint32), oracle_u32(self.oracle.sgd_momentum(self.h, name, n)))
                la, lb = self.a.last_buffer(name, n), self.b.last_buffer(name, n)
                assert (la is None) == (lb is None) and (la is None or np.array_equal(la, lb)), name
            else:
                sa, sb = self.a.state(name, n), self.b.state(name, n)
                for q in (0, 1):
                    assert np.array_equal(sa[q].view(np.uint32), sb[q].view(np.uint32)), name
                assert np.float32(sa[2]).view(np.uint32) == np.float32(sb[2]).view(np.uint32) and sa[3] == sb[3], name
                if self.h is not None:
                    so = self.oracle.adam_state(self.h, name, n)
                    assert np.array_equal(sa[0].view(np.uint32), oracle_u32(so[0])), name
                    assert np.array_equal(sa[1].view(np.uint32), oracle_u32(so[1])), name
        if self.kind == "sgd":
            assert self.a.iteration == self.b.iteration
            self.a.check()
            self.b.check()
        else:
            self.a.check_device()
            self.b.check_device()


def oracle_u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


KINDS = {
    "sgd": ("sgd", dict(lr=0.05, momentum=0.9)),
    "adam": ("adam", dict(lr=0.01, weight_decay=0.01)),
}


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("T", [1, 2, G, G + 1, 2 * G + 1])
def test_group_sizes(gpu, oracle, scratch, T, kind):
    """1. One, part of one, exactly one, one and a bit, two and a bit launch
    groups; per_rank over PR, flags 0-3 and both families mixed in one batch.
    A group of sixteen here sums to more than 8 Mi parameters, so the winner
    word cap closes launches too."""
    import torch
    from stellatrain_amd.engine import scatter_merge_check
    r = _Run(torch, gpu, oracle, scratch, *KINDS[kind])
    specs = _specs(T, 100)
    assert T < 4 or {s["flag"] for s in specs} == {0, 1, 2, 3}
    assert T < G or max(_plan(specs)) < G  # here the cap closes every launch; full groups: the next test
    r.step(specs, prebuilt=T % 2 == 0)
    if kind == "sgd":
        assert r.a.iteration == T
    r.compare()
    scatter_merge_check()
    r.close()


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("T", [G, G + 1, 2 * G + 1])
def test_full_launch_groups(gpu, oracle, scratch, T, kind):
    """1b. Tensors small enough that the group limit, not the cap, closes the
    launches: exactly G tensors in one launch (every slot of the table and of
    the hand-off words), G + 1 and 2G + 1 across the boundary, ticketed and
    copy-through tensors mixed within each."""
    import torch
    from stellatrain_amd.engine import scatter_merge_check
    specs = _small_specs(T, 150)
    assert _plan(specs) == [G] * (T // G) + ([T % G] if T % G else [])
    assert {s["flag"] for s in specs} == {0, 1, 3} and {s["family"] for s in specs} == {"unique", "encoded", "raw"}
    r = _Run(torch, gpu, oracle, scratch, *KINDS[kind])
    r.step(specs, prebuilt=T == G + 1)
    r.step([dict(s, seed=s["seed"] + 1000) for s in specs])  # the slots' words again, after a first use
    if kind == "sgd":
        assert r.a.iteration == 2 * T
    r.compare()
    scatter_merge_check()
    r.close()


ITER_OPTS = {
    "sgd_momentum": ("sgd", dict(lr=0.05, momentum=0.9), True),
    "sgd_nesterov_wd": ("sgd", dict(lr=0.05, momentum=0.9, nesterov=True, weight_decay=0.01), True),
    "sgd_smart": ("sgd", dict(lr=0.05, momentum=0.9, dampening=0.1, smart_momentum=True), True),
    "adam": ("adam", dict(lr=0.01, weight_decay=0.01), True),
    "adam_amsgrad": ("adam", dict(lr=0.01, weight_decay=0.01, amsgrad=True), False),  # its running max follows the stream order
}


@pytest.mark.parametrize("opt", list(ITER_OPTS))
def test_three_batched_iterations(gpu, oracle, scratch, opt):
    """2. Three consecutive batched calls on the same names with index sets
    that differ per call (elements skip iterations; every third task copies
    through); amsgrad takes the per-tensor path inside the batch call."""
    import torch
    from stellatrain_amd.engine import scatter_merge_check
    kind, opts, with_oracle = ITER_OPTS[opt]
    r = _Run(torch, gpu, oracle, scratch, kind, opts, with_oracle)
    T = G + 1
    for c in range(3):
        r.step(_specs(T, 200 + 7 * c, unique_every=3))
        if kind == "sgd":
            assert r.a.iteration == r.b.iteration == (c + 1) * T
    r.compare()
    if opt == "sgd_smart":
        # every task took its own iteration: task i of call c ran at c * T + i
        for i in (0, 5, T - 1):
            la = r.a.last_buffer(f"t{i}", W.n_of(i % 4))
            assert la.max() == 2 * T + i
        assert r.a.iteration == 3 * T
    if kind == "adam":
        assert r.a.state("t0", W.n_of(0))[3] == 4  # the next tick after three calls
    scatter_merge_check()
    r.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_non_batchable_tasks_inside_a_batch(gpu, oracle, scratch, kind):
    """3. An empty task, a world-2 task and a repeated name in the middle of a
    batch: identical to the sequence; the empty task's count is 0 and its
    momentum buffer exists."""
    import torch
    from stellatrain_amd.engine import scatter_merge_check
    r = _Run(torch, gpu, oracle, scratch, *KINDS[kind])
    w1 = lambda name, pr, flag, seed: dict(name=name, family="encoded", per_rank=pr, flag=flag, seed=seed, world=1)  # noqa: E731
    specs = [w1("a", 1025, 1, 300), w1("b", 9, 0, 301),
             dict(name="c", family="encoded", per_rank=0, flag=1, seed=0, world=1),
             w1("d", 4099, 3, 302),
             dict(name="e", family="encoded", per_rank=1025, flag=1, seed=303, world=2),
             w1("f", 1023, 2, 304), w1("a", 1024, 1, 305), w1("g", 7, 3, 306), w1("f", 1025, 2, 307)]
    r.step(specs)
    got_c = r.a.merge_optimize_batch([])  # and an empty batch is nothing
    assert got_c == []
    n = W.n_of(1)
    if kind == "sgd":
        assert r.a.iteration == len(specs)
        mc = r.a.momentum_buffer("c", n)
        assert mc is not None and not mc.any()
    else:
        assert r.a.state("c", n)[3] == 2 and r.a.state("a", n)[3] == 3
    pa, pb, po = r.params["c"]
    assert np.array_equal(pa.cpu().numpy(), BASE[:n] + np.float32(2))  # untouched
    r.compare()
    assert not bool(scratch.dense.view(torch.int32).any()) and not bool(scratch.mark.any())
    scatter_merge_check()
    r.close()


def test_scratch_is_shared_with_per_tensor_calls(gpu, oracle, scratch):
    """4. A per-tensor scatter_merge on the same stream before and after the
    batches gives the oracle's result (the winner words were left zero)."""
    import torch
    from stellatrain_amd import scatter_merge
    from stellatrain_amd.engine import scatter_merge_check
    flag, per_rank = 0, 4099
    n = W.n_of(flag)
    streams = W.make_streams(oracle, "encoded", per_rank, flag, 1, seed=9)
    idx, val, ei, ev, _ = W.expected(oracle, streams, per_rank, n)
    di, dv = torch.from_numpy(idx.view(np.int32)).to(gpu), torch.from_numpy(val).to(gpu)

    def single():
        got = _sorted(*scatter_merge(di, dv, per_rank, 1, n))
        assert np.array_equal(got[0], ei) and np.array_equal(got[1], ev.view(np.uint32))

    single()
    rs = _Run(torch, gpu, oracle, scratch, *KINDS["sgd"])
    ra = _Run(torch, gpu, oracle, scratch, *KINDS["adam"])
    rs.step(_specs(G + 1, 400))
    single()
    ra.step(_specs(G + 1, 400))
    single()
    rs.compare()
    ra.compare()
    scatter_merge_check()
    rs.close()
    ra.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_misaligned_buffers_inside_a_batch(gpu, oracle, scratch, kind):
    """5. Every stream buffer one element into a larger tensor (only
    element-aligned: the loaders' single-load path), all four flags."""
    import torch
    from stellatrain_amd.engine import scatter_merge_check
    r = _Run(torch, gpu, oracle, scratch, *KINDS[kind])
    specs = [dict(name=f"m{i}", family=W.FAMILIES[i % 2], per_rank=[1025, 4099, 9][i % 3], flag=[1, 3, 0, 2][i % 4],
                  seed=500 + i, world=1) for i in range(8)]
    specs.append(dict(name="m8", family="unique", per_rank=1025, flag=3, seed=508, world=1))
    r.step(specs, place=_odd)
    r.compare()
    scatter_merge_check()
    r.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_prebuilt_tasks_keep_their_allocated_scratch(gpu, oracle, scratch, kind):
    """6. A world-2 item with dense / mark left to the array, run twice from one
    prebuilt MergeTasks with allocations in between: the scratch the array
    allocated stays its own (and zero), so both calls give the sequence's and
    the oracle's merged stream."""
    import torch
    from stellatrain_amd import MergeTasks
    from stellatrain_amd.engine import scatter_merge_check
    r = _Run(torch, gpu, oracle, scratch, *KINDS[kind])
    specs = [dict(name="p0", family="encoded", per_rank=1025, flag=1, seed=600, world=1),
             dict(name="p1", family="encoded", per_rank=1025, flag=1, seed=601, world=2),
             dict(name="p2", family="raw", per_rank=4099, flag=3, seed=602, world=1),
             dict(name="p3", family="encoded", per_rank=1023, flag=3, seed=603, world=2),
             dict(name="p4", family="unique", per_rank=1025, flag=1, seed=604, world=1)]
    n = W.n_of(1)
    items, seq = [], []
    for s in specs:
        streams, ei, ev = _case(oracle, s["family"], s["per_rank"], s["flag"], s["seed"], s["world"])
        pa, pb, po = r._param(s["name"], n)
        dev = [(_up(torch, gpu, wi), _up(torch, gpu, wv), f) for wi, wv, f in streams]
        items.append((pa, s["name"], dev, s["per_rank"]))  # no dense, no mark
        seq.append((pb, dev, po, ei, ev))
    tasks = MergeTasks(items)
    del items
    junk = []
    for c in range(2):
        # what the caching allocator hands out next is filled with non-zero words
        junk += [torch.full((n,), 3.0, dtype=torch.float32, device=gpu) for _ in range(4)]
        junk += [torch.full((n,), 7, dtype=torch.uint8, device=gpu) for _ in range(4)]
        got = r.a.merge_optimize_batch(tasks)
        assert got is tasks.outputs
        for s, g, (pb, dev, po, ei, ev) in zip(specs, got, seq):
            kw = dict(dense=scratch.dense[:n], mark=scratch.mark[:n]) if s["world"] > 1 else {}
            ref = _sorted(*r.b.merge_optimize_wire(pb, s["name"], dev, s["per_rank"], **kw))
            ga = _sorted(*g)
            assert np.array_equal(ga[0], ref[0]) and np.array_equal(ga[1], ref[1]), (c, s)
            assert np.array_equal(ga[0], ei) and np.array_equal(ga[1], ev.view(np.uint32)), (c, s)
            (oracle.sgd_apply if kind == "sgd" else oracle.adam_apply)(r.h, s["name"], po, ev, ei)
    r.compare()
    scatter_merge_check()
    r.close()


@pytest.mark.parametrize("opt", ["sgd_smart", "adam"])
def test_param_len_mismatch_refuses_the_whole_batch(gpu, oracle, scratch, opt):
    """7. A task whose param_len contradicts its name's state, or an earlier
    task of the same name in the batch, refuses the call before any state
    change: no iteration, no tick, no state for the good tasks beside it."""
    import torch
    from stellatrain_amd import CodecError
    kind, opts, _ = ITER_OPTS[opt]
    r = _Run(torch, gpu, oracle, scratch, kind, opts, with_oracle=False)
    mk = lambda name, seed: dict(name=name, family="encoded", per_rank=1025, flag=1, seed=seed, world=1)  # noqa: E731
    r.step([mk("x", 700), mk("y", 701)])
    n = W.n_of(1)
    streams = _case(oracle, "encoded", 1025, 1, 702)[0]
    dev = [(_up(torch, gpu, wi), _up(torch, gpu, wv), f) for wi, wv, f in streams]
    full, short = (torch.zeros(m, dtype=torch.float32, device=gpu) for m in (n, n - 1000))
    for items in ([(full, "z", dev, 1025), (short, "x", dev, 1025)],    # against the name's state
                  [(full, "z", dev, 1025), (full, "q", dev, 1025), (short, "q", dev, 1025)]):  # within the batch
        with pytest.raises(CodecError, match=f"task {len(items) - 1}: param_len") as e:
            r.a.merge_optimize_batch(items)
        assert e.value.code == -1
        if kind == "sgd":
            assert r.a.iteration == 2 and r.a.momentum_buffer("z", n) is None and r.a.last_buffer("z", n) is None
        else:
            assert r.a.state("x", n)[3] == 2 and r.a.state("z", n) is None and r.a.state("q", n) is None
    assert not bool(full.any()) and not bool(short.any())
    r.compare()
    r.close()
