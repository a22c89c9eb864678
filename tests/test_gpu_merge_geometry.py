"""GPU parity of the receiving side at every pointer phase, at tiny tensors and
at the tile edges: the MERGE decompress (``scatter_merge`` /
``scatter_merge_wire``), the fused steps (``merge_optimize[_wire]``), the plain
steps (``optimize_raw``) and one batched call (``merge_optimize_batch``).

Every buffer a call reads or writes is carved out of a sentinel-filled
allocation (``geometry.carve``): rank streams, outputs and parameters at every
phase of their element size, ``dense`` / ``mark`` 16-byte aligned (the API's
rule) with exactly n elements.  After every call the streams are unchanged, no
guard word around any buffer was written, the outputs past the count still
hold the sentinel, and ``dense`` / ``mark`` are zero.  A dropped index n, n + 1,
n + 63 lands on the guard behind the parameter and the scratch.

Expected values are the oracle chain ``wire_decode`` -> ``merge_decompress``
-> ``sgd_apply`` / ``adam_apply``, bit for bit with no NaN rule (the values are
tame).  The cases and what each is there for: tests/merge_geometry.py, pinned
on the CPU by tests/test_merge_geometry_host.py.
"""
from __future__ import annotations

import numpy as np
import pytest

import merge_geometry as M
from geometry import SENTINEL16, assert_guards, carve

pytestmark = pytest.mark.gpu

BASE = np.random.default_rng(29).standard_normal(1 << 14).astype(np.float32)


def _u(a):
    """The unsigned words of a host array (bits, not values)."""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.itemsize])


def _host(t):
    return _u(t.cpu().numpy())


def _put(torch, gpu, a, phase):
    """A host array in a carved device buffer at `phase` (the 16-bit wire forms
    int16-typed, u32 indices int32-typed)."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    t = torch.from_numpy(a.copy())
    v = carve(torch, gpu, t.numel(), t.dtype, phase)
    v.copy_(t)
    return v


def _zeros(torch, gpu, n, dtype):
    v = carve(torch, gpu, n, dtype, 0)
    v.zero_()
    return v


class _Scratch:
    """dense / mark of exactly n elements, 16-byte aligned, guards around them."""

    def __init__(self, torch, gpu, n):
        self.torch = torch
        self.dense = _zeros(torch, gpu, n, torch.float32)
        self.mark = _zeros(torch, gpu, n, torch.uint8)
        assert self.dense.data_ptr() % 16 == 0 and self.mark.data_ptr() % 16 == 0

    def nonzeros(self):
        t = self.torch
        return int(t.count_nonzero(self.dense.view(t.int32))) + int(t.count_nonzero(self.mark))

    def check(self, what):
        assert self.nonzeros() == 0, what
        assert_guards(self.dense, f"{what}: dense")
        assert_guards(self.mark, f"{what}: mark")


class _Call:
    """The carved buffers of one MERGE call: rank streams (wire form, or the
    decoded pairs back to back), outputs, count, and dense / mark at world > 1
    (a shared ``scratch`` cut to n, or the call's own)."""

    def __init__(self, torch, gpu, streams, n, m, k, decoded=None, scratch=None):
        self.torch, self.streams, self.world, self.m = torch, streams, len(streams), m
        flag = streams[0][2]
        self.dev = [(_put(torch, gpu, wi, M.phases(f, k, r)[0]), _put(torch, gpu, wv, M.phases(f, k, r)[1]), f)
                    for r, (wi, wv, f) in enumerate(streams)]
        self.decoded = decoded
        if decoded is not None:
            pi, pv, _, _ = M.phases(0, k)
            self.di, self.dv = _put(torch, gpu, decoded[0], pi), _put(torch, gpu, decoded[1], pv)
        _, _, po, pw = M.phases(flag, k)
        self.out_idx = carve(torch, gpu, m * self.world, torch.int32, po)
        self.out_val = carve(torch, gpu, m * self.world, torch.float32, pw)
        self.count = torch.full((1,), -7, dtype=torch.int32, device=gpu)
        self.scratch = scratch if scratch is not None else (_Scratch(torch, gpu, n) if self.world > 1 else None)
        self.n = n

    def kw(self):
        kw = dict(out_idx=self.out_idx, out_val=self.out_val, count=self.count)
        if self.world > 1:
            kw.update(dense=self.scratch.dense[:self.n], mark=self.scratch.mark[:self.n])
        return kw

    def fresh_outputs(self):
        self.out_idx.view(self.torch.int16).fill_(SENTINEL16 - 0x10000)
        self.out_val.view(self.torch.int16).fill_(SENTINEL16 - 0x10000)
        self.count.fill_(-7)

    def check(self, exp_idx, exp_val, what, untouched_tail=True):
        """Count, indices and value bits; the streams as they were; guards."""
        c = int(_host(self.count)[0])
        assert c == exp_idx.size, (what, c, exp_idx.size)
        gi, gv = _host(self.out_idx), _host(self.out_val)
        assert np.array_equal(gi[:c], exp_idx), what   # in order: ascending, or at world 1 the stream's
        assert np.array_equal(gv[:c], _u(exp_val)), what
        if untouched_tail:  # the emission stores nothing past the count
            assert (gi[c:] == 0xffa5ffa5).all() and (gv[c:] == 0xffa5ffa5).all(), what
        for r, ((di, dv, _), (wi, wv, _)) in enumerate(zip(self.dev, self.streams)):
            assert np.array_equal(_host(di), _u(wi)) and np.array_equal(_host(dv), _u(wv)), (what, r)
            assert_guards(di, f"{what}: rank {r} idx")
            assert_guards(dv, f"{what}: rank {r} val")
        if self.decoded is not None:
            assert np.array_equal(_host(self.di), _u(self.decoded[0])), what
            assert np.array_equal(_host(self.dv), _u(self.decoded[1])), what
            assert_guards(self.di, f"{what}: decoded idx")
            assert_guards(self.dv, f"{what}: decoded val")
        assert_guards(self.out_idx, f"{what}: out_idx")
        assert_guards(self.out_val, f"{what}: out_val")
        if self.world > 1:
            self.scratch.check(what)


def _expected(oracle, n, m, flag, world, seed, kind):
    """(streams, decoded idx, decoded val, expected idx, expected val): the
    oracle's merge -- at world 1 in stream order, as the device emits it (the
    same pairs: checked on the CPU)."""
    streams, idx, val, ei, ev, _ = M.case(oracle, n, m, flag, world, seed, kind)
    if world == 1:
        ei, ev = M.stream_order(idx, val, n)
    return streams, idx, val, ei, ev


def _merge_both(torch, gpu, oracle, n, m, kind, flag, world, k):
    """One case through scatter_merge_wire and through scatter_merge on the
    decoded pairs."""
    from stellatrain_amd import scatter_merge, scatter_merge_wire
    streams, idx, val, ei, ev = _expected(oracle, n, m, flag, world, 0, kind)
    what = (n, m, kind, flag, world)
    call = _Call(torch, gpu, streams, n, m, k, decoded=(idx, val))
    scatter_merge_wire(call.dev, m, n, **call.kw())
    call.check(ei, ev, what + ("wire",))
    call.fresh_outputs()
    scatter_merge(call.di, call.dv, m, world, n, **call.kw())
    call.check(ei, ev, what + ("decoded",))


# ---------------------------------------------------------------------------
# A. scatter_merge / scatter_merge_wire
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("world", M.WORLDS)
@pytest.mark.parametrize("flag", M.FLAGS)
def test_merge_tiny(gpu, oracle, flag, world):
    """A. n = 1 .. 33 (every lane of the mark tile a ragged one below 16),
    per_rank 0, 1, min(n, 4), n and n + 3."""
    import torch
    from stellatrain_amd.engine import scatter_merge_check
    for k, n, m, kind in M.merge_cases("tiny"):
        if kind == "unique" and world != 1:
            continue
        _merge_both(torch, gpu, oracle, n, m, kind, flag, world, k)
    scatter_merge_check()


@pytest.mark.parametrize("world", M.EDGE_WORLDS)
@pytest.mark.parametrize("flag", M.EDGE_FLAGS)
def test_merge_edges(gpu, oracle, flag, world):
    """A. n and per_rank within one of 1,024, 4,096, 8,192 (and n of 65,536:
    with u16 indices the saturating family)."""
    import torch
    from stellatrain_amd.engine import scatter_merge_check
    for k, n, m, kind in M.merge_cases("edge"):
        if kind == "unique" and (world != 1 or (flag & 1 and n > 32768)):
            continue
        _merge_both(torch, gpu, oracle, n, m, kind, flag, world, k)
    scatter_merge_check()


# ---------------------------------------------------------------------------
# B. the second round of the tile-count scan
# ---------------------------------------------------------------------------
def test_merge_second_scan_round(gpu, oracle):
    """B. n = 2^24 + 4,096 + 5 at world 2: 4,098 tiles, so mark_scan carries its
    running count into a second round of two tiles, the last one ragged; then a
    tiny tensor on the same (device, stream) scratch, whose tile counts must
    not be the large call's."""
    import torch
    from stellatrain_amd import scatter_merge_wire
    from stellatrain_amd.engine import scatter_merge_check, scatter_merge_release
    n, m = M.SIZE_SCAN, M.SCAN_PER_RANK
    scratch = _Scratch(torch, gpu, n)
    for flag in (0, 3):
        streams, idx, val, ei, ev, st = M.scan_case(oracle, flag)
        call = _Call(torch, gpu, streams, n, m, 4 + flag, scratch=scratch)
        scatter_merge_wire(call.dev, m, n, **call.kw())
        assert scratch.nonzeros() == 0
        call.check(ei, ev, ("scan", flag))
    for sn, sm in ((33, 36), (17, 4)):
        _merge_both(torch, gpu, oracle, sn, sm, "planted", 0, M.SCAN_WORLD, 1)
    scatter_merge_check()
    scatter_merge_release()


# ---------------------------------------------------------------------------
# C. the fused steps
# ---------------------------------------------------------------------------
class _Opt:
    """A device optimizer and its oracle twin."""

    def __init__(self, oracle, opt):
        from stellatrain_amd import SparseAdam, SparseSGD
        self.oracle, self.sgd = oracle, opt in M.SGD_OPTS
        self.opts = M.SGD_OPTS[opt] if self.sgd else M.ADAM_OPTS[opt]
        self.dev = (SparseSGD if self.sgd else SparseAdam)(**self.opts)
        self.h = oracle.sgd_new(**self.opts) if self.sgd else oracle.adam_new(**self.opts)

    def apply(self, name, po, grad, gidx):
        (self.oracle.sgd_apply if self.sgd else self.oracle.adam_apply)(self.h, name, po, grad, gidx)

    def compare_state(self, name, n, what, other=None):
        """The name's state against the oracle's (and a twin handle's)."""
        o, d = self.oracle, self.dev
        if self.sgd:
            for got, exp in ((d.momentum_buffer(name, n), o.sgd_momentum(self.h, name, n)),
                             (d.last_buffer(name, n), o.sgd_last(self.h, name, n) if self.opts.get("smart_momentum")
                              else None)):
                if got is not None and exp is not None:
                    assert np.array_equal(_u(got), _u(exp)), what
            assert not self.opts.get("momentum") or d.momentum_buffer(name, n) is not None, what
            assert d.iteration == o.sgd_iter(self.h), what
            if other is not None:
                for f in (d.momentum_buffer, d.last_buffer):
                    x, y = f(name, n), getattr(other, f.__name__)(name, n)
                    assert (x is None) == (y is None) and (x is None or np.array_equal(_u(x), _u(y))), what
        else:
            sa, so = d.state(name, n), o.adam_state(self.h, name, n)
            assert sa is not None and so is not None, what
            for q in (0, 1):
                assert np.array_equal(_u(sa[q]), _u(so[q])), (what, q)
            assert _u(np.float32(sa[2])) == _u(np.float32(so[2])) and sa[3] == so[3], what
            if other is not None:
                sb = other.state(name, n)
                assert all(np.array_equal(_u(sa[q]), _u(sb[q])) for q in (0, 1)) and sa[3] == sb[3], what

    def close(self):
        if self.sgd:
            self.dev.check()
            self.oracle.sgd_free(self.h)
        else:
            self.dev.check_device()
            self.oracle.adam_free(self.h)


@pytest.mark.parametrize("world", M.STEP_WORLDS)
@pytest.mark.parametrize("opt", list(M.SGD_OPTS) + list(M.ADAM_OPTS))
def test_fused_steps(gpu, oracle, opt, world):
    """C. Four calls on one name per size, wire form and decoded alternating,
    on a parameter carved at a rotating phase: the parameter in full, the
    merged stream and the optimizer state against the oracle.  The dropped
    indices n, n + 1, n + 63 are the guard words behind the parameter."""
    import torch
    from stellatrain_amd.engine import scatter_merge_check
    for k, n, m, flag, phase in M.step_cases():
        t = _Opt(oracle, opt)
        po = (BASE[:n] + np.float32(k % 7)).astype(np.float32)
        param = _put(torch, gpu, po, phase)
        scratch = _Scratch(torch, gpu, n) if world > 1 else None
        for c in range(M.STEP_CALLS):
            kind = M.step_kind(world, c) if 0 < m <= n else "planted"
            streams, idx, val, ei, ev = _expected(oracle, n, m, flag, world, c, kind)
            what = (opt, world, n, m, flag, c, kind)
            call = _Call(torch, gpu, streams, n, m, k + c, decoded=(idx, val), scratch=scratch)
            if c % 2 == 0:
                t.dev.merge_optimize_wire(param, "w", call.dev, m, **call.kw())
            else:
                t.dev.merge_optimize(param, "w", call.di, call.dv, m, world, **call.kw())
            call.check(ei, ev, what)
            t.apply("w", po, ev, ei)  # in the order the device steps (amsgrad's running maximum follows it)
            assert np.array_equal(_host(param), _u(po)), what
            assert_guards(param, f"{what}: param")
        t.compare_state("w", n, (opt, world, n, m, flag))
        t.close()
    scatter_merge_check()


# ---------------------------------------------------------------------------
# D. optimize_raw
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["nesterov_wd", "smart", "adam", "amsgrad"])
def test_optimize_raw(gpu, oracle, opt):
    """D. sgd_apply<false / true>, adam_apply and adam_apply_ams on carved grad,
    gidx and param: grad_len over the 1,024 tile edges, and a device length of
    grad_len - 1 and of 0 below a larger capacity whose tail holds valid
    indices with gradients of 1e6."""
    import torch
    k = 0
    for grad_len in M.RAW_LENS:
        for cap, dlen in M.raw_variants(grad_len):
            pg, pi, pp = M.TRIPLES_RAW[k % len(M.TRIPLES_RAW)]
            k += 1
            t = _Opt(oracle, opt)
            po = (BASE[:M.RAW_N] * np.float32(3)).astype(np.float32)
            param = _put(torch, gpu, po, pp)
            dl = None if dlen is None else torch.tensor([dlen], dtype=torch.int32, device=gpu)
            eff = grad_len if dlen is None else dlen
            for c in range(3):
                gidx, grad = M.raw_case(grad_len, cap, c)
                what = (opt, grad_len, cap, dlen, c, (pg, pi, pp))
                d_grad, d_gidx = _put(torch, gpu, grad, pg), _put(torch, gpu, gidx, pi)
                t.dev.optimize_raw(param, "r", d_grad, d_gidx, grad_len=cap, d_grad_len=dl)
                t.apply("r", po, grad[:eff], gidx[:eff])
                assert np.array_equal(_host(param), _u(po)), what
                assert np.array_equal(_host(d_grad), _u(grad)) and np.array_equal(_host(d_gidx), _u(gidx)), what
                for v, nm in ((param, "param"), (d_grad, "grad"), (d_gidx, "gidx")):
                    assert_guards(v, f"{what}: {nm}")
            assert eff == 0 or not np.array_equal(po, BASE[:M.RAW_N] * np.float32(3))
            t.compare_state("r", M.RAW_N, (opt, grad_len, cap, dlen))
            t.close()


# ---------------------------------------------------------------------------
# E. one batched call over tiny and tile-edge tensors
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("world", M.BATCH_WORLDS)
@pytest.mark.parametrize("opt", ["smart", "adam"])
def test_batched_small_tensors(gpu, oracle, opt, world):
    """E. 24 tasks of n = 1 .. 8,199 in one merge_optimize_batch call, one of
    them empty, a group of sixteen closing in the middle; parameters carved at
    rotating phases; two iterations from one prebuilt MergeTasks (the second on
    new streams written into the same receive buffers).  Each task against the
    oracle and against merge_optimize_wire on a twin handle; the launches
    against the closing rule of codec.h."""
    import torch
    from stellatrain_amd import MergeTasks, SparseAdam, SparseSGD, merge_batch_launches
    from stellatrain_amd.engine import scatter_merge_check
    specs = M.batch_specs(world)
    t = _Opt(oracle, opt)
    twin = (SparseSGD if t.sgd else SparseAdam)(**t.opts)
    scratch = _Scratch(torch, gpu, max(M.BATCH_N)) if world > 1 else None
    calls, params, items = [], [], []
    for i, (name, n, m, flag, phase) in enumerate(specs):
        streams = M.case(oracle, n, m, flag, world, 0, "planted")[0]
        call = _Call(torch, gpu, streams, n, m, i, scratch=scratch)
        po = (BASE[:n] + np.float32(i)).astype(np.float32)
        pa, pb = _put(torch, gpu, po, phase), torch.from_numpy(po.copy()).to(gpu)
        kw = call.kw()
        items.append((pa, name, call.dev, m, kw.get("dense"), kw.get("mark"), call.out_idx, call.out_val, call.count))
        calls.append(call)
        params.append((pa, pb, po))
    tasks = MergeTasks(items)
    plan = M.batch_plan(specs)
    want = sum((2 if world == 1 else world + 4) if g else (0 if world == 1 else 3) for g in plan)
    for it in range(2):
        if it:  # new streams arrive in the same buffers
            for call, (name, n, m, flag, _) in zip(calls, specs):
                call.streams = M.case(oracle, n, m, flag, world, it, "planted")[0]
                for (di, dv, _), (wi, wv, _) in zip(call.dev, call.streams):
                    di.copy_(torch.from_numpy(_u(wi).view(np.int16 if wi.itemsize == 2 else np.int32).copy()))
                    dv.copy_(torch.from_numpy(wv.view(np.int16).copy() if wv.itemsize == 2 else wv.copy()))
        before = merge_batch_launches()
        got = t.dev.merge_optimize_batch(tasks)
        assert got is tasks.outputs
        assert merge_batch_launches() - before == want, (plan, want)
        for call, (name, n, m, flag, _), (pa, pb, po) in zip(calls, specs, params):
            streams, idx, val, ei, ev = _expected(oracle, n, m, flag, world, it, "planted")
            what = (opt, world, it, name, n, m, flag)
            call.check(ei, ev, what, untouched_tail=it == 0)
            t.apply(name, po, ev, ei)
            assert np.array_equal(_host(pa), _u(po)), what
            assert_guards(pa, f"{what}: param")
            # the per-tensor twin (its outputs are its own)
            kw = dict(dense=scratch.dense[:n], mark=scratch.mark[:n]) if world > 1 else {}
            oi, ov, cnt = twin.merge_optimize_wire(pb, name, call.dev, m, **kw)
            c = int(_host(cnt)[0])
            assert c == ei.size and np.array_equal(_host(oi)[:c], ei) and np.array_equal(_host(ov)[:c], _u(ev)), what
            assert np.array_equal(_host(pb), _u(po)), what
    for (name, n, m, flag, _) in specs:
        t.compare_state(name, n, (opt, world, name), other=twin)
    if t.sgd:
        assert t.dev.iteration == twin.iteration == 2 * len(specs)
        twin.check()
    else:
        twin.check_device()
    t.close()
    scatter_merge_check()


# ---------------------------------------------------------------------------
# F. publish_params on replicas of fewer than 16 elements
# ---------------------------------------------------------------------------
def _publish_task(torch, gpu, n, c, k):
    """(item, check) of one publish task over n <= 33 elements: the master, the
    index stream (c published slots -- the last element, element 0, an index
    >= n among them where they fit -- then stale slots holding valid indices)
    and one float32, bfloat16 and float16 replica, all carved; every replica
    starts as the complement of the converted master."""
    import publish_cases as P
    from geometry import PHASES2
    rng = np.random.default_rng([n, c, k])
    master = (BASE[64 * k:64 * k + n] * np.float32(7)).astype(np.float32)
    idx = rng.permutation(n).astype(np.uint32)[:c]
    for q, j in enumerate((n - 1, 0)[:c]):
        at = np.flatnonzero(idx == j)
        if at.size:
            idx[at[0]] = idx[q]
        idx[q] = j
    if c == n and k % 2:
        idx = np.arange(n, dtype=np.uint32)    # one ascending run to the replica's last element (the vector stores)
    elif c >= 3:
        idx[c - 1] = (n, n + 1, n + 63, 0xffffffff)[k % 4]
    stale = rng.integers(0, n, 5, dtype=np.uint32)
    slots = np.concatenate([idx, stale]).astype(np.uint32)
    param = _put(torch, gpu, master, M.PHASES4[k % 4])
    d_idx = _put(torch, gpu, slots, M.PHASES4[(k + 1) % 4])
    d_cnt = torch.tensor([c], dtype=torch.int32, device=gpu)
    reps = []
    for r, (dt, tdt) in enumerate(((P.DT_F32, torch.float32), (P.DT_BF16, torch.bfloat16), (P.DT_F16, torch.float16))):
        start = ~P.cvt_bits(master, dt)
        phase = M.PHASES4[(k + r) % 4] if dt == P.DT_F32 else PHASES2[(k + r) % len(PHASES2)]
        v = carve(torch, gpu, n, tdt, phase)
        v.view(torch.int32 if dt == P.DT_F32 else torch.int16).copy_(
            torch.from_numpy(start.view(np.int32 if dt == P.DT_F32 else np.int16).copy()))
        reps.append((v, dt, start))

    def check(what):
        assert np.array_equal(_host(param), _u(master)) and np.array_equal(_host(d_idx), slots), what
        assert_guards(param, f"{what}: param")
        assert_guards(d_idx, f"{what}: idx")
        for v, dt, start in reps:
            exp, pub = P.expected_replica(start, master, slots, c, dt)
            assert not P.is_nan_bits(exp, dt).any() and pub.sum() == np.unique(idx[idx < n]).size, what
            got = _host(v.view(torch.int32 if dt == P.DT_F32 else torch.int16))
            assert np.array_equal(got, exp), (what, dt, np.flatnonzero(got != exp)[:8])
            assert_guards(v, f"{what}: replica {dt}")

    return (param, d_idx, d_cnt, [v for v, _, _ in reps]), check


def test_publish_tiny_replicas(gpu):
    """F. Parameters and replicas of 1 .. 33 elements (tests/test_gpu_publish.py
    starts at 8,199), every buffer carved: single tasks at counts 0, 1,
    min(n, 4) and n, then all of them in one batched call."""
    import torch
    from stellatrain_amd import publish_params
    k = 0
    batch = []
    for n in M.TINY_N:
        for c in sorted({0, 1, min(n, 4), n}):
            item, check = _publish_task(torch, gpu, n, c, k)
            publish_params([item])
            check(("single", n, c))
            batch.append(_publish_task(torch, gpu, n, c, k + 1) + ((n, c),))
            k += 1
    publish_params([item for item, _, _ in batch])
    for _, check, nc in batch:
        check(("batch",) + nc)
