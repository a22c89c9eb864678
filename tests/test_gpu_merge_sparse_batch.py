"""GPU parity of the batched sparse MERGE step (``merge_optimize_sparse_batch``):
every task's merged stream against the numpy model of test_gpu_merge_sparse,
and parameters, state and streams against a twin handle that runs
``merge_optimize_sparse`` per tensor in the same order -- bit for bit."""
from __future__ import annotations


import numpy as np
import pytest

from test_gpu_merge_sparse import OPTS, TILE, VALS, decode, host, make, model, upload

pytestmark = pytest.mark.gpu

NS = [1, 33, 4095, 4096, 4097, 3 * 4096 + 5, 70001]


def streams_for(n, per_rank, world, seed, kind):
    """"mixed": make()'s streams, wire flags mixed.  Else flag 0 with every index >= n ("none"), at 0
    ("zero"), or inside tile 1 ("tile1")."""
    if kind == "mixed":
        return make(n, per_rank, world, seed)
    rng = np.random.default_rng([n, per_rank, world, seed])
    idx = {"none": lambda: n + rng.integers(0, 3, per_rank), "zero": lambda: np.zeros(per_rank),
           "tile1": lambda: rng.integers(TILE, 2 * TILE, per_rank)}[kind]
    return [(idx().astype(np.uint32), VALS[rng.integers(0, VALS.size, per_rank)], 0) for _ in range(world)]


def run_calls(torch, gpu, opt, specs, calls=3):
    """`calls` batched calls on specs = [(name, n, per_rank, world, kind)] against the model and the twin's
    loop; returns the launches of the last call."""
    from stellatrain_amd import SparseAdam, SparseSGD, merge_batch_launches
    from stellatrain_amd.engine import scatter_merge_check
    kind, kw = OPTS[opt]
    a, b = ((SparseSGD if kind == "sgd" else SparseAdam)(**kw) for _ in range(2))
    lens = {name: n for name, n, *_ in specs}
    p0 = {name: torch.from_numpy(np.random.default_rng(n).standard_normal(n).astype(np.float32)).to(gpu)
          for name, n in lens.items()}
    pa, pb = ({k: v.clone() for k, v in p0.items()} for _ in range(2))
    for call in range(calls):
        items, want = [], []
        for q, (name, n, pr, world, sk) in enumerate(specs):
            st = streams_for(n, pr, world, 16 * call + q, sk)
            oi = torch.full((pr * world,), -91, dtype=torch.int32, device=gpu)
            ov = torch.full((pr * world,), -91.0, dtype=torch.float32, device=gpu)
            items.append((pa[name], name, upload(torch, gpu, st), pr, None, None, oi, ov))
            want.append(model([decode(wi, wv, f, pr) for wi, wv, f in st], n))
        before = merge_batch_launches()
        outs = a.merge_optimize_sparse_batch(items)
        launches = merge_batch_launches() - before
        for q, (name, n, pr, world, sk) in enumerate(specs):
            what = (opt, call, q, n, pr, world, sk)
            bi, bv, bc = b.merge_optimize_sparse(pb[name], name, items[q][2], pr)
            (oi, ov, oc), (ei, ev) = outs[q], want[q]
            c = int(host(oc)[0])
            assert c == int(host(bc)[0]) == ei.size, what
            assert np.array_equal(host(oi, c), ei) and np.array_equal(host(ov, c), ev.view(np.uint32)), what
            assert np.array_equal(host(bi, c), ei) and np.array_equal(host(bv, c), ev.view(np.uint32)), what
            assert (oi[c:] == -91).all() and (ov[c:] == -91.0).all(), what  # nothing written past the count
        for name in lens:
            assert np.array_equal(host(pa[name]), host(pb[name])), (opt, call, name)
    assert any(not np.array_equal(host(pa[k]), host(p0[k])) for k in lens)
    for name, n in lens.items():
        if kind == "sgd":
            assert np.array_equal(a.momentum_buffer(name, n).view(np.uint32), b.momentum_buffer(name, n).view(np.uint32))
            if kw.get("smart_momentum"):
                assert np.array_equal(a.last_buffer(name, n), b.last_buffer(name, n)), name
        else:
            sa, sb = a.state(name, n), b.state(name, n)
            assert all(np.array_equal(sa[q].view(np.uint32), sb[q].view(np.uint32)) for q in (0, 1)), name
            assert np.float32(sa[2]).view(np.uint32) == np.float32(sb[2]).view(np.uint32) and sa[3] == sb[3], name
    if kind == "sgd":
        assert a.iteration == b.iteration == calls * len(specs)
        a.check()
    else:
        a.check_device()
    scatter_merge_check()
    return launches


@pytest.mark.parametrize("order", ["up", "down"])
@pytest.mark.parametrize("world", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("opt", list(OPTS))
def test_one_group_of_mixed_tensors(gpu, opt, world, order):
    """Odd sizes around the tile in both orders (tile0 non-trivial), per_rank cycling, a tensor in the
    middle whose every index is >= n; three calls."""
    import torch
    ns = NS if order == "up" else NS[::-1]
    specs = [(f"w{q}", n, (1, 9, 600)[q % 3], world, "mixed") for q, n in enumerate(ns)]
    specs.insert(3, ("empty", 4097, 9, world, "none"))
    run_calls(torch, gpu, opt, specs)


@pytest.mark.parametrize("case", ["17 tasks", "repeated name", "world change"])
def test_closing_a_group(gpu, case):
    import torch
    if case == "17 tasks":
        specs = [(f"w{q}", NS[q % 7], 9, 2, "mixed") for q in range(17)]
    elif case == "repeated name":  # results in order, as the loop: the second task on w0 sees the first's step
        specs = [("w0", 4097, 600, 2, "mixed"), ("w1", 33, 9, 2, "mixed"), ("w0", 4097, 600, 2, "mixed")]
    else:
        specs = [(f"w{q}", 4097, 9, w, "mixed") for q, w in enumerate([2, 2, 3, 3, 1])]
    want = {"17 tasks": 12, "repeated name": 12, "world change": 18}[case]
    assert run_calls(torch, gpu, "smart", specs) == want


@pytest.mark.parametrize("ntasks, world, want", [(16, 2, 6), (17, 8, 16)])
def test_launch_counts(gpu, ntasks, world, want):
    import torch
    specs = [(f"w{q}", 4097, 9, world, "mixed") for q in range(ntasks)]
    assert run_calls(torch, gpu, "sgd", specs, calls=1) == want


def test_one_tile_holding_many_tensors_worth_of_pairs(gpu):
    """5,000 pairs per rank inside one tile of the group's second tensor (the streamed segment past the
    register-held records), and a tensor whose every pair is index 0."""
    import torch
    specs = [("a", 70001, 600, 3, "mixed"), ("b", 70001, 5000, 3, "tile1"), ("c", 33, 9, 3, "zero"),
             ("d", 4097, 9, 3, "mixed")]
    assert run_calls(torch, gpu, "adam", specs) == 6


def test_refusals(gpu):
    """Null d_dense / d_mark at world > 1 is accepted; a null name and a bad flag are refused with the
    task's index and advance nothing."""
    import torch
    from stellatrain_amd import MergeTasks, PublishTasks, SparseSGD
    from stellatrain_amd._capi import StgRankStream, lib
    from stellatrain_amd.engine import scatter_merge_check
    L, o = lib(), SparseSGD(lr=0.05, momentum=0.9)
    p = [torch.zeros(100, device=gpu) for _ in range(3)]
    st = upload(torch, gpu, make(100, 9, 2, 0))
    t = MergeTasks([(p[q], f"w{q}", st, 9) for q in range(3)], sparse=True)
    fn = L.stg_merge_optimize_sgd_sparse_batch_device
    name, ranks = t.array[1].name, t._keep[2][0]  # (the field itself reads back as a view of the task)
    t.array[1].name = None
    assert fn(o._h, t.array, 3, None) == -1 and L.stg_last_error().startswith(b"task 1:")
    t.array[1].name = name
    bad = (StgRankStream * 2)(ranks[0], StgRankStream(ranks[1].d_idx, ranks[1].d_val, 4))
    t.array[2].ranks = bad
    assert fn(o._h, t.array, 3, None) == -1
    assert L.stg_last_error().startswith(b"task 2:") and b"flag" in L.stg_last_error()
    t.array[2].ranks = ranks
    assert o.iteration == 0 and not any(x.any() for x in p)
    assert t.array[0].d_dense is None and t.array[0].d_mark is None
    o.merge_optimize_sparse_batch(t)
    assert o.iteration == 3 and all(int(host(c)[0]) > 0 for _, _, c in t.outputs) and all(x.any() for x in p)
    assert PublishTasks.from_merge(t, [[torch.zeros(100, device=gpu)]] * 3).count == 3  # as from a dense array
    o.check()
    scatter_merge_check()
